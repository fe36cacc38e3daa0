"""cvxpnpl_amd -- MI355X-native batched absolute-pose SDP solver.

Drop-in for the hot path of SergioRAgostinho/cvxpnpl (pnp / pnl / pnpl) plus batched
variants that solve tens of thousands to millions of independent problems per launch.
"""
__version__ = "0.1.0"

from ._lib import VARIANT_FULL, VARIANT_RC  # noqa: F401
from .api import (BatchResult, assemble_batch, assemble_subsets, ipm_batch, pack_cost, pnl, pnl_batch, pnp, pnp_batch, pnpl, pnpl_batch, recover_multi,  # noqa: F401
                  recover_multi_batch, recover_multi_device, refit_update, sample_minimal_sets, score_hypotheses, select_best, solve_cost_batch, solve_relaxation, solve_relaxation_rc)
from .grad import pnl_batch_diff, pnp_batch_diff, pnpl_batch_diff, pose_vjp, pose_vjp_host  # noqa: F401
from .refine import RefineResult, refine_pose_batch, refine_pose_batch_host, refine_scenes  # noqa: F401
from .refine_robust import RobustRefineResult, refine_pose_batch_robust, refine_pose_batch_robust_host, refine_scenes_robust  # noqa: F401
from .refine_robust_auto import (RobustAutoResult, RobustCovariance, RobustScale, refine_pose_batch_robust_auto, refine_pose_batch_robust_auto_host,  # noqa: F401
                                 refine_scenes_robust_auto, robust_covariance_batch, robust_covariance_host, robust_covariance_scenes, robust_scale_batch,
                                 robust_scale_batch_host, robust_scale_scenes)
from .refine_robust_grad import refine_pose_batch_robust_diff, refine_vjp_robust, refine_vjp_robust_host, refine_vjp_scenes_robust  # noqa: F401
from .refine_grad import pose_passthrough, refine_pose_batch_diff, refine_vjp, refine_vjp_host, refine_vjp_scenes  # noqa: F401
from .ransac import ransac_pnl, ransac_pnl_batch, ransac_pnp_batch, ransac_pnpl, ransac_pnpl_batch  # noqa: F401
from .ransac import (adaptive_init_msac, msac_gain_host, score_active_msac, score_scenes_msac, select_scenes_msac,  # noqa: F401
                     update_active_msac)
from .ransac import lo_assemble_active, lo_assemble_host, lo_init, lo_thresholds, lo_update_active  # noqa: F401
from .ransac import lo_assemble_pnpl_active, lo_assemble_pnpl_host, lo_update_pnpl_active  # noqa: F401
