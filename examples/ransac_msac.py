"""Robust PnP for a set of frames with MSAC scoring: 48 synthetic scenes of 100 correspondences, 30 % clutter and 1 px of noise, 128
hypotheses each at a threshold of 4 px.  Most scenes tie on the inlier count -- many minimal sets explain all the inliers -- and the lowest
index decides; scoring="msac" selects by the truncated quadratic cost instead and lands closer to the true pose among the SAME draws
(cvxpnpl_amd.ransac.ransac_pnp_batch(scoring="msac"); not in the reference)."""
import numpy as np
import torch

import _scene  # noqa: F401
from cvxpnpl_amd import ransac, synth

F, H, THRESH = 48, 128, 4.0
frames = [synth.make_ransac(1, n_corr=100, outlier_frac=0.3, sigma=1.0, seed=100 + f) for f in range(F)]
xs, Xs = [d["scene_2d"] for d in frames], [d["scene_3d"] for d in frames]
R_gt = np.stack([d["R_gt"] for d in frames])
kw = dict(n_hyp=H, thresh=THRESH, seed=0, refit=False, device=torch.device("cuda:0"))   # no refit: the selected minimal hypotheses themselves
cnt = ransac.ransac_pnp_batch(xs, Xs, synth.K_KINECT, **kw)
msac = ransac.ransac_pnp_batch(xs, Xs, synth.K_KINECT, scoring="msac", **kw)
err_c = np.degrees(synth.geodesic(cnt["R"].cpu().numpy(), R_gt))
err_m = np.degrees(synth.geodesic(msac["R"].cpu().numpy(), R_gt))
# the gain of the count call's winners, by the scoring kernel: the MSAC winner of the same draws cannot gain less
sc = ransac.pack_scenes(xs, Xs, synth.K_KINECT, device=kw["device"])
gain_c, _ = ransac.score_scenes_msac(sc, cnt["R"], cnt["t"], THRESH)
assert msac["scoring"] == "msac" and msac["score"].shape == (F,) and (msac["score"] >= gain_c).all()
assert (msac["n_inliers"] <= cnt["n_inliers"]).all()   # ... as it cannot count more
same = int((msac["best_index"] == cnt["best_index"]).sum())
assert err_m.mean() <= 0.85 * err_c.mean(), (err_m.mean(), err_c.mean())
print(f"{F} frames, {H} hypotheses each: rotation error of the count winner mean {err_c.mean():.3f} deg (median {np.median(err_c):.3f}), of the "
      f"MSAC winner mean {err_m.mean():.3f} deg (median {np.median(err_m):.3f}); the same hypothesis in {same} frames, MSAC closer in "
      f"{int((err_m < err_c).sum())}, farther in {int((err_m > err_c).sum())}")
