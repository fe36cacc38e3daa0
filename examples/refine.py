"""Robust PnP with a reprojection polish: 12 synthetic frames with 30 % clutter and 1 px noise through ransac_pnp_batch, without and with
polish=True (cvxpnpl_amd.refine.refine_scenes over the consensus set, one more launch; not in the reference), and the covariance of the
polished pose of the first frame."""
import numpy as np
import torch

import _scene  # noqa: F401
from cvxpnpl_amd import ransac, refine, synth

sizes = [int(v) for v in np.round(np.geomspace(60, 400, 12))]
frames = [synth.make_ransac(1, n_corr=m, outlier_frac=0.3, sigma=1.0, seed=300 + f) for f, m in enumerate(sizes)]
args = ([d["scene_2d"] for d in frames], [d["scene_3d"] for d in frames], synth.K_KINECT)
kw = dict(n_hyp=256, thresh=3.0, seed=1, device=torch.device("cuda:0"))
plain = ransac.ransac_pnp_batch(*args, **kw)
polished = ransac.ransac_pnp_batch(*args, polish=True, **kw)
assert (polished["n_inliers"] >= plain["n_inliers"]).all()                     # a polished pose is kept only when it holds the consensus
status, cost = polished["refine"]["status"].cpu().numpy(), polished["refine"]["cost"].cpu().numpy()
assert np.isin(status, (0, 1)).all() and (cost[:, 1] <= cost[:, 0]).all()
gap = [float(np.mean([synth.geodesic(o["R"][f].cpu().numpy()[None], d["R_gt"][None])[0] for f, d in enumerate(frames)])) for o in (plain, polished)]
assert gap[1] < 2e-2
rms = np.sqrt(cost / (2.0 * plain["n_inliers"].numpy()[:, None]))
print(f"{len(frames)} frames: rms pixel error of the consensus set {rms[:, 0].mean():.3f} -> {rms[:, 1].mean():.3f} px, "
      f"mean rotation error {gap[0]:.2e} -> {gap[1]:.2e} rad, inliers {int(plain['n_inliers'].sum())} -> {int(polished['n_inliers'].sum())}")

# the covariance of one polished pose, from its own inliers
d, off = frames[0], polished["offsets"].cpu().numpy()
sc = ransac.pack_scenes(args[0][:1], args[1][:1], synth.K_KINECT, device=kw["device"])
res = refine.refine_scenes(sc, polished["R"][:1].contiguous(), polished["t"][:1].contiguous(),
                           mask_pts=polished["inliers"][off[0]:off[1]].view(torch.uint8).contiguous(), want_cov=True)
sd = torch.sqrt(torch.diagonal(res.cov[0])).cpu().numpy()
assert int(res.status[0]) == 0 and np.isfinite(sd).all()
print(f"frame 0: sigma of the rotation {np.linalg.norm(sd[:3]):.2e} rad, of the translation {np.linalg.norm(sd[3:]):.2e}")
