"""Robust PnPL for a set of frames with a hypothesis budget PER SCENE and draws guided by the matcher's scores: 24 synthetic scenes of 60
points and 40 lines whose share of clutter runs from 0 to 60 %.  With confidence=0.99 every scene stops as soon as the standard rule says
it has drawn enough minimal sets for its own inlier share, counted over points and lines together; n_hyp = 1024 is only the cap.  With
quality= / line_quality= (one scale for both) the first hypotheses come from the best-ranked correspondences of the union
(cvxpnpl_amd.ransac.ransac_pnpl_batch(confidence=..., quality=..., line_quality=...); not in the reference)."""
import numpy as np
import torch

import _scene  # noqa: F401
from cvxpnpl_amd import ransac, synth

F, CAP, P, L = 24, 1024, 60, 40
shares = np.linspace(0.0, 0.6, F)
frames = [synth.make_ransac_pnpl(P, L, outlier_frac=float(s), sigma=0.5, seed=400 + f) for f, s in enumerate(shares)]
rs = np.random.RandomState(5)
# a matcher's confidence that knows something, not everything: inliers score U(0.2, 1), clutter U(0, 0.8), points and lines alike
score = lambda inl: np.where(inl, rs.uniform(0.2, 1.0, len(inl)), rs.uniform(0.0, 0.8, len(inl)))
qp, ql = [score(d["inlier_pts"]) for d in frames], [score(d["inlier_lines"]) for d in frames]
args = tuple([d[k] for d in frames] for k in ("pts_2d", "line_2d", "pts_3d", "line_3d")) + (synth.K_KINECT,)
kw = dict(n_hyp=CAP, thresh=2.0, seed=1, confidence=0.99, round_hyp=64, device=torch.device("cuda:0"))
plain = ransac.ransac_pnpl_batch(*args, **kw)
guided = ransac.ransac_pnpl_batch(*args, quality=qp, line_quality=ql, **kw)
assert guided["pool_full"] == CAP and "pool_full" not in plain

for out in (plain, guided):
    used = out["hyp_used"].numpy()
    R, mp, ml = out["R"].cpu().numpy(), out["inliers_pts"].cpu().numpy(), out["inliers_lines"].cpu().numpy()
    op, ol = out["offsets"].cpu().numpy(), out["line_offsets"].cpu().numpy()
    worst = 0.0
    for f, d in enumerate(frames):
        mine = np.concatenate([mp[op[f]:op[f + 1]], ml[ol[f]:ol[f + 1]]])
        truth = np.concatenate([d["inlier_pts"], d["inlier_lines"]])
        gap = float(synth.geodesic(R[f][None], d["R_gt"][None])[0])
        worst = max(worst, gap)
        assert int(out["n_inliers"][f]) == mine.sum() >= 0.9 * truth.sum() and (mine & ~truth).sum() <= 2 and gap < 2e-2, (f, mine.sum(), truth.sum(), gap)
        assert used[f] % 64 == 0 and 64 <= used[f] <= CAP, (f, used[f])
    assert used[0] == 64 and used[:4].max() == 64            # clean scenes stop after the first round
    assert used[-1] > used[0] and used.sum() < F * CAP // 2   # cluttered scenes draw more; the set draws a fraction of the fixed budget
    print(f"{'guided' if 'pool_full' in out else 'uniform'}: {F} frames, {int(used.sum())} hypotheses solved in {out['rounds']} rounds instead of "
          f"{F * CAP} (per scene {used.min()} .. {used.max()}), worst rotation error {worst:.2e} rad")
# pool_full = 0 turns the guidance off: the unguided call, bit for bit
off = ransac.ransac_pnpl_batch(*args, quality=qp, line_quality=ql, pool_full=0, **kw)
assert torch.equal(off["R"].view(torch.int64), plain["R"].view(torch.int64)) and torch.equal(off["hyp_used"], plain["hyp_used"])
assert torch.equal(off["inliers_pts"], plain["inliers_pts"]) and torch.equal(off["inliers_lines"], plain["inliers_lines"])
