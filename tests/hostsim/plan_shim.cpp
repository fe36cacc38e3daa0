// TEST-ONLY: cvxplan::plan_solve / validate (csrc/launch_plan.h) behind a C entry for ctypes (tests/test_launch_plan.py).
#include <string.h>

#include "../../cvxpnpl_amd/csrc/launch_plan.h"

extern "C" {

struct PlanFlat {
    int32_t valid, too_large; // valid = 0: the options were refused, err holds the message and nothing else is filled in
    int32_t layout, last_layout, handoff_at, first;
    int64_t first_grid;
    int32_t first_check, rescue_from, f32_sweeps_until;
    double dual_shift;
    int32_t rescue, split, ws_stride, needs_workspace, n_follow;
    int32_t kind[cvxplan::MAX_FOLLOW], stride[cvxplan::MAX_FOLLOW], full[cvxplan::MAX_FOLLOW], two_queues[cvxplan::MAX_FOLLOW];
    int64_t grid[cvxplan::MAX_FOLLOW];
    char err[256];
};

void plan_default_opts(cvxpnpl_opts_t *opts) { cvxplan::public_defaults(opts); }

// limits: rs_lane, rs_full, resume_grid_max, ipmq_grid_max, wpb
void plan_flat(int64_t batch, int32_t n_p, int32_t n_l, int32_t cost_seam, const cvxpnpl_opts_t *opts, const int32_t *limits, PlanFlat *out)
{
    memset(out, 0, sizeof(*out));
    if (!cvxplan::validate(opts, out->err, sizeof(out->err))) return;
    out->valid = 1;
    const cvxplan::Limits lim = {limits[0], limits[1], limits[2], limits[3], limits[4]};
    const cvxplan::SolvePlan p = cvxplan::plan_solve(batch, n_p, n_l, cost_seam != 0, opts, lim);
    out->too_large = p.too_large;
    if (p.too_large) return;
    out->layout = p.layout; out->last_layout = p.last_layout; out->handoff_at = p.handoff_at; out->first = p.first; out->first_grid = p.first_grid;
    out->first_check = p.o.first_check; out->rescue_from = p.o.rescue_from; out->f32_sweeps_until = p.o.f32_sweeps_until; out->dual_shift = p.o.dual_shift;
    out->rescue = p.rescue; out->split = p.split; out->ws_stride = p.ws_stride; out->needs_workspace = p.needs_workspace; out->n_follow = p.n_follow;
    for (int i = 0; i < p.n_follow; ++i) {
        out->kind[i] = p.follow[i].kind; out->grid[i] = p.follow[i].grid; out->stride[i] = p.follow[i].stride;
        out->full[i] = p.follow[i].full; out->two_queues[i] = p.follow[i].two_queues;
    }
}

} // extern "C"
