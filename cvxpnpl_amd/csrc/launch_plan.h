// launch_plan.h -- the launch policy of one solve as a pure host function: options and launch size in, the kernels to launch out.
// Nothing here touches HIP: cvxpnpl_hip.hip (launch_solve) executes the plan, tests/hostsim/plan_shim.cpp builds this header with a
// host compiler so that tests/test_launch_plan.py can check every decision without a GPU.
#pragma once
#include <stddef.h>
#include <stdint.h>
#include <stdio.h>

#include "../../include/cvxpnpl_amd.h"
#include "solver_core.h"

namespace cvxplan {

// launch constants of the kernel headers (cvxw::RS_LANE, RS_FULL, RESUME_GRID_MAX, WPB; cvxi::IPMQ_GRID_MAX), handed in by the caller
struct Limits { int rs_lane, rs_full, resume_grid_max, ipmq_grid_max, wpb; };

// the first kernel of a solve: exactly the instantiations the library ships
enum FirstKernel : int {
    K_WAVE_FULL, K_WAVE_RC,             // cvxw::solve_wave_kernel<VAR>
    K_LANE2_F32, K_LANE2_F64,           // solve_lane2_kernel<f64_sweeps> (lane_kernel.hip)
    K_QUAD,                             // cvxq::solve_quad_kernel<0, 2, 16, false, VAR_FULL>
    K_QUAD_F64,                         //                        <0, 2, 16, true,  VAR_FULL>
    K_QUAD_PENTA,                       //                        <0, 2, 12, false, VAR_FULL>
    K_QUAD_RC,                          //                        <0, 2, 16, false, VAR_RC>
    K_QUAD_RC_F64,                      //                        <0, 2, 16, true,  VAR_RC>
    K_QUAD_MINIMAL,                     //                        <2, 3, 16, false, VAR_FULL>
    K_QUAD_MINIMAL_F64                  //                        <2, 2, 16, true,  VAR_FULL>
};

// the launches behind the first kernel
enum FollowKind : int {
    F_RESUME, // cvxw::resume_wave_kernel[_rc]: the parked problems of the resume queue, one per wavefront
    F_IPM,    // cvxi::ipm_quad_kernel<VAR>: the rescue queue through the interior-point solve into the resume queue
    F_RESCUE  // cvxw::rescue_wave_kernel[_rc]: the rescue queue (two_queues: and the resume queue) with the fused interior-point solve
};
struct FollowUp {
    int kind;
    int64_t grid;
    int stride;      // doubles per parked problem the launch reads (ipm: writes)
    bool full;       // the parked slots hold the quad schedule's record (RS_FULL), not the lane schedule's
    bool two_queues; // rescue behind a quad phase: both queues in one launch
};
constexpr int MAX_FOLLOW = 4; // (quad schedule, split interior-point path: two rounds of ipm + resume)

struct SolvePlan {
    bool too_large;       // the batch does not fit one launch: nothing else is filled in
    cvx::Opts o;          // resolved options (first_check, rescue_from, f32_sweeps_until, dual_shift by layout / size / variant)
    int layout;           // the schedule that runs (CVXPNPL_LAYOUT_LANE / WAVE / QUAD)
    int last_layout;      // what cvxpnpl_last_layout() reports (PENTA for the twelve-lane quad kernel)
    int handoff_at;       // length of the quad / lane phase; 0: the first kernel is the wave kernel
    int first;            // FirstKernel
    int64_t first_grid;
    bool rescue, split;   // interior-point path in force; as kernels of its own (ipm + resume) rather than fused into the rescue kernel
    int ws_stride;        // doubles per parked problem of the workspace this solve needs
    bool needs_workspace;
    int n_follow;
    FollowUp follow[MAX_FOLLOW];
};

inline void public_defaults(cvxpnpl_opts_t *opts)
{
    cvx::Opts o = cvx::default_opts();
    opts->eps = o.eps; opts->max_iters = o.max_iters; opts->rho = o.rho; opts->alpha = o.alpha;
    opts->first_check = 0 /* by layout, see cvxpnpl_amd.h */; opts->check_every = o.check_every; opts->res_tol = o.res_tol;
    opts->jacobi_sweeps = o.jacobi_sweeps; opts->jacobi_tol = o.jacobi_tol; opts->warm_start = o.warm_start; opts->rho_tail = o.rho_tail; opts->tail_from = o.tail_from; opts->lane_iters = -1; opts->layout = CVXPNPL_LAYOUT_AUTO; opts->variant = CVXPNPL_VARIANT_FULL;
    opts->adapt_every = o.adapt_every; opts->adapt_from = o.adapt_from; opts->adapt_mu = o.adapt_mu; opts->adapt_tau = o.adapt_tau;
    opts->stall_from = o.stall_from; opts->stall_lam = o.stall_lam; opts->stall_res = o.stall_res; opts->stall_drop = o.stall_drop;
    opts->rescue_from = o.rescue_from;
    opts->f32_sweeps_until = -1;
    opts->sweep_schedule = 1;
    opts->dual_shift = -1.0; /* by variant */
    opts->dual_refine = -1;
    opts->struct_size = (uint32_t)sizeof(cvxpnpl_opts_t);
}

inline cvx::Opts to_core(const cvxpnpl_opts_t *opts)
{
    cvx::Opts o = cvx::default_opts();
    if (opts) {
        o.eps = opts->eps; o.max_iters = opts->max_iters; o.rho = opts->rho; o.alpha = opts->alpha;
        o.first_check = opts->first_check; o.check_every = opts->check_every; o.res_tol = opts->res_tol;
        o.jacobi_sweeps = opts->jacobi_sweeps; o.jacobi_tol = opts->jacobi_tol; o.warm_start = opts->warm_start; o.rho_tail = opts->rho_tail; o.tail_from = opts->tail_from;
        o.variant = opts->variant;
        o.adapt_every = opts->adapt_every; o.adapt_from = opts->adapt_from; o.adapt_mu = opts->adapt_mu; o.adapt_tau = opts->adapt_tau;
        o.stall_from = opts->stall_from; o.stall_lam = opts->stall_lam; o.stall_res = opts->stall_res; o.stall_drop = opts->stall_drop;
        o.rescue_from = opts->rescue_from;
        o.f32_sweeps_until = opts->f32_sweeps_until;
        o.sweep_schedule = opts->sweep_schedule != 0;
        o.dual_shift = opts->dual_shift < 0.0 ? (opts->variant == CVXPNPL_VARIANT_RC ? 0.006 : cvx::DUAL_SHIFT_DEFAULT) : opts->dual_shift; // (rc, 50 k problems: 17.3 M poses/s without, 17.3 / 18.4 / 18.3 M with 0.015 / 0.006 / 0.001)
        o.dual_refine = opts->dual_refine != 0;
    }
    if (o.f32_sweeps_until < 0) o.f32_sweeps_until = cvx::F32_SWEEPS_DEFAULT;
    return o;
}

// false (and the message in err) for an options block no entry point accepts; NULL = the defaults, always valid
inline bool validate(const cvxpnpl_opts_t *opts, char *err, size_t err_len)
{
    if (!opts) return true;
    if (opts->struct_size != (uint32_t)sizeof(cvxpnpl_opts_t)) {
        // a caller built against another revision of cvxpnpl_opts_t: refuse rather than read fields that are not there
        snprintf(err, err_len, "cvxpnpl: options block of %u bytes, this library's cvxpnpl_opts_t has %zu (cvxpnpl_default_opts / cvxpnpl_opts_size)",
                 opts->struct_size, sizeof(cvxpnpl_opts_t));
        return false;
    }
    if (opts->max_iters < 1 || opts->f32_sweeps_until < -1 || opts->f32_sweeps_until > cvx::F32_SWEEPS_DEFAULT || !(opts->rho > 0) || !(opts->eps > 0) || opts->check_every < 1 || opts->first_check < 0 ||
        (opts->variant != CVXPNPL_VARIANT_FULL && opts->variant != CVXPNPL_VARIANT_RC) || opts->adapt_every < 0 ||
        (opts->adapt_every > 0 && !(opts->adapt_mu >= 1.0 && opts->adapt_tau > 1.0)) || opts->rescue_from < -1 || !((opts->dual_shift >= 0.0 && opts->dual_shift <= 1.0) || opts->dual_shift == -1.0) || opts->dual_refine < -1 || opts->dual_refine > 1) {
        snprintf(err, err_len, "cvxpnpl: bad options");
        return false;
    }
    // layouts: the public enum only (the experiment layouts 9-13 of rounds 2-5 are recorded in profiles/, their code is in the history)
    if (!(opts->layout >= CVXPNPL_LAYOUT_AUTO && opts->layout <= CVXPNPL_LAYOUT_PENTA)) {
        snprintf(err, err_len, "cvxpnpl: bad options (layout %d is not one of CVXPNPL_LAYOUT_*)", opts->layout);
        return false;
    }
    return true;
}

// The launches of one solve of `batch` problems with n_p point and n_l line correspondences each (cost_seam: the caller brought the
// cost instead, cvxpnpl_solve_cost_batch).  opts: validated, or NULL.
inline SolvePlan plan_solve(int64_t batch, int n_p, int n_l, bool cost_seam, const cvxpnpl_opts_t *opts, const Limits &lim)
{
    SolvePlan p = {};
    const int64_t lane_grid = (batch + 63) / 64;
    if (lane_grid > 0x7fffffffLL) { p.too_large = true; return p; }
    cvx::Opts &o = p.o;
    o = to_core(opts);
    if (!opts) o.first_check = 0; // (by layout, below)
    const int req_layout = opts ? opts->layout : CVXPNPL_LAYOUT_AUTO;
    const int req_iters = opts ? opts->lane_iters : -1; // the caller's length of the first phase (<= 0: default)
    const int n_corr = n_p + n_l;
    // The 16-equality variant (benchmarks/toolkit/methods/rc.py): wave-per-problem and the quad schedule (the constraint set is a
    // template parameter of the kernels); the lane kernels and the twelve-lane geometry are built for the full set.
    const bool rc = o.variant == cvx::VAR_RC;
    // Minimal problems (four correspondences; the cost seam does not say): 18 iterations on average and a fifth of them beyond 32 --
    // the lane-hybrid schedule would park nearly all of them for the one-problem-per-wavefront phase.  They stay four per wavefront
    // for 24 iterations instead, like the rc variant: 50 k problems 11.2 -> 12.4 M poses/s (lane_iters 16 / 24 / 32 / 40: 12.1 / 12.4 /
    // 11.7-12.2 / 12.3; five correspondences and more: the lane-hybrid schedule wins, 36.8 against 33.6 M at N = 5).  A caller's
    // lane_iters takes the launch out of this schedule.  (minimal implies the quad layout below: AUTO, >= 2560 problems, 24 < max_iters.)
    const bool minimal = !cost_seam && n_corr <= 4 && !rc && req_layout == CVXPNPL_LAYOUT_AUTO && batch >= 2560 && o.max_iters > 24 && req_iters <= 0;

    // AUTO, by launch size (measured on one MI355X, M poses/s, PnP N = 10, one launch stream; wave / quad: profiles/r02/layout_sweep.txt,
    // quad / lane-hybrid with the register-budgeted first phase: profiles/r03/layout_sweep2.txt, two problem sets per size):
    //   wave / quad      2 k: 19.7 / 17.3    5 k: 27.9 / 34.1    10 k: 33.8 / 51.7
    //   quad / lane     10 k: 51.6, 49.1 / 36.7, 41.0    16 k: 52.0, 73.5 / 48.7, 63.3    20 k: 74.5, 72.8 / 79.6, 73.4
    //                   24 k: 74.5, 75.6 / 95.4, 86.8    32 k: 87.2, 87.7 / 115.0, 124.8   125 k: 113 / 247
    // * below 2560 problems a wavefront per problem: every SIMD gets work and a finished problem frees its slot at once;
    // * from there four problems per wavefront (one per DPP row): 2.5x fewer instructions per problem;
    // * from 20 000 the lane-hybrid schedule (64 problems per wavefront for the first lane_iters iterations): fewest instructions
    //   per problem, but it needs ~20 k problems to give every SIMD a wavefront (round 2, general scalar core: crossover 24 576).
    //   (with every sweep in float64 the crossover is the same: quad / lane 16 k: 58.0 / 57.0, 20 k: 59.0 / 59.6, 24 k: 62.2 / 75.9, 32 k: 67.9 / 99.0 -- profiles/r04/f64_layout_crossover.txt)
    // The problems the quad phase leaves open are finished by the same wavefront, those of the lane phase by a second kernel,
    // one per wavefront in both cases.
    const int by_size = batch < 2560 ? CVXPNPL_LAYOUT_WAVE : ((batch < 20000 || minimal) ? CVXPNPL_LAYOUT_QUAD : CVXPNPL_LAYOUT_LANE);
    const int asked = req_layout == CVXPNPL_LAYOUT_AUTO ? by_size : req_layout;
    const bool lane_req = asked == CVXPNPL_LAYOUT_LANE && !rc;  // (rc: a LANE / PENTA request runs the quad schedule)
    const bool penta_req = asked == CVXPNPL_LAYOUT_PENTA && !rc;
    const bool wave_req = asked == CVXPNPL_LAYOUT_WAVE;

    // Length of the lane phase: right after the first certificate attempt (opts.first_check: 6 by default in this layout) -- later is
    // slower (round 1, first attempt at 5: hand-off at 5 / 6 / 7: 110 / 105 / 100 M at 125 k) -- and never past 6 iterations: from then on
    // the few problems still open are the slow / ambiguous ones (twin candidates, tails), which belong to the wave-per-problem kernel --
    // one of them would hold 63 idle lanes, so the lane kernel is built without that logic.
    const int fc_lane = o.first_check > 0 ? o.first_check : 6;
    const int lane_iters = req_iters <= 0 ? (fc_lane < 6 ? fc_lane : 6) : (req_iters < 6 ? req_iters : 6);
    // The register-budgeted lane kernel (lane_core.h) covers the schedule of the defaults: one attempt, right at the hand-off point,
    // warm-started eigen-solves.  A lane request with any other combination of options runs the next-best schedule for its size
    // (quad from 2 560 problems, wave below) with THAT layout's defaults, and cvxpnpl_last_layout() says what ran.
    const bool lane_ok = lane_req && fc_lane == lane_iters && lane_iters >= 2 && o.warm_start != 0;
    const bool lane_refused = lane_req && !lane_ok;

    // Length of the quad phase.  7: measured (4 problem sets at 10 k, same box): 5: 0.242 ms, 7: 0.233, 8: 0.235, 10: 0.240; 24 k: 7 = 10
    // (round 1, second phase as a call: 8-12).  rc: the weaker relaxation certifies after ~21 iterations instead of 5 (N = 10): a longer
    // first phase, 36 (profiles/r03/rc_tune.txt: 28 / 36 / 44 within 1 %), up to 48 -- still inside the wave kernel's own single-precision
    // window of 64.  A caller's lane_iters is capped at 16 otherwise: the quad phase is the YOUNG part of a solve, its slow survivors belong
    // to the wave-per-problem phase.  Minimal problems and the rc variant run 24 / 36-48 iterations here, in single-precision sweeps by
    // default -- inside the window of 64 that opts.f32_sweeps_until allows and the host experiment covers; device A/B against float64
    // sweeps: profiles/r04/f32_phase_ab.txt.  (A refused lane request: the caller's lane_iters was meant for the lane phase.)
    const int quad_default = rc ? 36 : (minimal ? 24 : 7);
    const int quad_cap = (rc || minimal) ? 48 : 16;
    const int quad_asked = req_iters > 0 ? req_iters : quad_default;
    const int quad_iters = lane_refused ? 7 : (quad_asked < quad_cap ? quad_asked : quad_cap);

    // The layout that runs.  A quad phase that would use up the iteration cap leaves the solve to the wave kernel.
    const bool quad_req = !wave_req && !lane_ok && (!lane_refused || batch >= 2560);
    const int layout = lane_ok ? CVXPNPL_LAYOUT_LANE : ((quad_req && o.max_iters > quad_iters) ? CVXPNPL_LAYOUT_QUAD : CVXPNPL_LAYOUT_WAVE);
    const bool quad = layout == CVXPNPL_LAYOUT_QUAD;
    const bool f64_phase = o.f32_sweeps_until < quad_iters; // float64 sweeps in the quad phase (A/B mode)
    // the REQUEST (five problems per wavefront) and the kernel that serves it are separate: with float64 sweeps the twelve-lane geometry
    // does not exist and the request runs the sixteen-lane quad kernel
    const bool penta = quad && penta_req && !f64_phase;
    // fewer iterations allowed than the lane phase would run: the wave kernel does the whole solve (reported as the lane layout)
    const bool lane_hybrid = layout == CVXPNPL_LAYOUT_LANE && o.max_iters > lane_iters;
    p.layout = layout;
    p.last_layout = penta ? CVXPNPL_LAYOUT_PENTA : layout;

    // First certificate attempt (0 = by layout): after 5 iterations 94 % of N = 10 problems certify, after 6 99 %.  In the lane-hybrid
    // schedule every problem that fails the first attempt is parked and resumed one per wavefront, so the later attempt pays for its
    // extra iteration: 125 k problems 157 -> 164 M poses/s, PnPL 100 k 116 -> 126 M.  The quad and wave layouts keep 5 (quad with 6, launch
    // time relative to 5 over 4 problem sets per size: 3 k 0.93, 5 k 1.07, 8 k 1.02, 10 k 0.98, 12 k 1.07, 16 k 1.03, 20 k 1.02, 24 k 0.97;
    // wave: -12 % at 2 k).
    // Four-correspondence problems in the schedule that queues its survivors: an attempt costs the whole wavefront two to three
    // iterations' worth -- at three wavefronts per SIMD the certificate's code is the part that spills -- and these problems need 14-20
    // iterations on average: first attempt after 17 (profiles/r04/minimal_tune*.txt, 50 k problems / config 5, M per second: first attempt
    // after 7: 13.0 / 21.3, 9: 13.5 / 22.4, 13: 14.5 / 23.5, 17: 14.9 / 24.0, 21: 14.5 / 23.9; every third iteration instead of every second: same).
    // rc: nothing certifies before ~10 iterations; 5 ... 15 within 3 %; in the quad schedule 19 instead of 11 (profiles/r04/rc_tune_r04.txt:
    // 50 k problems 18.3 -> 19.3 M poses/s, 10 k 9.0 -> 9.3 M).
    if (o.first_check <= 0) o.first_check = rc ? (quad ? 19 : 11) : (minimal ? 17 : (layout == CVXPNPL_LAYOUT_LANE ? 6 : 5));

    // Interior-point path for the problems still open after rescue_from iterations (ipm_wave.h): its queue lives in the workspace.
    // -1 (default): by problem size.  Slow convergence is a property of minimal and near-minimal configurations
    // (profiles/r02/remaining_iters.jsonl, 100 k problems each, first-order iterations only: with N = 4 / 5 / 6 / 7 correspondences
    // 21 % / 3.8 % / 0.7 % / 0.14 % of the problems are still open after 32 iterations and 27 % / 17 % / 12 % / 6 % of those need more
    // than the ~75 iterations an interior-point solve costs, slowest 1 455 / 1 037 / 581 / 227; with N = 8 the slowest takes 99, with
    // N = 10 (1 M problems) 61, and a problem that is open after 48 finishes within the next 3-25).  A threshold below the natural tail
    // of a workload sends problems through a 0.3 ms solve they did not need and ends the launch later: 100 k problems with N = 8
    // 1.05 ms without the path, 1.35 ms with 96; 1 M with N = 10 4.46 / 4.75 ms with 96 / 32; against that 10 k problems with N = 4
    // 4.77 / 1.78 ms, N = 6 (100 k) 3.42 / 1.91 ms without / with 32, N = 7 (100 k) 1.71 / 1.49 ms without / with 64.
    // rc: the weaker relaxation is tight less often, and a problem whose relaxation is not tight crawls to max_iters -- 13 of 10 000
    // N = 10 problems run all 2 500 iterations, 10 ms per launch whatever the layout (profiles/r03/rc_rate.txt) -- while the typical
    // problem certifies after ~19 iterations (median; p90 33): hand over at 48 whatever the size (profiles/r03/rc_tune.txt, 50 k
    // problems: 48 / 64 / 80 / 96 -> 2.92 / 3.10 / 3.46 / 3.63 ms, same outcomes).
    const int n_size = cost_seam ? 8 : n_corr;
    if (o.rescue_from < 0) o.rescue_from = rc ? 48 : (n_size <= 6 ? 32 : (n_size == 7 ? 64 : 128));
    p.rescue = o.rescue_from > 0 && o.max_iters > o.rescue_from;
    // The interior-point path comes in two builds.  Fused (cvxw::rescue_wave_kernel: the solve compiled into a resume kernel, one launch
    // behind the first kernel) where it is a safety net -- seven correspondences and more: its queue is empty in nearly every launch and
    // one more (empty) launch would cost the 10 k-problem step 2 %.  Split (cvxi::ipm_quad_kernel + the plain resume kernel) where
    // problems really go through it -- at most five correspondences, the 16-equality variant: a fifth of the four-point problems
    // (measured, split / fused, M poses/s: N = 4 50 k 17.96 / 15.07, config 5 25.6 / 24.7, N = 5 100 k 37.3 / 35.8, N = 6 125 k 73.1 / 75.5:
    // profiles/r05/ipm_quad_ab.txt).
    p.split = p.rescue && (rc || (!cost_seam && n_corr <= 5));

    // ONE workspace per solve, with the stride of the schedule that runs (quad: RS_FULL doubles per parked problem, lane and the split
    // path behind a wave kernel: RS_LANE)
    p.ws_stride = quad ? lim.rs_full : ((lane_hybrid || p.split) ? lim.rs_lane : 0);
    p.needs_workspace = p.rescue || quad || lane_hybrid;

    // the first kernel
    if (quad) {
        // four problems per wavefront (penta: five) for the first quad_iters iterations.  A wavefront finishes its own survivors; only
        // planar scenes, recognised before the first iteration, are queued for the launch behind it.
        // Four-correspondence problems: EVERY survivor of the 24-iteration first phase goes to that queue instead -- 59 % of these
        // wavefronts end with survivors, most of which are headed for the interior-point path anyway, and without the wave-per-problem
        // code the kernel runs three wavefronts per SIMD (168 registers; with float64 sweeps two).  Measured
        // (profiles/r04/quad_mode2_minimal.txt): 50 k four-point problems 12.4 -> 13.1 M poses/s, config 5 19.8 -> 21.3 M hypotheses/s
        // (with the first attempt after 17 iterations, above: 14.9 / 24.0 M); the same schedule LOSES on the N = 10 launches, whose few
        // survivors then start late (profiles/r04/tail_experiments.txt).
        p.first = minimal ? (f64_phase ? K_QUAD_MINIMAL_F64 : K_QUAD_MINIMAL)
                : penta   ? K_QUAD_PENTA
                : rc      ? (f64_phase ? K_QUAD_RC_F64 : K_QUAD_RC)
                          : (f64_phase ? K_QUAD_F64 : K_QUAD);
        p.first_grid = penta ? (batch + 4) / 5 : (batch + 3) / 4;
        p.handoff_at = quad_iters;
    } else if (lane_hybrid) {
        // 64 problems per wavefront for the first lane_iters iterations, survivors resumed one per wavefront
        p.first = o.f32_sweeps_until >= lane_iters ? K_LANE2_F32 : K_LANE2_F64;
        p.first_grid = lane_grid;
        p.handoff_at = lane_iters;
    } else {
        p.first = rc ? K_WAVE_RC : K_WAVE_FULL;
        p.first_grid = (batch + lim.wpb - 1) / lim.wpb;
        if (layout == CVXPNPL_LAYOUT_WAVE && p.first_grid > 0x7fffffffLL) { p.too_large = true; return p; } // (a lane request cut down to the wave kernel: not checked, as ever)
    }

    // the launches behind it (the resume kernel leaves the queue counter at zero for the next solve: no memset per call)
    const int64_t rgrid = batch < lim.resume_grid_max ? batch : lim.resume_grid_max;
    const int64_t ipm_groups = (batch + 3) / 4;
    const FollowUp resume_lane = {F_RESUME, rgrid, lim.rs_lane, false, false};
    const FollowUp resume_full = {F_RESUME, rgrid, lim.rs_full, true, false};
    const FollowUp ipm = {F_IPM, ipm_groups < lim.ipmq_grid_max ? ipm_groups : lim.ipmq_grid_max, p.ws_stride, quad, false};
    int &n = p.n_follow;
    if (quad) {
        if (p.split) {
            // the wavefronts' own slow survivors (rescue queue) through the interior-point kernel into the resume queue, behind the planar
            // scenes parked there; a parked problem that reaches rescue_from in the resume kernel takes the second round
            for (int round = 0; round < 2; ++round) { p.follow[n++] = ipm; p.follow[n++] = resume_full; }
        } else if (p.rescue) p.follow[n++] = FollowUp{F_RESCUE, 2 * rgrid, lim.rs_full, true, true};
        else p.follow[n++] = resume_full;
    } else {
        if (lane_hybrid) p.follow[n++] = resume_lane;
        if (p.split) { p.follow[n++] = ipm; p.follow[n++] = resume_lane; }
        else if (p.rescue) p.follow[n++] = FollowUp{F_RESCUE, rgrid, lim.rs_full, true, false};
    }
    return p;
}

} // namespace cvxplan
