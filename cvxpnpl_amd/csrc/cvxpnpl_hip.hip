// cvxpnpl_hip.hip -- HIP kernels (gfx950) and the C ABI of include/cvxpnpl_amd.h.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stdio.h>
#include <string.h>
#include <unistd.h>

#include <map>
#include <memory>
#include <mutex>
#include <vector>
#include <utility>

#include "../../include/cvxpnpl_amd.h"
#include "problem_io.h"
#include "solver_core.h"
#include "lane_core.h"
#include "batch_args.h"
#include "wave_kernel.h"
#include "quad_kernel.h"
#include "ipm_quad.h"
#include "score_kernel.h"
#include "assemble_kernel.h"
#include "synth_kernel.h"
#include "recover_kernel.h"
#include "launch_plan.h"
#include "solver_entry.h"

namespace {

using cvxb::BatchArgs; // (batch_args.h: shared with lane_kernel.hip)
using cvxse::fail;      // (the error text, the correspondence block and the limit of one launch: solver_entry.h)
using cvxse::hip_error;
using cvxse::launched;
using cvxse::over_grid;

// (solve_lane2_kernel, the first phase of the lane-hybrid schedule: lane_kernel.hip, a translation unit of its own -- cvxb::launch_lane2)

// results of one shard as the 13-doubles-per-pose records the multi-GPU gather exchanges: R (9, row-major), t (3), status
__global__ void __launch_bounds__(256) pack_kernel(int64_t batch, const double *R, const double *t, const int32_t *status, double *out)
{
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= batch * 13) return;
    const int64_t b = i / 13;
    const int k = (int)(i - b * 13);
    out[i] = k < 9 ? R[b * 9 + k] : (k < 12 ? t[b * 3 + (k - 9)] : (double)status[b]);
}

__global__ void __launch_bounds__(64) assemble_kernel(BatchArgs a, double *Bout, double *Qout)
{
    int64_t b = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (b >= a.batch) return;
    cvx::ProblemView pv = cvx::make_view(b, a.n_p, a.p2, a.p3, a.n_l, a.l2, a.l3, a.K, a.K_per_problem);
    double B[27], Q9[45];
    bool ok = cvx::assemble(pv, B, Q9);
    for (int i = 0; i < 27; ++i) Bout[b * 27 + i] = ok ? B[i] : NAN;
    if (Qout)
        for (int i = 0; i < 45; ++i) Qout[b * 45 + i] = ok ? Q9[i] : NAN;
}

// Assembly for subsets of ONE scene: problem b takes the correspondences m with mask[b][m] != 0 (the refit of a RANSAC consensus set:
// the mask is what cvxs::score_kernel wrote, so that the size of the set never has to travel to the host).  One lane per problem; the
// Gram sums are the ones of cvx::assemble, taken about the same kind of centre (median of the subset's first three points: any centre is
// exact).  Fewer than three correspondences give a singular N^T N: NaN, as cvx::assemble reports it.
__global__ void __launch_bounds__(64) assemble_subsets_kernel(int64_t batch, int n_corr, const double *s2, const double *s3, const uint8_t *mask, const double *K,
                                                              double *Bout, double *Qout, int32_t *count)
{
    const int64_t b = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (b >= batch) return;
    double Kc[9], Ki[9], det;
    for (int i = 0; i < 9; ++i) Kc[i] = K[i];
    cvx::inv3(Kc, Ki, det);
    cvx::Gram g;
    cvx::gram_zero(g);
    // centre of the Gram sums: the median of the subset's OWN first three correspondences (round 5 took the scene's first three whether
    // selected or not: a non-finite or far-away outlier among them spoilt every subset, also those that mask it out -- advisor)
    const uint8_t *mk = mask + b * n_corr;
    double c[3] = {0.0, 0.0, 0.0}, first3[9];
    int nf = 0;
    for (int m = 0; m < n_corr && nf < 3; ++m)
        if (mk[m]) {
#pragma unroll
            for (int k = 0; k < 3; ++k) // (static indices: the array stays in registers)
                if (nf == k) { first3[3 * k] = s3[3 * m]; first3[3 * k + 1] = s3[3 * m + 1]; first3[3 * k + 2] = s3[3 * m + 2]; }
            ++nf;
        }
    if (nf > 0) cvx::shift_centre(nf, first3, 0, nullptr, c);
    int n = 0;
    for (int m = 0; m < n_corr; ++m) {
        if (!mk[m]) continue;
        cvx::gram_add_point(g, Ki, s2[2 * m], s2[2 * m + 1], s3[3 * m] - c[0], s3[3 * m + 1] - c[1], s3[3 * m + 2] - c[2]);
        ++n;
    }
    double B[27], Q9[45];
    bool ok = n >= 3 && cvx::gram_finish(g, B, Q9) && (det == det) && det != 0.0;
    for (int i = 0; i < 3; ++i)
        for (int j = 0; j < 3; ++j) B[i * 9 + 3 * j + i] += c[j];
    for (int i = 0; i < 27; ++i) Bout[b * 27 + i] = ok ? B[i] : NAN;
    for (int i = 0; i < 45; ++i) Qout[b * 45 + i] = ok ? Q9[i] : NAN;
    if (count) count[b] = n;
}

// Scratch of the hybrid schedules, one per (device, stream): [0, 256) the counters of the two queues (resume: ints 0..2,
// rescue: ints 16..18), then the entries of the resume queue and of the rescue queue
// (int32, -1 = empty; batch + RESUME_GRID_MAX of them each) and the parked iterates [batch][56] doubles (only the
// slots of parked problems are touched).  Either the library's own allocation (grow-only while in use, freed by
// cvxpnpl_release_workspace) or memory the caller registered with cvxpnpl_set_workspace (e.g. from torch's
// caching allocator).  The queue is self-cleaning (cvxw::resume_wave_kernel): it is initialised once.
// Offsets depend on the CAPACITY (problems) of the allocation, not on the batch of a launch, so that launches of
// different sizes agree on where the queue ends and the iterates begin.  The parked region is sized for the slot stride
// of the schedule that asked for the most (lane: 56 doubles per problem, quad: 240).
struct Workspace { void *ptr = nullptr; size_t bytes = 0; int64_t cap = 0; size_t parked_bytes = 0; bool owned = true; };
std::mutex g_ws_mutex;
std::map<std::pair<int, void *>, Workspace> g_ws;
thread_local int g_last_layout = 0; // the layout the last solve of this thread ran (cvxpnpl_last_layout)

// One solve is two or three dependent launches that share the queue and the parked-iterate buffer of their (device, stream):
// host threads calling on the SAME stream (ctypes drops the GIL; torch's default stream is shared by every thread) must not
// interleave them (A.first, B.first, A.resume: B would overwrite A's parked slots and A's resume kernel would drain B's queue
// entries with A's pointers), and the workspace must not be freed / regrown between a thread's pointer fetch and its launches.
// So the launches of a solve, from get_workspace to the last kernel, run under the mutex of their (device, stream); threads on
// different streams do not contend.  (Round 2 had dropped the global launch mutex of round 1: the advisor's finding.)
std::mutex g_lm_mutex;
std::map<std::pair<int, void *>, std::unique_ptr<std::mutex>> g_launch_mutexes; // never erased: a mutex may be held while its workspace goes
std::mutex &launch_mutex(int dev, void *stream)
{
    std::lock_guard<std::mutex> lock(g_lm_mutex);
    std::unique_ptr<std::mutex> &p = g_launch_mutexes[std::make_pair(dev, stream)];
    if (!p) p.reset(new std::mutex);
    return *p;
}

size_t queue_entries_bytes(int64_t cap) { return ((size_t)(cap + cvxw::RESUME_GRID_MAX) * sizeof(int32_t) + 255) & ~(size_t)255; }
size_t hybrid_queue_bytes(int64_t cap) { return 256 + 2 * queue_entries_bytes(cap); }
size_t hybrid_ws_bytes(int64_t cap) { return hybrid_queue_bytes(cap) + (size_t)cap * cvxw::RS_FULL * sizeof(double); } // any schedule
int64_t hybrid_capacity(size_t bytes) // largest capacity whose layout fits (any schedule)
{
    if (bytes < hybrid_ws_bytes(1)) return 0;
    int64_t cap = (int64_t)(bytes / (2 * sizeof(int32_t) + cvxw::RS_FULL * sizeof(double))) + 1; // an upper bound, then down to the first fit
    while (cap > 0 && hybrid_ws_bytes(cap) > bytes) --cap;
    return cap;
}

// counter zero, every queue entry -1 (0xFF bytes), on the stream; the parked iterates need no initialisation
bool init_workspace(void *p, int64_t cap, void *stream)
{
    if (hipMemsetAsync(p, 0xFF, hybrid_queue_bytes(cap), (hipStream_t)stream) != hipSuccess) return false;
    return hipMemsetAsync(p, 0, 256, (hipStream_t)stream) == hipSuccess;
}

struct WsView { int32_t *count, *entries, *rq_count, *rq_entries; double *parked; };

int get_workspace(int64_t batch, int stride, void *stream, WsView &v) // 0, or -2 with the message written
{
    int dev = 0;
    if (hipGetDevice(&dev) != hipSuccess) return fail(-2, "cvxpnpl: hipGetDevice failed");
    std::lock_guard<std::mutex> lock(g_ws_mutex);
    Workspace &w = g_ws[std::make_pair(dev, stream)];
    const size_t need_parked = (size_t)batch * stride * sizeof(double);
    if (w.cap < batch || w.parked_bytes < need_parked) {
        if (!w.owned)
            return fail(-2, "cvxpnpl: the registered workspace holds %lld problems, the launch has %lld (cvxpnpl_workspace_bytes)", (long long)w.cap,
                        (long long)batch);
        const int64_t cap = w.cap > batch ? w.cap : batch;
        const size_t parked = w.parked_bytes > need_parked ? w.parked_bytes : need_parked;
        if (w.ptr) { (void)hipStreamSynchronize((hipStream_t)stream); (void)hipFree(w.ptr); }
        w.ptr = nullptr; w.bytes = 0; w.cap = 0; w.parked_bytes = 0;
        const size_t bytes = hybrid_queue_bytes(cap) + parked;
        if (hipMalloc(&w.ptr, bytes) != hipSuccess || !init_workspace(w.ptr, cap, stream)) {
            if (w.ptr) (void)hipFree(w.ptr);
            w.ptr = nullptr;
            return fail(-2, "cvxpnpl: workspace allocation failed (%zu bytes)", bytes);
        }
        w.bytes = bytes; w.cap = cap; w.parked_bytes = parked;
    }
    v.count = (int32_t *)w.ptr;
    v.entries = (int32_t *)((char *)w.ptr + 256);
    v.rq_count = v.count + 16;
    v.rq_entries = (int32_t *)((char *)w.ptr + 256 + queue_entries_bytes(w.cap));
    v.parked = (double *)((char *)w.ptr + hybrid_queue_bytes(w.cap));
    return 0;
}

// The variant dispatch: a launch of `rc` under the 16-equality ablation (cvx::VAR_RC), else of `full` (the reference's 22 equalities).
// (`rc` first: the kernels come out in the device text in the order the callers name them, and tools/device_asm_diff.py compares text.)
static_assert((int)CVXPNPL_VARIANT_FULL == (int)cvx::VAR_FULL && (int)CVXPNPL_VARIANT_RC == (int)cvx::VAR_RC, "the public variants are cvx::Variant");
template <class... A>
void launch_variant(int variant, void (*rc)(A...), void (*full)(A...), int64_t grid, int block, hipStream_t s, const A &...args)
{
    hipLaunchKernelGGL(variant == cvx::VAR_RC ? rc : full, dim3((unsigned)grid), dim3((unsigned)block), 0, s, args...);
}

void launch_wave(int64_t wgrid, hipStream_t s, const cvxw::WaveArgs &w, const cvx::Opts &o)
{
    launch_variant(o.variant, cvxw::solve_wave_kernel<cvx::VAR_RC>, cvxw::solve_wave_kernel<cvx::VAR_FULL>, wgrid, 64 * cvxw::WPB, s, w, o);
}

void launch_resume(int64_t rgrid, hipStream_t s, const cvxw::WaveArgs &w, const cvx::Opts &o, int32_t *count, int32_t *entries, const double *ws, bool full)
{
    cvxw::ResumeArgs ra;
    ra.a = w; ra.o = o; ra.count_p = count; ra.entries = entries; ra.ws = ws;
    ra.ws_stride = full ? cvxw::RS_FULL : cvxw::RS_LANE; ra.ws_full = full ? 1 : 0;
    ra.count2 = nullptr; ra.entries2 = nullptr; ra.grid1 = 0;
    launch_variant(o.variant, cvxw::resume_wave_kernel_rc, cvxw::resume_wave_kernel, rgrid, 64, s, ra);
}

// last launch of a solve with opts.rescue_from in force: the problems the other kernels gave up on (w.rq_count / w.rq_entries) and,
// in the quad layout (count != null), the parked problems of the resume queue as well -- one launch for both
void launch_rescue(int64_t batch, hipStream_t s, const cvxw::WaveArgs &w, const cvx::Opts &o, int32_t *count = nullptr, int32_t *entries = nullptr,
                   const double *ws = nullptr)
{
    const int64_t rgrid = batch < cvxw::RESUME_GRID_MAX ? batch : cvxw::RESUME_GRID_MAX;
    cvxw::ResumeArgs ra;
    ra.a = w; ra.o = o; ra.count_p = w.rq_count; ra.entries = w.rq_entries; ra.ws = ws; ra.ws_stride = cvxw::RS_FULL; ra.ws_full = 1;
    ra.count2 = count; ra.entries2 = entries; ra.grid1 = (int)rgrid;
    launch_variant(o.variant, cvxw::rescue_wave_kernel_rc, cvxw::rescue_wave_kernel, count ? 2 * rgrid : rgrid, 64, s, ra);
}

// split interior-point path: the rescue queue through cvxi::ipm_quad_kernel (four solves per wavefront, ipm_quad.h) into the resume queue
// (a launch of the resume kernel follows)
void launch_ipm(int64_t batch, hipStream_t s, const cvxw::WaveArgs &w, const cvx::Opts &o, int32_t *count, int32_t *entries)
{
    const int64_t groups = (batch + 3) / 4;
    const int64_t grid = groups < cvxi::IPMQ_GRID_MAX ? groups : cvxi::IPMQ_GRID_MAX;
    cvxi::IpmQuadArgs ia;
    ia.batch = batch; ia.rho = o.rho; ia.rho_tail = o.rho_tail; ia.tail_from = o.tail_from;
    ia.rq_count = w.rq_count; ia.rq_entries = w.rq_entries; ia.count = count; ia.entries = entries; ia.ws = w.rq_ws; ia.stride = w.rq_stride;
    ia.entries_cap = (int)(batch + cvxw::RESUME_GRID_MAX < 0x7fffffffLL ? batch + cvxw::RESUME_GRID_MAX : 0x7fffffffLL);
    ia.qs_in = nullptr; ia.z_out = nullptr; ia.s_out = nullptr; ia.gap_out = nullptr; ia.it_out = nullptr;
    launch_variant(o.variant, cvxi::ipm_quad_kernel<cvx::VAR_RC>, cvxi::ipm_quad_kernel<cvx::VAR_FULL>, grid, 64, s, ia);
}

// The argument block of a launch from an entry point's correspondence parameters, everything else null ...
BatchArgs batch_inputs(int64_t batch, int32_t n_p, const double *p2, const double *p3, int32_t n_l, const double *l2, const double *l3, const double *K,
                       int32_t K_per_problem)
{
    BatchArgs a;
    memset(&a, 0, sizeof(a));
    a.batch = batch; a.n_p = n_p; a.n_l = n_l; a.K_per_problem = K_per_problem;
    a.p2 = p2; a.p3 = p3; a.l2 = l2; a.l3 = l3; a.K = K;
    return a;
}

// ... and the outputs of a solve
void batch_outputs(BatchArgs &a, double *R, double *t, int32_t *status, int32_t *iters, double *cost, double *Z, int32_t *work)
{
    a.R = R; a.t = t; a.cost = cost; a.Z = Z; a.status = status; a.iters = iters; a.work = work;
}

// The wave kernels' view of an argument block: the same fields, then the queue of the interior-point path (filled by launch_solve).
cvxw::WaveArgs wave_args(const BatchArgs &a)
{
    cvxw::WaveArgs w;
    w.batch = a.batch; w.n_p = a.n_p; w.n_l = a.n_l; w.K_per_problem = a.K_per_problem;
    w.p2 = a.p2; w.p3 = a.p3; w.l2 = a.l2; w.l3 = a.l3; w.K = a.K;
    w.R = a.R; w.t = a.t; w.cost = a.cost; w.Z = a.Z; w.status = a.status; w.iters = a.iters; w.work = a.work;
    w.Q45 = a.Q45; w.B27 = a.B27;
    w.rq_count = nullptr; w.rq_entries = nullptr; w.rq_ws = nullptr; w.rq_stride = 0;
    return w;
}

} // namespace

// diagnostics: a copy with W bytes per lane and a known byte count, against which bench.py calibrates rocprofv3's
// FETCH_SIZE / WRITE_SIZE for this path's access widths (the MI355X guide calibrates only wide streaming reads)
namespace cvxd {
template <int W>
__global__ void __launch_bounds__(256) calibration_copy_kernel(const char *src, char *dst, int64_t nbytes)
{
    const int64_t n = nbytes / W;
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (int64_t)gridDim.x * 256) {
        if (W == 4) reinterpret_cast<uint32_t *>(dst)[i] = reinterpret_cast<const uint32_t *>(src)[i];
        if (W == 8) reinterpret_cast<double *>(dst)[i] = reinterpret_cast<const double *>(src)[i];
        if (W == 16) reinterpret_cast<double2 *>(dst)[i] = reinterpret_cast<const double2 *>(src)[i];
    }
}
} // namespace cvxd

// Wavefront slots of a device for one instantiation of the quad kernel (one-wavefront blocks): resident blocks per CU times the CU count --
// the blocks of a launch from this index on start when a block of the first round retires (cvxq::QuadArgs::first_round).  Asked once per
// device and instantiation; <= 0: unknown, the kernel then gives no block a start priority.
template <int MODE, int OCC, int LPP, bool F64SW, int VAR>
static int quad_first_round(int dev)
{
#ifdef CVXQ_NO_PRIO
    return 0;
#else
    static std::mutex mu;
    static int slots[64] = {}; // 0: not asked yet, -1: the query failed
    if (dev < 0 || dev >= 64) return 0;
    std::lock_guard<std::mutex> g(mu);
    if (!slots[dev]) {
        int per_cu = 0, cus = 0;
        const bool ok = hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu, cvxq::solve_quad_kernel<MODE, OCC, LPP, F64SW, VAR>, 64, 0) == hipSuccess &&
                        hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev) == hipSuccess && per_cu > 0 && cus > 0;
        slots[dev] = ok ? per_cu * cus : -1;
        if (!ok) (void)hipGetLastError(); // (not an error of the solve)
    }
    return slots[dev];
#endif
}
template <int MODE, int OCC = 2, int LPP = 16, bool F64SW = false, int VAR = cvx::VAR_FULL>
static void launch_quad(int64_t qgrid, hipStream_t s, cvxq::QuadArgs &qa, int dev)
{
    qa.first_round = quad_first_round<MODE, OCC, LPP, F64SW, VAR>(dev);
    hipLaunchKernelGGL((cvxq::solve_quad_kernel<MODE, OCC, LPP, F64SW, VAR>), dim3((unsigned)qgrid), dim3(64), 0, s, qa);
}

// The order an entry point runs its checks in: its arguments (sizes, the pointers a launch would read or write, the scalars: one
// condition, one message, -1), the zero-size no-op (0), what depends on the size (the limit of one launch, scratch: -1), then the launch
// and its report (-2).  So an empty call with bad arguments is refused.  The entries that deviate: cvxpnpl_solve_batch,
// cvxpnpl_solve_cost_batch and cvxpnpl_sample_minimal_sets take the no-op first (an empty call may pass anything);
// cvxpnpl_assemble_subsets and cvxpnpl_ipm_batch have the limit of one launch among their arguments; cvxpnpl_select_best,
// cvxpnpl_refit_update and cvxpnpl_calibration_copy have no empty call.  A null d_B of the two assemblies is refused without a message
// (the text of an earlier failure stays), as is everything cvxpnpl_recover_multi_batch refuses (host_recover.cpp).
extern "C" {

void cvxpnpl_default_opts(cvxpnpl_opts_t *opts) { cvxplan::public_defaults(opts); }

size_t cvxpnpl_opts_size(void) { return sizeof(cvxpnpl_opts_t); }

int cvxpnpl_last_layout(void) { return g_last_layout; }

static int check_args(int64_t batch, int32_t n_p, const double *p2, const double *p3, int32_t n_l, const double *l2,
                      const double *l3, const double *K)
{
    if (cvxse::bad_corr_block(batch, n_p, p2, p3, n_l, l2, l3, K) || (n_p == 0 && n_l == 0))
        return fail(-1, "cvxpnpl: bad arguments (batch=%lld n_p=%d n_l=%d)", (long long)batch, n_p, n_l);
    return 0;
}

// the launches of one solve (shared by the correspondence entry and the cost entry): the policy is cvxplan::plan_solve (launch_plan.h),
// this function executes what it decided
static int launch_solve(const BatchArgs &a, const cvxpnpl_opts_t *opts, void *stream)
{
    static constexpr cvxplan::Limits limits = {cvxw::RS_LANE, cvxw::RS_FULL, cvxw::RESUME_GRID_MAX, cvxi::IPMQ_GRID_MAX, cvxw::WPB};
    const int64_t batch = a.batch;
    if (!a.R || !a.t || !a.status) return fail(-1, "cvxpnpl: R, t and status outputs are required");
    if (!cvxplan::validate(opts, cvxse::err_buf(), 512)) return -1;
    const cvxplan::SolvePlan p = cvxplan::plan_solve(batch, a.n_p, a.n_l, a.Q45 != nullptr, opts, limits);
    if (p.too_large) return fail(-1, "cvxpnpl: batch too large for one launch");
    int cur_dev = 0;
    if (hipGetDevice(&cur_dev) != hipSuccess) return fail(-2, "cvxpnpl: hipGetDevice failed");
    std::lock_guard<std::mutex> launch_lock(launch_mutex(cur_dev, stream)); // (see launch_mutex)
    hipStream_t s = (hipStream_t)stream;
    g_last_layout = p.last_layout;
    // ONE workspace view per solve: a second fetch with a larger stride may free and reallocate the buffer, and queue pointers taken
    // from the first would dangle
    WsView wv = {nullptr, nullptr, nullptr, nullptr, nullptr};
    if (p.needs_workspace && get_workspace(batch, p.ws_stride, stream, wv)) return -2;
    const cvx::Opts &o = p.o;
    cvxw::WaveArgs w = wave_args(a);
    w.rq_count = p.rescue ? wv.rq_count : nullptr; w.rq_entries = p.rescue ? wv.rq_entries : nullptr; // the interior-point path's queue
    w.rq_ws = p.split ? wv.parked : nullptr; w.rq_stride = p.split ? p.ws_stride : 0;
    cvxq::QuadArgs qa;
    qa.a = w; qa.o = o; qa.handoff_at = p.handoff_at; qa.qcount = wv.count; qa.qentries = wv.entries; qa.ws = wv.parked; qa.first_round = 0; // (first_round: launch_quad)
    switch (p.first) {
    case cvxplan::K_WAVE_FULL: case cvxplan::K_WAVE_RC: launch_wave(p.first_grid, s, w, o); break; // (by o.variant)
    case cvxplan::K_LANE2_F32: case cvxplan::K_LANE2_F64:
        cvxb::launch_lane2(p.first == cvxplan::K_LANE2_F64, (unsigned)p.first_grid, 64u, (void *)s, a, o, p.handoff_at, wv.count, wv.entries, wv.parked);
        break;
    case cvxplan::K_QUAD_MINIMAL_F64: launch_quad<2, 2, 16, true>(p.first_grid, s, qa, cur_dev); break;
    case cvxplan::K_QUAD_MINIMAL: launch_quad<2, 3>(p.first_grid, s, qa, cur_dev); break;
    case cvxplan::K_QUAD_PENTA: launch_quad<0, 2, 12>(p.first_grid, s, qa, cur_dev); break;
    case cvxplan::K_QUAD_RC_F64: launch_quad<0, 2, 16, true, cvx::VAR_RC>(p.first_grid, s, qa, cur_dev); break;
    case cvxplan::K_QUAD_RC: launch_quad<0, 2, 16, false, cvx::VAR_RC>(p.first_grid, s, qa, cur_dev); break;
    case cvxplan::K_QUAD_F64: launch_quad<0, 2, 16, true>(p.first_grid, s, qa, cur_dev); break;
    case cvxplan::K_QUAD: launch_quad<0, 2>(p.first_grid, s, qa, cur_dev); break;
    }
    for (int i = 0; i < p.n_follow; ++i) {
        const cvxplan::FollowUp &f = p.follow[i];
        if (f.kind == cvxplan::F_IPM) launch_ipm(batch, s, w, o, wv.count, wv.entries);
        else if (f.kind == cvxplan::F_RESUME) launch_resume(f.grid, s, w, o, wv.count, wv.entries, wv.parked, f.full);
        else if (f.two_queues) launch_rescue(batch, s, w, o, wv.count, wv.entries, wv.parked); // (both queues in one launch)
        else launch_rescue(batch, s, w, o);
    }
    return launched("solve kernel launch");
}

int cvxpnpl_solve_batch(int64_t batch, int32_t n_p, const double *d_pts_2d, const double *d_pts_3d, int32_t n_l,
                        const double *d_line_2d, const double *d_line_3d, const double *d_K, int32_t K_per_problem,
                        const cvxpnpl_opts_t *opts, double *d_R, double *d_t, int32_t *d_status, int32_t *d_iters,
                        double *d_cost, double *d_Z, int32_t *d_work, void *stream)
{
    if (batch == 0) return 0; /* empty batch: nothing to do (pointers may be NULL) */
    if (check_args(batch, n_p, d_pts_2d, d_pts_3d, n_l, d_line_2d, d_line_3d, d_K)) return -1;
    BatchArgs a = batch_inputs(batch, n_p, d_pts_2d, d_pts_3d, n_l, d_line_2d, d_line_3d, d_K, K_per_problem);
    batch_outputs(a, d_R, d_t, d_status, d_iters, d_cost, d_Z, d_work);
    return launch_solve(a, opts, stream);
}

int cvxpnpl_solve_cost_batch(int64_t batch, const double *d_Q45, const double *d_B27, const cvxpnpl_opts_t *opts, double *d_R,
                             double *d_t, int32_t *d_status, int32_t *d_iters, double *d_cost, double *d_Z, int32_t *d_work, void *stream)
{
    if (batch == 0) return 0;
    if (batch < 0 || !d_Q45 || !d_B27) return fail(-1, "cvxpnpl_solve_cost_batch: bad arguments (batch=%lld)", (long long)batch);
    BatchArgs a = batch_inputs(batch, 0, nullptr, nullptr, 0, nullptr, nullptr, nullptr, 0); // (no correspondences: the cost itself)
    a.Q45 = d_Q45; a.B27 = d_B27;
    batch_outputs(a, d_R, d_t, d_status, d_iters, d_cost, d_Z, d_work);
    return launch_solve(a, opts, stream);
}

int cvxpnpl_assemble_batch(int64_t batch, int32_t n_p, const double *d_pts_2d, const double *d_pts_3d, int32_t n_l,
                           const double *d_line_2d, const double *d_line_3d, const double *d_K, int32_t K_per_problem,
                           double *d_B, double *d_Q45, void *stream)
{
    if (check_args(batch, n_p, d_pts_2d, d_pts_3d, n_l, d_line_2d, d_line_3d, d_K) || !d_B) return -1;
    if (batch == 0) return 0;
    const BatchArgs a = batch_inputs(batch, n_p, d_pts_2d, d_pts_3d, n_l, d_line_2d, d_line_3d, d_K, K_per_problem);
    const int block = 64;
    hipLaunchKernelGGL(assemble_kernel, dim3((unsigned)((batch + block - 1) / block)), dim3(block), 0, (hipStream_t)stream, a, d_B, d_Q45);
    return launched("assemble_kernel launch");
}

int cvxpnpl_assemble_subsets(int64_t batch, int32_t n_corr, const double *d_scene_2d, const double *d_scene_3d, const uint8_t *d_mask, const double *d_K,
                             double *d_B, double *d_Q45, int32_t *d_count, void *stream)
{
    if (batch < 0 || n_corr < 1 || (batch + 63) / 64 > cvxse::GRID_MAX || (batch > 0 && (!d_scene_2d || !d_scene_3d || !d_mask || !d_K || !d_B || !d_Q45)))
        return fail(-1, "cvxpnpl_assemble_subsets: bad arguments");
    if (batch == 0) return 0;
    hipLaunchKernelGGL(assemble_subsets_kernel, dim3((unsigned)((batch + 63) / 64)), dim3(64), 0, (hipStream_t)stream, batch, (int)n_corr, d_scene_2d, d_scene_3d,
                       d_mask, d_K, d_B, d_Q45, d_count);
    return launched("assemble_subsets_kernel launch");
}

size_t cvxpnpl_assemble_large_scratch_bytes(int64_t batch, int32_t n_p, int32_t n_l)
{
    if (batch <= 0 || n_p < 0 || n_l < 0) return 0;
    return (size_t)batch * cvxa::asm_blocks((int64_t)n_p + 2 * (int64_t)n_l, batch) * 60 * sizeof(double);
}

int cvxpnpl_assemble_large_batch(int64_t batch, int32_t n_p, const double *d_pts_2d, const double *d_pts_3d, int32_t n_l,
                                 const double *d_line_2d, const double *d_line_3d, const double *d_K, int32_t K_per_problem,
                                 double *d_B, double *d_Q45, void *d_scratch, size_t scratch_bytes, void *stream)
{
    if (check_args(batch, n_p, d_pts_2d, d_pts_3d, n_l, d_line_2d, d_line_3d, d_K) || !d_B) return -1;
    if (batch == 0) return 0;
    if (batch > 65535) return fail(-1, "cvxpnpl_assemble_large_batch: at most 65535 problems per call (got %lld)", (long long)batch);
    const size_t need = cvxpnpl_assemble_large_scratch_bytes(batch, n_p, n_l);
    if (!d_scratch || scratch_bytes < need)
        return fail(-1, "cvxpnpl_assemble_large_batch: scratch of %zu bytes needed (cvxpnpl_assemble_large_scratch_bytes), got %zu", need, scratch_bytes);
    cvxa::AsmArgs a;
    a.batch = batch; a.n_p = n_p; a.n_l = n_l; a.K_per_problem = K_per_problem;
    a.nblk = cvxa::asm_blocks((int64_t)n_p + 2 * (int64_t)n_l, batch);
    a.p2 = d_pts_2d; a.p3 = d_pts_3d; a.l2 = d_line_2d; a.l3 = d_line_3d; a.K = d_K;
    a.partial = (double *)d_scratch;
    a.Bout = d_B; a.Qout = d_Q45;
    if (cvxa::asm_tpb((int64_t)n_p + 2 * (int64_t)n_l, batch) == cvxa::ASM_TPB)
        hipLaunchKernelGGL(cvxa::assemble_large_kernel<cvxa::ASM_TPB>, dim3((unsigned)a.nblk, (unsigned)batch), dim3(cvxa::ASM_TPB), 0, (hipStream_t)stream, a);
    else // short problems or many of them: one wavefront per workgroup (cvxa::asm_tpb)
        hipLaunchKernelGGL(cvxa::assemble_large_kernel<cvxa::ASM_TPB_NARROW>, dim3((unsigned)a.nblk, (unsigned)batch), dim3(cvxa::ASM_TPB_NARROW), 0, (hipStream_t)stream, a);
    if (a.nblk > 1) // several workgroups per problem: their partial sums are added in a fixed order by a second kernel
        hipLaunchKernelGGL(cvxa::assemble_finish_kernel, dim3((unsigned)((batch + 63) / 64)), dim3(64), 0, (hipStream_t)stream, a, d_B, d_Q45);
    return launched("assemble_large_kernel launch");
}

int cvxpnpl_synth_batch(int64_t batch, int32_t n_p, int32_t n_l, double sigma, uint64_t seed, const double *d_K, double *d_pts_2d,
                        double *d_pts_3d, double *d_line_2d, double *d_line_3d, double *d_R_gt, double *d_t_gt, void *stream)
{
    if (cvxse::bad_corr_block(batch, n_p, d_pts_2d, d_pts_3d, n_l, d_line_2d, d_line_3d, d_K) || !(sigma >= 0.0)) return fail(-1, "cvxpnpl_synth_batch: bad arguments");
    if (batch == 0) return 0;
    cvxg::SynthArgs a;
    a.batch = batch; a.n_p = n_p; a.n_l = n_l; a.sigma = sigma; a.length = 0.6 /* synth.py:55 */; a.seed = seed; a.K = d_K;
    a.p2 = d_pts_2d; a.p3 = d_pts_3d; a.l2 = d_line_2d; a.l3 = d_line_3d; a.R_gt = d_R_gt; a.t_gt = d_t_gt;
    const int64_t nrec = (int64_t)n_p + 2 * (int64_t)n_l, n = batch * (nrec > 0 ? nrec : 1), grid = (n + 255) / 256;
    if (over_grid(grid, "cvxpnpl_synth_batch: too many records for one launch")) return -1;
    hipLaunchKernelGGL(cvxg::synth_kernel, dim3((unsigned)grid), dim3(256), 0, (hipStream_t)stream, a);
    return launched("synth_kernel launch");
}

int cvxpnpl_pose_errors(int64_t batch, const double *d_R_gt, const double *d_t_gt, const double *d_R, const double *d_t, double *d_ang_deg,
                        double *d_trans, void *stream)
{
    if (batch < 0 || !d_R_gt || !d_t_gt || !d_R || !d_t || !d_ang_deg || !d_trans) return fail(-1, "cvxpnpl_pose_errors: bad arguments");
    if (batch == 0) return 0;
    hipLaunchKernelGGL(cvxg::pose_error_kernel, dim3((unsigned)((batch + 255) / 256)), dim3(256), 0, (hipStream_t)stream, batch, d_R_gt, d_t_gt, d_R, d_t,
                       d_ang_deg, d_trans);
    return launched("pose_error_kernel launch");
}

int cvxpnpl_disambiguate(int64_t batch, const double *d_R_all, const double *d_t_all, const int32_t *d_n_poses, const double *d_K,
                         const double *d_R_gt, const double *d_t_gt, const double *d_support, int32_t n_support, double *d_R, double *d_t,
                         int32_t *d_index, void *stream)
{
    if (batch < 0 || !d_R_all || !d_t_all || !d_n_poses || !d_K || !d_R_gt || !d_t_gt || (n_support > 0 && !d_support) || n_support < 0 || !d_R || !d_t || !d_index)
        return fail(-1, "cvxpnpl_disambiguate: bad arguments");
    if (batch == 0) return 0;
    hipLaunchKernelGGL(cvxg::disambiguate_kernel, dim3((unsigned)((batch + 255) / 256)), dim3(256), 0, (hipStream_t)stream, batch, d_R_all, d_t_all,
                       d_n_poses, d_K, d_R_gt, d_t_gt, d_support, n_support, d_R, d_t, d_index);
    return launched("disambiguate_kernel launch");
}

int cvxpnpl_recover_multi_device(int64_t batch, const int32_t *d_status, const double *d_Z55, const double *d_B27, const double *d_Q45,
                                 double *d_R_out, double *d_t_out, int32_t *d_n_poses, void *stream)
{
    if (batch < 0 || !d_Z55 || !d_B27 || !d_R_out || !d_t_out || !d_n_poses) return fail(-1, "cvxpnpl_recover_multi_device: bad arguments");
    if (batch == 0) return 0;
    hipLaunchKernelGGL(cvxr::recover_multi_kernel, dim3((unsigned)((batch + 63) / 64)), dim3(64), 0, (hipStream_t)stream, batch, d_status, d_Z55, d_B27,
                       d_Q45, d_R_out, d_t_out, d_n_poses);
    return launched("recover_multi_kernel launch");
}

// Ordering between two streams of one device without a HIP event on the producing stream: the producer enqueues a one-lane kernel
// that stores `value` to a flag in device memory (release, device scope); the consumer enqueues a one-wavefront kernel that sleeps
// and polls until the flag has reached it.  (A hipEventRecord between two kernels of a stream costs that stream ~17 us on this
// stack -- rocprofv3 trace of bench.py --force-dist: 17.6 us between the end of a solve and the start of the next against 2 us
// without the event; this pair costs it ~2 us.)  The flag only ever grows (the store is an atomic max); d_flag points to TWO words, the
// flag and the wait's "gave up" mark.  The wait is BOUNDED and therefore fails open: a consumer must read d_flag[1] after every
// synchronisation at which it consumes what the waits ordered, and discard those results when it is set (include/cvxpnpl_amd.h).
__global__ void stream_write_value_kernel(unsigned long long *flag, unsigned long long value)
{
    __threadfence();
    // max, not store: write kernels enqueued on different streams may complete out of order and the flag must never move backwards
    __hip_atomic_fetch_max(flag, value, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_AGENT);
}
// closed = true (cvxpnpl_stream_wait_value): a wait that gives up HOLDS its stream until the host has acknowledged the give-up
// (cvxpnpl_stream_wait_gave_up clears flag[1]); nobody acknowledging within ack_polls (~2^25 polls, half a minute) is a caller bug and ends in a
// trap -- loud, never a consumer silently reading unfinished results.  closed = false (cvxpnpl_stream_wait_value_bounded): the explicit
// fail-open form of rounds 3-5.
__global__ void stream_wait_value_kernel(unsigned long long *flag, unsigned long long value, unsigned long long max_polls, int closed, unsigned long long ack_polls)
{
    // bounded (max_polls > 0): if the two streams share a hardware queue the producer's kernel sits BEHIND this one and the flag can never
    // arrive -- after max_polls polls of ~1 us (cvxpnpl_stream_wait_value: 2^18, ~0.25 s) the wait gives up and says so in flag[1]
    // (the caller falls back to an event); max_polls = 0: wait for as long as it takes
    for (unsigned long long spin = 0; max_polls == 0 || spin < max_polls; ++spin) {
        if (__hip_atomic_load(flag, __ATOMIC_ACQUIRE, __HIP_MEMORY_SCOPE_AGENT) >= value) return;
        __builtin_amdgcn_s_sleep(32);
    }
    __hip_atomic_store(flag + 1, 1ull, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_SYSTEM);
    if (!closed) return;
    for (unsigned long long spin = 0; spin < ack_polls; ++spin) {
        if (__hip_atomic_load(flag + 1, __ATOMIC_ACQUIRE, __HIP_MEMORY_SCOPE_SYSTEM) == 0ull) return; // acknowledged: the caller knows
        __builtin_amdgcn_s_sleep(64);
    }
    __builtin_trap();
}

int cvxpnpl_stream_write_value(uint64_t *d_flag, uint64_t value, void *stream)
{
    if (!d_flag) return fail(-1, "cvxpnpl_stream_write_value: null flag");
    hipLaunchKernelGGL(stream_write_value_kernel, dim3(1), dim3(1), 0, (hipStream_t)stream, (unsigned long long *)d_flag, (unsigned long long)value);
    return launched("stream_write_value_kernel launch");
}

static int launch_wait(uint64_t *d_flag, uint64_t value, uint64_t max_polls, int closed, void *stream)
{
    if (!d_flag) return fail(-1, "cvxpnpl_stream_wait_value: null flag");
    hipLaunchKernelGGL(stream_wait_value_kernel, dim3(1), dim3(1), 0, (hipStream_t)stream, (unsigned long long *)d_flag, (unsigned long long)value,
                       (unsigned long long)max_polls, closed, 1ull << 25);
    return launched("stream_wait_value_kernel launch");
}

int cvxpnpl_stream_wait_value_bounded(uint64_t *d_flag, uint64_t value, uint64_t max_polls, void *stream) { return launch_wait(d_flag, value, max_polls, 0, stream); }

int cvxpnpl_stream_wait_value(uint64_t *d_flag, uint64_t value, void *stream) { return launch_wait(d_flag, value, 1ull << 18, 1, stream); }

// The give-up word is read (and cleared) on a stream of the library's own, so that the call works while a closed wait holds `stream`.
static hipStream_t ack_stream()
{
    static std::mutex mu;
    static hipStream_t s[64] = {};
    int dev = 0;
    if (hipGetDevice(&dev) != hipSuccess || dev < 0 || dev >= 64) return nullptr;
    std::lock_guard<std::mutex> g(mu);
    if (!s[dev] && hipStreamCreateWithFlags(&s[dev], hipStreamNonBlocking) != hipSuccess) s[dev] = nullptr;
    return s[dev];
}

int cvxpnpl_stream_wait_gave_up(uint64_t *d_flag, int32_t clear, void *stream)
{
    if (!d_flag) return fail(-1, "cvxpnpl_stream_wait_gave_up: null flag");
    hipStream_t as = ack_stream();
    if (!as) return fail(-2, "cvxpnpl_stream_wait_gave_up: no stream for the acknowledgement");
    for (;;) {
        // (the state of `stream` is sampled BEFORE the word: when the stream was already idle no wait of it can set the word afterwards)
        const hipError_t q = hipStreamQuery((hipStream_t)stream);
        if (q != hipSuccess && q != hipErrorNotReady) return hip_error("cvxpnpl_stream_wait_gave_up (stream)", q);
        unsigned long long w = 0;
        hipError_t e = hipMemcpyAsync(&w, d_flag + 1, sizeof(w), hipMemcpyDeviceToHost, as);
        if (e == hipSuccess) e = hipStreamSynchronize(as);
        if (e == hipSuccess && w != 0 && clear) {
            e = hipMemsetAsync(d_flag + 1, 0, sizeof(w), as); // releases a closed wait that is holding `stream`
            if (e == hipSuccess) e = hipStreamSynchronize(as);
        }
        if (e != hipSuccess) return hip_error("cvxpnpl_stream_wait_gave_up", e);
        if (w != 0) return 1;
        if (q == hipSuccess) return 0; // everything the waits ordered is complete, and none gave up
        usleep(50);
    }
}

int cvxpnpl_pack_results(int64_t batch, const double *d_R, const double *d_t, const int32_t *d_status, double *d_packed, void *stream)
{
    if (batch < 0 || !d_R || !d_t || !d_status || !d_packed) return fail(-1, "cvxpnpl_pack_results: bad arguments");
    if (batch == 0) return 0;
    const int64_t n = batch * 13, grid = (n + 255) / 256;
    if (over_grid(grid, "cvxpnpl_pack_results: batch too large for one launch")) return -1;
    hipLaunchKernelGGL(pack_kernel, dim3((unsigned)grid), dim3(256), 0, (hipStream_t)stream, batch, d_R, d_t, d_status, d_packed);
    return launched("pack_kernel launch");
}

int cvxpnpl_select_best(int64_t n_hyp, const int32_t *d_count, const double *d_R, const double *d_t, const int32_t *d_status, const double *d_K,
                        int32_t n_corr, const double *d_pts_2d, const double *d_pts_3d, double thresh_px, double *d_out_R, double *d_out_t,
                        int32_t *d_head, uint8_t *d_mask, void *stream)
{
    if (n_hyp < 1 || n_hyp > 0x7fffffffLL || n_corr < 0 || !d_count || !d_R || !d_t || !d_status || !d_K || !d_out_R || !d_out_t || !d_head ||
        (n_corr > 0 && (!d_pts_2d || !d_pts_3d || !d_mask)) || !(thresh_px > 0.0))
        return fail(-1, "cvxpnpl_select_best: bad arguments");
    cvxs::SelectArgs a{n_hyp, d_count, d_R, d_t, d_status, d_K, n_corr, d_pts_2d, d_pts_3d, thresh_px, d_out_R, d_out_t, d_head, d_mask};
    hipLaunchKernelGGL(cvxs::select_best_kernel, dim3(1), dim3(cvxs::SELECT_BLOCK), 0, (hipStream_t)stream, a);
    return launched("select_best_kernel launch");
}

int cvxpnpl_refit_update(const double *d_fit_R, const double *d_fit_t, const int32_t *d_fit_status, const int32_t *d_fit_count, const double *d_K,
                         int32_t n_corr, const double *d_pts_2d, const double *d_pts_3d, double thresh_px, double *d_R, double *d_t, int32_t *d_head,
                         uint8_t *d_mask, void *stream)
{
    if (n_corr < 0 || !d_fit_R || !d_fit_t || !d_fit_status || !d_fit_count || !d_K || !d_R || !d_t || !d_head ||
        (n_corr > 0 && (!d_pts_2d || !d_pts_3d || !d_mask)) || !(thresh_px > 0.0))
        return fail(-1, "cvxpnpl_refit_update: bad arguments");
    cvxs::RefitArgs a{d_fit_R, d_fit_t, d_fit_status, d_fit_count, d_K, n_corr, d_pts_2d, d_pts_3d, thresh_px, d_R, d_t, d_head, d_mask};
    hipLaunchKernelGGL(cvxs::refit_update_kernel, dim3(1), dim3(cvxs::SELECT_BLOCK), 0, (hipStream_t)stream, a);
    return launched("refit_update_kernel launch");
}

int cvxpnpl_score_hypotheses(int64_t n_hyp, const double *d_R, const double *d_t, const int32_t *d_status, uint32_t usable_mask,
                             const double *d_K, int32_t n_corr, const double *d_pts_2d, const double *d_pts_3d, double thresh_px,
                             int32_t *d_count, uint8_t *d_mask, void *stream)
{
    if (n_hyp < 0 || n_corr < 0 || !d_R || !d_t || !d_K || !d_count || (n_corr > 0 && (!d_pts_2d || !d_pts_3d)) || !(thresh_px > 0.0))
        return fail(-1, "cvxpnpl_score_hypotheses: bad arguments");
    if (n_hyp == 0) return 0;
    const int64_t grid = (n_hyp + cvxs::SCORE_BLOCK - 1) / cvxs::SCORE_BLOCK;
    if (over_grid(grid, "cvxpnpl_score_hypotheses: too many hypotheses for one launch")) return -1;
    cvxs::ScoreArgs a;
    a.n_hyp = n_hyp; a.R = d_R; a.t = d_t; a.status = d_status; a.usable_mask = usable_mask; a.K = d_K;
    a.n_corr = n_corr; a.p2 = d_pts_2d; a.p3 = d_pts_3d; a.thresh = thresh_px; a.count = d_count; a.mask = d_mask;
    hipLaunchKernelGGL(cvxs::score_kernel, dim3((unsigned)grid), dim3(cvxs::SCORE_BLOCK), 0, (hipStream_t)stream, a);
    return launched("score_kernel launch");
}

int cvxpnpl_sample_minimal_sets(int64_t n_hyp, int32_t n_corr, const double *d_scene_2d, const double *d_scene_3d, int32_t k, uint64_t seed,
                                int32_t *d_idx, double *d_pts_2d, double *d_pts_3d, void *stream)
{
    if (n_hyp == 0) return 0; /* a no-op, as the header says: the (empty) outputs may be NULL */
    if (n_hyp < 0 || k < 1 || k > cvxs::SAMPLE_KMAX || n_corr < k || !d_scene_2d || !d_scene_3d || !d_pts_2d || !d_pts_3d)
        return fail(-1, "cvxpnpl_sample_minimal_sets: bad arguments (n_hyp=%lld n_corr=%d k=%d)", (long long)n_hyp, n_corr, k);
    const int64_t grid = (n_hyp + 255) / 256;
    if (over_grid(grid, "cvxpnpl_sample_minimal_sets: too many hypotheses for one launch")) return -1;
    cvxs::SampleArgs a;
    a.n_hyp = n_hyp; a.n_corr = n_corr; a.k = k; a.seed = seed; a.s2 = d_scene_2d; a.s3 = d_scene_3d; a.idx = d_idx; a.p2 = d_pts_2d; a.p3 = d_pts_3d;
    hipLaunchKernelGGL(cvxs::sample_sets_kernel, dim3((unsigned)grid), dim3(256), 0, (hipStream_t)stream, a);
    return launched("sample_sets_kernel launch");
}

size_t cvxpnpl_workspace_bytes(int64_t max_batch) { return max_batch > 0 ? hybrid_ws_bytes(max_batch) : 0; }

int cvxpnpl_set_workspace(void *d_workspace, size_t bytes, void *stream)
{
    int dev = 0;
    if (hipGetDevice(&dev) != hipSuccess) return fail(-2, "cvxpnpl: hipGetDevice failed");
    std::lock_guard<std::mutex> launch_lock(launch_mutex(dev, stream)); // no solve of this stream is between its launches
    std::lock_guard<std::mutex> lock(g_ws_mutex);
    Workspace &w = g_ws[std::make_pair(dev, stream)];
    if (w.ptr && w.owned) { (void)hipStreamSynchronize((hipStream_t)stream); (void)hipFree(w.ptr); }
    w = Workspace();
    if (!d_workspace) return 0; // back to the library's own allocation
    const int64_t cap = hybrid_capacity(bytes);
    if (cap <= 0) { g_ws.erase(std::make_pair(dev, stream)); return fail(-1, "cvxpnpl_set_workspace: %zu bytes hold no problem (cvxpnpl_workspace_bytes)", bytes); }
    if (!init_workspace(d_workspace, cap, stream)) { g_ws.erase(std::make_pair(dev, stream)); return hip_error("cvxpnpl_set_workspace", hipGetLastError()); }
    w.ptr = d_workspace; w.bytes = bytes; w.cap = cap; w.parked_bytes = bytes - hybrid_queue_bytes(cap); w.owned = false;
    return 0;
}

int cvxpnpl_release_workspace(void *stream, int32_t all_streams)
{
    int dev = 0;
    if (hipGetDevice(&dev) != hipSuccess) return fail(-2, "cvxpnpl: hipGetDevice failed");
    std::vector<void *> streams;
    {
        std::lock_guard<std::mutex> lock(g_ws_mutex);
        for (auto &kv : g_ws)
            if (kv.first.first == dev && (all_streams || kv.first.second == stream)) streams.push_back(kv.first.second);
    }
    for (void *st : streams) { // lock order as in a solve: the stream's launch mutex, then the workspace table
        std::lock_guard<std::mutex> launch_lock(launch_mutex(dev, st));
        std::lock_guard<std::mutex> lock(g_ws_mutex);
        auto it = g_ws.find(std::make_pair(dev, st));
        if (it == g_ws.end()) continue;
        if (it->second.ptr && it->second.owned) { (void)hipStreamSynchronize((hipStream_t)st); (void)hipFree(it->second.ptr); }
        g_ws.erase(it);
    }
    return 0;
}

int cvxpnpl_ipm_batch(int64_t batch, const double *d_Qs55, int32_t variant, double *d_Z100, double *d_S100, double *d_gap, int32_t *d_iters, void *stream)
{
    if (batch < 0 || !d_Qs55 || !d_Z100 || !d_S100 || !d_gap || !d_iters || (variant != CVXPNPL_VARIANT_FULL && variant != CVXPNPL_VARIANT_RC) || (batch + 3) / 4 > cvxse::GRID_MAX)
        return fail(-1, "cvxpnpl_ipm_batch: bad arguments");
    if (batch == 0) return 0;
    cvxi::IpmQuadArgs ia;
    memset(&ia, 0, sizeof(ia));
    ia.batch = batch; ia.rho = 1.0; ia.rho_tail = 1.0;
    ia.qs_in = d_Qs55; ia.z_out = d_Z100; ia.s_out = d_S100; ia.gap_out = d_gap; ia.it_out = d_iters;
    launch_variant(variant, cvxi::ipm_quad_kernel<cvx::VAR_RC>, cvxi::ipm_quad_kernel<cvx::VAR_FULL>, (batch + 3) / 4, 64, (hipStream_t)stream, ia); // (CVXPNPL_VARIANT_* are cvx::VAR_*)
    return launched("ipm_quad_kernel launch");
}

int cvxpnpl_calibration_copy(const void *d_src, void *d_dst, int64_t nbytes, int32_t bytes_per_lane, void *stream)
{
    if (!d_src || !d_dst || nbytes <= 0 || (bytes_per_lane != 4 && bytes_per_lane != 8 && bytes_per_lane != 16) || nbytes % 16)
        return fail(-1, "cvxpnpl_calibration_copy: bad arguments");
    const dim3 grid(4096), block(256);
    if (bytes_per_lane == 4) hipLaunchKernelGGL(cvxd::calibration_copy_kernel<4>, grid, block, 0, (hipStream_t)stream, (const char *)d_src, (char *)d_dst, nbytes);
    if (bytes_per_lane == 8) hipLaunchKernelGGL(cvxd::calibration_copy_kernel<8>, grid, block, 0, (hipStream_t)stream, (const char *)d_src, (char *)d_dst, nbytes);
    if (bytes_per_lane == 16) hipLaunchKernelGGL(cvxd::calibration_copy_kernel<16>, grid, block, 0, (hipStream_t)stream, (const char *)d_src, (char *)d_dst, nbytes);
    return launched("calibration_copy_kernel launch");
}

void *cvxpnpl_event_create(void)
{
    hipEvent_t ev;
    if (hipEventCreate(&ev) != hipSuccess) return nullptr;
    return (void *)ev;
}
int cvxpnpl_event_record(void *event, void *stream)
{
    hipError_t e = hipEventRecord((hipEvent_t)event, (hipStream_t)stream);
    return e == hipSuccess ? 0 : hip_error("hipEventRecord", e);
}
int cvxpnpl_event_elapsed_ms(void *start, void *stop, float *ms)
{
    hipError_t e = hipEventSynchronize((hipEvent_t)stop);
    if (e != hipSuccess) return hip_error("hipEventSynchronize", e);
    e = hipEventElapsedTime(ms, (hipEvent_t)start, (hipEvent_t)stop);
    return e == hipSuccess ? 0 : hip_error("hipEventElapsedTime", e);
}
void cvxpnpl_event_destroy(void *event) { if (event) hipEventDestroy((hipEvent_t)event); }

const char *cvxpnpl_last_error(void) { return cvxse::err_buf(); }
const char *cvxpnpl_version(void) { return "cvxpnpl_amd 0.1.0 (gfx950)"; }
int cvxpnpl_device_count(void)
{
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess) return 0;
    return n;
}

} // extern "C"

#ifdef CVXW_PROFILE
// diagnostics build only (tools/phase_profile.py): read and reset the per-phase cycle counters
extern "C" int cvxpnpl_debug_phase_cycles(unsigned long long *out32, int reset)
{
    if (hipMemcpyFromSymbol(out32, HIP_SYMBOL(cvxw::g_phase_cycles), 32 * sizeof(unsigned long long)) != hipSuccess) return -1;
    if (reset) {
        unsigned long long z[32] = {0};
        if (hipMemcpyToSymbol(HIP_SYMBOL(cvxw::g_phase_cycles), z, sizeof(z)) != hipSuccess) return -1;
    }
    return 0;
}
#endif
