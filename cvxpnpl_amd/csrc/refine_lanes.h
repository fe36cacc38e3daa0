// refine_lanes.h -- how a problem's correspondences are spread over the lanes of the device, for refine_core.h's each / sum<N> / any
// interface: GroupLanes<RPL> (16 lanes per problem, four problems per wavefront) and BlockLanes (one workgroup of 256 per problem).  Shared
// by the refinement's kernels (refine_kernel.h) and those of its backward pass (refine_vjp_kernel.h).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "refine_core.h"

namespace cvxr {

constexpr int TPB = 256;
constexpr int WAVES = TPB / 64;

template <int RPL>
struct GroupLanes {
    Prob pb;
    int lane;
    Rec rec[RPL > 0 ? RPL : 1];
    __device__ __forceinline__ void load()
    {
        if (RPL > 0) CVX_UNROLL for (int j = 0; j < RPL; ++j) {
            rec_load(pb, lane + 16 * j, rec[j]);
            __builtin_amdgcn_sched_barrier(0);
        }
    }
    template <class F>
    __device__ __forceinline__ void each(F f)
    {
        if (RPL > 0) {
            CVX_UNROLL for (int j = 0; j < RPL; ++j) {
                f(rec[j]);
                __builtin_amdgcn_sched_barrier(0); // one record at a time: interleaved, their temporaries do not fit the register file
            }
        } else {
            const int n = pb.n_p + pb.n_l;
            for (int k = lane; k < n; k += 16) {
                Rec r;
                rec_load(pb, k, r);
                f(r);
            }
        }
    }
    template <int N>
    __device__ __forceinline__ void sum(double *v)
    {
        CVX_UNROLL for (int i = 0; i < N; ++i) {
            double x = v[i];
            x += __shfl_xor(x, 8, 16);
            x += __shfl_xor(x, 4, 16);
            x += __shfl_xor(x, 2, 16);
            x += __shfl_xor(x, 1, 16);
            v[i] = x;
            if ((i & 7) == 7) __builtin_amdgcn_sched_barrier(0); // (eight chains in flight hide the exchange latency; all N at once spill)
        }
    }
    __device__ __forceinline__ bool any(bool p) { return __any(p) != 0; }
};

struct BlockLanes {
    Prob pb;
    double *red; // LDS [WAVES + 1][ACC_N]: the wavefronts' partial sums, then the totals
    template <class F>
    __device__ __forceinline__ void each(F f)
    {
        const int n = pb.n_p + pb.n_l;
        for (int64_t k = threadIdx.x; k < n; k += TPB) { // (int64: k + TPB may pass 2^31)
            Rec r;
            rec_load(pb, (int)k, r);
            f(r);
        }
    }
    template <int N>
    __device__ __forceinline__ void sum(double *v)
    {
        const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
        CVX_UNROLL for (int i = 0; i < N; ++i) {
            double x = v[i];
            CVX_UNROLL for (int m = 32; m >= 1; m >>= 1) x += __shfl_xor(x, m, 64);
            v[i] = x;
            if ((i & 7) == 7) __builtin_amdgcn_sched_barrier(0); // (eight butterflies in flight hide the exchange latency; all N at once spill)
        }
        if (lane == 0) CVX_UNROLL for (int i = 0; i < N; ++i) red[wave * ACC_N + i] = v[i]; // (ONE guarded block: a guard per element costs registers)
        __syncthreads();
        if (threadIdx.x < N) { // lane i adds the wavefronts' partials of sum i, in a fixed order
            double x = red[threadIdx.x];
            CVX_UNROLL for (int w = 1; w < WAVES; ++w) x += red[w * ACC_N + threadIdx.x];
            red[WAVES * ACC_N + threadIdx.x] = x;
        }
        __syncthreads();
        CVX_UNROLL for (int i = 0; i < N; ++i) v[i] = red[WAVES * ACC_N + i]; // every lane: the same totals
        __syncthreads();
    }
    // (every lane of the workgroup holds the same state; the vote tells the compiler that the loop's exit is uniform -- taken as a per-lane
    // exit, every value that lives past the loop is kept twice)
    __device__ __forceinline__ bool any(bool p) { return __any(p) != 0; }
};

} // namespace cvxr
