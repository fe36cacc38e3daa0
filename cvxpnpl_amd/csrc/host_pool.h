// host_pool.h -- the thread pool of the host entry points (plain C++17, no HIP): the items [0, n) in contiguous chunks, one thread per chunk.
#pragma once
#include <stdint.h>

#include <algorithm>
#include <thread>
#include <vector>

namespace cvxh {

// work(lo, hi) over [0, n).  n_threads <= 0: the hardware's concurrency; never more threads than items; one thread is the caller's own.
// An item belongs to one chunk whatever the thread count, so every item is computed by the same code on the same inputs.
template <class F>
void for_chunks(int64_t n, int32_t n_threads, F work)
{
    int nt = n_threads > 0 ? n_threads : (int)std::thread::hardware_concurrency();
    if (nt < 1) nt = 1;
    if ((int64_t)nt > n) nt = n > 0 ? (int)n : 1;
    if (nt == 1) { work((int64_t)0, n); return; }
    std::vector<std::thread> pool;
    const int64_t chunk = (n + nt - 1) / nt;
    for (int k = 0; k < nt; ++k) {
        const int64_t lo = k * chunk, hi = std::min<int64_t>(n, lo + chunk);
        if (lo < hi) pool.emplace_back(work, lo, hi);
    }
    for (auto &th : pool) th.join();
}

} // namespace cvxh
