// host_pool.h — the host planners' shared runtime (the ILU analysis, the SpMV
// planner; host_pool.cpp): memory for their large arrays, then their threads
// (Task, the parallel loops over a persistent worker pool), env_int and the
// plan digests' Fnv. Nothing here knows about either planner.
//
// The analysis builds a few hundred MB of host arrays per pattern (levels,
// plans, the downloaded pattern and symbolic data) and frees them when it
// returns. With glibc's defaults every array of >= 32 MiB (and most of the
// smaller ones) is a fresh anonymous mapping, so each analysis pays one page
// fault + zeroing per 4 KiB on first touch. Measured on the MI355X box
// (config 3, 21 matrices, 3rd of 3 reps): 490 ms as is, 317 ms with
// GLIBC_TUNABLES=glibc.malloc.hugetlb=1, 290 ms with freed memory kept in the
// heap (mmap/trim thresholds raised) — the library cannot set either for its
// caller's process, so it keeps its own blocks:
//
//   * blocks of >= kPoolMin bytes come from a process-wide cache of 2-MiB
//     aligned blocks (transparent huge pages requested with madvise: one
//     fault per 2 MiB when a block is first touched) and go back to it when
//     freed, so the next array of that size class is already mapped;
//   * the cache keeps at most RSP_HOST_POOL_MB (default 1024) of free blocks;
//     beyond that a freed block is returned to the system;
//   * smaller blocks use the global operator new.
//
// Thread-safe (one mutex: the analysis allocates from its worker threads).
#ifndef RSP_HOST_POOL_H
#define RSP_HOST_POOL_H

#include <stddef.h>
#include <stdint.h>
#include <stdlib.h>
#include <string.h>

#include <algorithm>
#include <exception>
#include <functional>
#include <new>
#include <thread>
#include <type_traits>
#include <utility>
#include <vector>

namespace rsp_an {

inline int env_int(const char *name, int dflt) {
    const char *v = getenv(name);
    return (v && *v) ? atoi(v) : dflt;
}

void *pool_get(size_t bytes);            // >= kPoolMin bytes; throws std::bad_alloc
void pool_put(void *p, size_t bytes);    // bytes as given to pool_get
constexpr size_t kPoolMin = 1u << 20;

template <typename T>
struct PoolAlloc {
    using value_type = T;
    PoolAlloc() noexcept = default;
    template <typename U>
    PoolAlloc(const PoolAlloc<U> &) noexcept {}
    // elements added by resize() / a size constructor are value-initialised
    // (zeroed), unless resize_uninit (below) is on the stack of this thread
    template <typename U, typename... A>
    void construct(U *p, A &&...a) {
        ::new ((void *)p) U(static_cast<A &&>(a)...);
    }
    template <typename U>
    void construct(U *p) {
        if (uninit_scope())
            ::new ((void *)p) U;
        else
            ::new ((void *)p) U();
    }
    static bool &uninit_scope() {
        static thread_local bool on = false;
        return on;
    }
    T *allocate(size_t n) {
        const size_t b = n * sizeof(T);
        if (b >= kPoolMin) return static_cast<T *>(pool_get(b));
        return static_cast<T *>(::operator new(b));
    }
    void deallocate(T *p, size_t n) noexcept {
        const size_t b = n * sizeof(T);
        if (b >= kPoolMin)
            pool_put(p, b);
        else
            ::operator delete(p);
    }
    template <typename U>
    bool operator==(const PoolAlloc<U> &) const noexcept { return true; }
    template <typename U>
    bool operator!=(const PoolAlloc<U> &) const noexcept { return false; }
};

// the analysis' vectors
template <typename T>
using hvec = std::vector<T, PoolAlloc<T>>;

// v.resize(n) without zeroing the new elements (trivial T only): for arrays
// that a transfer or a loop overwrites whole right after (round 6: zeroing
// the downloaded pattern, update pointers and stages cost ~3 x 4 B per
// stored entry of serial memset per analysis)
template <typename T>
void resize_uninit(hvec<T> &v, size_t n) {
    static_assert(std::is_trivially_default_constructible<T>::value, "trivial types only");
    bool &on = PoolAlloc<T>::uninit_scope();
    on = true;
    try {
        v.resize(n);
    } catch (...) {
        on = false;
        throw;
    }
    on = false;
}

// A helper thread of the analysis whose exception (std::bad_alloc from the
// pool, say) is carried to join(), which rethrows it in the caller; the
// destructor joins too, so a caller that unwinds first never leaves it
// running over the caller's locals (nor calls std::terminate).
class Task {
    std::exception_ptr err_;
    std::thread t_;

  public:
    template <typename F>
    explicit Task(F f) : t_([this, f] {
          try {
              f();
          } catch (...) {
              err_ = std::current_exception();
          }
      }) {}
    Task(const Task &) = delete;
    Task &operator=(const Task &) = delete;
    void join() {
        if (t_.joinable()) t_.join();
        if (err_) std::rethrow_exception(std::exchange(err_, nullptr));
    }
    ~Task() {
        if (t_.joinable()) t_.join();
    }
};

// Host worker threads for the analysis: OMP_NUM_THREADS (the box's share of
// its cores; the machine may have many more) or the hardware count, <= 64.
int host_threads();

// body(b) for b in [0, nb) on up to `team` threads of the worker pool (the
// caller included); a block's exception is rethrown in the caller once every
// block has finished.
void pool_run(int nb, int team, const std::function<void(int)> &body);

// f(r0, r1) over contiguous row blocks of [0, n) on host_threads() threads.
template <typename F>
void parallel_rows(int n, F f) {
    const int nt = n < 8192 ? 1 : host_threads();
    if (nt == 1) {
        f(0, n);
        return;
    }
    pool_run(nt, nt, [&](int t) { f((int)((long long)n * t / nt), (int)((long long)n * (t + 1) / nt)); });
}

// f(lo, hi) over [0, n) in at most host_threads() contiguous blocks of at
// least `grain`.
template <typename F>
void pfor(long long n, long long grain, F f) {
    const int nt = (int)std::max<long long>(1, std::min<long long>(host_threads(), n / std::max(grain, 1LL)));
    if (nt <= 1) {
        if (n > 0) f(0LL, n);
        return;
    }
    pool_run(nt, nt, [&](int t) { f(n * t / nt, n * (t + 1) / nt); });
}

// pfor behind a non-template entry point (ilu_blocks, spmv_plan, api_ilu_analysis)
void parallel_for(long long n, long long grain, const std::function<void(long long, long long)> &f);

// f(j) for j in [0, n), items handed out dynamically (uneven item costs:
// levels, segments, chunks); `work` estimates the total cost to size the team.
// Items are claimed in runs of about n / (64 team) (one claim per item made
// the many tiny levels of a deep DAG — 13 k on matrix-new_3 — cost ~1 ms
// per loop in claims alone; round 5).
template <typename F>
void pfor_dyn(int n, long long work, long long grain, F f) {
    const int nt = (int)std::max<long long>(1, std::min<long long>({(long long)host_threads(), (long long)n,
                                                                     work / std::max(grain, 1LL)}));
    if (nt <= 1) {
        for (int j = 0; j < n; j++) f(j);
        return;
    }
    const int run = std::max(1, n / (64 * nt));
    pool_run((n + run - 1) / run, nt, [&](int b) {
        for (int j = b * run, e = std::min(n, j + run); j < e; j++) f(j);
    });
}

// FNV-1a over 8-byte words (bytes for the tail): the plan digests
// (rsp_an::digest, rsp_plan::digest)
struct Fnv {
    uint64_t h = 1469598103934665603ULL;
    void bytes(const void *p, size_t n) {
        const unsigned char *c = (const unsigned char *)p;
        size_t i = 0;
        for (; i + 8 <= n; i += 8) {
            uint64_t w;
            memcpy(&w, c + i, 8);
            h = (h ^ w) * 1099511628211ULL;
        }
        for (; i < n; i++) h = (h ^ c[i]) * 1099511628211ULL;
    }
    template <typename V>
    void vec(const hvec<V> &v) {
        const uint64_t n = v.size();
        bytes(&n, sizeof(n));
        if (!v.empty()) bytes(v.data(), v.size() * sizeof(V));
    }
};

}  // namespace rsp_an

#endif
