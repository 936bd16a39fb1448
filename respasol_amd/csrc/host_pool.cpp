// host_pool.cpp — the host planners' shared runtime (host_pool.h): the block
// cache behind PoolAlloc and the worker pool behind the parallel loops.

#include "host_pool.h"

#include <stdlib.h>
#include <sys/mman.h>

#include <atomic>
#include <condition_variable>
#include <deque>
#include <map>
#include <memory>
#include <mutex>
#include <unordered_map>

namespace rsp_an {

// Block cache behind PoolAlloc (host_pool.h).
namespace {
constexpr size_t kHugePage = 2u << 20;
struct BlockCache {
    std::mutex m;
    std::multimap<size_t, void *> free_blocks;    // size -> block
    std::unordered_map<void *, size_t> live;      // block -> size
    size_t cached = 0;
    size_t cap = (size_t)std::max(0, env_int("RSP_HOST_POOL_MB", 1024)) << 20;
};
BlockCache &block_cache() {
    static BlockCache *c = new BlockCache();  // never destroyed: blocks may be freed during exit
    return *c;
}
}  // namespace

void *pool_get(size_t bytes) {
    const size_t r = (bytes + kHugePage - 1) & ~(kHugePage - 1);
    BlockCache &c = block_cache();
    {
        std::lock_guard<std::mutex> g(c.m);
        auto it = c.free_blocks.lower_bound(r);
        if (it != c.free_blocks.end() && it->first <= r + r / 4 + kHugePage) {  // best fit, little slack
            void *p = it->second;
            const size_t s = it->first;
            c.free_blocks.erase(it);
            c.cached -= s;
            c.live[p] = s;
            return p;
        }
    }
    void *p = nullptr;
    if (posix_memalign(&p, kHugePage, r) != 0 || !p) throw std::bad_alloc();
    (void)madvise(p, r, MADV_HUGEPAGE);  // a hint: without THP the block is just a block
    std::lock_guard<std::mutex> g(c.m);
    c.live[p] = r;
    return p;
}

void pool_put(void *p, size_t) {
    if (!p) return;
    BlockCache &c = block_cache();
    {
        std::lock_guard<std::mutex> g(c.m);
        auto it = c.live.find(p);
        if (it == c.live.end()) return;  // not ours (cannot happen through PoolAlloc)
        const size_t s = it->second;
        c.live.erase(it);
        if (c.cached + s <= c.cap) {
            c.free_blocks.emplace(s, p);
            c.cached += s;
            return;
        }
    }
    free(p);
}

// Host worker threads for the analysis: OMP_NUM_THREADS (the box's share of
// its cores; the machine may have many more) or the hardware count, <= 64.
int host_threads() {
    int t = env_int("OMP_NUM_THREADS", 0);
    if (t <= 0) t = (int)std::thread::hardware_concurrency();
    return std::max(1, std::min(t, 64));
}

// Persistent worker threads for the parallel loops below. A loop used to
// spawn and join its team each time (~0.2-0.5 ms per loop at 16 threads, and
// an analysis runs ~35 loops: tens of ms on a small matrix). A loop is a job
// of `nb` blocks claimed through an atomic counter; the calling thread works
// on its own job too, so a job always finishes even when every worker is busy
// (nested or concurrent loops: the plans of L, L^T and the factor run at the
// same time). Block boundaries are the same as before, so are the plans.
// Workers are created on first use (as many as host_threads() - 1 asks for,
// growing if a later call asks for more), detached, and live as long as the
// process.
class Pool {
    struct Job {
        std::function<void(int)> body;
        int nb = 0;
        std::atomic<int> next{0}, done{0};
        std::mutex m;
        std::condition_variable cv;
        std::exception_ptr err;  // the first exception of a block (rethrown by run)
        void work() {
            for (int b; (b = next.fetch_add(1, std::memory_order_relaxed)) < nb;) {
                try {
                    body(b);
                } catch (...) {
                    std::lock_guard<std::mutex> g(m);
                    if (!err) err = std::current_exception();
                }
                if (done.fetch_add(1, std::memory_order_acq_rel) + 1 == nb) {
                    std::lock_guard<std::mutex> g(m);
                    cv.notify_all();
                }
            }
        }
    };
    std::mutex m_;
    std::condition_variable cv_;
    std::deque<std::shared_ptr<Job>> q_;
    int workers_ = 0;

    void worker() {
        for (;;) {
            std::shared_ptr<Job> j;
            {
                std::unique_lock<std::mutex> g(m_);
                cv_.wait(g, [&] { return !q_.empty(); });
                j = std::move(q_.front());
                q_.pop_front();
            }
            j->work();
        }
    }

  public:
    static Pool &get() {
        static Pool *p = new Pool();  // never destroyed: its threads outlive static destructors
        return *p;
    }
    // body(b) for b in [0, nb) on up to `team` threads (the caller included)
    void run(int nb, int team, const std::function<void(int)> &body) {
        if (nb <= 0) return;
        team = std::max(1, std::min(team, nb));
        if (team == 1) {
            for (int b = 0; b < nb; b++) body(b);
            return;
        }
        auto j = std::make_shared<Job>();
        j->body = body;
        j->nb = nb;
        {
            std::lock_guard<std::mutex> g(m_);
            for (; workers_ < team - 1; workers_++) std::thread([this] { worker(); }).detach();
            for (int t = 1; t < team; t++) q_.push_back(j);
        }
        if (team == 2)
            cv_.notify_one();
        else
            cv_.notify_all();
        j->work();
        std::unique_lock<std::mutex> g(j->m);
        j->cv.wait(g, [&] { return j->done.load(std::memory_order_acquire) == nb; });
        // every block has finished (no worker still runs body over the
        // caller's locals): a block's exception is the caller's now
        if (j->err) std::rethrow_exception(j->err);
    }
};

void pool_run(int nb, int team, const std::function<void(int)> &body) { Pool::get().run(nb, team, body); }

void parallel_for(long long n, long long grain, const std::function<void(long long, long long)> &f) {
    pfor(n, grain, [&](long long a, long long b) { f(a, b); });
}

}  // namespace rsp_an
