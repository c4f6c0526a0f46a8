// TEST INFRASTRUCTURE: fiber runtime behind tests/sim/hip_host_shim.h (see there).
#include <ucontext.h>
#include <atomic>
#include <thread>
#include <vector>
#include "hip_host_shim.h"

namespace storm { thread_local __attribute__((aligned(16))) char smem[160 * 1024]; }

namespace simrt {
namespace {
enum { RUN = 0, WAIT_BLOCK = 1, WAIT_WAVE = 2, DONE = 3 };
constexpr size_t STACK = 96 * 1024;
struct Fiber { ucontext_t ctx; int state; Idx tid; };
struct Wave { int arrived, ndone, nlanes; const void* in[64]; alignas(16) char out[64][64]; };
struct Block {
    dim3 grid, block; Idx bid; int nthreads, cur, n_done, n_barrier;
    std::vector<Fiber> f; std::vector<Wave> waves; ucontext_t sched;
    const std::function<void()>* body;
};
thread_local Block* g_blk = nullptr;
thread_local std::vector<char> g_stacks;

void fiber_main() {
    Block& B = *g_blk;
    (*B.body)();
    Fiber& me = B.f[B.cur];
    me.state = DONE;
    B.n_done++;
    B.waves[B.cur / 64].ndone++;
    swapcontext(&me.ctx, &B.sched);
}

// ---- wave schedules (STORM_SIM_WAVES, documented in hip_host_shim.h) ----------------------------------------------------
enum { ASCENDING = 0, REVERSE, FIRST, LAST, SEEDED };
struct Sched { int mode; uint64_t seed; };
const Sched& sched() {                                   // read once per loaded library, like STORM_SIM_DMA
    static const Sched v = [] {
        const char* e = getenv("STORM_SIM_WAVES");
        if (!e || !e[0]) return Sched{ASCENDING, 0};
        if (!strcmp(e, "reverse")) return Sched{REVERSE, 0};
        if (!strcmp(e, "first")) return Sched{FIRST, 0};
        if (!strcmp(e, "last")) return Sched{LAST, 0};
        if (!strncmp(e, "seed:", 5) && e[5]) { char* end; const uint64_t n = strtoull(e + 5, &end, 10); if (!*end) return Sched{SEEDED, n}; }
        fprintf(stderr, "simrt: STORM_SIM_WAVES=%s is none of reverse / first / last / seed:<n>\n", e);
        abort();
    }();
    return v;
}
inline uint64_t mix(uint64_t x) {                        // splitmix64's finaliser: the counter-based generator of the seeded schedule
    x += 0x9e3779b97f4a7c15ull; x = (x ^ (x >> 30)) * 0xbf58476d1ce4e5b9ull; x = (x ^ (x >> 27)) * 0x94d049bb133111ebull;
    return x ^ (x >> 31);
}
// lowest runnable lane of a wave, or -1 (lanes keep ascending order in every schedule)
inline int runnable(const Block& B, int w) {
    const int end = std::min(B.nthreads, 64 * w + 64);
    for (int i = 64 * w; i < end; ++i) if (B.f[i].state == RUN) return i;
    return -1;
}
inline bool release_barrier(Block& B) {
    if (B.n_barrier == 0 || B.n_barrier != B.nthreads - B.n_done) return false;
    for (auto& f : B.f) if (f.state == WAIT_BLOCK) f.state = RUN;
    B.n_barrier = 0;
    return true;
}
// The schedules other than the ascending sweep.  All state is in B and on this stack: workgroups run on several OS threads.
void run_skewed(Block& B, const Sched& sc, int nw) {
    const uint64_t blk = B.bid.x + (uint64_t)B.grid.x * (B.bid.y + (uint64_t)B.grid.y * B.bid.z);
    uint64_t step = 0;
    while (B.n_done < B.nthreads) {
        bool progressed = false;
        if (sc.mode == REVERSE) {                        // the sweep with waves in descending order
            for (int w = nw - 1; w >= 0; --w)
                for (int i = 64 * w, end = std::min(B.nthreads, 64 * w + 64); i < end; ++i) {
                    if (B.f[i].state != RUN) continue;
                    B.cur = i;
                    swapcontext(&B.sched, &B.f[i].ctx);
                    progressed = true;
                }
        } else {                                         // one fiber of the chosen wave, then choose again
            int pick = -1;
            if (sc.mode == FIRST) { for (int w = 0; w < nw && pick < 0; ++w) pick = runnable(B, w); }
            else if (sc.mode == LAST) { for (int w = nw - 1; w >= 0 && pick < 0; --w) pick = runnable(B, w); }
            else {
                int cand[16], nc = 0;                    // (a workgroup has at most 1024 threads)
                for (int w = 0; w < nw; ++w) { const int i = runnable(B, w); if (i >= 0) cand[nc++] = i; }
                if (nc) pick = cand[mix(mix(sc.seed ^ mix(blk)) + step++) % (uint64_t)nc];
            }
            if (pick >= 0) {
                B.cur = pick;
                swapcontext(&B.sched, &B.f[pick].ctx);
                continue;
            }
        }
        if (release_barrier(B)) progressed = true;
        if (!progressed) { fprintf(stderr, "simrt: deadlock (divergent barrier / collective?)\n"); abort(); }
    }
}

void run_block(Block& B) {
    g_blk = &B;
    if (g_stacks.size() < STACK * (size_t)B.nthreads) g_stacks.resize(STACK * (size_t)B.nthreads);
    const unsigned bx = B.block.x, by = B.block.y;
    for (int i = 0; i < B.nthreads; ++i) {
        Fiber& f = B.f[i];
        f.state = RUN;
        f.tid = Idx{(unsigned)i % bx, ((unsigned)i / bx) % by, (unsigned)i / (bx * by)};
        getcontext(&f.ctx);
        f.ctx.uc_stack.ss_sp = g_stacks.data() + STACK * (size_t)i;
        f.ctx.uc_stack.ss_size = STACK;
        f.ctx.uc_link = nullptr;
        makecontext(&f.ctx, fiber_main, 0);
    }
    const int nw = (B.nthreads + 63) / 64;
    B.waves.assign(nw, Wave());
    for (int w = 0; w < nw; ++w) { B.waves[w].arrived = 0; B.waves[w].ndone = 0; B.waves[w].nlanes = std::min(64, B.nthreads - 64 * w); }
    B.n_done = 0; B.n_barrier = 0;
    const Sched sc = sched();
    if (sc.mode != ASCENDING) { run_skewed(B, sc, nw); g_blk = nullptr; return; }
    while (B.n_done < B.nthreads) {
        bool progressed = false;
        for (int i = 0; i < B.nthreads; ++i) {
            if (B.f[i].state != RUN) continue;
            B.cur = i;
            swapcontext(&B.sched, &B.f[i].ctx);
            progressed = true;
        }
        if (B.n_barrier > 0 && B.n_barrier == B.nthreads - B.n_done) {
            for (auto& f : B.f) if (f.state == WAIT_BLOCK) f.state = RUN;
            B.n_barrier = 0;
            progressed = true;
        }
        if (!progressed) { fprintf(stderr, "simrt: deadlock (divergent barrier / collective?)\n"); abort(); }
    }
    g_blk = nullptr;
}
}  // namespace

Idx thread_idx() { return g_blk->f[g_blk->cur].tid; }
Idx block_idx() { return g_blk->bid; }
dim3 block_dim() { return g_blk->block; }
dim3 grid_dim() { return g_blk->grid; }

void block_barrier() {
    Block& B = *g_blk;
    Fiber& me = B.f[B.cur];
    me.state = WAIT_BLOCK;
    B.n_barrier++;
    swapcontext(&me.ctx, &B.sched);
}

void wave_collective(const void* my_in, void* my_out, size_t out_bytes, CollFn fn, long long ctx) {
    Block& B = *g_blk;
    const int tid = B.cur, w = tid / 64, lane = tid % 64;
    Wave& W = B.waves[w];
    W.in[lane] = my_in;
    W.arrived++;
    const int active = W.nlanes - W.ndone;
    if (W.arrived == active) {
        if (active != W.nlanes) { fprintf(stderr, "simrt: wave collective with exited lanes\n"); abort(); }
        fn(W.in, W.out, W.nlanes, ctx);
        W.arrived = 0;
        for (int l = 0; l < W.nlanes; ++l) if (B.f[w * 64 + l].state == WAIT_WAVE) B.f[w * 64 + l].state = RUN;
    } else {
        Fiber& me = B.f[tid];
        me.state = WAIT_WAVE;
        swapcontext(&me.ctx, &B.sched);
    }
    memcpy(my_out, W.out[lane], out_bytes);
}

void launch(dim3 grid, dim3 block, size_t lds_bytes, const std::function<void()>& body) {
    if (lds_bytes > sizeof(storm::smem)) { fprintf(stderr, "simrt: LDS request %zu too large\n", lds_bytes); abort(); }
    const long long nblocks = (long long)grid.x * grid.y * grid.z;
    const int nthreads = (int)(block.x * block.y * block.z);
    unsigned hw = std::thread::hardware_concurrency();
    const int nworkers = (int)std::max(1LL, std::min<long long>(hw ? hw : 4, nblocks));
    std::atomic<long long> next(0);
    auto worker = [&]() {
        Block B;
        B.grid = grid; B.block = block; B.nthreads = nthreads; B.body = &body;
        B.f.resize(nthreads);
        for (;;) {
            const long long k = next.fetch_add(1);
            if (k >= nblocks) break;
            B.bid = Idx{(unsigned)(k % grid.x), (unsigned)((k / grid.x) % grid.y), (unsigned)(k / ((long long)grid.x * grid.y))};
            run_block(B);
        }
    };
    if (nworkers == 1) { worker(); return; }
    std::vector<std::thread> th;
    for (int i = 0; i < nworkers; ++i) th.emplace_back(worker);
    for (auto& t : th) t.join();
}
}  // namespace simrt
