// TEST INFRASTRUCTURE: a hazard zoo for the simulator's schedules (STORM_SIM_WAVES x STORM_SIM_DMA, hip_host_shim.h).
// Toy kernels written with the project's own primitives (raw_barrier, dma16, vm_wait, wave_sync), each as a correct twin and
// a BROKEN twin that differs by one barrier or one wait.  tests/test_sim_schedules.py asserts that every correct twin is exact
// under every schedule and pins the schedules under which each broken twin goes wrong: the proof that a schedule detects what
// it claims to.  Compiled only into libstorm_sim.so (tests/sim/build_sim.py); never part of the product library, and a broken
// twin never runs on a GPU.
//
// Every kernel is one workgroup of two waves.  A wave_sync stands for the yield points a real kernel has inside a phase (its
// MFMAs and shuffles): under the default sweep every wave advances one yield point per turn, so two of them between a read and
// the write that races with it keep the default schedule from ever seeing the race.
#include <string>
#include "common.h"

namespace storm {
constexpr int ZOO_THREADS = 128;

__device__ inline void zoo_clear(int words) {            // LDS is thread-local storage on the host: a run must not see the last one's data
    extern __shared__ __attribute__((aligned(16))) char smem[];
    int* const lds = reinterpret_cast<int*>(smem);
    for (int i = (int)threadIdx.x; i < words; i += ZOO_THREADS) lds[i] = 0;
    raw_barrier();
}

// Read after write: wave `producer` writes 64 words, the other wave reads them (mirrored, so no lane reads its own slot of
// the row) after `work` yield points of its own.  BROKEN: no barrier between the write and the read.
__global__ void zoo_raw(const int* src, unsigned* out, int producer, int work, int broken) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    int* const lds = reinterpret_cast<int*>(smem);
    const int wave = (int)threadIdx.x >> 6, lane = (int)threadIdx.x & 63;
    zoo_clear(64);
    if (wave == producer) lds[lane] = src[lane];
    else for (int i = 0; i < work; ++i) wave_sync();
    if (!broken) raw_barrier();
    if (wave != producer) out[lane] = (unsigned)lds[63 - lane];
}

// Write after read across a phase: a two-slot ring, one barrier per tile.  Tile t + 1 is written into the slot tile t - 1 was
// read from; the barrier of tile t is what says every wave has finished that read.  BROKEN: the refill is issued one barrier
// early, so a wave that is a whole phase behind (still reading tile t - 1) sees tile t + 1.
__global__ void zoo_war_ring(const int* src, unsigned* out, int ntiles, int broken) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    int* const ring = reinterpret_cast<int*>(smem);
    const int tid = (int)threadIdx.x;
    zoo_clear(2 * ZOO_THREADS);
    ring[tid] = src[tid];
    unsigned acc = 0;
    for (int t = 0; t < ntiles; ++t) {
        int* const next = ring + ((t + 1) & 1) * ZOO_THREADS;
        if (broken && t + 1 < ntiles) next[tid] = src[(t + 1) * ZOO_THREADS + tid];
        raw_barrier();
        if (!broken && t + 1 < ntiles) next[tid] = src[(t + 1) * ZOO_THREADS + tid];
        const int* const cur = ring + (t & 1) * ZOO_THREADS;
        acc = acc * 31u + (unsigned)cur[(tid + 64) & 127] + (unsigned)cur[tid];      // the other wave's word and this lane's own
        wave_sync();
        wave_sync();
    }
    out[tid] = acc;
}

// The same ring filled by LDS-DMA (16 B per lane).  BROKEN: the refill is issued before the barrier instead of after it.  A copy
// that lands at once overwrites what a lagging wave still reads; a copy that lands late hides the mistake.
__global__ void zoo_dma_war(const int* src, unsigned* out, int ntiles, int broken) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    const int tid = (int)threadIdx.x, wave = tid >> 6, lane = tid & 63;
    constexpr int SLOT = ZOO_THREADS * 16;
    zoo_clear(2 * SLOT / 4);
    const u32x4 srd = make_srd(src, (uint32_t)(ntiles * SLOT));
    auto issue = [&](int t) { dma16(srd, (uint32_t)(t * SLOT + tid * 16), 0u, smem + (t & 1) * SLOT + wave * 1024, lane); };
    issue(0);
    unsigned acc = 0;
    for (int t = 0; t < ntiles; ++t) {
        vm_wait<0>();
        if (broken && t + 1 < ntiles) issue(t + 1);
        raw_barrier();
        if (!broken && t + 1 < ntiles) issue(t + 1);
        const int* const cur = reinterpret_cast<const int*>(smem + (t & 1) * SLOT);
        for (int e = 0; e < 4; ++e) acc = acc * 31u + (unsigned)cur[((tid + 64) & 127) * 4 + e];
        wave_sync();
    }
    out[tid] = acc;
}

// Fragment before wait: each tile is copied, waited for, published by the barrier and read.  BROKEN: the wait stands after the
// read.  Only a copy that lands as late as it may shows it.
__global__ void zoo_dma_raw(const int* src, unsigned* out, int ntiles, int broken) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    const int tid = (int)threadIdx.x, wave = tid >> 6, lane = tid & 63;
    constexpr int SLOT = ZOO_THREADS * 16;
    zoo_clear(2 * SLOT / 4);
    const u32x4 srd = make_srd(src, (uint32_t)(ntiles * SLOT));
    unsigned acc = 0;
    for (int t = 0; t < ntiles; ++t) {
        dma16(srd, (uint32_t)(t * SLOT + tid * 16), 0u, smem + (t & 1) * SLOT + wave * 1024, lane);
        if (!broken) vm_wait<0>();
        raw_barrier();
        const int* const cur = reinterpret_cast<const int*>(smem + (t & 1) * SLOT);
        for (int e = 0; e < 4; ++e) acc = acc * 31u + (unsigned)cur[((tid + 64) & 127) * 4 + e];
        wave_sync();
        if (broken) vm_wait<0>();
    }
    out[tid] = acc;
}
}  // namespace storm

// Test-only entry point.  src: ntiles tiles (raw_*: 64 words; war_ring: 128 words a tile; dma_*: 512 words a tile); out: 128 words
// (raw_*: the first 64).  Returns 0, or -1 for an unknown kernel name.
extern "C" int storm_sim_zoo(const char* kernel, int broken, const int* src, int ntiles, unsigned* out) {
    using namespace storm;
    const dim3 grid(1), block(ZOO_THREADS);
    const std::string k(kernel);
    if (k == "raw_below") hipLaunchKernelGGL(zoo_raw, grid, block, 256, nullptr, src, out, 0, 0, broken);
    else if (k == "raw_below_busy") hipLaunchKernelGGL(zoo_raw, grid, block, 256, nullptr, src, out, 0, 2, broken);
    else if (k == "raw_above_busy") hipLaunchKernelGGL(zoo_raw, grid, block, 256, nullptr, src, out, 1, 2, broken);
    else if (k == "war_ring") hipLaunchKernelGGL(zoo_war_ring, grid, block, 1024, nullptr, src, out, ntiles, broken);
    else if (k == "dma_war") hipLaunchKernelGGL(zoo_dma_war, grid, block, 4096, nullptr, src, out, ntiles, broken);
    else if (k == "dma_raw") hipLaunchKernelGGL(zoo_dma_raw, grid, block, 4096, nullptr, src, out, ntiles, broken);
    else return -1;
    return 0;
}
