// The diagnostic builds of walk_composite_lds (walk_kernels.hip), kept out of the kernel's text: the kernel declares one
// WalkClock and calls its hooks; in the product's build every hook is empty and the clock holds nothing.
//
//   -DC5_WALK_STAMPS=1  the in-kernel phase clock (scripts/stamp_walk.py) and the launch timeline (scripts/walk_timeline.py,
//                       share_timeline.py).  ONE WAVEFRONT IN 67 (every XCD in turn) sums, per phase of a step, the shader
//                       cycles between stamps (s_memtime; tick = shader cycle) and lane 0 adds them to g_walk_stamps; the
//                       other 66 run the product's instruction stream, so that the sampled wavefronts see the memory
//                       system, the LDS and the issue ports as loaded as the product's do.  (Stamping every wavefront —
//                       the round-2 build — made a step five times slower: 28 wavefronts per CU queueing for s_memtime five
//                       times per step, and 14 same-address atomics per wavefront at the end of the launch.)
//   -DC5_WALK_STAMPS=2  the coherence statistics on top (expensive).
//   -DC5_ISA_MARKERS=1  scripts/walk_isa.py: the phase boundaries as comments in the assembly of the PRODUCT's kernel (an
//                       empty asm statement: no instruction; the script checks that the loop's instruction count is the
//                       product's).
#pragma once

#include <hip/hip_runtime.h>

#ifndef C5_WALK_STAMPS
#define C5_WALK_STAMPS 0
#endif

namespace c5 {

#if C5_WALK_STAMPS
#define C5_STAMP(clock, k) (clock).stamp(k)

__device__ unsigned long long g_walk_stamps[16];
// launch timeline: per workgroup {start, end} in s_memrealtime ticks (100 MHz, one clock for the whole chip) and
// {XCC_ID | HW_ID << 8, wavefront-steps}; zero = the workgroup had no ray (scripts/walk_timeline.py)
constexpr unsigned kTraceBlocks = 131072u;
__device__ unsigned long long g_walk_trace[4 * kTraceBlocks];

struct WalkClock {
    bool on;  // wave-uniform: this wavefront is one of the sampled
    unsigned long long trace_begin, t_prev, t_begin;
    unsigned long long acc[8] = {0, 0, 0, 0, 0, 0, 0, 0};
    unsigned runs = 0, distinct = 0, iters = 0, lanes = 0;
#if C5_WALK_STAMPS > 1
    unsigned next_staged = 0, next_total = 0;
    int nb_before = -1;
#endif

    __device__ __forceinline__ void begin() {
        on = (blockIdx.x % 67u) == 5u;  // a stride that visits every XCD (blockIdx & 7) in turn
        trace_begin = __builtin_amdgcn_s_memrealtime();
        t_prev = __builtin_amdgcn_s_memtime();
        t_begin = t_prev;
    }
    __device__ __forceinline__ void stamp(int k) {
        if (on) {
            const unsigned long long t_now = __builtin_amdgcn_s_memtime();
            acc[k] += t_now - t_prev;
            t_prev = t_now;
        }
    }
    __device__ __forceinline__ void settle() {  // what a phase has in flight is charged to it
        if (on) asm volatile("s_waitcnt vmcnt(0) lgkmcnt(0)" ::: "memory");
    }
    // behind the election: steps and lane-steps; build 2: runs of equal ids against distinct ids among the walking lanes
    __device__ __forceinline__ void elected(unsigned long long needs, int nb, int lane, int n_runs) {
        iters += 1u;
        lanes += static_cast<unsigned>(__popcll(needs));
#if C5_WALK_STAMPS > 1
        unsigned long long seen = 0ull;  // lanes whose id already occurred in a lower lane
        for (int l = 0; l < 64; ++l) {
            const int v = __builtin_amdgcn_readlane(nb, l);
            if (v < 0) continue;
            seen |= __builtin_amdgcn_ballot_w64(nb == v && lane > l);
        }
        runs += static_cast<unsigned>(n_runs);
        distinct += static_cast<unsigned>(__popcll(needs & ~seen));
#endif
    }
    __device__ __forceinline__ void parked() {  // loads landed, pieces parked in LDS
        settle();
        stamp(3);
    }
    __device__ __forceinline__ void leaving(int nb) {  // (by the lanes that stepped) the cell the step was taken in
#if C5_WALK_STAMPS > 1
        nb_before = nb;
#endif
    }
    // record read back, geometry, exit face, (re-entry); build 2: how often is a ray's NEXT cell one this step already
    // staged (some lane's current cell)?
    __device__ __forceinline__ void stepped(bool need, int nb) {
#if C5_WALK_STAMPS > 1
        if (on) {
            bool hit = false;
            for (int l = 0; l < 64; ++l) {
                const int v = __builtin_amdgcn_readlane(nb_before, l);
                if (v >= 0 && need && nb == v) hit = true;
            }
            next_staged += static_cast<unsigned>(__popcll(__builtin_amdgcn_ballot_w64(hit)));
            next_total += static_cast<unsigned>(__popcll(__builtin_amdgcn_ballot_w64(need && nb >= 0)));
        }
#endif
        settle();
        stamp(4);
    }
    __device__ __forceinline__ void end(int lane) {
        if (lane == 0 && blockIdx.x < kTraceBlocks) {
            unsigned xcc, hw;
            asm volatile("s_getreg_b32 %0, hwreg(HW_REG_XCC_ID)" : "=s"(xcc));
            asm volatile("s_getreg_b32 %0, hwreg(HW_REG_HW_ID)" : "=s"(hw));
            unsigned long long* t = g_walk_trace + 4ull * blockIdx.x;
            t[0] = trace_begin;
            t[1] = __builtin_amdgcn_s_memrealtime();
            t[2] = (static_cast<unsigned long long>(hw) << 8) | (xcc & 0xffu);
            t[3] = iters;
        }
        if (lane == 0 && on) {
            for (int k = 0; k < 5; ++k) atomicAdd(&g_walk_stamps[k], acc[k]);
            atomicAdd(&g_walk_stamps[8], __builtin_amdgcn_s_memtime() - t_begin);  // whole loop
            atomicAdd(&g_walk_stamps[9], 1ull);                                    // wavefronts
            atomicAdd(&g_walk_stamps[10], static_cast<unsigned long long>(runs));
            atomicAdd(&g_walk_stamps[11], static_cast<unsigned long long>(distinct));
#if C5_WALK_STAMPS > 1
            atomicAdd(&g_walk_stamps[14], static_cast<unsigned long long>(next_staged));
            atomicAdd(&g_walk_stamps[15], static_cast<unsigned long long>(next_total));
#endif
            atomicAdd(&g_walk_stamps[12], static_cast<unsigned long long>(iters));
            atomicAdd(&g_walk_stamps[13], static_cast<unsigned long long>(lanes));
        }
    }
};

// read by the scripts through the library's symbol table (definitions: this header is walk_kernels.hip's alone)
extern "C" int c5_debug_walk_trace(unsigned long long* out, int n_blocks, int reset) {
    if (n_blocks > static_cast<int>(kTraceBlocks)) n_blocks = static_cast<int>(kTraceBlocks);
    if (hipMemcpyFromSymbol(out, HIP_SYMBOL(g_walk_trace), 32ull * n_blocks) != hipSuccess) return 1;
    if (reset) {
        void* p = nullptr;
        if (hipGetSymbolAddress(&p, HIP_SYMBOL(g_walk_trace)) != hipSuccess) return 1;
        if (hipMemset(p, 0, sizeof(unsigned long long) * 4 * kTraceBlocks) != hipSuccess) return 1;
    }
    return 0;
}
extern "C" int c5_debug_walk_stamps(unsigned long long* out16, int reset) {
    if (hipMemcpyFromSymbol(out16, HIP_SYMBOL(g_walk_stamps), 16 * sizeof(unsigned long long)) != hipSuccess) return 1;
    if (reset) {
        unsigned long long z[16] = {};
        if (hipMemcpyToSymbol(HIP_SYMBOL(g_walk_stamps), z, sizeof(z)) != hipSuccess) return 1;
    }
    return 0;
}
#else  // the product, and the marked build
#if defined(C5_ISA_MARKERS)
#define C5_STAMP(clock, k) asm volatile("; C5_PHASE_END " #k)
#else
#define C5_STAMP(clock, k) \
    do {                   \
    } while (0)
#endif

struct WalkClock {
    __device__ __forceinline__ void begin() {}
    __device__ __forceinline__ void elected(unsigned long long, int, int, int) {}
    __device__ __forceinline__ void parked() { C5_STAMP(*this, 3); }
    __device__ __forceinline__ void leaving(int) {}
    __device__ __forceinline__ void stepped(bool, int) { C5_STAMP(*this, 4); }
    __device__ __forceinline__ void end(int) {}
};
#endif

}  // namespace c5
