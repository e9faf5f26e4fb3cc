// What the two walk kernels (walk_kernels.hip) share, and the steps of walk_composite_lds that stand on their own: the tuning
// values, the emission/absorption of a segment, the leader election, the row-cost and counter epilogue.  Every function is
// inlined into the kernel and keeps no per-lane state of its own.  A step is only here if the kernels' machine code stays
// what it was with it (scripts/kernel_isa_digest.py): the compiler's register allocation is sensitive to how a step is cut.
#pragma once

#include <hip/hip_runtime.h>

#include "device_types.hpp"
#include "kernels.hpp"
#include "walk_common.hpp"
#include "walk_plan.hpp"

namespace c5 {

// ------------------------------------------------------------------------------------------
// Tuning values, decided long ago; the measurements that decided them stay with them.
// ------------------------------------------------------------------------------------------
// Distinct cells staged per wavefront and step (more: direct loads), and wavefronts per SIMD of the register-staged kernel.
// Measured on the C3 frame at 8x8 tiles (7 distinct cells per step on average): 16 slots / 6 wavefronts per SIMD 0.663 ms;
// 32 slots 0.753 (LDS then caps the CU at 5 workgroups); 8 slots 0.735 (direct-load fallback too often); 7 wavefronts per
// SIMD (72 VGPRs, 14 spilled) 0.662.
constexpr int kStageSlots = 14;
constexpr int kWalkWaves = 6;
// Wavefronts per SIMD of the LDS-DMA kernel: 8 (62 VGPRs with the emission integrated at once).  Measured on the
// exit-record kernel (C3 frame / C3 at 4800x3600 / C2 ball, walk ms): 7 wavefronts with the emission deferred into the
// next step's load shadow 0.4942 / 1.671 / 0.0965; emission at once, 7 wavefronts 0.4954 / 1.678 / 0.0956; emission at
// once, 8 wavefronts 0.4786 / 1.618 / 0.0944; deferred, 8 wavefronts (64 VGPRs, 12 B of scratch) 0.4832 / 1.622 / 0.1043.
constexpr int kDmaWaves = 8;
constexpr unsigned kBuckets1 = 256;  // first leader table of the election (power of two)
// One staged cell in LDS, 16-byte units: the 8 of its ExitRecord + 1 pad.  144 bytes = 36 banks: sixteen consecutive
// slots start on sixteen different 4-bank columns (slots s and s + 16 share theirs), so the lanes of a 16-lane group
// read their cells without bank conflicts; a DMA pass (64 lanes, destinations lane-linear) stages seven whole slots,
// its pad lanes idle.  (A stride of 8 units would let a pass stage eight, at the price of two-way conflicts between
// slots of equal parity.)
constexpr int kSlotStride = 9;
constexpr int kDmaSlots = 64 / kSlotStride;  // whole slots per DMA pass

using V2 = double __attribute__((ext_vector_type(2)));  // 16 bytes as one SSA value (never an alloca)
__device__ __forceinline__ D2 as_d2(V2 v) { return D2{v.x, v.y}; }
using LdsInts = const __attribute__((address_space(3))) int*;

// flags a ray carries in the top bits of its segment count
constexpr unsigned kOverflowBit = 0x80000000u;  // the ray hit the step bound
constexpr unsigned kSkippedBit = 0x40000000u;   // the ray met an entry inside a stretch it had walked (next_entry)
constexpr unsigned kClippedBit = 0x20000000u;   // (SPLIT) the ray goes on beyond the job's slab

// a wavefront's part of the election's LDS: leader tables of kBuckets1 and 64 buckets + the cell id of every slot
constexpr int kElectInts = kBuckets1 + 128;
constexpr int kSlotIds = kBuckets1 + 64;  // where the slots' cell ids begin

// ------------------------------------------------------------------------------------------
// The emission/absorption of one segment.
// ------------------------------------------------------------------------------------------
// One step in the reference's own arithmetic (line.cpp:220-224):
//   C = Q - alpha * I;   I = (Q - C * exp(-alpha * dz)) / alpha
// with every product and sum rounded separately (no FMA contraction), so that the recurrence —
// including its cancellation noise for tiny alpha — follows the reference's to the last bits of exp.
// The final division is a multiplication by the per-cell reciprocal (<= 1 ulp apart, not amplified).
template <bool kSmallArg = false>
__device__ __forceinline__ double reference_emission_step(double I, double alpha_c, double q, double inv_alpha,
                                                          double dz) {
#pragma clang fp contract(off)
    const double C = q - alpha_c * I;
    const double arg = -alpha_c * dz;
    const double e = kSmallArg ? exp_small_nonpositive(arg) : exp_nonpositive(arg);
    return (q - C * e) * inv_alpha;
}

// ORDER 0: back to front, the reference's recurrence (NaN alpha propagates like there).  ORDER 1: front to back,
// I = sum_k T_k (Q/alpha)(1 - e^{-alpha dz}); T_{k+1} = T_k e^{-alpha dz}, skipped once T fell below the cut-off.
// aux: 1 / alpha (order 0) or Q / alpha (order 1), as the record has it.  short_exp: the argument lies in (-1/8, 0].
struct Light {
    double I, T;  // the integral so far; ORDER 1: the transmittance in front of the segment
};
template <int ORDER>
__device__ __forceinline__ Light emission_step(double I, double T, double t_cutoff, double alpha_c, double aux, double q, double dz,
                                               bool short_exp) {
    if (ORDER == 0) {
        if (alpha_c != 0.0)  // line.cpp:220-224
            I = short_exp ? reference_emission_step<true>(I, alpha_c, q, aux, dz) : reference_emission_step<false>(I, alpha_c, q, aux, dz);
    } else if (T >= t_cutoff) {
        const double ex = short_exp ? exp_small_nonpositive(-alpha_c * dz) : exp_nonpositive(-alpha_c * dz);
        I = fma(T * aux, 1.0 - ex, I);
        T *= ex;
    }
    return Light{I, T};
}

// the frame's counters are kept in kCounterShards copies; a wavefront adds to the copy of its index in the launch
__device__ __forceinline__ FrameCounters* counter_shard(FrameCounters* counters, unsigned wave_index) {
    return counters + (wave_index % kCounterShards);
}

// ------------------------------------------------------------------------------------------
// 1. lanes in the same cell -> one slot.  Returns the lane's slot; n_runs: the slots in use.
//
// Neighbouring rays drift out of phase, so equal ids are rarely ADJACENT along the lanes: the C3
// frame has 22-27 runs of equal ids per step but only 7-17 distinct cells (8 in a 16x4 tile).
// Elect one leader per distinct cell through a table of kBuckets1 buckets in LDS (7 cells share
// a bucket in one step of twelve at 256 buckets, in one of three at 64): every walking lane
// writes (id << 6 | lane) to bucket hash(id) — ids of this kernel have 25 bits — and reads the
// bucket's winner back: one LDS round trip tells it the winner's lane AND whether the winner
// is in the same cell.  All lanes of a cell hash alike, so they follow the winner together or
// stay unresolved together (bucket shared with another cell); the unresolved go through a
// second table with another hash, and whoever is left after that leads itself.
// ------------------------------------------------------------------------------------------
__device__ __forceinline__ int elect_slots(int* my_elect, bool need, unsigned long long needs, int nb, int lane, int& n_runs) {
    const unsigned unb = static_cast<unsigned>(nb);
    const unsigned h1 = (unb ^ (unb >> 8)) & (kBuckets1 - 1u);
    const int ticket = static_cast<int>((unb << 6) | static_cast<unsigned>(lane));
    if (need) my_elect[h1] = ticket;
    __builtin_amdgcn_wave_barrier();
    const int won = my_elect[h1];  // lanes without a ray read some old ticket: harmless, they match nothing
    __builtin_amdgcn_wave_barrier();
    int w = won & 63;
    const bool other = (won >> 6) != nb;
    const bool open = need && other;
    if ((__builtin_amdgcn_ballot_w64(other) & needs) != 0ull) {  // wave-uniform; about one step in twelve
        const unsigned t = unb >> 6;
        const unsigned h2 = (unb + t + (t << 2) + (unb >> 12)) & 63u;
        if (open) my_elect[kBuckets1 + h2] = ticket;
        __builtin_amdgcn_wave_barrier();
        const int won2 = my_elect[kBuckets1 + h2];
        __builtin_amdgcn_wave_barrier();
        if (open) w = ((won2 >> 6) == nb) ? (won2 & 63) : lane;
    }
    // (uicmp: the compare straight into a lane mask; ballot() of this bool went through a 0/1 register)
    const unsigned long long heads =
        __builtin_amdgcn_uicmp(static_cast<unsigned>(w), static_cast<unsigned>(lane), 32 /* eq */) & needs;
    n_runs = __builtin_popcountll(heads);
    // a leader's slot = leaders below it.  The leaders post their cell id for the loader lanes
    // (my_elect[kSlotIds + slot]; slots not in use keep an older, still valid id) while everybody
    // fetches its leader's slot.
    const int rank = static_cast<int>(__builtin_amdgcn_mbcnt_hi(
        static_cast<uint32_t>(heads >> 32), __builtin_amdgcn_mbcnt_lo(static_cast<uint32_t>(heads), 0u)));
    if (need && w == lane) my_elect[kSlotIds + rank] = nb;
    const int slot = __builtin_amdgcn_ds_bpermute(w << 2, rank);
    __builtin_amdgcn_wave_barrier();
    return slot;
}

// segments per image row (load balancing of row blocks across GPUs): reduce over the lanes of a wavefront that share a
// row (WW consecutive lanes), one atomic per row and wavefront.  l: the lane; lrow: its row
template <int TILE>
__device__ __forceinline__ void post_row_cost(const WalkParams& P, int l, int lrow, unsigned n_seg) {
    using TS = TileShape<TILE>;
    unsigned rs = n_seg;
#pragma unroll
    for (int d = TS::WW / 2; d >= 1; d >>= 1) rs += __shfl_xor(rs, d);
    if ((l % TS::WW) == 0 && rs && lrow < P.im.n_local_rows) atomicAdd(P.row_cost + lrow, rs);
}

// per-wavefront statistics -> one atomic each (lane 0 only)
__device__ __forceinline__ void count_overlap(const WalkParams& P, unsigned s_skip) {
    if (s_skip) {
        atomicAdd(&P.counters->overlap_rays, s_skip);
        atomicAdd(P.sticky + 2, s_skip);
    }
}
__device__ __forceinline__ void count_frame(const WalkParams& P, FrameCounters* fc, unsigned s_seg, unsigned s_step, unsigned s_cov, unsigned s_ent,
                                            unsigned s_sol, unsigned s_ovf) {
    if (s_seg) atomicAdd(&fc->seg_tiles, static_cast<unsigned long long>(s_seg) | (1ull << kCounterHighShift));
    if (s_step | s_cov) atomicAdd(&fc->steps_cov, static_cast<unsigned long long>(s_step) | (static_cast<unsigned long long>(s_cov) << kCounterHighShift));
    if (s_ent | s_sol) atomicAdd(&fc->ent_solid, static_cast<unsigned long long>(s_ent) | (static_cast<unsigned long long>(s_sol) << kCounterHighShift));
    if (s_ovf) {  // (shard 0, beside entry_overflow: the two words a frame's status is read from; rare, never contended)
        atomicAdd(&P.counters->walk_overflow, s_ovf);
        atomicAdd(P.sticky + 1, s_ovf);
    }
}

}  // namespace c5
