// step_wg.hip -- the workgroup-specialised force (wg_force) and the kernels built on it: k_accel_wg and k_lm_step_wg, the
// dominant kernel of the massive-body path (one launch per integrator step for N > 512 targets; dispatch.cpp chooses).
// Compiled once per evaluation order of the point-mass term (pair_ns.h), -ffp-contract=off (parity is bit for bit).
//
// WHAT IT DOES. The acceleration of a body is the sum over all sources in the reference's order, so the adds of one body are one
// dependent chain (a dependent v_add_f64 issues every 8.4 cycles from one wave, v_rsq_f64 / v_rcp_f64 cost ~17 issue cycles, other
// f64 ops ~4.1-5: scripts/ubench/lat.hip). ONE wave of a workgroup, the chain wave, carries those chains for all the workgroup's
// bodies -- 3 * WB of its 64 lanes -- and reads the contributions from LDS; the pair waves (lane = source) compute them, 64 sources
// (a tile) at a time, and write them there as rows [3 * body + component][source].
//
// THE 16-BODY WORKGROUP (N > 2048 targets), twelve waves, wave k on SIMD k % 4, three per SIMD, <= 168 VGPRs each:
//   * SIMD 0: wave 0 the one-body pair wave (body 0), wave 4 the chain wave at raised issue priority, wave 8 the tail wave;
//     SIMDs 1-3: three pair waves each for the bodies 1-5, 6-10, 11-15 (wg_force, 16-body overload).
//   * Tiles go in PHASES: tiles 0 and 1 singly (the chain wave starts early), then three tiles per phase, one s_barrier per phase:
//     23 barriers for the 64 tiles of N = 4096. Of the three pair waves of a SIMD each takes ONE tile of the phase (its rank).
//   * The deal is 14 / 14 / 14 / 6 units (body, source tile) per phase: ranks 0 and 1 carry the five bodies of their SIMD, rank 2
//     (the third tile) four; the fifth bodies (5, 10, 15) against the third tile are one block of the tail wave on SIMD 0, beside
//     the one-body wave's three units (wg_pair_wave_deal, wg_tail_wave_phases, wg_pair_wave_solo).
//   * Six 25 KB LDS tile buffers, tile t in buffer t % 6: the pair waves write one phase while the chain wave sums the one before.
//     The THIRD tile of a phase is written one interval late by every one of its producers, out of registers, at the head of their
//     next block (orders 0, 4 and 5); the schedule and the buffer lifetimes are stated above phase_start.
//   * k_lm_step_wg: the tail wave loads the 2 L history values while the others work, receives the new acceleration through LDS
//     and does Cowell's velocity, the solout sample and the predictor.
// THE SMALL FORMS, for target counts that would leave CUs without a 16-body workgroup (wg_force, the other overload):
//   * 8 bodies, SIX waves (`DUO`; 1024 < targets <= 2048): four pair waves of two bodies, chain, tail; big tiles of two tiles per
//     barrier (big_start). The twelve-wave 8-body form, one body per pair wave, stays selectable (EPH_WG_BODIES=8).
//   * 4 bodies (<= 1024 targets): one body per pair wave, one barrier per tile, TWO chain waves on alternate tiles (wg_force_split).
//
// HISTORY AND EVIDENCE, by round, under profiles/: r02 / r03_step_kernel_evidence.md (the layout and its six retired rivals, the
// split form), r04 (what the barriers cost, LDS counters instead), r05 (the six-wave form), r07 (one barrier per 192 sources and the
// deal by source tile: 33.2 against 36.0 us per step at N = 4096), r08 (14 / 14 / 14 / 6: 31.3 against 33.3), r09 (the late third
// tile: 29.9 against 31.3), step_wg_refactor.md (this file's present shape, same device code). Variants that were measured and
// rejected are patches under scripts/experiments/ (README.md there); a measured negative result that guards one line stands beside
// that line.
#include <algorithm>
#include <type_traits>
#include <utility>

#include "pair_ns.h"

#ifndef EPH_EXPERIMENTS
#define EPH_EXPERIMENTS 0
#endif
// tuning builds only (scripts/build_exp.sh NAME -DEPH_EXPERIMENTS=1 -DEPH_WG_SIDE=k): 1 = the chain wave skips its sums (pair side
// alone), 2 = the pair waves skip their tiles (chain side alone), 3 = the pair waves of SIMDs 1-3 skip theirs (SIMD 0 alone: its six
// units per phase and the chain); results are then meaningless. Compile-time on purpose: the same two tests as run-time flags cost
// the default path 3.6 us per step.
#if !EPH_EXPERIMENTS || !defined(EPH_WG_SIDE)
#undef EPH_WG_SIDE
#define EPH_WG_SIDE 0
#endif
// ablations for the same tuning builds (results meaningless): 1 = pair waves keep their contributions in registers (no ds_write),
// 2 = no barrier inside the tile loops -- what the floor model of profiles/r04_step_kernel_evidence.md is calibrated with
#if !EPH_EXPERIMENTS || !defined(EPH_WG_ABLATE)
#undef EPH_WG_ABLATE
#define EPH_WG_ABLATE 0
#endif
// the entry of k_lm_step_wg (profiles/step_entry.md). EPH_WG_ENTRY_ARGS: 1 = the hot scalars come from the leading, preloaded
// kernel arguments, 0 = from the by-value block behind them as before. EPH_WG_HIST_AT: where the tail wave of the 16-body form issues
// its history loads -- 0 at its entry, 1 behind its first tile loads, 2 behind barrier B_0.
#if !EPH_EXPERIMENTS || !defined(EPH_WG_ENTRY_ARGS)
#undef EPH_WG_ENTRY_ARGS
#define EPH_WG_ENTRY_ARGS 1
#endif
#if !EPH_EXPERIMENTS || !defined(EPH_WG_HIST_AT)
#undef EPH_WG_HIST_AT
#define EPH_WG_HIST_AT 1
#endif
#define WG_LOOP_BARRIER() do { if constexpr (!(EPH_WG_ABLATE & 2)) __syncthreads(); } while (0)

// The SIX-WAVE 8-body workgroup (round 5; `DUO` in the templates below, wb code 9 in the launcher): four pair waves x two bodies, a
// chain wave, a tail wave, 76 KB of LDS. Built to put TWO workgroups on a CU at N = 4096 so that one's barrier drain is covered by
// the other's arithmetic -- that lost badly (56.9 against 36.1 us: two chain waves and sixteen bodies of pair work share the four
// SIMDs with no say in the placement) -- but ONE such workgroup per CU beats the twelve-wave 8-body form (one body per pair wave: a
// bare dependent chain per wave) wherever that one was used: 1280 / 1536 / 1792 / 2048 bodies 13.2 / 14.8 / 16.3 / 17.7 against
// 14.0 / 15.6 / 17.1 / 18.6 us per step, bit-identical. dispatch.cpp takes it for 1024 < targets <= 2048.
// profiles/r05_step_kernel_evidence.md.

namespace eph {
namespace EPH_PV_NS {

constexpr int kWgBodies = 16;

// -DEPH_EXPERIMENTS=1 -DEPH_WG_STAMPS=1 (tuning build; the product carries none): lane 0 of every wave of workgroup 7 of k_lm_step_wg
// stores the shader clock (s_memtime) at 0 its entry, 1 its first tile data arrived (the wave waits for them there), 2 its arrival at
// barrier B_0, 3 behind B_0, 4 behind the tile loop, 5 behind the barrier that hands the acceleration over, 6 its end; the 16-body
// form only. eph_wg_stamps (order 0) copies the last launch's out: scripts/step_entry_stamps.py, profiles/step_entry.md.
#if !EPH_EXPERIMENTS || !defined(EPH_WG_STAMPS)
#undef EPH_WG_STAMPS
#define EPH_WG_STAMPS 0
#endif
#if EPH_WG_STAMPS
__device__ unsigned long long g_wg_stamps[12][8];
#define WG_STAMP(k) do { if (blockIdx.x == 7 && (threadIdx.x & 63) == 0) g_wg_stamps[threadIdx.x >> 6][k] = __builtin_amdgcn_s_memtime(); } while (0)
#define WG_STAMP_DATA(k) do { asm volatile("s_waitcnt vmcnt(0)" ::: "memory"); WG_STAMP(k); } while (0)
#else
#define WG_STAMP(k) do {} while (0)
#define WG_STAMP_DATA(k) do {} while (0)
#endif
constexpr int kDuoThreads = 64 * 6;                  // the duo form: waves 0-3 pair (two bodies each), 4 chain, 5 tail
constexpr int kDuoTailWave = 5;
constexpr int kWgChainWave = 4;                      // the chain wave (wave 4: lands on SIMD 0)
constexpr int kWgTailWave = 8;                       // the step kernel's tail wave (SIMD 0 too)
constexpr int kWgThreads = 64 * 12;
constexpr int kWgTileBufs = 6;                       // LDS tile buffers of the phase and big-tile schedules (tile t in buffer t % 6)
constexpr int kWgSplitBufs = 3;                      // ... of the barrier-per-64 schedule (4-body workgroups, two chain waves)

// a pair wave's own bodies: NB of them from body `first` on, BS apart (bodies beyond n are clamped copies of body n - 1). Wave-uniform,
// and the compiler keeps them in scalar registers; pinned into vector registers instead: 34.20-34.34 against 33.16-33.31 us per step
// at N = 4096, alternating on one box
template <int NB, int BS = 1, typename PosPtr>
__device__ __forceinline__ void wg_load_own(PosPtr pos, int n, int first, double (&xi)[NB], double (&yi)[NB], double (&zi)[NB]) {
#pragma unroll
    for (int b = 0; b < NB; ++b) {
        const int ii = min(first + BS * b, n - 1);
        xi[b] = pos[ii].x;
        yi[b] = pos[ii].y;
        zi[b] = pos[ii].z;
    }
}
// lane = source: the lane's body of source tile t (past the last tile: the last tile again; past body n - 1: that body)
template <typename PosPtr>
__device__ __forceinline__ Body4 load_src(PosPtr pos, int n, int tiles, int lane, int t) {
    const int j = min(t, tiles - 1) * kTile + lane;
    return pos[j < n ? j : n - 1];
}

// pair wave: NB bodies (local indices b0..) against the 64 sources in pj -> rows of `tile`
template <int NB>
__device__ __forceinline__ void wg_pair_tile(const double (&xi)[NB], const double (&yi)[NB], const double (&zi)[NB],
                                             const Body4 &pj, bool ieee, double *tile, int b0, int lane) {
    // (the workgroup's own tile goes to the IEEE form as a whole -- n2 = 0 on the self lanes fails the range test of the wave.
    // Giving those lanes a harmless in-range operand instead, since the chain wave discards what they produce, was measured twice:
    // no gain in round 2, 40.1 vs 40.0 us; SLOWER on the phase schedule, 35.19-35.30 against 33.53-33.64 us per step at N = 4096 --
    // the lane compares sit in front of every tile of every wave, the IEEE form in one phase of 23:
    // scripts/experiments/wg_diag_patch.patch)
    PairPre pre[NB];
    unsigned worst = ieee ? kRangeSpan : mu_key(pj.mu), low = ~0u;   // max of the range keys: one add + one max per body
#pragma unroll
    for (int b = 0; b < NB; ++b) {
        pre[b] = pair_pre(xi[b], yi[b], zi[b], pj);
        worst = max(worst, range_key(pre[b].n2));
        low = min(low, pre[b].lo);
    }
    worst = max(worst, low_key(low));
    double c[3 * NB];
    if (__builtin_amdgcn_ballot_w64(worst >= kRangeSpan) == 0) {
#pragma unroll
        for (int b = 0; b < NB; ++b) pair_finish<true>(pre[b], pj.mu, c[3 * b], c[3 * b + 1], c[3 * b + 2]);
    } else {   // the tile holding the workgroup's own bodies (n2 = 0 on the self lane) or an operand outside the guarded ranges
#pragma unroll
        for (int b = 0; b < NB; ++b) pair_finish<false>(pre[b], pj.mu, c[3 * b], c[3 * b + 1], c[3 * b + 2]);
    }
#pragma unroll
    for (int q = 0; q < 3 * NB; ++q) {
        if constexpr (EPH_WG_ABLATE & 1) asm volatile("" ::"v"(c[q]));
        else tile[(3 * b0 + q) * kRow + lane] = c[q];
    }
}

// Barrier-per-64-sources schedule (every wave executes tiles + 1 barriers): B_0 after tiles 0 and 1 are in LDS; iteration t:
// pair waves produce tile t + 2 into buffer (t + 2) % 3 while the chain waves sum tile t from buffer t % 3; barrier.
template <int NB, typename PosPtr>
__device__ __forceinline__ void wg_pair_wave(PosPtr pos, int n, int i0, int b0, double *C, int lane, int tiles, int tdiag, int wbuf) {
    double xi[NB], yi[NB], zi[NB];
    wg_load_own<NB>(pos, n, i0 + b0, xi, yi, zi);
    Body4 pj = load_src(pos, n, tiles, lane, 0);
    Body4 pjn = load_src(pos, n, tiles, lane, 1);
    wg_pair_tile<NB>(xi, yi, zi, pj, tdiag == 0, C, b0, lane);
    pj = pjn;
    pjn = load_src(pos, n, tiles, lane, 2);
    if (tiles > 1) wg_pair_tile<NB>(xi, yi, zi, pj, tdiag == 1, C + wbuf, b0, lane);
    __syncthreads();
    for (int t = 0; t < tiles; ++t) {
        if (t + 2 < tiles) {
            pj = pjn;
            pjn = load_src(pos, n, tiles, lane, t + 3);
            wg_pair_tile<NB>(xi, yi, zi, pj, tdiag == t + 2, C + ((t + 2) % kWgSplitBufs) * wbuf, b0, lane);
        }
        __syncthreads();
    }
}

// two 64-source tiles at once: 2 x NB independent interactions, written stage by stage (pair_finish_staged, pair_term.h)
template <int NB>
__device__ __forceinline__ void wg_pair_tile2(const double (&xi)[NB], const double (&yi)[NB], const double (&zi)[NB],
                                              const Body4 &pa, const Body4 &pb, bool ieee, double *tile_a, double *tile_b,
                                              int b0, int lane) {
    PairPre pre[2 * NB];
    unsigned worst = ieee ? kRangeSpan : max(mu_key(pa.mu), mu_key(pb.mu)), low = ~0u;
#pragma unroll
    for (int b = 0; b < NB; ++b) {
        pre[b] = pair_pre(xi[b], yi[b], zi[b], pa);
        pre[NB + b] = pair_pre(xi[b], yi[b], zi[b], pb);
        worst = max(worst, max(range_key(pre[b].n2), range_key(pre[NB + b].n2)));
        low = min(low, min(pre[b].lo, pre[NB + b].lo));
    }
    worst = max(worst, low_key(low));
    double c[6 * NB];
    if (__builtin_amdgcn_ballot_w64(worst >= kRangeSpan) == 0) {
        // (round 2 wrote the stages out WITHOUT pinning the order and the scheduler put them back: 37.38 vs 37.04 us)
        if constexpr (kPairStaged) {
            double mus[2 * NB];
#pragma unroll
            for (int b = 0; b < NB; ++b) { mus[b] = pa.mu; mus[NB + b] = pb.mu; }
            pair_finish_staged<2 * NB>(pre, mus, c);
        } else {
#pragma unroll
            for (int b = 0; b < NB; ++b) {
                pair_finish<true>(pre[b], pa.mu, c[3 * b], c[3 * b + 1], c[3 * b + 2]);
                pair_finish<true>(pre[NB + b], pb.mu, c[3 * (NB + b)], c[3 * (NB + b) + 1], c[3 * (NB + b) + 2]);
            }
        }
        // (writing each interaction's three values as soon as they exist, instead of the burst below, was measured too:
        // 36.9 vs 37.0 us, although SQ_LDS_DATA_FIFO_FULL is raised 13 % of the time -- profiles/r02_pmc2.json)
    } else {
#pragma unroll
        for (int b = 0; b < NB; ++b) {
            pair_finish<false>(pre[b], pa.mu, c[3 * b], c[3 * b + 1], c[3 * b + 2]);
            pair_finish<false>(pre[NB + b], pb.mu, c[3 * (NB + b)], c[3 * (NB + b) + 1], c[3 * (NB + b) + 2]);
        }
    }
#pragma unroll
    for (int q = 0; q < 3 * NB; ++q) {
        if constexpr (EPH_WG_ABLATE & 1) {
            asm volatile("" ::"v"(c[q]), "v"(c[3 * NB + q]));
        } else {
            tile_a[(3 * b0 + q) * kRow + lane] = c[q];
            tile_b[(3 * b0 + q) * kRow + lane] = c[3 * NB + q];
        }
    }
}

// Layout 3 barrier schedule (the 8-body workgroups; the 16-body one: phase_start below). The 64-source tiles are grouped into "big" tiles, one barrier each: big tiles 0 and 1 are
// single tiles (so the chain wave starts after two tiles, not four: its wait for the first barrier was 2.7 us of a
// 42 us launch), every later one is two tiles. Every wave executes TB + 1 barriers: B_0 after big tiles 0 and 1 are
// in LDS; iteration K: pair waves produce big tile K + 2 while the chain wave sums big tile K (and prefetches the head
// of K + 1, complete since the previous barrier); barrier. Tile t lives in LDS buffer t % 6; the tiles alive at any time
// span at most six consecutive indices.
// (Single tiles at the END as well -- the pair waves run two big tiles ahead, so the chain wave sums the last two alone --
// were measured: 37.6-37.7 vs 37.0 us at N = 4096, 18.6 vs 18.3 at 2048, 12.05 vs 11.9 at 1024. Not kept.)
__device__ __forceinline__ int big_start(int K) { return K < 2 ? K : 2 * K - 2; }
__device__ __forceinline__ int big_count(int tiles) { return tiles <= 2 ? tiles : 2 + (tiles - 2 + 1) / 2; }
// (Round 4 measured what the loop's barriers cost -- pair side alone 34.4 us, 33.4 without its LDS writes, 28.6 without the
// barriers either -- and replaced them by LDS counters: pair waves free-running up to two big tiles ahead, each adding 1 to a counter
// behind its ds_writes, the chain wave polling that counter and publishing how far it has consumed. Bit-identical and SLOWER: 37.9
// against 36.3 us at N = 4096, 19.6 against 18.6 at 2048 (39.1 with memory-model fences, which also wait for the prefetched global
// loads). The barrier keeps the write bursts of ten waves and the chain wave's reads in separate phases of the one LDS pipe.
// profiles/r04_step_kernel_evidence.md section 4; the patch: scripts/experiments/wg_counter_sync.patch.)
template <int NB, typename PosPtr>
__device__ __forceinline__ void wg_pair_wave_big(PosPtr pos, int n, int i0, int b0, double *C, int lane, int tiles, int tdiag, int wbuf) {
    double xi[NB], yi[NB], zi[NB];
    // (wg_load_own written out: through the helper the six-wave step kernels of order 4 come out with other registers)
#pragma unroll
    for (int b = 0; b < NB; ++b) {
        const int ii = min(i0 + b0 + b, n - 1);
        xi[b] = pos[ii].x;
        yi[b] = pos[ii].y;
        zi[b] = pos[ii].z;
    }
    // (Measured and NOT kept, rounds 3 and 4, each bit-identical: source rows addressed as uniform tile base + loop-invariant lane
    // offset -- ten VALU fewer per interval -- 36.7 against 36.2 us; two intervals per trip with the prefetched register sets
    // trading places instead of being copied 38.7; own bodies' positions through scalar loads 36.4; the first source tiles requested
    // before the own positions 36.3; nontemporal stores of the tail wave 36.1 (nothing): profiles/r04_step_kernel_evidence.md.)
    auto produce = [&](int K, const Body4 &pa, const Body4 &pb) {          // big tile K
        const int t = big_start(K);
        if (t >= tiles || EPH_WG_SIDE == 2) return;
        double *ta = C + (t % kWgTileBufs) * wbuf, *tb = C + ((t + 1) % kWgTileBufs) * wbuf;
        if (K >= 2 && t + 1 < tiles) wg_pair_tile2<NB>(xi, yi, zi, pa, pb, tdiag == t || tdiag == t + 1, ta, tb, b0, lane);
        else wg_pair_tile<NB>(xi, yi, zi, pa, tdiag == t, ta, b0, lane);
    };
    const int TB = big_count(tiles);
    Body4 pa = load_src(pos, n, tiles, lane, 0), pb = load_src(pos, n, tiles, lane, 1);
    Body4 na = load_src(pos, n, tiles, lane, 2), nb = load_src(pos, n, tiles, lane, 3);
    produce(0, pa, pa);
    produce(1, pb, pb);
    __syncthreads();
    for (int K = 0; K < TB; ++K) {
        pa = na; pb = nb;
        na = load_src(pos, n, tiles, lane, big_start(K + 3));
        nb = load_src(pos, n, tiles, lane, big_start(K + 3) + 1);
        produce(K + 2, pa, pb);
        WG_LOOP_BARRIER();
    }
}
// a wave with no tile work: TB + 1 barriers like everybody
__device__ __forceinline__ void wg_idle_wave(int tiles) {
    __syncthreads();
    for (int T = 0; T < big_count(tiles); ++T) WG_LOOP_BARRIER();
}

// ---- the 16-body workgroup: pair work dealt by SOURCE TILE, one barrier per 192 sources ------------------------------------------
// The same six tile buffers as two sets of three: phases 0 and 1 are the single tiles 0 and 1 (the chain wave starts as early as
// before), phase P >= 2 is the tiles 3 P - 4 .. 3 P - 2. Tile t lives in buffer t % 6, so even phases >= 2 own buffers {2, 3, 4}, odd
// ones {5, 0, 1}; the single tiles (buffers 0 and 1) have been summed two barriers before phase 3 writes there. The chain wave sums
// phase P while the pair waves work on phase P + 1. Rounds 7 and 8: every tile of a phase written before the phase's barrier,
// phase_count(tiles) barriers for every wave -- B_0 after tile 0 is in LDS, then one behind every phase but the last.
//
// Round 9, the LATE THIRD TILE. Call the tiles of a three-tile phase P a, b, c (c = phase_start(P) + 2; the single-tile phases and a
// last phase of one or two tiles have none). Every producer of c -- the rank-2 waves of SIMDs 1-3, the three-body block of wave 8,
// the third interaction of the one-body wave -- computes it in interval P as before (interval P: between barriers B_(P-1) and
// B_P), keeps the contributions in registers across B_P and issues the ds_writes inside its block of interval P + 1, where its own
// arithmetic covers their drain; a and b are written before B_P as before. The chain wave therefore sums, behind B_I, the tiles
// {c(I-1), a(I), b(I)}: still three consecutive tiles in source order with the same prefetch pattern, two tiles (a, b) behind B_2,
// and, when the LAST phase has a c, that tile alone behind one more barrier: interval_count(tiles) barriers for every wave.
// Buffer lifetimes, tile t in buffer t % 6 as before: c(P) is written in interval P + 1 and read in interval P + 2; the next user of
// its buffer is c(P + 2), written in interval P + 3. a(P) and b(P) are written in interval P and read in P + 1; their buffers are
// next written in P + 2 (a(P + 2), b(P + 2)). Tiles 0 and 1 are read in intervals 1 and 2, their buffers next written in
// intervals 3 (b(3)) and 4 (c(3)). No buffer is written while it is read -- with SIX buffers, and only because EVERY producer of c
// is late: the one-body wave writing c(P) early would overwrite c(P - 2) while the chain wave reads it. In the interval of the
// first c there is nothing held yet; the block then stores zeros to that c's own buffer, idle until the real values follow one
// interval later (the block stays free of a branch around the stores).
// (The same deferral for EVERY tile of a phase, all ten write bursts at the head of the next phase and the chain wave one phase
// further behind, was round 7: bit-identical and 1.4 us slower, 35.53-35.63 against 34.15-34.25. Different s_setprio levels for the
// three pair waves of a SIMD on top of the late third tile: three us slower, scripts/experiments/wg_rank_prio.patch.)
// Orders 0, 4 and 5 only: with the same schedule orders 1, 2, 3 and 6 LOSE about 2.2 us per step (35.36 / 35.36 / 39.76 / 38.64
// against 33.12 / 33.49 / 37.56 / 36.07 at N = 4096, the stores at the head in the generated code of all of them) and keep the
// schedule of round 8, third tiles written before their phase's barrier (profiles/r09_step_kernel_evidence.md section 6).
constexpr bool kWgLateThird = kPairVariant == 0 || kPairVariant == 4 || kPairVariant == 5;
static_assert(kWgTileBufs == 6, "the late third tile needs tile t + 6 to be written two intervals after tile t was read");
__device__ __forceinline__ int phase_start(int P) { return P < 2 ? P : 3 * P - 4; }
__device__ __forceinline__ int phase_count(int tiles) { return tiles <= 2 ? tiles : 2 + (tiles - 2 + 2) / 3; }
__device__ __forceinline__ int phase_tiles(int P, int tiles) { return P < 2 ? 1 : min(3, tiles - phase_start(P)); }
// barriers of the tile loop: one more than phases when the last phase has a third tile
__device__ __forceinline__ int interval_count(int tiles) { return phase_count(tiles) + (kWgLateThird && tiles >= 5 && (tiles - 2) % 3 == 0); }
// the tiles the chain wave sums behind barrier B_I: [chain_first(I), chain_first(I + 1)) cut at `tiles`
__device__ __forceinline__ int chain_first(int I) { return kWgLateThird ? (I <= 2 ? I : 3 * I - 5) : phase_start(I); }

// the staged term for M = MA + MB interactions in two runs (the division orders 4 and 6 carry six more doubles per interaction
// through the stages: five at once do not fit 168 VGPRs)
template <int MA, int MB>
__device__ __forceinline__ void pair_finish_staged_split(const PairPre (&pre)[MA + MB], const double (&mu)[MA + MB], double (&c)[3 * (MA + MB)]) {
    PairPre pa[MA], pb[MB];
    double ma[MA], mb[MB], ca[3 * MA], cb[3 * MB];
#pragma unroll
    for (int k = 0; k < MA; ++k) { pa[k] = pre[k]; ma[k] = mu[k]; }
#pragma unroll
    for (int k = 0; k < MB; ++k) { pb[k] = pre[MA + k]; mb[k] = mu[MA + k]; }
    pair_finish_staged<MA>(pa, ma, ca);
    pair_finish_staged<MB>(pb, mb, cb);
#pragma unroll
    for (int k = 0; k < 3 * MA; ++k) c[k] = ca[k];
#pragma unroll
    for (int k = 0; k < 3 * MB; ++k) c[3 * MA + k] = cb[k];
}

// the held rows of a third tile (wg_pair_block, LATE) -> their tile buffer: bodies b0, b0 + BS, ..., rows 3 * body + component
template <int NB, int BS>
__device__ __forceinline__ void wg_store_held(double *tile, int b0, int lane, const double (&held)[3 * NB]) {
#pragma unroll
    for (int q = 0; q < 3 * NB; ++q) {
        if constexpr (EPH_WG_ABLATE & 1) asm volatile("" ::"v"(held[q]));
        else tile[(3 * (b0 + BS * (q / 3)) + q % 3) * kRow + lane] = held[q];
    }
}

// NB bodies (local indices b0..) against NT 64-source tiles: NB * NT independent interactions behind ONE range test, the staged
// arithmetic (pair_finish_staged, pair_term.h), then the write burst. BS: the stride of the bodies (local indices b0, b0 + BS, ...;
// rows 3 * body + component).
// LATE (the late third tile, phase_start above): the contributions of the LAST tile are not written but left in `held`, and what
// `held` brought in -- the same rows of the third tile of the phase before -- is written to `held_tile` at the HEAD of the block,
// before the pre-stage: behind the barrier the LDS store path has nothing else to do (the chain wave opens its interval with reads),
// and a third of the producers is not the burst of all ten that round 7 put there. Measured at N = 4096, us per step, parent
// 31.14-31.26: at the head 29.79-29.98; behind the range test 33.30-33.45 (the compiler spreads the stores over the pre-stage);
// between two runs of the staged arithmetic 32.42-32.50; behind the arithmetic 31.67-31.86 (profiles/r09_step_kernel_evidence.md;
// the switch: scripts/experiments/wg_late_at.patch).
template <int NB, int NT, int BS = 1, bool LATE = false>
__device__ __forceinline__ void wg_pair_block(const double (&xi)[NB], const double (&yi)[NB], const double (&zi)[NB],
                                              const Body4 (&pj)[NT], bool ieee, double *const (&tile)[NT], int b0, int lane,
                                              double (&held)[3 * NB], double *held_tile) {
    constexpr int M = NB * NT;
    if constexpr (LATE) wg_store_held<NB, BS>(held_tile, b0, lane, held);
    PairPre pre[M];
    double mus[M];
    unsigned worst = ieee ? kRangeSpan : 0u, low = ~0u;
#pragma unroll
    for (int s = 0; s < NT; ++s) {
        worst = max(worst, mu_key(pj[s].mu));
#pragma unroll
        for (int b = 0; b < NB; ++b) {
            const int k = s * NB + b;
            pre[k] = pair_pre(xi[b], yi[b], zi[b], pj[s]);
            mus[k] = pj[s].mu;
            worst = max(worst, range_key(pre[k].n2));
            low = min(low, pre[k].lo);
        }
    }
    worst = max(worst, low_key(low));
    double c[3 * M];
    if (__builtin_amdgcn_ballot_w64(worst >= kRangeSpan) == 0) {
        if constexpr (kPairStaged && M == 5 && (kPairVariant == 4 || kPairVariant == 6)) {
            pair_finish_staged_split<3, 2>(pre, mus, c);
        } else if constexpr (kPairStaged) {
            pair_finish_staged<M>(pre, mus, c);
        } else {
#pragma unroll
            for (int k = 0; k < M; ++k) pair_finish<true>(pre[k], mus[k], c[3 * k], c[3 * k + 1], c[3 * k + 2]);
        }
    } else {   // the tile holding the workgroup's own bodies (n2 = 0 on the self lane) or an operand outside the guarded ranges
#pragma unroll
        for (int k = 0; k < M; ++k) pair_finish<false>(pre[k], mus[k], c[3 * k], c[3 * k + 1], c[3 * k + 2]);
    }
#pragma unroll
    for (int s = 0; s < NT - LATE; ++s) {
#pragma unroll
        for (int q = 0; q < 3 * NB; ++q) {
            if constexpr (EPH_WG_ABLATE & 1) asm volatile("" ::"v"(c[3 * NB * s + q]));
            else tile[s][(3 * (b0 + BS * (q / 3)) + q % 3) * kRow + lane] = c[3 * NB * s + q];
        }
    }
    if constexpr (LATE) {
#pragma unroll
        for (int q = 0; q < 3 * NB; ++q) held[q] = c[3 * NB * (NT - 1) + q];
    }
}
template <int NB, int NT, int BS = 1>
__device__ __forceinline__ void wg_pair_block(const double (&xi)[NB], const double (&yi)[NB], const double (&zi)[NB],
                                              const Body4 (&pj)[NT], bool ieee, double *const (&tile)[NT], int b0, int lane) {
    double none[3 * NB];
    wg_pair_block<NB, NT, BS, false>(xi, yi, zi, pj, ieee, tile, b0, lane, none, nullptr);
}

// A pair wave of SIMDs 1-3: the bodies b0.. of its SIMD group against ONE tile of every phase, the tile given by the wave's rank
// among the three waves of its SIMD -- one source tile loaded per wave and phase. In the single-tile phases rank 0 has the tile
// and the other two only meet the barrier. Round 8: 14 / 14 / 14 / 6 units (body, source tile) per three-tile phase instead of
// 15 / 15 / 15 / 3 -- ranks 0 and 1 carry the five bodies of the group (NB = 5), rank 2, which only ever has the THIRD tile of a
// three-tile phase, the first four (NB = 4); the fifth bodies of the three groups (local bodies 5, 10, 15) against that tile are ONE
// block of wave 8 on SIMD 0 (NB = 3, BS = 5, rank 2: the same loop), written to the rows the rank-2 waves would have written.
// `hook`: called once behind the wave's first tile loads -- the step kernel's tail wave issues its history loads there, so that they
// queue behind the loads everybody waits for at B_0 and not in front of them (EPH_WG_HIST_AT, tuning builds: 0 at the kernel's entry
// as before, 2 behind B_0; 32.9 / 33.4 / 32.8 us per step for 1 / 0 / 2 at one phase of the code, profiles/step_entry.md)
struct WgNoHook { __device__ __forceinline__ void operator()() const {} };
template <int NB, int BS = 1, typename PosPtr, typename Hook = WgNoHook>
__device__ __forceinline__ void wg_pair_wave_deal(PosPtr pos, int n, int i0, int b0, int rank, double *C, int lane, int tiles, int tdiag, int wbuf,
                                                  Hook &&hook = Hook{}) {
    double xi[NB], yi[NB], zi[NB];
    wg_load_own<NB, BS>(pos, n, i0 + b0, xi, yi, zi);
    auto tile_of = [&](int P) { return P < 2 ? (rank == 0 ? P : tiles) : phase_start(P) + rank; };   // >= tiles: none
    constexpr bool kOff = EPH_WG_SIDE == 2 || (EPH_WG_SIDE == 3 && BS == 1);
    const int NI = interval_count(tiles);
    [[maybe_unused]] const int NP = kWgLateThird ? phase_count(tiles) : NI;
    if constexpr (NB == 5 || !kWgLateThird) {   // ranks 0 and 1: tiles a and b, written before the phase's barrier
        auto produce = [&](int t, const Body4 &pj) {
            if (t >= tiles || kOff) return;
            const Body4 src[1] = {pj};
            double *const dst[1] = {C + (t % kWgTileBufs) * wbuf};
            wg_pair_block<NB, 1, BS>(xi, yi, zi, src, t == tdiag, dst, b0, lane);
        };
        Body4 pj = load_src(pos, n, tiles, lane, tile_of(0)), pjn = load_src(pos, n, tiles, lane, tile_of(1));
        if constexpr (EPH_WG_HIST_AT == 1) hook();
        WG_STAMP_DATA(1);
        produce(tile_of(0), pj);
        WG_STAMP(2);
        __syncthreads();
        WG_STAMP(3);
        if constexpr (EPH_WG_HIST_AT == 2) hook();
        for (int P = 1; P < NP; ++P) {
            pj = pjn;
            pjn = load_src(pos, n, tiles, lane, tile_of(P + 1));
            produce(tile_of(P), pj);
            WG_LOOP_BARRIER();
        }
        if (NI > NP) WG_LOOP_BARRIER();                 // the last phase's third tile is written behind the phase's barrier
    } else {                   // rank 2: tile c of every three-tile phase, computed in its interval and written in the next
        static_assert(NB < 5, "the late loop is the rank-2 waves' (four bodies) and wave 8's (three)");
        double held[3 * NB];
#pragma unroll
        for (int q = 0; q < 3 * NB; ++q) held[q] = 0.0;
        int tprev = tile_of(2);                         // nothing held in the interval of the first c: zeros to its own buffer
        Body4 pj, pjn = load_src(pos, n, tiles, lane, tile_of(2));
        if constexpr (EPH_WG_HIST_AT == 1) hook();
        WG_STAMP_DATA(1);
        WG_STAMP(2);
        __syncthreads();
        WG_STAMP(3);
        if constexpr (EPH_WG_HIST_AT == 2) hook();
        for (int I = 1; I < NI; ++I) {
            const int t = I < 2 ? tiles : tile_of(I);
            if (I >= 2) {
                pj = pjn;
                pjn = load_src(pos, n, tiles, lane, tile_of(I + 1));
            }
            double *const late = C + (tprev % kWgTileBufs) * wbuf;
            if (kOff) {
            } else if (t < tiles) {
                const Body4 src[1] = {pj};
                double *const dst[1] = {nullptr};       // the block's only tile is held
                wg_pair_block<NB, 1, BS, true>(xi, yi, zi, src, t == tdiag, dst, b0, lane, held, late);
                tprev = t;
            } else if (tprev < tiles && I > 2) {       // behind the last c: its writes alone
                wg_store_held<NB, BS>(late, b0, lane, held);
                tprev = tiles;
            }
            WG_LOOP_BARRIER();
        }
    }
}
// The one-body pair wave of the chain wave's SIMD: body 0 against every tile of the phase (three interactions at once)
template <typename PosPtr>
__device__ __forceinline__ void wg_pair_wave_solo(PosPtr pos, int n, int i0, double *C, int lane, int tiles, int tdiag, int wbuf) {
    double xi[1], yi[1], zi[1];
    wg_load_own<1>(pos, n, i0, xi, yi, zi);
    auto load_phase = [&](int P, Body4 (&s)[3]) {
        const int t = phase_start(P);
        s[0] = load_src(pos, n, tiles, lane, t);
        if (P >= 2) { s[1] = load_src(pos, n, tiles, lane, t + 1); s[2] = load_src(pos, n, tiles, lane, t + 2); }
    };
    const int NI = interval_count(tiles), NP = kWgLateThird ? phase_count(tiles) : NI;
    // the third interaction of a three-tile phase is held over the barrier like the rank-2 waves' tiles (phase_start above)
    double held[3] = {0.0, 0.0, 0.0};
    int tprev = tiles;                                  // the tile in `held` (tiles: none)
    auto write_held = [&]() {
        if (tprev >= tiles) return;
        double *const late = C + (tprev % kWgTileBufs) * wbuf;
        wg_store_held<1, 1>(late, 0, lane, held);
        tprev = tiles;
    };
    auto produce = [&](int P, const Body4 (&s)[3]) {
        if (EPH_WG_SIDE == 2) return;
        if (P >= NP) { write_held(); return; }
        const int t = phase_start(P), cnt = phase_tiles(P, tiles);
        if (cnt == 3) {
            double *const dst[3] = {C + (t % kWgTileBufs) * wbuf, C + ((t + 1) % kWgTileBufs) * wbuf,
                                    kWgLateThird ? nullptr : C + ((t + 2) % kWgTileBufs) * wbuf};
            // (the upper bound first: stated as one expression the two scalar compares and their s_and come out in another order
            // than in the code that was measured -- harmless, and no longer `same` for scripts/compare_kernels.py)
            const bool below = tdiag < t + 3, own = tdiag >= t && below;
            // (nothing held in the interval of the first c: zeros to its own buffer)
            double *const late = C + ((tprev < tiles ? tprev : t + 2) % kWgTileBufs) * wbuf;
            wg_pair_block<1, 3, 1, kWgLateThird>(xi, yi, zi, s, own, dst, 0, lane, held, late);
            if constexpr (kWgLateThird) tprev = t + 2;
        } else {   // the single tiles and a short last phase
            write_held();
            auto one = [&](int k, const Body4 &pj) {
                const Body4 src[1] = {pj};
                double *const dst[1] = {C + ((t + k) % kWgTileBufs) * wbuf};
                wg_pair_block<1, 1>(xi, yi, zi, src, tdiag == t + k, dst, 0, lane);
            };
            one(0, s[0]);
            if (cnt > 1) one(1, s[1]);
        }
    };
    Body4 s[3], sn[3];
    load_phase(0, s);
    load_phase(1, sn);
    WG_STAMP_DATA(1);
    produce(0, s);
    WG_STAMP(2);
    __syncthreads();
    WG_STAMP(3);
    for (int P = 1; P < NI; ++P) {                      // (P = NP, when the last phase has a third tile: its writes alone)
#pragma unroll
        for (int k = 0; k < 3; ++k) s[k] = sn[k];
        load_phase(P + 1, sn);
        produce(P, s);
        WG_LOOP_BARRIER();
    }
}

// chain over a full tile whose first two chunks are already in q[0], q[1], nothing prefetched behind it (the last tile of a phase:
// the next phase's buffers are being written until the barrier)
__device__ __forceinline__ double chain_full_q(const double *row, double2 (&q)[4][8], double acc) {
    load_chunk(row, 2, q[2]);
    acc = add_chunk(q[0], acc);
    load_chunk(row, 3, q[3]);
    acc = add_chunk(q[1], acc);
    acc = add_chunk(q[2], acc);
    return add_chunk(q[3], acc);
}
// chain over a full tile whose first two chunks are already in q[0], q[1]; leaves the first two chunks of the
// NEXT tile (row_next, complete since the previous barrier) in q[0], q[1]
__device__ __forceinline__ double chain_full_pf(const double *row, const double *row_next, double2 (&q)[4][8],
                                                double acc) {
    load_chunk(row, 2, q[2]);
    acc = add_chunk(q[0], acc);
    load_chunk(row, 3, q[3]);
    acc = add_chunk(q[1], acc);
    load_chunk(row_next, 0, q[0]);
    acc = add_chunk(q[2], acc);
    load_chunk(row_next, 1, q[1]);
    return add_chunk(q[3], acc);
}

// The 4-body workgroups (512 < N <= 1024 targets, where the step IS the chain wave's time) with TWO chain
// waves taking ALTERNATE tiles: while one adds the 64 sources of tile t out of its registers, the other reads tile t + 1
// into its own (a wave's ds_read_b128 and its dependent adds do not overlap; two waves' do), and the 3 * WB partial sums
// change hands through LDS at every tile's barrier. Same number of LDS reads as one chain wave (the split by LANE doubled
// them). One barrier per 64-source tile (three tile buffers), pair waves two tiles ahead.
// MEASURED (bit-identical; us per step, split | default): N = 640 9.29 | 9.83, 1024 11.74 | 12.01, 1536 16.10 | 15.37,
// 2048 19.58 | 18.34 -- a gain only where four bodies per workgroup leave the pair side idle anyway; with eight one-body
// pair waves a barrier per tile makes the pair side (one interaction per wave and tile: a bare dependent chain) the
// slower one. Producing the tiles in pairs in every other interval to get two interleaved interactions back: 10.4 / 13.0 /
// 18.7 / 23.0, worse still (the reader waits out the double intervals). Default: the 4-body workgroups only.
// (profiles/r03_step_kernel_evidence.md section 1b; the switch that applied it to the 8-body workgroups or to none:
// scripts/experiments/wg_tile_split_knob.patch)
constexpr bool wg_tile_split(int wb) { return wb == 4; }
constexpr int wg_split_wave_b(int wb) { return wb == 8 ? 11 : 6; }   // an idle wave of another SIMD than the chain wave's
// body of the one-body pair wave `wave` in the 8- / 4-body workgroups (-1: not a pair wave)
template <int WB>
__device__ __forceinline__ int wg_small_body(int wave) {
    if constexpr (WB == 8) {
        switch (wave) { case 1: return 0; case 2: return 1; case 3: return 2; case 5: return 3; case 6: return 4; case 7: return 5;
                        case 9: return 6; case 10: return 7; default: return -1; }
    } else {
        switch (wave) { case 1: return 0; case 2: return 1; case 3: return 2; case 5: return 3; default: return -1; }
    }
}
template <int WB, typename PosPtr>
__device__ __forceinline__ double wg_force_split(PosPtr pos, int n, int i0, double init, double *C, int tid) {
    constexpr int kRows = 3 * WB, kBuf = kRows * kRow;
    const int lane = tid & 63, wave = tid >> 6;
    const int tiles = (n + kTile - 1) / kTile;
    const int tdiag = i0 / kTile;
    double *H = C + kWgSplitBufs * kBuf;                // hand-over: H[lane] = running sum, H[64 + lane] = closed lower sum
    const int body = wg_small_body<WB>(wave);
    if (body >= 0) { wg_pair_wave<1>(pos, n, i0, body, C, lane, tiles, tdiag, kBuf); return 0.0; }
    const bool isA = wave == kWgChainWave, isB = wave == wg_split_wave_b(WB);
    if (!isA && !isB) { for (int t = 0; t <= tiles; ++t) __syncthreads(); return 0.0; }
    const int ch = lane < kRows ? lane : kRows - 1;
    const double *row = C + ch * kRow;
    const int gself = (i0 % kTile) / WB;
    const int li = (i0 % kTile) + ch / 3;
    double acc = init, accL = 0.0;
    double2 q[4][8];
    auto plain = [&](int t) { return t < tiles && t != tdiag && min(kTile, n - t * kTile) == kTile; };
    auto preload = [&](int t) {
        const double *r = row + (t % kWgSplitBufs) * kBuf;
        load_chunk(r, 0, q[0]); load_chunk(r, 1, q[1]); load_chunk(r, 2, q[2]); load_chunk(r, 3, q[3]);
    };
    __syncthreads();                                    // B_0: tiles 0 and 1 ready
    if (isA && plain(0)) preload(0);
    for (int t = 0; t < tiles; ++t) {
        const bool mine = ((t & 1) != 0) == isB;
        if (mine) {
            if (t > 0) { acc = H[lane]; accL = H[64 + lane]; }
            if (plain(t)) {
                acc = add_chunk(q[0], acc); acc = add_chunk(q[1], acc); acc = add_chunk(q[2], acc); acc = add_chunk(q[3], acc);
            } else {
                chain_masked<WB>(row + (t % kWgSplitBufs) * kBuf, min(kTile, n - t * kTile), t == tdiag ? gself : -1, li, acc, accL);
            }
            H[lane] = acc;
            H[64 + lane] = accL;
        } else if (plain(t + 1)) {
            preload(t + 1);                             // complete since the previous barrier
        }
        __syncthreads();
    }
    return isA ? H[64 + lane] + H[lane] : 0.0;
}

// wave 8 of the 16-body workgroup in the tile loop (the tail wave of k_lm_step_wg, between loading its history and the integrator's
// work; in k_accel_wg its only work): the fifth bodies of the three SIMD groups against the third tile of every three-tile phase,
// behind one range test and one ballot, through pair_finish_staged<3>. (The same six units per phase on SIMD 0 with the one-body
// wave carrying all of them and this wave only meeting the barriers -- two waves beside the chain's adds instead of three -- measured
// 31.41-31.56 against 31.18-31.36 us per step: scripts/experiments/wg_solo6.patch.)
constexpr int kWgShedFirst = 5, kWgShedStride = 5, kWgShedBodies = 3;
template <typename PosPtr, typename Hook = WgNoHook>
__device__ __forceinline__ void wg_tail_wave_phases(PosPtr pos, int n, int i0, double *C, int lane, int tiles, int tdiag, int wbuf,
                                                    Hook &&hook = Hook{}) {
    wg_pair_wave_deal<kWgShedBodies, kWgShedStride>(pos, n, i0, kWgShedFirst, 2, C, lane, tiles, tdiag, wbuf, hook);
}

// ---- wg_force<WB, DUO>: the force of a workgroup ------------------------------------------------------------------------------------
// Returns on chain-wave lane ch < 3 * WB: component ch % 3 of body i0 + ch / 3 (init + the reference-order sum over the other
// bodies). Every thread of the workgroup must call it. TWO functions of that name, one per design: the 16-body phase schedule and
// the big-tile / split schedules of the 8- and 4-body workgroups; they share the opening lines and nothing else. (Two overloads and
// not two functions behind a forwarding wg_force: through one more level of inlining the optimiser makes other code of the 8-body
// kernels -- 3168 instead of 3376 lines for k_accel_wg<8>, order 0 -- and nobody has measured that code:
// profiles/step_wg_refactor.md.) The chain wave's dependent adds issue ahead of the pair wave of its SIMD (s_setprio; the same
// library with and without, alternating on one box: 36.3 against 36.8 us per step at N = 4096 on two boxes of the pool, 36.2 either
// way on a third; nothing at the chain-bound sizes).

// The 16-body workgroup. Roles of the twelve waves (wave k runs on SIMD k % 4, so waves k and k + 4 share a SIMD whatever the start
// of the hardware's cyclic order): wave id = 1, 2, 3 (mod 4) are the pair waves of SIMD group id % 4 -- bodies 1-5, 6-10, 11-15 -- and
// take the tile of the phase given by their rank id >> 2 (rank 2: the first four bodies only); wave 0 is the one-body pair wave
// (body 0) beside the chain wave (4) and the tail wave (8: bodies 5, 10, 15 against the third tile). TWO copies of the pair loop of
// SIMDs 1-3, five bodies and four, the first body and the rank run-time scalars (inlining the loop once per role measured 0.15 us
// slower in round 4 and is 40 KB more code per evaluation order).
template <int WB = kWgBodies, bool DUO = false, typename PosPtr, std::enable_if_t<WB == kWgBodies && !DUO, int> = 0>
__device__ __forceinline__ double wg_force(PosPtr pos, int n, int i0, double init, double *C, int tid) {
    constexpr int kRows = 3 * WB, kBuf = kRows * kRow;   // chains of the chain wave, doubles per LDS tile buffer
    const int lane = tid & 63, wave = tid >> 6;
    const int tiles = (n + kTile - 1) / kTile;
    const int tdiag = i0 / kTile;
    const int w = __builtin_amdgcn_readfirstlane(wave);
    if (w == 0) { wg_pair_wave_solo(pos, n, i0, C, lane, tiles, tdiag, kBuf); return 0.0; }
    if ((w & 3) && w < 8) { wg_pair_wave_deal<5>(pos, n, i0, 5 * (w & 3) - 4, w >> 2, C, lane, tiles, tdiag, kBuf); return 0.0; }
    if (w & 3) { wg_pair_wave_deal<4>(pos, n, i0, 5 * (w & 3) - 4, 2, C, lane, tiles, tdiag, kBuf); return 0.0; }
    // (k_lm_step_wg gives this wave the integrator's work around the same call)
    if (w == kWgTailWave) { wg_tail_wave_phases(pos, n, i0, C, lane, tiles, tdiag, kBuf); return 0.0; }
    // the chain wave
    const int ch = lane < kRows ? lane : kRows - 1;
    const double *row = C + ch * kRow;
    const int gself = (i0 % kTile) / WB;
    const int li = (i0 % kTile) + ch / 3;
    double acc = init, accL = 0.0;
    double2 q[4][8];
    __builtin_amdgcn_s_setprio(3);
    // phases of up to three tiles. Until the barrier that ends phase P every buffer outside P is being written, so a phase
    // opens with the load of its own first two chunks; inside a phase tile t + 1 is prefetched while tile t is summed.
    // Behind barrier B_P the complete tiles are c of phase P - 1 and a, b of phase P (phase_start above).
    const int NP = interval_count(tiles);
    WG_STAMP(2);
    __syncthreads();                              // B_0: tile 0 ready
    WG_STAMP(3);
    for (int P = 0; P < NP; ++P) {
        const int t0 = chain_first(P), nt = min(chain_first(P + 1), tiles) - t0;
        // three whole tiles of other workgroups' bodies (all but a handful of phases): written out, the prefetch registers
        // never change hands. (As a loop over the tiles of the phase with the masked form inside, the optimiser left it rolled
        // and rotated the 128 prefetch registers through moves behind an lgkmcnt(0): 40.3 us per step at N = 4096.)
        const bool whole = nt == 3 && (tdiag < t0 || tdiag > t0 + 2) && n - (t0 + 2) * kTile >= kTile;
        if constexpr (EPH_WG_SIDE == 1) {
        } else if (whole) {
            const double *r0 = row + (t0 % kWgTileBufs) * kBuf, *r1 = row + ((t0 + 1) % kWgTileBufs) * kBuf;
            const double *r2 = row + ((t0 + 2) % kWgTileBufs) * kBuf;
            load_chunk(r0, 0, q[0]);
            load_chunk(r0, 1, q[1]);
            acc = chain_full_pf(r0, r1, q, acc);
            acc = chain_full_pf(r1, r2, q, acc);
            acc = chain_full_q(r2, q, acc);
        } else {   // the single tiles, the phase with the workgroup's own tile, a short or ragged last phase
            for (int t = t0; t < t0 + nt; ++t) {
                const double *r = row + (t % kWgTileBufs) * kBuf;
                const int cnt = min(kTile, n - t * kTile);
                if (t != tdiag && cnt == kTile) { acc = chain_full(r, acc); continue; }
                // (li made opaque per tile: hoisted out of this loop, the 64 "is this source my own body" lane masks of
                // chain_masked are 128 scalar registers held across the whole kernel)
                int lit = li;
                asm volatile("" : "+v"(lit));
                chain_masked<WB>(r, cnt, t == tdiag ? gself : -1, lit, acc, accL);
            }
        }
        if (P + 1 < NP) WG_LOOP_BARRIER();        // these tiles consumed, the next ready
    }
    return accL + acc;
}

// The 8- and 4-body workgroups: the 4-body one on the barrier-per-tile schedule with two chain waves (wg_force_split); the 8-body
// ones on the big-tile schedule (big_start above), with SIX waves (DUO: waves 0-3 two bodies each, 4 the chain, 5 the tail) or
// TWELVE (one body per pair wave, SIMD 0 left to the chain wave: its cost per tile does not depend on how many of its lanes carry a
// chain, so with one workgroup per CU the step takes the chain wave's time).
template <int WB, bool DUO = false, typename PosPtr, std::enable_if_t<WB != kWgBodies || DUO, int> = 0>
__device__ __forceinline__ double wg_force(PosPtr pos, int n, int i0, double init, double *C, int tid) {
    constexpr int kRows = 3 * WB, kBuf = kRows * kRow;
    const int lane = tid & 63, wave = tid >> 6;
    const int tiles = (n + kTile - 1) / kTile;
    const int tdiag = i0 / kTile;
    if constexpr (DUO) {
        static_assert(WB == 8, "the duo form is the 8-body workgroup with two bodies per pair wave");
        const int w = __builtin_amdgcn_readfirstlane(wave);
        if (w < 4) { wg_pair_wave_big<2>(pos, n, i0, 2 * w, C, lane, tiles, tdiag, kBuf); return 0.0; }
        if (w == kDuoTailWave) { wg_idle_wave(tiles); return 0.0; }
    } else if constexpr (wg_tile_split(WB)) {
        return wg_force_split<WB>(pos, n, i0, init, C, tid);
    } else {
        const int body = wg_small_body<WB>(wave);
        if (body >= 0) { wg_pair_wave_big<1>(pos, n, i0, body, C, lane, tiles, tdiag, kBuf); return 0.0; }
        if (wave != kWgChainWave) { wg_idle_wave(tiles); return 0.0; }
    }
    // the chain wave
    const int ch = lane < kRows ? lane : kRows - 1;
    const double *row = C + ch * kRow;
    const int gself = (i0 % kTile) / WB;
    const int li = (i0 % kTile) + ch / 3;
    double acc = init, accL = 0.0;
    double2 q[4][8];
    if constexpr (DUO) __builtin_amdgcn_s_setprio(3);
    const int TB = big_count(tiles);
    __syncthreads();                                  // B_0: tiles 0 and 1 ready
    load_chunk(row, 0, q[0]);
    load_chunk(row, 1, q[1]);
    for (int T = 0; T < TB; ++T) {
#pragma unroll
        for (int hf = 0; hf < 2; ++hf) {
            const int t = big_start(T) + hf;
            if (t >= tiles || (T < 2 && hf)) break;
            const double *r = row + (t % kWgTileBufs) * kBuf;
            const double *rn = row + ((t + 1) % kWgTileBufs) * kBuf;   // complete since the previous barrier
            const int cnt = min(kTile, n - t * kTile);
            if constexpr (EPH_WG_SIDE == 1) {
            } else if (t != tdiag && cnt == kTile) {
                acc = chain_full_pf(r, rn, q, acc);
            } else {
                chain_masked<WB>(r, cnt, t == tdiag ? gself : -1, li, acc, accL);
                load_chunk(rn, 0, q[0]);
                load_chunk(rn, 1, q[1]);
            }
        }
        WG_LOOP_BARRIER();                            // big tile T consumed, big tile T + 2 ready
    }
    return accL + acc;
}

constexpr int wg_lds_doubles(int wb, bool duo = false) { return (wg_tile_split(wb) && !duo ? kWgSplitBufs * 3 * wb * kRow + 128 : kWgTileBufs * 3 * wb * kRow); }

template <int WB = kWgBodies>
__global__ void __launch_bounds__(kWgThreads) k_accel_wg(int n, int npad, const Body4 *__restrict__ pos,
                                                         const double *__restrict__ acc_init, double *__restrict__ acc_out,
                                                         int lo, int hi, KickDrift kd) {
    __shared__ __attribute__((aligned(16))) double C[wg_lds_doubles(WB)];
    const int tid = threadIdx.x, lane = tid & 63;
    const int i0 = lo + blockIdx.x * WB;
    const int my_i = i0 + lane / 3, cc = lane % 3;
    const bool owner = (tid >> 6) == kWgChainWave && lane < 3 * WB && my_i < hi;
    const double init = (owner && acc_init) ? acc_init[cc * npad + my_i] : 0.0;
    const double a = wg_force<WB>(pos, n, i0, init, C, tid);
    if (owner) {
        acc_out[cc * npad + my_i] = a;
        if (kd.v) kick_drift_one(kd, (size_t)cc * npad + my_i, my_i, cc, a);
    }
}

// ONE launch per integrator step: slot `cur` of the ring holds the already predicted positions of the level being completed;
// this launch evaluates its acceleration (reference-order all-pairs sum), recovers its velocity (Cowell), stores the solout sample
// if one is due, predicts the positions of the NEXT level and publishes them (ring + packed ping-pong buffer) -- the kernel
// boundary is the only grid-wide synchronisation a step needs.
// (amdgpu_waves_per_eu(3, 3): for the twelve-wave forms it restates what __launch_bounds__(768) already implies -- three waves per
// SIMD, 168 VGPRs -- and changes nothing in their code; for the six-wave DUO form it is a choice (its 1.5 waves per SIMD would
// allow 256 VGPRs): that form was measured WITH it (17.7 against 18.6 us at 2048 bodies, round 5) and ships as measured.)
//
// THE PHASE OF THE CODE. The step time depends on where the kernel's code lies modulo 32 bytes: s_nop (4 bytes each) at the entry of
// the otherwise unchanged kernel move <12, 16> of order 0 between 29.6-29.9 us per step (an odd number) and 32.1-33.6 (an even one)
// at N = 4096, period 8 s_nop = 32 bytes; the six-wave form at 2048 bodies between 17.3 and 17.8. Nearly every instruction of the
// tile loops is 8 bytes long, and the instruction fetch evidently pays for the ones that straddle its 32-byte windows. So an edit
// that changes the length of the entry by an odd number of dwords -- removing the kernarg loads did -- costs 3 us unless the phase is
// put back: kWgEntryPad is the number of s_nop behind the entry. One value serves every form, both L and all seven evaluation orders
// (each level or faster than before at 4096 / 2048 / 1024 bodies: profiles/step_entry.md). Whoever changes the length of the code in
// front of the role switch re-takes the scan (scripts/build_exp.sh NAME -DEPH_EXPERIMENTS=1 -DEPH_WG_PAD=k, k = 0 .. 7).
constexpr int kWgEntryPad = 5;
//
// THE ARGUMENTS. pos_cur, n, lo, hi, npad and cur are leading plain arguments and arrive in scalar registers (kernarg preload, a
// compile flag of this file: build.py), the whole LmArgs follows by value and is read where a role needs the rest: the tail wave
// alone. No wave waits for the kernarg segment in front of the role switch; every pair role's first memory instructions are the loads
// of its own bodies and its first source tiles.
template <int L, int WB = kWgBodies, bool DUO = false>
__global__ void __launch_bounds__(DUO ? kDuoThreads : kWgThreads) __attribute__((amdgpu_waves_per_eu(3, 3)))
k_lm_step_wg(const Body4 *pos_cur_, int n_, int lo_, int hi_, int npad_, int cur_, const LmArgs a) {
    constexpr int kRows = 3 * WB;
    if constexpr (WB == kWgBodies && !DUO) WG_STAMP(0);
    const Body4 *const pos_cur = EPH_WG_ENTRY_ARGS ? pos_cur_ : a.pos_cur;
    const int n = EPH_WG_ENTRY_ARGS ? n_ : a.n, lo = EPH_WG_ENTRY_ARGS ? lo_ : a.lo, hi = EPH_WG_ENTRY_ARGS ? hi_ : a.hi;
    const int npad = EPH_WG_ENTRY_ARGS ? npad_ : a.npad, cur = EPH_WG_ENTRY_ARGS ? cur_ : a.cur;
    __shared__ __attribute__((aligned(16))) double C[wg_lds_doubles(WB, DUO)];
    const int tid = threadIdx.x, lane = tid & 63;
    const bool chain_wave = (tid >> 6) == kWgChainWave;
    // the wave that does the integrator's work around the force; wave-uniform by construction, and told so (a scalar
    // branch keeps the history registers out of the other roles' live ranges)
    const bool tail_wave = __builtin_amdgcn_readfirstlane(tid >> 6) == (DUO ? kDuoTailWave : kWgTailWave);
    const int i0 = lo + blockIdx.x * WB;
    const int cb = lane / 3, cc = lane % 3;
    const int my_i = i0 + cb;
    const bool owner = tail_wave && lane < kRows && my_i < hi;
    const size_t lvl = (size_t)3 * npad;
    const size_t off = (size_t)cc * npad + (owner ? my_i : 0);
    // the tail wave's whole life is this branch, so its history registers are live across this code only (through
    // wg_force's role switch the allocator would keep them alive in every role and spill)
    // the code behind the entry at its measured 32-byte phase (kWgEntryPad above); the tuning builds' EPH_WG_PAD overrides it
#if EPH_EXPERIMENTS && defined(EPH_WG_PAD)
    asm volatile(".rept %0\n s_nop 0\n .endr" ::"n"(EPH_WG_PAD));
#else
    asm volatile(".rept %0\n s_nop 0\n .endr" ::"n"(kWgEntryPad));
#endif
    if (tail_wave) {
        double yv[L], av[L];   // yv[j] / av[j]: level (new - j); av[0] is filled after the force
        auto load_history = [&]() {
#pragma unroll
            for (int j = 0; j < L; ++j) {
                const int slot = (cur + j) % L;
                yv[j] = a.Y[slot * lvl + off];
                av[j] = j > 0 ? a.A[slot * lvl + off] : 0.0;
            }
        };
        constexpr bool kPhaseTail = WB == kWgBodies && !DUO;
        if constexpr (!kPhaseTail || EPH_WG_HIST_AT == 0) load_history();
        // (Forming everything that does not need the new acceleration here, ahead of the barriers, was built and measured:
        // 37.55 vs 37.2 us per step at N = 4096 -- the early arithmetic takes issue slots from the pair wave and the chain wave
        // of this SIMD when they are the critical path, and the tail's work was not on it.)
        const int tiles = (n + kTile - 1) / kTile;
        if constexpr (wg_tile_split(WB) && !DUO) {
            for (int t = 0; t <= tiles; ++t) __syncthreads();                             // one barrier per tile there
        } else if constexpr (WB == kWgBodies && !DUO) {
            wg_tail_wave_phases(pos_cur, n, i0, C, lane, tiles, i0 / kTile, 3 * WB * kRow, load_history);
        } else {
            wg_idle_wave(tiles);
        }
        if constexpr (kPhaseTail) WG_STAMP(4);
        __syncthreads();                              // the chain wave's result is in LDS
        if constexpr (kPhaseTail) WG_STAMP(5);
        if (owner) {
            const double anew = C[lane];
            a.A[(size_t)cur * lvl + off] = anew;
            {
                double prev[L];
#pragma unroll
                for (int j = 0; j < L - 1; ++j) prev[j] = av[j + 1];
                prev[L - 1] = 0.0;
                a.V[off] = lm_cowell<L>(anew, prev, yv[0], yv[1], a.cw, a.h, a.hc);
            }
            maybe_sample(a.samp, my_i, cc, a.step, yv[0]);
            if (a.do_predict) {
                av[0] = anew;
                const double ynext = lm_predict<L>(yv, av, a.wa, a.wb, a.hh);
                const int nslot = (cur + L - 1) % L;
                a.Y[(size_t)nslot * lvl + off] = ynext;
                reinterpret_cast<double *>(a.pos_next + my_i)[cc] = ynext;
            }
        }
        if constexpr (kPhaseTail) WG_STAMP(6);
    } else {
        const double anew = wg_force<WB, DUO>(pos_cur, n, i0, 0.0, C, tid);
        if constexpr (WB == kWgBodies && !DUO) WG_STAMP(4);
        if (chain_wave && lane < kRows) C[lane] = anew;    // every tile buffer is dead after the loop's last barrier
        __syncthreads();
        if constexpr (WB == kWgBodies && !DUO) WG_STAMP(5);
    }
}

// ---- launchers (wb = bodies per workgroup: 16, 8 or 4; dispatch.cpp chooses) --------------------------------------------------
int accel_wg(hipStream_t s, int wb, int n, int npad, const Body4 *pos, const double *acc_init, double *acc_out, int lo, int hi,
             const KickDrift &kd) {
    const dim3 grid((hi - lo + wb - 1) / wb), block(kWgThreads);
    if (wb == 8) hipLaunchKernelGGL(k_accel_wg<8>, grid, block, 0, s, n, npad, pos, acc_init, acc_out, lo, hi, kd);
    else if (wb == 4) hipLaunchKernelGGL(k_accel_wg<4>, grid, block, 0, s, n, npad, pos, acc_init, acc_out, lo, hi, kd);
    else hipLaunchKernelGGL(k_accel_wg<16>, grid, block, 0, s, n, npad, pos, acc_init, acc_out, lo, hi, kd);
    return launched("k_accel_wg");
}
int lm_step_wg(hipStream_t s, int wb, const LmArgs &a) {
    if (wb == 9) {                                          // the six-wave 8-body form (dispatch.cpp: 1024 < targets <= 2048; EPH_WG_BODIES=9)
        const dim3 grid((a.hi - a.lo + 7) / 8), block(kDuoThreads);
        if (a.L == 12) hipLaunchKernelGGL((k_lm_step_wg<12, 8, true>), grid, block, 0, s, a.pos_cur, a.n, a.lo, a.hi, a.npad, a.cur, a);
        else if (a.L == 13) hipLaunchKernelGGL((k_lm_step_wg<13, 8, true>), grid, block, 0, s, a.pos_cur, a.n, a.lo, a.hi, a.npad, a.cur, a);
        else return EPH_ERR_UNSUPPORTED;
        return launched("k_lm_step_wg (six waves)");
    }
    const dim3 grid((a.hi - a.lo + wb - 1) / wb), block(kWgThreads);
    if (a.L == 12 && wb == 8) hipLaunchKernelGGL((k_lm_step_wg<12, 8>), grid, block, 0, s, a.pos_cur, a.n, a.lo, a.hi, a.npad, a.cur, a);
    else if (a.L == 13 && wb == 8) hipLaunchKernelGGL((k_lm_step_wg<13, 8>), grid, block, 0, s, a.pos_cur, a.n, a.lo, a.hi, a.npad, a.cur, a);
    else if (a.L == 12 && wb == 4) hipLaunchKernelGGL((k_lm_step_wg<12, 4>), grid, block, 0, s, a.pos_cur, a.n, a.lo, a.hi, a.npad, a.cur, a);
    else if (a.L == 13 && wb == 4) hipLaunchKernelGGL((k_lm_step_wg<13, 4>), grid, block, 0, s, a.pos_cur, a.n, a.lo, a.hi, a.npad, a.cur, a);
    else if (a.L == 12) hipLaunchKernelGGL((k_lm_step_wg<12, 16>), grid, block, 0, s, a.pos_cur, a.n, a.lo, a.hi, a.npad, a.cur, a);
    else if (a.L == 13) hipLaunchKernelGGL((k_lm_step_wg<13, 16>), grid, block, 0, s, a.pos_cur, a.n, a.lo, a.hi, a.npad, a.cur, a);
    else return EPH_ERR_UNSUPPORTED;
    return launched("k_lm_step_wg");
}

}  // namespace EPH_PV_NS
}  // namespace eph

#if EPH_WG_STAMPS && EPH_PAIR_VARIANT == 0
// the stamps of the last k_lm_step_wg<L, 16> launch (order 0): [wave][point], 12 x 8 shader-clock values
extern "C" __attribute__((visibility("default"))) int eph_wg_stamps(unsigned long long *out) {
    if (hipDeviceSynchronize() != hipSuccess) return 1;
    return hipMemcpyFromSymbol(out, HIP_SYMBOL(eph::pv0::g_wg_stamps), sizeof(unsigned long long) * 12 * 8) == hipSuccess ? 0 : 1;
}
#endif
