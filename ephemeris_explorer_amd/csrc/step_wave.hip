// step_wave.hip -- the one-wave-per-block force (wave_force) and the kernels built on it: k_accel (a = init + sum), k_lm_step
// (one fused linear-multistep step per launch) and k_lm_persistent (33..64 bodies, many steps per launch). Chosen for
// N <= 512 targets (dispatch.cpp); above that the workgroup-specialised force of step_wg.hip is the faster one.
// Compiled once per evaluation order of the point-mass term (pair_ns.h). -ffp-contract=off: the reference (Rust) never fuses
// a*b+c and parity is defined bit for bit, so every sum is written in the reference's operation order and must stay un-fused.
// Reference citations are relative to the reference repository root.
#include <algorithm>
#include <initializer_list>
#include <type_traits>
#include <utility>

#include "pair_ns.h"

namespace eph {
namespace EPH_PV_NS {

// ------------------------------------------------------------------------------------------------------
// Software-pipelined tile step. While the ordered sum of tile t (phase B: 64 dependent v_add_f64 fed from LDS)
// advances, the same wave finishes the pair arithmetic of tile t+1 (22 VALU ops per body: in-range sqrt,
// reciprocal, scaling) and starts tile t+2 (8 ops per body: differences and squared distance). With one wave per
// SIMD nothing else can fill the issue slots a dependent add leaves empty, so the two instruction streams are
// interleaved explicitly, one chain add after every few independent pair ops, and pinned with
// sched_barrier (VALU may not cross; SALU / VMEM / DS may) -- the compiler's own schedule clusters the chain.
// ------------------------------------------------------------------------------------------------------

template <int BPW>
struct TileCtx {                 // registers of the pipelined tile steps
    PairPre pre[2][BPW];         // ping-pong: differences of the tile being finished / of the one after it
    double mu[2];                // source mu belonging to pre[k]
    Body4 src[2];                // prefetched sources, two steps ahead
    double c[3 * BPW];           // contributions being produced
    double y[BPW], g[BPW], h[BPW], r[BPW], d[BPW], p[BPW], tmp[BPW];
    double2 q[4][8];             // the LDS row being summed, four 16-element chunks
    double acc;
};

// stage S (0..21) of pair_finish<true> for body B on w.pre[PH]; same operations, same order as sqrt_inrange /
// rcp_inrange. Returns the value written (for the scheduling anchor).
template <int BPW, int PH, int S, int B>
__device__ __forceinline__ double &pair_stage(TileCtx<BPW> &w) {
    const PairPre &in = w.pre[PH][B];
    const double x = in.n2;
    if constexpr (S == 0) { w.y[B] = __builtin_amdgcn_rsq(x); return w.y[B]; }
    else if constexpr (S == 1) { w.g[B] = x * w.y[B]; return w.g[B]; }
    else if constexpr (S == 2) { w.h[B] = w.y[B] * 0.5; return w.h[B]; }
    else if constexpr (S == 3) { w.r[B] = __builtin_fma(-w.h[B], w.g[B], 0.5); return w.r[B]; }
    else if constexpr (S == 4) { w.g[B] = __builtin_fma(w.g[B], w.r[B], w.g[B]); return w.g[B]; }
    else if constexpr (S == 5) { w.h[B] = __builtin_fma(w.h[B], w.r[B], w.h[B]); return w.h[B]; }
    else if constexpr (S == 6) { w.d[B] = __builtin_fma(-w.g[B], w.g[B], x); return w.d[B]; }
    else if constexpr (S == 7) { w.g[B] = __builtin_fma(w.d[B], w.h[B], w.g[B]); return w.g[B]; }
    else if constexpr (S == 8) { w.d[B] = __builtin_fma(-w.g[B], w.g[B], x); return w.d[B]; }
    else if constexpr (S == 9) { w.g[B] = __builtin_fma(w.d[B], w.h[B], w.g[B]); return w.g[B]; }       // sqrt(n2)
    else if constexpr (S == 10) { w.p[B] = x * w.g[B]; return w.p[B]; }                                 // n2*sqrt(n2)
    // S11-13: the reciprocal's seed, 8 h^3 from the square root's refined h (inv_r3_seeded, pair_term.h)
    else if constexpr (S == 11) { w.r[B] = w.h[B] * w.h[B]; return w.r[B]; }
    else if constexpr (S == 12) { w.r[B] = w.r[B] * w.h[B]; return w.r[B]; }
    else if constexpr (S == 13) { w.r[B] = w.r[B] * 8.0; return w.r[B]; }
    else if constexpr (S == 14) { w.d[B] = __builtin_fma(-w.p[B], w.r[B], 1.0); return w.d[B]; }
    else if constexpr (S == 15) { w.r[B] = __builtin_fma(w.r[B], w.d[B], w.r[B]); return w.r[B]; }
    else if constexpr (S == 16) { w.d[B] = __builtin_fma(-w.p[B], w.r[B], 1.0); return w.d[B]; }
    else if constexpr (S == 17) { w.r[B] = __builtin_fma(w.d[B], w.r[B], w.r[B]); return w.r[B]; }      // 1/(n2*sqrt(n2))
    else if constexpr (S == 18) { w.h[B] = w.mu[PH] * w.r[B]; return w.h[B]; }
    else if constexpr (S == 19) { w.c[3 * B + 0] = in.dx * w.h[B]; return w.c[3 * B + 0]; }
    else if constexpr (S == 20) { w.c[3 * B + 1] = in.dy * w.h[B]; return w.c[3 * B + 1]; }
    else { w.c[3 * B + 2] = in.dz * w.h[B]; return w.c[3 * B + 2]; }
}
// stage S (0..7) of pair_pre for body B: w.src[PH] -> w.pre[PH ^ 1]
template <int BPW, int PH, int S, int B>
__device__ __forceinline__ double &pre_stage(TileCtx<BPW> &w, const double (&xi)[BPW], const double (&yi)[BPW],
                                             const double (&zi)[BPW]) {
    PairPre &p = w.pre[PH ^ 1][B];
    const Body4 &pj = w.src[PH];
    if constexpr (S == 0) { p.dx = pj.x - xi[B]; return p.dx; }
    else if constexpr (S == 1) { p.dy = pj.y - yi[B]; return p.dy; }
    else if constexpr (S == 2) { p.dz = pj.z - zi[B]; return p.dz; }
    else if constexpr (S == 3) { p.n2 = p.dx * p.dx; return p.n2; }
    else if constexpr (S == 4) { w.tmp[B] = p.dy * p.dy; return w.tmp[B]; }
    else if constexpr (S == 5) { p.n2 = p.n2 + w.tmp[B]; return p.n2; }
    else if constexpr (S == 6) { w.tmp[B] = p.dz * p.dz; return w.tmp[B]; }
    else { p.n2 = p.n2 + w.tmp[B]; return p.n2; }
}
// chain adds M0 .. M1-1 of the 64 of this tile, each anchored so no pass can sink it past the next barrier
template <int BPW, int M0, int M1>
__device__ __forceinline__ void chain_adds(TileCtx<BPW> &w, const double *row) {
    if constexpr (M0 < M1) {
        if constexpr (M0 == 8) load_chunk(row, 2, w.q[2]);
        if constexpr (M0 == 24) load_chunk(row, 3, w.q[3]);
        const double2 &e = w.q[M0 / 16][(M0 % 16) / 2];
        w.acc = w.acc + ((M0 & 1) ? e.y : e.x);
        asm volatile("" : "+v"(w.acc));
        chain_adds<BPW, M0 + 1, M1>(w, row);
    }
}
// One slot of the fused instruction stream: op K of the 30*BPW pair ops, then its share of the 64 chain adds.
// The chain starts a quarter of the way in (the LDS reads issued at the top need ~130 cycles to land, and an
// in-order wave would otherwise sit on the first add with independent work queued behind it).
template <int BPW, int PH, int K>
__device__ __forceinline__ void fused_op(TileCtx<BPW> &w, const double (&xi)[BPW], const double (&yi)[BPW],
                                         const double (&zi)[BPW], const double *row_cur, double *tile_nxt, int lane) {
    constexpr int kOps = 30 * BPW;            // 22 finish + 8 pre per body
    constexpr int kLead = kOps / 4;
    constexpr int S = K / BPW, B = K % BPW;
    // every op is anchored with an empty asm: IR passes may otherwise sink pure arithmetic past the barriers
    // (towards its use in the next loop iteration) and undo the interleave
    if constexpr (S < 22) {
        double &v = pair_stage<BPW, PH, S, B>(w);
        asm volatile("" : "+v"(v));
        if constexpr (S == 21) {              // body B finished: publish its contributions to the OTHER LDS buffer
            tile_nxt[(3 * B + 0) * kRow + lane] = w.c[3 * B + 0];
            tile_nxt[(3 * B + 1) * kRow + lane] = w.c[3 * B + 1];
            tile_nxt[(3 * B + 2) * kRow + lane] = w.c[3 * B + 2];
        }
    } else {
        double &v = pre_stage<BPW, PH, S - 22, B>(w, xi, yi, zi);
        asm volatile("" : "+v"(v));
    }
    if constexpr (K >= kLead) {
        constexpr int J = K - kLead, kSpan = kOps - kLead;
        chain_adds<BPW, J * 64 / kSpan, (J + 1) * 64 / kSpan>(w, row_cur);
    }
    __builtin_amdgcn_sched_barrier(kSchedMask);
}
template <int BPW, int PH, int... K>
__device__ __forceinline__ void fused_ops(TileCtx<BPW> &w, const double (&xi)[BPW], const double (&yi)[BPW],
                                          const double (&zi)[BPW], const double *row_cur, double *tile_nxt, int lane,
                                          std::integer_sequence<int, K...>) {
    (fused_op<BPW, PH, K>(w, xi, yi, zi, row_cur, tile_nxt, lane), ...);
}

// Pipelined step PH (0/1 = ping-pong phase), processing tile t:
//   in : w.pre[PH], w.mu[PH] = tile t+1 (guarded in range); w.src[PH] = sources of tile t+2;
//        LDS buffer PH holds the contributions of tile t
//   out: contributions of tile t+1 in LDS buffer PH^1; w.pre[PH^1], w.mu[PH^1] = tile t+2; w.acc advanced over tile t
template <int BPW, int PH>
__device__ __forceinline__ void tile_step_fast(TileCtx<BPW> &w, const double (&xi)[BPW], const double (&yi)[BPW],
                                               const double (&zi)[BPW], const double *row_cur, double *tile_nxt,
                                               int lane) {
    load_chunk(row_cur, 0, w.q[0]);
    load_chunk(row_cur, 1, w.q[1]);
    fused_ops<BPW, PH>(w, xi, yi, zi, row_cur, tile_nxt, lane, std::make_integer_sequence<int, 30 * BPW>{});
    w.mu[PH ^ 1] = w.src[PH].mu;
}

// ------------------------------------------------------------------------------------------------------
// wave_force<BPW>: one wave64 computes the accelerations of BPW consecutive bodies i0..i0+BPW-1 in EXACTLY the
// reference's summation order (NewtonianGravity::eval, nbody.rs:22-38):
//     ddy[i] = ((init + c(0,i)) + ... + c(i-1,i))  +  ((0 + c(i,i+1)) + ... + c(i,n-1))
// Phase A: lane = source body j of the current 64-body tile; BPW independent interactions per lane go to a
//          wave-private LDS tile C[chain][j]  (chain = body*3 + component, row stride kRow doubles).
// Phase B: lane = chain (< 3*BPW); walks its row in j order with one dependent v_add_f64 per source.
// The sqrt/divide-heavy phase A is fully parallel; only the 3 adds per interaction are ordered. Full tiles away
// from the wave's own bodies are software-pipelined (A of tile t+1 overlaps B of tile t, sources two tiles ahead
// in flight); the tile holding the wave's bodies and a ragged last tile take the masked, un-pipelined form.
// Returns, on lane `ch` < 3*BPW, component ch%3 of body i0 + ch/3.
// ------------------------------------------------------------------------------------------------------
template <int BPW, bool SINGLE_TILE = false, typename PosPtr>
__device__ __forceinline__ double wave_force(PosPtr pos, int n, int i0, double init, double *C, int lane) {
    static_assert(kTile % BPW == 0, "BPW must divide the tile");
    double xi[BPW], yi[BPW], zi[BPW];
#pragma unroll
    for (int b = 0; b < BPW; ++b) {
        const int ii = min(i0 + b, n - 1);
        xi[b] = pos[ii].x;
        yi[b] = pos[ii].y;
        zi[b] = pos[ii].z;
    }
    const bool chain_lane = lane < 3 * BPW;
    const int ch = chain_lane ? lane : 3 * BPW - 1;
    const double *row = C + ch * kRow;
    const int tiles = (n + kTile - 1) / kTile;
    const int tfull = n / kTile;
    const int tdiag = i0 / kTile;                     // wave-uniform: i0 % BPW == 0 and BPW divides 64
    const int gself = (i0 % kTile) / BPW;
    const int li = (i0 % kTile) + ch / 3;
    double acc = init;   // lower chain (sources before the body), continues from the caller's value
    double accL = 0.0;

    auto load_src = [&](int t) -> Body4 {
        const int j = t * kTile + lane;
        return pos[j < n ? j : n - 1];
    };
    auto store_tile = [&](const double(&c)[3 * BPW]) {
#pragma unroll
        for (int q = 0; q < 3 * BPW; ++q) C[q * kRow + lane] = c[q];
    };
    // un-pipelined tile (holds the wave's own bodies and/or is the ragged last one): IEEE arithmetic throughout
    // (n2 = 0 on the self lane), masked chain
    auto special = [&](int t) {
        const Body4 pj = load_src(t);
        double c[3 * BPW];
#pragma unroll
        for (int b = 0; b < BPW; ++b)
            pair_finish<false>(pair_pre(xi[b], yi[b], zi[b], pj), pj.mu, c[3 * b], c[3 * b + 1], c[3 * b + 2]);
        store_tile(c);
        wave_lds_fence();
        if (chain_lane) chain_masked<BPW>(row, min(kTile, n - t * kTile), t == tdiag ? gself : -1, li, acc, accL);
        wave_lds_fence();
    };
    // pipelined run over the full tiles [tb, te), none of which holds the wave's bodies.
    // LDS is double buffered: step t sums buffer t&1 while the contributions of tile t+1 go to the other one.
    constexpr int kBuf = 3 * BPW * kRow;
    auto run = [&](int tb, int te) {
        if (tb >= te) return;
        TileCtx<BPW> w;
        {
            const Body4 pj = load_src(tb);
            double c[3 * BPW];
#pragma unroll
            for (int b = 0; b < BPW; ++b)
                pair_finish<false>(pair_pre(xi[b], yi[b], zi[b], pj), pj.mu, c[3 * b], c[3 * b + 1], c[3 * b + 2]);
            store_tile(c);                                  // tile tb -> buffer 0
        }
        {
            const Body4 pj = load_src(min(tb + 1, te - 1));
#pragma unroll
            for (int b = 0; b < BPW; ++b) w.pre[0][b] = pair_pre(xi[b], yi[b], zi[b], pj);
            w.mu[0] = pj.mu;
        }
        w.src[0] = load_src(min(tb + 2, te - 1));
        w.src[1] = load_src(min(tb + 3, te - 1));
        w.acc = acc;
        wave_lds_fence();
        // one step: PH = (t - tb) & 1
        auto step = [&](auto ph, int t) {
            constexpr int PH = decltype(ph)::value;
            const double *row_cur = row + PH * kBuf;
            double *tile_nxt = C + (PH ^ 1) * kBuf;
            unsigned worst = mu_key(w.mu[PH]), low = ~0u;
#pragma unroll
            for (int b = 0; b < BPW; ++b) { worst = max(worst, range_key(w.pre[PH][b].n2)); low = min(low, w.pre[PH][b].lo); }
            const bool all_in_range = __builtin_amdgcn_ballot_w64(max(worst, low_key(low)) >= kRangeSpan) == 0;
            if (kPairVariant == 0 && all_in_range) {        // the hand-interleaved stream restates variant 0 only
                tile_step_fast<BPW, PH>(w, xi, yi, zi, row_cur, tile_nxt, lane);
            } else {                                        // an operand near the end of the exponent range
#pragma unroll
                for (int b = 0; b < BPW; ++b) {
                    if (kPairVariant != 0 && all_in_range)
                        pair_finish<true>(w.pre[PH][b], w.mu[PH], w.c[3 * b], w.c[3 * b + 1], w.c[3 * b + 2]);
                    else
                        pair_finish<false>(w.pre[PH][b], w.mu[PH], w.c[3 * b], w.c[3 * b + 1], w.c[3 * b + 2]);
                    w.pre[PH ^ 1][b] = pair_pre(xi[b], yi[b], zi[b], w.src[PH]);
                }
#pragma unroll
                for (int q = 0; q < 3 * BPW; ++q) tile_nxt[q * kRow + lane] = w.c[q];
                w.mu[PH ^ 1] = w.src[PH].mu;
                w.acc = chain_full(row_cur, w.acc);
            }
            w.src[PH] = load_src(min(t + 4, te - 1));       // two steps ahead
            wave_lds_fence();
        };
        int t = tb;
        for (; t + 1 < te - 1; t += 2) {
            step(std::integral_constant<int, 0>{}, t);
            step(std::integral_constant<int, 1>{}, t + 1);
        }
        if (t < te - 1) {                                   // odd number of steps: last tile sits in buffer 1
            step(std::integral_constant<int, 0>{}, t);
            w.acc = chain_full(row + kBuf, w.acc);
        } else {
            w.acc = chain_full(row, w.acc);
        }
        acc = w.acc;
        wave_lds_fence();
    };

    if (SINGLE_TILE) {          // n <= 64 (persistent kernel): one masked tile, no pipeline code at all
        special(0);
        return accL + acc;
    }
    run(0, min(tdiag, tfull));
    special(tdiag);
    if (tdiag < tfull) {
        run(tdiag + 1, tfull);
        if (tfull < tiles) special(tfull);
    }
    return accL + acc;   // ddy[i] += output_i
}

// ------------------------------------------------------------------------------------------------------
// k_accel: a = init + sum, SoA [3][npad] output. One wave per block, BPW bodies per wave.
// ------------------------------------------------------------------------------------------------------
template <int BPW>
__global__ void __launch_bounds__(64) k_accel(int n, int npad, const Body4 *__restrict__ pos,
                                              const double *__restrict__ acc_init, double *__restrict__ acc_out,
                                              int lo, int hi, KickDrift kd) {
    __shared__ __attribute__((aligned(16))) double C[2 * 3 * BPW * kRow];   // double buffered contribution tile
    const int lane = threadIdx.x;
    const int i0 = lo + blockIdx.x * BPW;          // targets [lo, hi): the whole system, or this rank's shard
    const int cb = lane / 3, cc = lane % 3;
    const int my_i = i0 + cb;
    const bool owner = lane < 3 * BPW && my_i < hi;
    const double init = (owner && acc_init) ? acc_init[cc * npad + my_i] : 0.0;
    const double a = wave_force<BPW>(pos, n, i0, init, C, lane);
    if (owner) {
        acc_out[cc * npad + my_i] = a;
        if (kd.v) kick_drift_one(kd, (size_t)cc * npad + my_i, my_i, cc, a);
    }
}

// ------------------------------------------------------------------------------------------------------
// k_lm_step: ONE launch per integrator step (all CUs). Slot `cur` of the ring holds the already predicted
// positions of the level being completed; this launch
//   1. evaluates its acceleration (reference-order all-pairs sum),
//   2. recovers its velocity (Cowell),
//   3. stores the solout sample if one is due,
//   4. predicts the positions of the NEXT level and publishes them (ring + packed ping-pong buffer),
// so the kernel boundary is the only grid-wide synchronisation a step needs.
// History reads are issued before the pair loop so their latency hides under it.
// ------------------------------------------------------------------------------------------------------
template <int BPW, int L>
__global__ void __launch_bounds__(64) k_lm_step(const LmArgs a) {
    __shared__ __attribute__((aligned(16))) double C[2 * 3 * BPW * kRow];   // double buffered contribution tile
    const int lane = threadIdx.x;
    const int i0 = a.lo + blockIdx.x * BPW;
    const int cb = lane / 3, cc = lane % 3;
    const int my_i = i0 + cb;
    const bool owner = lane < 3 * BPW && my_i < a.hi;
    const size_t lvl = (size_t)3 * a.npad;
    const size_t off = (size_t)cc * a.npad + (owner ? my_i : 0);

    double yv[L], av[L];   // yv[j]/av[j]: level (new - j); av[0] is filled after the force
#pragma unroll
    for (int j = 0; j < L; ++j) {
        const int slot = (a.cur + j) % L;
        yv[j] = a.Y[slot * lvl + off];           // non-owner lanes read body 0 (unused): no exec-masked loads
        av[j] = j > 0 ? a.A[slot * lvl + off] : 0.0;
    }

    const double anew = wave_force<BPW>(a.pos_cur, a.n, i0, 0.0, C, lane);
    if (!owner) return;

    a.A[(size_t)a.cur * lvl + off] = anew;
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
        const int nslot = (a.cur + L - 1) % L;
        a.Y[(size_t)nslot * lvl + off] = ynext;
        reinterpret_cast<double *>(a.pos_next + my_i)[cc] = ynext;
    }
}

// ------------------------------------------------------------------------------------------------------
// k_lm_persistent: n <= 64 (one tile). The whole system lives in one workgroup's LDS and registers and the
// kernel runs `nsteps` integrator steps per launch (a 32-body step is ~1e3 pair interactions: launch latency
// would dominate a per-step launch). 8 waves (two per SIMD, 256 VGPRs each); wave w owns bodies w*BPW..; lane ch of that wave owns the
// (body, component) chain ch for the force, the velocity, the history ring and the predictor, so the only data
// shared between threads are the packed positions sP (two barriers per step).
// On entry slot `cur` is a COMPLETE level (Y, A, V); on exit slot (cur - nsteps) mod L is.
// ------------------------------------------------------------------------------------------------------
template <int BPW, int L>
__global__ void __launch_bounds__(512) k_lm_persistent(const LmArgs a, long long nsteps) {
    constexpr int kWaves = 8;
    __shared__ __attribute__((aligned(16))) double C[kWaves][3 * BPW * kRow];
    __shared__ __attribute__((aligned(32))) Body4 sP[kTile];
    __shared__ double ringY[L][3 * kTile];   // [slot][body*3 + comp]
    __shared__ double ringA[L][3 * kTile];

    const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
    const int i0 = w * BPW;
    const int cb = lane / 3, cc = lane % 3;
    const int my_i = i0 + cb;
    const bool owner = lane < 3 * BPW && my_i < a.n;
    const size_t lvl = (size_t)3 * a.npad;
    const size_t off = (size_t)cc * a.npad + (owner ? my_i : 0);
    const int ro = owner ? my_i * 3 + cc : 0;

    if (tid < kTile) sP[tid] = a.pos_cur[tid < a.n ? tid : a.n - 1];
    if (owner) {
#pragma unroll
        for (int s = 0; s < L; ++s) {
            ringY[s][ro] = a.Y[s * lvl + off];
            ringA[s][ro] = a.A[s * lvl + off];
        }
    }
    double v = owner ? a.V[off] : 0.0;
    int cur = a.cur;
    __syncthreads();

    for (long long s = 1; s <= nsteps; ++s) {
        double yv[L], av[L];
#pragma unroll
        for (int j = 0; j < L; ++j) {
            const int slot = (cur + j) % L;
            yv[j] = ringY[slot][ro];
            av[j] = ringA[slot][ro];
        }
        const double ynew = lm_predict<L>(yv, av, a.wa, a.wb, a.hh);
        const int nslot = (cur + L - 1) % L;
        if (owner) {
            ringY[nslot][ro] = ynew;
            reinterpret_cast<double *>(&sP[my_i])[cc] = ynew;
        }
        __syncthreads();   // new positions visible to every wave
        const double anew = wave_force<BPW, true>(sP, a.n, i0, 0.0, C[w], lane);
        if (owner) {
            ringA[nslot][ro] = anew;
            v = lm_cowell<L>(anew, av, ynew, yv[0], a.cw, a.h, a.hc);
            maybe_sample(a.samp, my_i, cc, (uint32_t)s, ynew);
        }
        cur = nslot;
        __syncthreads();   // every wave done reading sP before the next predictor overwrites it
    }

    if (owner) {
#pragma unroll
        for (int s = 0; s < L; ++s) {
            a.Y[s * lvl + off] = ringY[s][ro];
            a.A[s * lvl + off] = ringA[s][ro];
        }
        a.V[off] = v;
        // leave both packed buffers consistent with the newest level
        reinterpret_cast<double *>(a.pos_next + my_i)[cc] = ringY[cur][ro];
        reinterpret_cast<double *>(const_cast<Body4 *>(a.pos_cur) + my_i)[cc] = ringY[cur][ro];
    }
}

// ---- launchers ---------------------------------------------------------------------------------------------------------------
int accel_wave(hipStream_t s, int bpw, int n, int npad, const Body4 *pos, const double *acc_init, double *acc_out, int lo, int hi,
               const KickDrift &kd) {
    const int nt = hi - lo;
    const dim3 grid((nt + bpw - 1) / bpw), block(64);
    switch (bpw) {
        case 1: hipLaunchKernelGGL(k_accel<1>, grid, block, 0, s, n, npad, pos, acc_init, acc_out, lo, hi, kd); break;
        case 2: hipLaunchKernelGGL(k_accel<2>, grid, block, 0, s, n, npad, pos, acc_init, acc_out, lo, hi, kd); break;
        case 4: hipLaunchKernelGGL(k_accel<4>, grid, block, 0, s, n, npad, pos, acc_init, acc_out, lo, hi, kd); break;
        default: hipLaunchKernelGGL(k_accel<8>, grid, block, 0, s, n, npad, pos, acc_init, acc_out, lo, hi, kd); break;
    }
    return launched("k_accel");
}
template <int L>
static int lm_step_wave_L(hipStream_t s, int bpw, const LmArgs &a) {
    const int nt = a.hi - a.lo;
    const dim3 grid((nt + bpw - 1) / bpw), block(64);
    switch (bpw) {
        case 1: hipLaunchKernelGGL((k_lm_step<1, L>), grid, block, 0, s, a); break;
        case 2: hipLaunchKernelGGL((k_lm_step<2, L>), grid, block, 0, s, a); break;
        case 4: hipLaunchKernelGGL((k_lm_step<4, L>), grid, block, 0, s, a); break;
        default: hipLaunchKernelGGL((k_lm_step<8, L>), grid, block, 0, s, a); break;
    }
    return launched("k_lm_step");
}
int lm_step_wave(hipStream_t s, int bpw, const LmArgs &a) {
    if (a.L == 12) return lm_step_wave_L<12>(s, bpw, a);
    if (a.L == 13) return lm_step_wave_L<13>(s, bpw, a);
    return EPH_ERR_UNSUPPORTED;
}
template <int L>
static int lm_persistent_L(hipStream_t s, const LmArgs &a, int64_t nsteps) {
    const int per_wave = (a.n + 7) / 8;
    const dim3 grid(1), block(512);
    if (per_wave <= 1) hipLaunchKernelGGL((k_lm_persistent<1, L>), grid, block, 0, s, a, (long long)nsteps);
    else if (per_wave <= 2) hipLaunchKernelGGL((k_lm_persistent<2, L>), grid, block, 0, s, a, (long long)nsteps);
    else if (per_wave <= 4) hipLaunchKernelGGL((k_lm_persistent<4, L>), grid, block, 0, s, a, (long long)nsteps);
    else hipLaunchKernelGGL((k_lm_persistent<8, L>), grid, block, 0, s, a, (long long)nsteps);
    return launched("k_lm_persistent");
}
int lm_persistent(hipStream_t s, const LmArgs &a, int64_t nsteps) {
    if (a.L == 12) return lm_persistent_L<12>(s, a, nsteps);
    if (a.L == 13) return lm_persistent_L<13>(s, a, nsteps);
    return EPH_ERR_UNSUPPORTED;
}

}  // namespace EPH_PV_NS
}  // namespace eph
