// step_double_small.hip -- k_lm_double_small: the steady ELM2 steps of a `<Double>` handle (double_state.h) of at most 32 bodies
// in ONE workgroup, `nsteps` integrator steps per launch. A sibling of k_lm_small (step_small.hip), not a flag on it: the pair
// phase, the LDS rows and the two ordered row sums are that kernel's, statement for statement; what differs is the (body,
// component) thread, which carries the value AND the error part of the L history levels of y and runs the predictor on
// Double's operators. Compiled once per evaluation order of the point-mass term (pair_ns.h).
#include <initializer_list>
#include <type_traits>
#include <utility>

#include "pair_ns.h"
#include "double_state.h"

namespace eph {
namespace EPH_PV_NS {

// the step loop unrolled over the L ring rotations: copy K runs at rotation (L - K) % L   (as step_small.hip's small_steps)
template <typename Step, int... Ks>
__device__ __forceinline__ void double_small_steps(Step &step, long long &s, long long nsteps, int &rot, bool &more,
                                                   std::integer_sequence<int, Ks...>) {
    constexpr int L = sizeof...(Ks);
    (void)std::initializer_list<int>{(more ? (step(std::integral_constant<int, (L - Ks) % L>{}, s),
                                              rot = (L - Ks + L - 1) % L, more = ++s <= nsteps, 0)
                                           : 0)...};
}
constexpr int kDoubleSmallThreads = 512;   // eight waves: one unordered pair per thread (496 at 32 bodies), the 3 n chains x 2 halves in waves 0-2
constexpr int kDoubleSmallMaxN = 32;
constexpr int kDoubleSmallRow = 32 + 2;    // doubles per row: 16-byte aligned rows an odd number of 16-byte units apart
constexpr int kDoubleSmallRows = 3 * kDoubleSmallMaxN;
static_assert(kDoubleSmallMaxN == kGangMaxN, "launch_lm_double_small admits what the kernel's rows hold");

// What the owner thread of a (body, component) keeps for the whole launch: yv / ye / av[L] (value and error of y, acceleration)
// and the weights -- L + 2 doubles more than k_lm_small's (the error parts, the error of the level under construction, the
// velocity's). What its step costs more: sum1 and sum2 of ELM2::advance are chains of L Double additions, ten dependent f64
// operations each where the plain state has one. sum1 needs positions only and runs beside the pair arithmetic as in
// k_lm_small; sum2 starts with the NEW acceleration (j = 0 comes first in the reference's loop, and the additions do not
// commute in the error part), so all of it sits behind the force.
template <int L>
__global__ void __launch_bounds__(kDoubleSmallThreads) k_lm_double_small(const LmDoubleArgs d, long long nsteps) {
    __shared__ __attribute__((aligned(16))) double U[kDoubleSmallRows][kDoubleSmallRow];    // [body*3 + comp][source]: sources after the body
    __shared__ __attribute__((aligned(16))) double Lw[kDoubleSmallRows][kDoubleSmallRow];   //                        sources before the body
    __shared__ __attribute__((aligned(32))) Body4 sP[kTile];
    const LmArgs &a = d.a;

    const int tid = threadIdx.x, n = a.n;
    // chain threads: tid = (body*3 + comp)*2 + half   (half 0 = sources before, 1 = sources after)
    const int chain = tid >> 1, half = tid & 1;
    const bool chain_thread = chain < 3 * n;
    const bool owner = chain_thread && half == 0;     // the (body, comp) thread: history, velocity, predictor
    const bool owner_wave = __builtin_amdgcn_readfirstlane(tid >> 6) <= ((6 * n - 1) >> 6);
    const int my_i = chain_thread ? chain / 3 : 0, cc = chain_thread ? chain % 3 : 0;
    const size_t lvl = (size_t)3 * a.npad;
    const size_t off = (size_t)cc * a.npad + my_i;
    const int npairs = n * (n - 1) / 2;

    const int nrow = (n + 15) & ~15;   // row length the chains walk (the padding holds zeros)
    for (int k = tid; k < kDoubleSmallRows * kDoubleSmallRow; k += blockDim.x) { (&U[0][0])[k] = 0.0; (&Lw[0][0])[k] = 0.0; }
    if (tid < kTile) sP[tid] = a.pos_cur[tid < n ? tid : n - 1];
    // yv[j] / ye[j] / av[j] = level (newest - j) on entry
    double yv[L], ye[L], av[L], wa[L], wb[L];
#pragma unroll
    for (int j = 0; j < L; ++j) {
        const int slot = (a.cur + j) % L;
        yv[j] = a.Y[slot * lvl + off];
        ye[j] = d.YE[slot * lvl + off];
        av[j] = a.A[slot * lvl + off];
        wa[j] = a.wa[j]; wb[j] = a.wb[j];
    }
    const double hh = a.hh;
    Dbl v{owner ? a.V[off] : 0.0, owner ? d.VE[off] : 0.0};
    // this thread's unordered pair (i < j), row-major over the strict upper triangle, decoded once. A slot without a pair runs
    // pair (0, 1) again and stores nothing: straight-line code.
    int pi0 = 0, pj0 = 1;
    if (tid < npairs) {
        int i = 0;
        while ((i + 1) * (2 * n - i - 2) / 2 <= tid) ++i;
        pi0 = i;
        pj0 = i + 1 + (tid - i * (2 * n - i - 1) / 2);
    }
    const bool live0 = tid < npairs;
    __syncthreads();

    // the pair phase of k_lm_small: every thread runs the arithmetic, the wrapper-free sequences first, the range test that
    // validates them behind them; `before_branch()` pins the owner waves' sum1 among the sequences
    auto pair = [&](const double4 &vi, const double4 &vj, auto &&before_branch) {
        const double dx = vj.x - vi.x, dy = vj.y - vi.y, dz = vj.z - vi.z;
        const double n2 = dx * dx + dy * dy + dz * dz;
        double ax, ay, az, bx, by, bz;
        {
            const PairDen den = pair_den<true>(n2);
            pair_apply<true>(den, dx, dy, dz, vj.w, ax, ay, az);
            pair_apply<true>(den, -dx, -dy, -dz, vi.w, bx, by, bz);
        }
        asm volatile("" : "+v"(ax), "+v"(ay), "+v"(az), "+v"(bx), "+v"(by), "+v"(bz));
        before_branch();
        if (__builtin_amdgcn_ballot_w64(!in_range(n2)) != 0) {
            const PairDen den = pair_den<false>(n2);
            pair_apply<false>(den, dx, dy, dz, vj.w, ax, ay, az);
            pair_apply<false>(den, -dx, -dy, -dz, vi.w, bx, by, bz);
        }
        if (live0) {
            U[pi0 * 3 + 0][pj0] = ax;
            U[pi0 * 3 + 1][pj0] = ay;
            U[pi0 * 3 + 2][pj0] = az;
            Lw[pj0 * 3 + 0][pi0] = bx;
            Lw[pj0 * 3 + 1][pi0] = by;
            Lw[pj0 * 3 + 2][pi0] = bz;
        }
    };

    // ---- predictor (ELM2::advance) of the first step, in the (body, comp) threads
    Dbl ynew{0.0, 0.0};
    if (owner) {
        ynew = lm_predict_double<L>(yv, ye, av, wa, wb, hh);
        reinterpret_cast<double *>(&sP[my_i])[cc] = ynew.value;        // the force reads `.value`
    }
    // One step with the history ring at rotation R: level (newest - j) lives in yv / ye / av[(R + j) % L]; the new level
    // overwrites the oldest in place. Cowell's velocity is formed once, for the last level of the launch (nothing reads it before).
    auto step = [&](auto rc, long long s) {
        constexpr int R = decltype(rc)::value;
        constexpr int Rn = (R + L - 1) % L;            // slot of the oldest level = slot of the level being built
        lds_barrier();     // positions of the new level visible
        const double4 vi = *reinterpret_cast<const double4 *>(&sP[pi0]), vj = *reinterpret_cast<const double4 *>(&sP[pj0]);
        Dbl s1{0.0, 0.0};                              // (set and read in the owner waves only)
        if (owner_wave) {
            // ---- sum1 of the NEXT level's predictor: this level's position and the L - 1 before it
            double ly[L], le[L];
            ly[0] = ynew.value; le[0] = ynew.error;
#pragma unroll
            for (int j = 1; j < L; ++j) { ly[j] = yv[(R + j - 1) % L]; le[j] = ye[(R + j - 1) % L]; }
            s1 = lm_sum1_double<L>(ly, le, wa);
            pair(vi, vj, [&]() { asm volatile("" : "+v"(s1.value), "+v"(s1.error)); });
        } else {
            pair(vi, vj, []() {});
        }
        lds_barrier();     // contributions visible
        // ---- ordered chains: plain in-order sums over the rows (zeros outside each chain's range)
        double acc = 0.0;
        if (chain_thread) {
            const double *row = half ? &U[chain][0] : &Lw[chain][0];
            auto sum_blocks = [&](auto nb) {
                constexpr int NB = decltype(nb)::value;
                double2 r[8 * NB];
#pragma unroll
                for (int k = 0; k < 8 * NB; ++k) r[k] = *reinterpret_cast<const double2 *>(row + 2 * k);
#pragma unroll
                for (int k = 0; k < 8 * NB; ++k) {
                    acc = acc + r[k].x;
                    acc = acc + r[k].y;
                }
            };
            if (nrow == 16) sum_blocks(std::integral_constant<int, 1>{});
            else sum_blocks(std::integral_constant<int, 2>{});
        }
        const double other = dpp_xor1(acc);            // the partner half sits in the adjacent lane
        if (owner) {
            double la[L];
            la[0] = acc + other;                       // ddy[i] (lower sum) += output_i (upper sum); Double{value, error: +0.0}
#pragma unroll
            for (int j = 1; j < L; ++j) la[j] = av[(R + j - 1) % L];
            const Dbl s2 = lm_sum2_double<L>(la, wb);
            const Dbl ynext = dbl_add(s1, dbl_mul(s2, hh));   // *y = *sum1 + *sum2 * (h * h * Ratio::from_recip(BETA_D))
            if (s < nsteps) reinterpret_cast<double *>(&sP[my_i])[cc] = ynext.value;
            if (s == nsteps)                               // Cowell::update_velocity of the launch's last level
                v = lm_cowell_double<L>(la, ynew, Dbl{yv[R], ye[R]}, a.cw, a.h, a.hc);
            yv[Rn] = ynew.value;
            ye[Rn] = ynew.error;
            av[Rn] = la[0];
            ynew = ynext;
        }
        // the predictor writes sP after every pair thread of this step passed the barrier above; U / Lw are
        // rewritten only after the next "positions visible" barrier
    };
    int rot = 0;                                       // rotation after the steps taken so far
    {
        long long s = 1;
        bool more = nsteps >= 1;
        while (more) double_small_steps(step, s, nsteps, rot, more, std::make_integer_sequence<int, L>{});
    }

    if (owner) {
        const int cur = (int)(((long long)a.cur - nsteps % L + L) % L);   // slot of the newest level after nsteps
#pragma unroll
        for (int p = 0; p < L; ++p) {                     // register p holds level (newest - j), j = (p - rot) mod L
            const int j = (p - rot + L) % L;
            const int slot = (cur + j) % L;
            a.Y[slot * lvl + off] = yv[p];
            d.YE[slot * lvl + off] = ye[p];
            a.A[slot * lvl + off] = av[p];
            if (j == 0) {
                reinterpret_cast<double *>(a.pos_next + my_i)[cc] = yv[p];
                reinterpret_cast<double *>(const_cast<Body4 *>(a.pos_cur) + my_i)[cc] = yv[p];
            }
        }
        a.V[off] = v.value;
        d.VE[off] = v.error;
    }
}

int lm_double_small(hipStream_t s, const LmDoubleArgs &d, int64_t nsteps) {
    if (d.a.n > kDoubleSmallMaxN) return EPH_ERR_UNSUPPORTED;
    if (d.a.L == 12) hipLaunchKernelGGL(k_lm_double_small<12>, dim3(1), dim3(kDoubleSmallThreads), 0, s, d, (long long)nsteps);
    else if (d.a.L == 13) hipLaunchKernelGGL(k_lm_double_small<13>, dim3(1), dim3(kDoubleSmallThreads), 0, s, d, (long long)nsteps);
    else return EPH_ERR_UNSUPPORTED;
    return launched("k_lm_double_small");
}

}  // namespace EPH_PV_NS
}  // namespace eph
