// step_double_small.hip -- k_lm_double_small: the steady ELM2 steps of a `<Double>` handle (double_state.h) of at most 32 bodies
// in ONE workgroup, `nsteps` integrator steps per launch. A sibling of k_lm_small (step_small.hip), not a flag on it: the frame
// -- LDS rows, pair decode, pair phase, ordered row sums, step loop, ring slots -- is the frame of small_frame.h; what differs is
// the (body, component) thread, which carries the value AND the error part of the L history levels of y and runs the predictor
// on Double's operators. Compiled once per evaluation order of the point-mass term (pair_ns.h).
#include <initializer_list>
#include <type_traits>
#include <utility>

#include "pair_ns.h"
#include "double_state.h"

namespace eph {
namespace EPH_PV_NS {

#include "small_frame.h"

// What the owner thread of a (body, component) keeps for the whole launch: yv / ye / av[L] (value and error of y, acceleration)
// and the weights -- L + 2 doubles more than k_lm_small's (the error parts, the error of the level under construction, the
// velocity's). What its step costs more: sum1 and sum2 of ELM2::advance are chains of L Double additions, ten dependent f64
// operations each where the plain state has one. sum1 needs positions only and runs beside the pair arithmetic as in
// k_lm_small; sum2 starts with the NEW acceleration (j = 0 comes first in the reference's loop, and the additions do not
// commute in the error part), so all of it sits behind the force.
template <int L>
__global__ void __launch_bounds__(kSmallThreads) k_lm_double_small(const LmDoubleArgs d, long long nsteps) {
    __shared__ __attribute__((aligned(16))) double U[kSmallRows][kSmallRow];    // [body*3 + comp][source]: sources after the body
    __shared__ __attribute__((aligned(16))) double Lw[kSmallRows][kSmallRow];   //                        sources before the body
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
    small_zero_rows(U, Lw, tid);
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
    int pi0, pj0;                                      // this thread's unordered pair (i < j), decoded once
    small_decode(tid, n, npairs, pi0, pj0);
    const bool live0 = tid < npairs;
    __syncthreads();

    // the pair phase, one pair per thread; `before_branch()` pins the owner waves' sum1 among the wrapper-free sequences
    auto pair = [&](const double4 &vi, const double4 &vj, auto &&before_branch) {
        small_pair<false>(U, Lw, vi, vj, vi, vj, pi0, pj0, 0, 1, live0, false, before_branch);
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
        // ---- ordered chains: plain in-order sums over the rows; the partner half sits in the adjacent lane
        double acc = 0.0;
        if (chain_thread) acc = small_row_sum(half ? &U[chain][0] : &Lw[chain][0], nrow);
        const double other = dpp_xor1(acc);
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
        while (more) small_steps(step, s, nsteps, rot, more, std::make_integer_sequence<int, L>{});
    }

    if (owner) {
        const int cur = small_newest_slot<L>(a.cur, nsteps);
#pragma unroll
        for (int p = 0; p < L; ++p) {
            const int j = small_level<L>(p, rot);
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
    if (d.a.n > kSmallMaxN) return EPH_ERR_UNSUPPORTED;
    if (d.a.L == 12) hipLaunchKernelGGL(k_lm_double_small<12>, dim3(1), dim3(kSmallThreads), 0, s, d, (long long)nsteps);
    else if (d.a.L == 13) hipLaunchKernelGGL(k_lm_double_small<13>, dim3(1), dim3(kSmallThreads), 0, s, d, (long long)nsteps);
    else return EPH_ERR_UNSUPPORTED;
    return launched("k_lm_double_small");
}

}  // namespace EPH_PV_NS
}  // namespace eph
