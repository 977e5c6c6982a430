// step_srkn_small.hip -- k_srkn_small / k_srkn_double_small: the steps of a symplectic Runge-Kutta-Nystrom handle (SRKN::advance,
// integration/src/runge_kutta/nystrom/symplectic.rs:69-102) of at most 32 bodies in ONE workgroup, `nsteps` integrator steps of
// `stages` stages per launch -- one launch where the host loop of NBodyIntegration::srkn_step makes one (plain) or two (`<Double>`)
// per stage. Siblings of k_lm_small and k_lm_double_small on the frame of small_frame.h -- LDS rows, pair decode, pair phase,
// ordered row sums, partner exchange -- not a flag on either: a stage is a force evaluation and two multiply-adds per (body,
// component), there is no history ring and no predictor, so the (body, component) thread carries y, v and a (and the error parts of
// y and v on a compensated handle) and nothing runs beside the pair arithmetic. The two kernels differ in that state alone and
// share the stage loop through its type. All eight tables go through one instantiation: the stage count is a run-time value and
// the stage's two coefficients are read from the kernel arguments by the wave-uniform stage index (scalar loads, no register array).
// Compiled once per evaluation order of the point-mass term (pair_ns.h).
#include <initializer_list>
#include <type_traits>
#include <utility>

#include "pair_ns.h"
#include "double_state.h"

namespace eph {
namespace EPH_PV_NS {

#include "small_frame.h"

// What the owner thread of a (body, component) keeps for the whole launch, and the stage update on it.
struct SrknPlain {                                     // kick_drift_one of force_common.h / k_kick_drift of solout.hip
    static constexpr bool kSamples = true;
    double y = 0.0, v = 0.0;
    __device__ __forceinline__ void load(const SrknSmallArgs &a, size_t o) { y = a.Y[o]; v = a.V[o]; }
    __device__ __forceinline__ void kick_drift(double acc, double hb, double ha) {
        v = v + acc * hb;                              // *dy = *dy + *ddy * (h * C::B[s])
        y = y + v * ha;                                // *y = *y + *dy * (h * C::A[s])   (ha == 0 still executes: v may be inf / NaN)
    }
    __device__ __forceinline__ double position() const { return y; }
    __device__ __forceinline__ void store(const SrknSmallArgs &a, size_t o) const { a.Y[o] = y; a.V[o] = v; }
};
struct SrknDouble {                                    // kick_drift_double of double_state.h
    static constexpr bool kSamples = false;            // (eph_prop_create refuses a `<Double>` method)
    Dbl y{0.0, 0.0}, v{0.0, 0.0};
    __device__ __forceinline__ void load(const SrknSmallArgs &a, size_t o) { y = Dbl{a.Y[o], a.YE[o]}; v = Dbl{a.V[o], a.VE[o]}; }
    __device__ __forceinline__ void kick_drift(double acc, double hb, double ha) {
        v = dbl_add(v, dbl_mul(dbl_acc(acc), hb));
        y = dbl_add(y, dbl_mul(v, ha));
    }
    __device__ __forceinline__ double position() const { return y.value; }        // the force reads `.value`
    __device__ __forceinline__ void store(const SrknSmallArgs &a, size_t o) const {
        a.Y[o] = y.value; a.YE[o] = y.error;
        a.V[o] = v.value; a.VE[o] = v.error;
    }
};

template <typename State>
__device__ __forceinline__ void srkn_small_steps(SmallRowsT &U, SmallRowsT &Lw, Body4 (&sP)[kTile], const SrknSmallArgs &a,
                                                 long long nsteps) {
    const int tid = threadIdx.x, n = a.n;
    // chain threads: tid = (body*3 + comp)*2 + half   (half 0 = sources before, 1 = sources after)
    const int chain = tid >> 1, half = tid & 1;
    const bool chain_thread = chain < 3 * n;
    const bool owner = chain_thread && half == 0;     // the (body, comp) thread: y, v, a
    const int my_i = chain_thread ? chain / 3 : 0, cc = chain_thread ? chain % 3 : 0;
    const size_t off = (size_t)cc * a.npad + my_i;
    const int npairs = n * (n - 1) / 2;
    const int nrow = (n + 15) & ~15;   // row length the chains walk (the padding holds zeros)
    const int stages = a.stages;
    const bool fsal = a.fsal != 0;

    small_zero_rows(U, Lw, tid);
    if (tid < kTile) sP[tid] = a.pos[0][tid < n ? tid : n - 1];
    State st;
    double acc = 0.0;                                  // the last evaluated acceleration: the FSAL carry, across launches in ASR
    if (owner) { st.load(a, off); acc = a.ASR[off]; }
    // solout sampling schedule of this thread's body: the countdown of k_lm_small
    uint32_t samp_m = 0, samp_left = 0;
    uint64_t samp_slot = 0;
    double *samp_log = a.samp.log;
    if (State::kSamples && owner && a.samp.period) {
        samp_m = a.samp.period[my_i];
        samp_left = samp_m ? samp_m - a.samp.phase[my_i] % samp_m : 0;
        samp_slot = a.samp.offset[my_i];
    }
    int pi0, pj0;                                      // this thread's unordered pair (i < j), decoded once
    small_decode(tid, n, npairs, pi0, pj0);
    const bool live0 = tid < npairs;
    __syncthreads();

    uint32_t taken = a.starter_i;                      // SRKN.i
    for (long long step = 0; step < nsteps; ++step, ++taken) {
        for (int s = 0; s < stages; ++s) {
            // problem.ode.eval(t_stage, &problem.state.y, self.ddy.zero()): every stage but an FSAL table's first, which reuses the
            // previous step's last acceleration once there is one (wave-uniform)
            if (!fsal || s > 0 || taken == 0) {
                lds_barrier();     // stage positions visible
                const double4 vi = *reinterpret_cast<const double4 *>(&sP[pi0]), vj = *reinterpret_cast<const double4 *>(&sP[pj0]);
                small_pair<false>(U, Lw, vi, vj, vi, vj, pi0, pj0, 0, 1, live0, false, []() {});
                lds_barrier();     // contributions visible
                double sum = 0.0;
                if (chain_thread) sum = small_row_sum(half ? &U[chain][0] : &Lw[chain][0], nrow);
                const double other = dpp_xor1(sum);    // the partner half sits in the adjacent lane
                if (owner) acc = sum + other;          // ddy[i] (lower sum) += output_i (upper sum)
            }
            if (owner) {
                st.kick_drift(acc, a.hb[s], a.ha[s]);
                // written after every pair thread of this stage passed the barrier above; read after the next one
                reinterpret_cast<double *>(&sP[my_i])[cc] = st.position();
            }
        }
        if constexpr (State::kSamples) {
            if (samp_m && --samp_left == 0) {          // SplineInterpolators::solout_with  nbody.rs:389-397
                samp_log[samp_slot * 3 + cc] = st.position();
                samp_slot += 1;
                samp_left = samp_m;
            }
        }
    }

    if (owner) {
        st.store(a, off);
        a.ASR[off] = acc;
        reinterpret_cast<double *>(a.pos[0] + my_i)[cc] = st.position();
        reinterpret_cast<double *>(a.pos[1] + my_i)[cc] = st.position();
    }
}

__global__ void __launch_bounds__(kSmallThreads) k_srkn_small(const SrknSmallArgs a, long long nsteps) {
    __shared__ __attribute__((aligned(16))) double U[kSmallRows][kSmallRow];    // [body*3 + comp][source]: sources after the body
    __shared__ __attribute__((aligned(16))) double Lw[kSmallRows][kSmallRow];   //                        sources before the body
    __shared__ __attribute__((aligned(32))) Body4 sP[kTile];
    srkn_small_steps<SrknPlain>(U, Lw, sP, a, nsteps);
}
__global__ void __launch_bounds__(kSmallThreads) k_srkn_double_small(const SrknSmallArgs a, long long nsteps) {
    __shared__ __attribute__((aligned(16))) double U[kSmallRows][kSmallRow];
    __shared__ __attribute__((aligned(16))) double Lw[kSmallRows][kSmallRow];
    __shared__ __attribute__((aligned(32))) Body4 sP[kTile];
    srkn_small_steps<SrknDouble>(U, Lw, sP, a, nsteps);
}

int srkn_small(hipStream_t s, const SrknSmallArgs &a, int64_t nsteps) {
    if (a.n > kSmallMaxN) return EPH_ERR_UNSUPPORTED;
    hipLaunchKernelGGL(k_srkn_small, dim3(1), dim3(kSmallThreads), 0, s, a, (long long)nsteps);
    return launched("k_srkn_small");
}
int srkn_double_small(hipStream_t s, const SrknSmallArgs &a, int64_t nsteps) {
    if (a.n > kSmallMaxN) return EPH_ERR_UNSUPPORTED;
    hipLaunchKernelGGL(k_srkn_double_small, dim3(1), dim3(kSmallThreads), 0, s, a, (long long)nsteps);
    return launched("k_srkn_double_small");
}

}  // namespace EPH_PV_NS
}  // namespace eph
