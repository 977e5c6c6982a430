// step_srkn_small.hip -- k_srkn_small / k_srkn_double_small: the steps of a symplectic Runge-Kutta-Nystrom handle (SRKN::advance,
// integration/src/runge_kutta/nystrom/symplectic.rs:69-102) of at most 32 bodies in ONE workgroup, `nsteps` integrator steps of
// `stages` stages per launch -- one launch where the host loop of NBodyIntegration::srkn_step makes one (plain) or two (`<Double>`)
// per stage. Siblings of k_lm_small and k_lm_double_small on the frame of small_frame.h -- LDS rows, pair decode, pair phase,
// ordered row sums, partner exchange -- not a flag on either: a stage is a force evaluation and two multiply-adds per (body,
// component), there is no history ring and no predictor, so the (body, component) thread carries y, v and a (and the error parts of
// y and v on a compensated handle) and nothing runs beside the pair arithmetic. The two kernels differ in that state alone and
// share the stage loop through its type. All eight tables go through one instantiation: the stage count is a run-time value and
// the stage's two coefficients are read from the kernel arguments by the wave-uniform stage index (scalar loads, no register array).
// k_lm_startup_small, further down, runs the start-up of a linear multistep handle -- macro steps of four such steps, each closed
// by a force evaluation into the history ring -- on the same stage loop (srkn_small_step), alone or as a gang of one workgroup per
// system. k_srkn_small_many<SrknPlain> / <SrknDouble> are the step kernels' own gang form: a workgroup per system, each with its
// own step count.
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
    __device__ __forceinline__ void load(const SrknSmallArgs &a, size_t oy, size_t ov) { y = a.Y[oy]; v = a.V[ov]; }
    __device__ __forceinline__ void kick_drift(double acc, double hb, double ha) {
        v = v + acc * hb;                              // *dy = *dy + *ddy * (h * C::B[s])
        y = y + v * ha;                                // *y = *y + *dy * (h * C::A[s])   (ha == 0 still executes: v may be inf / NaN)
    }
    __device__ __forceinline__ double position() const { return y; }
    __device__ __forceinline__ void store_y(const SrknSmallArgs &a, size_t o) const { a.Y[o] = y; }
    __device__ __forceinline__ void store_v(const SrknSmallArgs &a, size_t o) const { a.V[o] = v; }
};
struct SrknDouble {                                    // kick_drift_double of double_state.h
    static constexpr bool kSamples = false;            // (eph_prop_create refuses a `<Double>` method)
    Dbl y{0.0, 0.0}, v{0.0, 0.0};
    __device__ __forceinline__ void load(const SrknSmallArgs &a, size_t oy, size_t ov) { y = Dbl{a.Y[oy], a.YE[oy]}; v = Dbl{a.V[ov], a.VE[ov]}; }
    __device__ __forceinline__ void kick_drift(double acc, double hb, double ha) {
        v = dbl_add(v, dbl_mul(dbl_acc(acc), hb));
        y = dbl_add(y, dbl_mul(v, ha));
    }
    __device__ __forceinline__ double position() const { return y.value; }        // the force reads `.value`
    __device__ __forceinline__ void store_y(const SrknSmallArgs &a, size_t o) const { a.Y[o] = y.value; a.YE[o] = y.error; }
    __device__ __forceinline__ void store_v(const SrknSmallArgs &a, size_t o) const { a.V[o] = v.value; a.VE[o] = v.error; }
};

// The roles of a thread in the frame, fixed for the launch.
// chain threads: tid = (body*3 + comp)*2 + half   (half 0 = sources before, 1 = sources after)
struct SrknRoles {
    int chain, half, my_i, cc;
    bool chain_thread, owner;                          // owner: the (body, comp) thread: y, v, a
    int nrow;                                          // row length the chains walk (the padding holds zeros)
    int npairs, pi0 = 0, pj0 = 1;                      // this thread's unordered pair (i < j), decoded once (decode)
    bool live0 = false;
    __device__ __forceinline__ explicit SrknRoles(int n) {
        const int tid = threadIdx.x;
        chain = tid >> 1; half = tid & 1;
        chain_thread = chain < 3 * n;
        owner = chain_thread && half == 0;
        my_i = chain_thread ? chain / 3 : 0; cc = chain_thread ? chain % 3 : 0;
        npairs = n * (n - 1) / 2;
        nrow = (n + 15) & ~15;
    }
    __device__ __forceinline__ void decode(int n) {
        const int tid = threadIdx.x;
        small_decode(tid, n, npairs, pi0, pj0);
        live0 = tid < npairs;
    }
};

// solout sampling schedule of the owner thread's body: the countdown of k_lm_small (SplineInterpolators::solout_with  nbody.rs:389-397)
struct SrknSampler {
    uint32_t m = 0, left = 0;
    uint64_t slot = 0;
    double *log = nullptr;
    __device__ __forceinline__ SrknSampler(const SampleArgs &sa, const SrknRoles &r, bool samples) {
        log = sa.log;
        if (samples && r.owner && sa.period) {
            m = sa.period[r.my_i];
            left = m ? m - sa.phase[r.my_i] % m : 0;
            slot = sa.offset[r.my_i];
        }
    }
    __device__ __forceinline__ void step_done(int cc, double position) {
        if (m && --left == 0) {
            log[slot * 3 + cc] = position;
            slot += 1;
            left = m;
        }
    }
};

// problem.ode.eval(t, &problem.state.y, ddy.zero()) at the positions in sP: the pair phase, this thread's ordered half-row sum and
// its partner's. The sum is the acceleration in the owner threads.
__device__ __forceinline__ double srkn_small_force(SmallRowsT &U, SmallRowsT &Lw, Body4 (&sP)[kTile], const SrknRoles &r) {
    lds_barrier();     // stage positions visible
    const double4 vi = *reinterpret_cast<const double4 *>(&sP[r.pi0]), vj = *reinterpret_cast<const double4 *>(&sP[r.pj0]);
    small_pair<false>(U, Lw, vi, vj, vi, vj, r.pi0, r.pj0, 0, 1, r.live0, false, []() {});
    lds_barrier();     // contributions visible
    double sum = 0.0;
    if (r.chain_thread) sum = small_row_sum(r.half ? &U[r.chain][0] : &Lw[r.chain][0], r.nrow);
    const double other = dpp_xor1(sum);                // the partner half sits in the adjacent lane
    return sum + other;                                // ddy[i] (lower sum) += output_i (upper sum)
}

// One SRKN step (symplectic.rs:69-102), the stage loop stated once for the step kernels and the start-up kernel. `acc` is the last
// evaluated acceleration (the FSAL carry), `taken` the steps the integrator has taken before this one.
template <typename State>
__device__ __forceinline__ void srkn_small_step(SmallRowsT &U, SmallRowsT &Lw, Body4 (&sP)[kTile], const SrknSmallArgs &a,
                                                const SrknRoles &r, State &st, double &acc, uint32_t taken) {
    const int stages = a.stages;
    const bool fsal = a.fsal != 0;
    for (int s = 0; s < stages; ++s) {
        // every stage but an FSAL table's first, which reuses the previous step's last acceleration once there is one (wave-uniform)
        if (!fsal || s > 0 || taken == 0) {
            const double f = srkn_small_force(U, Lw, sP, r);
            if (r.owner) acc = f;
        }
        if (r.owner) {
            st.kick_drift(acc, a.hb[s], a.ha[s]);
            // written after every pair thread of this stage passed the barrier above; read after the next one
            reinterpret_cast<double *>(&sP[r.my_i])[r.cc] = st.position();
        }
    }
}

template <typename State>
__device__ __forceinline__ void srkn_small_steps(SmallRowsT &U, SmallRowsT &Lw, Body4 (&sP)[kTile], const SrknSmallArgs &a,
                                                 long long nsteps) {
    const int tid = threadIdx.x, n = a.n;
    SrknRoles r(n);
    const size_t off = (size_t)r.cc * a.npad + r.my_i;
    small_zero_rows(U, Lw, tid);
    if (tid < kTile) sP[tid] = a.pos[0][tid < n ? tid : n - 1];
    State st;
    double acc = 0.0;                                  // the last evaluated acceleration: the FSAL carry, across launches in ASR
    if (r.owner) { st.load(a, off, off); acc = a.ASR[off]; }
    SrknSampler samp(a.samp, r, State::kSamples);
    r.decode(n);
    __syncthreads();

    uint32_t taken = a.starter_i;                      // SRKN.i
    for (long long step = 0; step < nsteps; ++step, ++taken) {
        srkn_small_step(U, Lw, sP, a, r, st, acc, taken);
        if constexpr (State::kSamples) samp.step_done(r.cc, st.position());
    }

    if (r.owner) {
        st.store_y(a, off);
        st.store_v(a, off);
        a.ASR[off] = acc;
        reinterpret_cast<double *>(a.pos[0] + r.my_i)[r.cc] = st.position();
        reinterpret_cast<double *>(a.pos[1] + r.my_i)[r.cc] = st.position();
    }
}

// k_lm_startup_small: `m` start-up macro steps of a linear multistep handle (LinearMultistepIntegrator::advance while
// starter.step_count() < ORDER, multistep/mod.rs:211-218) in one workgroup -- what NBodyIntegration::startup_macro_step queues as
// thirty launches per macro step. The working state is the ring's front: y and v stay in the owner thread, every macro step leaves its
// level (y, and the force there) in the slot that becomes the new front. a.Y / a.YE are the ring bases here and a.starter_i counts the
// substepper's steps. The same evaluations in the same order as the per-launch route: 1 + 25 m + 1 from a fresh handle.
template <typename State>
__device__ __forceinline__ void lm_startup_small(SmallRowsT &U, SmallRowsT &Lw, Body4 (&sP)[kTile], const LmStartupArgs &g) {
    const SrknSmallArgs &a = g.s;
    const int tid = threadIdx.x, n = a.n;
    SrknRoles r(n);
    const size_t off = (size_t)r.cc * a.npad + r.my_i, level = (size_t)3 * a.npad;
    small_zero_rows(U, Lw, tid);
    if (tid < kTile) sP[tid] = a.pos[0][tid < n ? tid : n - 1];
    const int L = g.L, substeps = g.substeps;
    int cur = g.cur;
    State st;
    double acc = 0.0;
    if (r.owner) { st.load(a, (size_t)cur * level + off, off); acc = a.ASR[off]; }
    SrknSampler samp(a.samp, r, State::kSamples);
    r.decode(n);
    __syncthreads();

    uint32_t taken = a.starter_i;
    if (taken == 0) {                                  // first call only: lm.advance_with(problem, no-op) -> current_ddy = f(y0)
        const double f = srkn_small_force(U, Lw, sP, r);
        if (r.owner) g.A[(size_t)cur * level + off] = f;
    }
    for (int d = 0; d < g.m; ++d) {
        // ring.front = (state, current_ddy): the level is built in the owner thread and lands in the slot in front of `cur`
        for (int q = 0; q < substeps; ++q, ++taken) srkn_small_step(U, Lw, sP, a, r, st, acc, taken);
        const double f = srkn_small_force(U, Lw, sP, r);   // current_ddy = f(y): evaluated, not taken from the FSAL carry
        cur = cur == 0 ? L - 1 : cur - 1;
        if (r.owner) {
            g.A[(size_t)cur * level + off] = f;
            st.store_y(a, (size_t)cur * level + off);
        }
        if constexpr (State::kSamples) samp.step_done(r.cc, st.position());
    }

    if (r.owner) {
        st.store_v(a, off);
        a.ASR[off] = acc;
        reinterpret_cast<double *>(a.pos[0] + r.my_i)[r.cc] = st.position();
        reinterpret_cast<double *>(a.pos[1] + r.my_i)[r.cc] = st.position();
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
// The gang form of the two kernels above (eph_nbody_advance_many, eph_prop_step_n_many): one workgroup per SYSTEM on the same
// srkn_small_steps, its arguments argv[blockIdx.x] -- the member's own system, table, step and STEP COUNT (every member stops at its
// own bound); nothing is shared between workgroups, and a grid above the CU count queues
template <typename State>
__global__ void __launch_bounds__(kSmallThreads) k_srkn_small_many(const SrknGangArgs *__restrict__ argv) {
    __shared__ __attribute__((aligned(16))) double U[kSmallRows][kSmallRow];
    __shared__ __attribute__((aligned(16))) double Lw[kSmallRows][kSmallRow];
    __shared__ __attribute__((aligned(32))) Body4 sP[kTile];
    const SrknGangArgs &g = argv[blockIdx.x];
    srkn_small_steps<State>(U, Lw, sP, g.s, g.nsteps);
}
// MANY: one workgroup per SYSTEM, its arguments argv[blockIdx.x] (eph_nbody_advance_many); nothing is shared between workgroups
template <typename State, bool MANY>
__global__ void __launch_bounds__(kSmallThreads) k_lm_startup_small(const LmStartupArgs a0, const LmStartupArgs *__restrict__ argv) {
    __shared__ __attribute__((aligned(16))) double U[kSmallRows][kSmallRow];
    __shared__ __attribute__((aligned(16))) double Lw[kSmallRows][kSmallRow];
    __shared__ __attribute__((aligned(32))) Body4 sP[kTile];
    lm_startup_small<State>(U, Lw, sP, MANY ? argv[blockIdx.x] : a0);
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
int srkn_small_many(hipStream_t s, const SrknGangArgs *argv_dev, int count) {
    hipLaunchKernelGGL((k_srkn_small_many<SrknPlain>), dim3((unsigned)count), dim3(kSmallThreads), 0, s, argv_dev);
    return launched("k_srkn_small_many");
}
int srkn_double_small_many(hipStream_t s, const SrknGangArgs *argv_dev, int count) {
    hipLaunchKernelGGL((k_srkn_small_many<SrknDouble>), dim3((unsigned)count), dim3(kSmallThreads), 0, s, argv_dev);
    return launched("k_srkn_small_many<Double>");
}
int lm_startup_small(hipStream_t s, const LmStartupArgs &a, bool compensated) {
    if (a.s.n > kSmallMaxN) return EPH_ERR_UNSUPPORTED;
    if (compensated) hipLaunchKernelGGL((k_lm_startup_small<SrknDouble, false>), dim3(1), dim3(kSmallThreads), 0, s, a, nullptr);
    else hipLaunchKernelGGL((k_lm_startup_small<SrknPlain, false>), dim3(1), dim3(kSmallThreads), 0, s, a, nullptr);
    return launched("k_lm_startup_small");
}
int lm_startup_small_many(hipStream_t s, const LmStartupArgs *argv_dev, int count) {
    static const LmStartupArgs none{};
    hipLaunchKernelGGL((k_lm_startup_small<SrknPlain, true>), dim3((unsigned)count), dim3(kSmallThreads), 0, s, none, argv_dev);
    return launched("k_lm_startup_small (gang)");
}

}  // namespace EPH_PV_NS
}  // namespace eph
