// double_step.hip -- the per-step kernels of a `<Double>` handle (double_state.h) that contain no point-mass term (compiled
// once): every case the single-workgroup kernel of step_double_small.hip does not serve -- more than 32 bodies, the start-up's
// SRKN substeps, SRKN methods, path 1. Correctness first: the force is the plain handle's force-only launch (values in, values
// out), and the compensated element-wise work of a step follows it in one launch, thread per (component, body).
#include "double_state.h"

namespace eph {

// One steady ELM2 step of a `<Double>` handle is   launch_accel(level cur) ; k_lm_double_step(level cur).
//   do_cowell : Cowell::update_velocity for level a.cur (its acceleration is in A[cur], the level before it in slot cur + 1)
//   do_predict: ELM2::advance's predictor for the level after a.cur, into ring slot cur - 1 (the oldest level's, read before
//               it is written: every thread owns its (component, body) of every level) and into the packed positions
template <int L>
__global__ void __launch_bounds__(256) k_lm_double_step(const LmDoubleArgs d) {
    const LmArgs &a = d.a;
    const int t = blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= 3 * a.n) return;
    const int my_i = t / 3, cc = t % 3;
    const size_t lvl = (size_t)3 * a.npad;
    const size_t off = (size_t)cc * a.npad + my_i;
    double yv[L], ye[L], av[L];
#pragma unroll
    for (int j = 0; j < L; ++j) {
        const int slot = (a.cur + j) % L;
        yv[j] = a.Y[slot * lvl + off];
        ye[j] = d.YE[slot * lvl + off];
        av[j] = a.A[slot * lvl + off];
    }
    if (d.do_cowell) {
        const Dbl v = lm_cowell_double<L>(av, Dbl{yv[0], ye[0]}, Dbl{yv[1], ye[1]}, a.cw, a.h, a.hc);
        a.V[off] = v.value;
        d.VE[off] = v.error;
    }
    if (a.do_predict) {
        const Dbl ynext = lm_predict_double<L>(yv, ye, av, a.wa, a.wb, a.hh);
        const int nslot = (a.cur + L - 1) % L;
        a.Y[(size_t)nslot * lvl + off] = ynext.value;
        d.YE[(size_t)nslot * lvl + off] = ynext.error;
        reinterpret_cast<double *>(a.pos_next + my_i)[cc] = ynext.value;   // mu is already in both packed buffers
    }
}

__global__ void __launch_bounds__(256) k_kick_drift_double(int n, int npad, const KickDriftDouble kd) {
    const int t = blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= 3 * n) return;
    const int body = t / 3, comp = t % 3;
    kick_drift_double(kd, (size_t)comp * npad + body, body, comp);
}

int launch_lm_double_step(hipStream_t s, const LmDoubleArgs &d) {
    if (d.a.n <= 0 || (!d.do_cowell && !d.a.do_predict)) return EPH_OK;
    const dim3 grid((3 * d.a.n + 255) / 256), block(256);
    if (d.a.L == 12) EPH_LAUNCH("k_lm_double_step", k_lm_double_step<12>, grid, block, s, d);
    else if (d.a.L == 13) EPH_LAUNCH("k_lm_double_step", k_lm_double_step<13>, grid, block, s, d);
    else return EPH_ERR_UNSUPPORTED;
    return EPH_OK;
}
int launch_kick_drift_double(hipStream_t s, int n, int npad, const KickDriftDouble &kd) {
    if (n <= 0) return EPH_OK;
    EPH_LAUNCH("k_kick_drift_double", k_kick_drift_double, dim3((3 * n + 255) / 256), dim3(256), s, n, npad, kd);
    return EPH_OK;
}

}  // namespace eph
