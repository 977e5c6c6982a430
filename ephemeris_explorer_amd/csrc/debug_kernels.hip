// debug_kernels.hip -- test hooks: the device halves (csrc/eph_debug.h) of eph_debug_pow / _div / _rsq and their kernels. Like
// debug_api.cpp, which holds the extern "C" entry points, linked into the test-hooks library and the tuning builds only.
#include "craft_device.h"
#include "eph_debug.h"
#include "host.h"

namespace eph {

__global__ void k_debug_pow(long long n, const double *__restrict__ x, double y, double *__restrict__ out) {
    const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) out[i] = cr_pow(x[i], y);
}

__global__ void k_debug_div(long long n, const double *__restrict__ a, const double *__restrict__ b,
                            double *__restrict__ fast, double *__restrict__ ieee) {
    const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    fast[i] = div_shared(a[i], b[i], rcp_refined(b[i]), in_range_div(b[i]));
    ieee[i] = a[i] / b[i];
}

int debug_div_device(int64_t n, const double *a, const double *b, double *fast, double *ieee) {
    EPH_GUARD_BEGIN
        if (n < 0 || (n > 0 && (!a || !b || !fast || !ieee))) return EPH_ERR_BAD_ARGUMENT;
        int st = check_device();
        if (st) return st;
        if (n == 0) return EPH_OK;
        DevBuf<double> da, db, df, di;
        if ((st = da.alloc(n)) || (st = db.alloc(n)) || (st = df.alloc(n)) || (st = di.alloc(n))) return st;
        EPH_HIP(hipMemcpy(da.p, a, sizeof(double) * n, hipMemcpyHostToDevice));
        EPH_HIP(hipMemcpy(db.p, b, sizeof(double) * n, hipMemcpyHostToDevice));
        EPH_LAUNCH("k_debug_div", k_debug_div, dim3((unsigned)((n + 255) / 256)), dim3(256), nullptr, (long long)n, da.p, db.p, df.p, di.p);
        EPH_HIP(hipMemcpy(fast, df.p, sizeof(double) * n, hipMemcpyDeviceToHost));
        EPH_HIP(hipMemcpy(ieee, di.p, sizeof(double) * n, hipMemcpyDeviceToHost));
        return EPH_OK;
    EPH_GUARD_END
}

// raw v_rsq_f64(x) and the h = 0.5 / sqrt(x) that the square root's coupled step leaves (the reciprocal's seed is 8 h^3):
// the two quantities the error-bound note of inv_r3_seeded (pair_term.h) starts from
__global__ void k_debug_rsq(long long n, const double *__restrict__ x, double *__restrict__ y, double *__restrict__ h1) {
    const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const double yy = __builtin_amdgcn_rsq(x[i]);
    const double g = x[i] * yy, h = yy * 0.5;
    const double r = __builtin_fma(-h, g, 0.5);
    y[i] = yy;
    h1[i] = __builtin_fma(h, r, h);
}
int debug_rsq_device(int64_t n, const double *x, double *rsq, double *h) {
    EPH_GUARD_BEGIN
        if (n < 0 || (n > 0 && (!x || !rsq || !h))) return EPH_ERR_BAD_ARGUMENT;
        int st = check_device();
        if (st) return st;
        if (n == 0) return EPH_OK;
        DevBuf<double> dx, dy, dh;
        if ((st = dx.alloc(n)) || (st = dy.alloc(n)) || (st = dh.alloc(n))) return st;
        EPH_HIP(hipMemcpy(dx.p, x, sizeof(double) * n, hipMemcpyHostToDevice));
        EPH_LAUNCH("k_debug_rsq", k_debug_rsq, dim3((unsigned)((n + 255) / 256)), dim3(256), nullptr, (long long)n, dx.p, dy.p, dh.p);
        EPH_HIP(hipMemcpy(rsq, dy.p, sizeof(double) * n, hipMemcpyDeviceToHost));
        EPH_HIP(hipMemcpy(h, dh.p, sizeof(double) * n, hipMemcpyDeviceToHost));
        return EPH_OK;
    EPH_GUARD_END
}

int debug_pow_device(int64_t n, const double *x, double y, double *out) {
    EPH_GUARD_BEGIN
        if (n < 0 || (n > 0 && (!x || !out))) return EPH_ERR_BAD_ARGUMENT;
        int st = check_device();
        if (st) return st;
        if (n == 0) return EPH_OK;
        DevBuf<double> dx, dout;
        if ((st = dx.alloc(n)) || (st = dout.alloc(n))) return st;
        EPH_HIP(hipMemcpy(dx.p, x, sizeof(double) * n, hipMemcpyHostToDevice));
        EPH_LAUNCH("k_debug_pow", k_debug_pow, dim3((unsigned)((n + 255) / 256)), dim3(256), nullptr, (long long)n, dx.p, y, dout.p);
        EPH_HIP(hipMemcpy(out, dout.p, sizeof(double) * n, hipMemcpyDeviceToHost));
        return EPH_OK;
    EPH_GUARD_END
}

}  // namespace eph
