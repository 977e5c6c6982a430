// craft_eval.hip -- where is every craft of a batch at epoch T, relative to body B: the batch-wide evaluator of the knot slabs a
// sweep leaves on the device (eph_craft_batch_eval). Reads the batch; changes nothing in it.
//
// Mirrors (paths relative to the reference repository root):
//   RelativeTrajectory::state_vector (reference first, `?`, one subtraction per component)   ephemeris/src/trajectory.rs:326-334
// over CubicHermiteSpline::state_vector and UniformSpline::state_vector, which are trajectory_eval.h's.
#include <algorithm>
#include <chrono>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <shared_mutex>

#include "craft_batch.h"
#include "trajectory_eval.h"

namespace eph {

// Shared epochs: the reference body's state is the same for every craft, so it is evaluated once per epoch, not once per lane.
__global__ void __launch_bounds__(64) k_craft_eval_reference(long long m, const double *__restrict__ at, int body,
                                                             const BodyEntry *__restrict__ bodies,
                                                             const double *__restrict__ coeffs, const int *__restrict__ ncoef,
                                                             double *__restrict__ ref /*[m][6]*/, uint8_t *__restrict__ ref_ok) {
    const long long e = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (e >= m) return;
    V3 p = {0.0, 0.0, 0.0}, v = {0.0, 0.0, 0.0};
    const bool ok = body_state_vector(BodyTable{bodies, coeffs, ncoef}, body, at[e], p, v);
    const double r[6] = {p.x, p.y, p.z, v.x, v.y, v.z};
#pragma unroll
    for (int d = 0; d < 6; ++d) ref[e * 6 + d] = ok ? r[d] : 0.0;
    ref_ok[e] = ok ? 1 : 0;
}

struct CraftEvalArgs {
    long long n;                 // craft = columns of the slabs
    int max_knots;
    const int *nknots;           // [craft]
    const int *perm;             // slab column -> craft (null: identity); the knot slabs' columns are lane positions
    const double *knot_t;        // [k][column]
    const double *knot_y;        // [k][6][column]
    long long m;                 // epochs of this pass
    const double *at;            // shared: [m]; per craft: [m][craft]
    int per_craft;
    int body;                    // reference body (table order) or -1
    const double *ref;           // shared epochs with a reference body: [m][6] and [m] from k_craft_eval_reference
    const uint8_t *ref_ok;
    BodyTable table;
    double *out_y;               // [m][6][column]
    uint8_t *inside;             // [m][column]
};

// One lane per slab COLUMN: the lanes of a wave read neighbouring words of a knot row wherever their knot indices agree; the
// craft-order translation happens once, at the copy to the caller (k_craft_eval_rows_out). One search per (craft, epoch); what was
// tried instead is told at hermite_state_vector (trajectory_eval.h).
__global__ void __launch_bounds__(256) k_craft_eval(const CraftEvalArgs a) {
    const long long col = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (col >= a.n) return;
    const long long n = a.n;
    const long long craft = a.perm ? a.perm[col] : col;
    const KnotColumn knots = {min(max(a.nknots[craft], 0), a.max_knots), n, a.knot_t + col, a.knot_y + col};
    for (long long e = 0; e < a.m; ++e) {
        const double x = a.per_craft ? a.at[e * n + craft] : a.at[e];
        V3 rp = {0.0, 0.0, 0.0}, rv = {0.0, 0.0, 0.0};
        bool ok = true;
        if (a.body >= 0) {                            // reference.state_vector(at)?   trajectory.rs:330
            if (a.per_craft) {
                ok = body_state_vector(a.table, a.body, x, rp, rv);
            } else {
                ok = a.ref_ok[e] != 0;
                rp = {a.ref[e * 6 + 0], a.ref[e * 6 + 1], a.ref[e * 6 + 2]};
                rv = {a.ref[e * 6 + 3], a.ref[e * 6 + 4], a.ref[e * 6 + 5]};
            }
        }
        V3 p = {0.0, 0.0, 0.0}, v = {0.0, 0.0, 0.0};
        ok = ok && hermite_state_vector(knots, x, p, v);
        if (ok && a.body >= 0) {                      // position - ref_position, velocity - ref_velocity
            p = sub(p, rp);
            v = sub(v, rv);
        }
        const double o[6] = {p.x, p.y, p.z, v.x, v.y, v.z};
#pragma unroll
        for (int d = 0; d < 6; ++d) a.out_y[(e * 6 + d) * n + col] = ok ? o[d] : 0.0;
        a.inside[e * n + col] = ok ? 1 : 0;
    }
}

// One pass of results from slab-column order on the device to craft order in the pinned staging buffer: gathered reads of device
// memory, every store to host memory coalesced.
__global__ void __launch_bounds__(256) k_craft_eval_rows_out(long long m, long long n, const int *__restrict__ slot_of,
                                                             const double *__restrict__ y, const uint8_t *__restrict__ in,
                                                             double *__restrict__ out_y, uint8_t *__restrict__ out_in) {
    const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const long long col = slot_of ? slot_of[i] : i;
    for (long long r = 0; r < m * 6; ++r) out_y[r * n + i] = y[r * n + col];
    if (out_in)
        for (long long e = 0; e < m; ++e) out_in[e * n + i] = in[e * n + col];
}

}  // namespace eph

using namespace eph;

#pragma GCC visibility push(default)
extern "C" {

int32_t eph_craft_batch_eval(eph_craft_batch *b, int64_t m, const double *at, int32_t per_craft, int32_t reference_body,
                             double *out_y, uint8_t *inside) {
    try {
        if (!b || m < 0 || (per_craft != 0 && per_craft != 1) || (m > 0 && !at) || (m > 0 && b->n > 0 && !out_y) ||
            reference_body < -1 || reference_body >= b->eph->n_bodies)
            return EPH_ERR_BAD_ARGUMENT;
        if (m == 0 || b->n == 0) return EPH_OK;
        const size_t n = (size_t)b->n;
        std::shared_lock<std::shared_mutex> table_lock(b->eph->mu, std::defer_lock);
        if (reference_body >= 0) table_lock.lock();
        EPH_HIP(hipSetDevice(b->device));
        // EPH_TRACE_CRAFT_EVAL=1 prints the call's kernel time and copy time (scripts/craft_eval_timing.py)
        const char *env = getenv("EPH_TRACE_CRAFT_EVAL");
        const bool trace = env && atoi(env) != 0;
        // passes over epochs: at most 256 MB of results each (one epoch at least), through one device block in slab-column order
        // and the pinned staging buffer in craft order
        const size_t epoch_bytes = n * (6 * sizeof(double) + 1);
        const long long per_pass = (long long)std::min<size_t>((size_t)m, std::max<size_t>(1, ((size_t)256 << 20) / epoch_bytes));
        const size_t y_count = (size_t)per_pass * 6 * n, in_count = (size_t)per_pass * n;
        DevBuf<double> d_at, d_y, d_ref;
        DevBuf<uint8_t> d_in, d_ref_ok;
        int st;
        if ((st = d_at.alloc(per_craft ? (size_t)per_pass * n : (size_t)m)) || (st = d_y.alloc(y_count)) || (st = d_in.alloc(in_count)))
            return st;
        const bool shared_ref = reference_body >= 0 && !per_craft;
        if (shared_ref && ((st = d_ref.alloc(6 * (size_t)m)) || (st = d_ref_ok.alloc((size_t)m)))) return st;
        PinnedStage stage(y_count * sizeof(double) + in_count);
        if (stage.status()) return stage.status();
        StreamIdleOnExit idle(b->stream);
        hipStream_t s = b->stream;
        hipError_t he;
        if (!per_craft) {
            EPH_HIP(hipMemcpyAsync(d_at.p, at, sizeof(double) * (size_t)m, hipMemcpyHostToDevice, s));
            if (shared_ref) {
                hipLaunchKernelGGL(k_craft_eval_reference, dim3((unsigned)((m + 63) / 64)), dim3(64), 0, s, (long long)m, d_at.p,
                                   (int)reference_body, b->eph->bodies.p, b->eph->coeffs.p, b->eph->ncoef.p, d_ref.p, d_ref_ok.p);
                if ((he = hipGetLastError()) != hipSuccess) { set_last_error("k_craft_eval_reference", he); return EPH_ERR_HIP; }
            }
        }
        const bool dealt = !b->h_slot.empty();          // the slabs' columns are lane positions (craft_sort)
        CraftEvalArgs a{};
        a.n = b->n; a.max_knots = b->max_knots; a.nknots = b->nknots.p; a.perm = dealt ? b->perm.p : nullptr;
        a.knot_t = b->knot_t.p; a.knot_y = b->knot_y.p;
        a.per_craft = per_craft; a.body = reference_body;
        a.table = {b->eph->bodies.p, b->eph->coeffs.p, b->eph->ncoef.p};
        a.out_y = d_y.p; a.inside = d_in.p;
        double *stage_y = static_cast<double *>(stage.dev());
        uint8_t *stage_in = reinterpret_cast<uint8_t *>(stage_y + y_count);
        const double *host_y = static_cast<const double *>(stage.host());
        const uint8_t *host_in = reinterpret_cast<const uint8_t *>(host_y + y_count);
        const dim3 grid((unsigned)((n + 255) / 256)), block(256);
        double kernel_ms = 0.0, copy_ms = 0.0;
        for (long long e0 = 0; e0 < m; e0 += per_pass) {
            const long long me = std::min<long long>(per_pass, m - e0);
            if (per_craft) EPH_HIP(hipMemcpyAsync(d_at.p, at + (size_t)e0 * n, sizeof(double) * (size_t)me * n, hipMemcpyHostToDevice, s));
            a.m = me;
            a.at = per_craft ? d_at.p : d_at.p + e0;
            a.ref = shared_ref ? d_ref.p + 6 * e0 : nullptr;
            a.ref_ok = shared_ref ? d_ref_ok.p + e0 : nullptr;
            if (trace) EPH_HIP(hipEventRecord(b->ev0, s));
            hipLaunchKernelGGL(k_craft_eval, grid, block, 0, s, a);
            if ((he = hipGetLastError()) != hipSuccess) { set_last_error("k_craft_eval", he); return EPH_ERR_HIP; }
            if (trace) EPH_HIP(hipEventRecord(b->ev1, s));
            hipLaunchKernelGGL(k_craft_eval_rows_out, grid, block, 0, s, me, (long long)n, dealt ? (const int *)b->slot_of.p : nullptr, (const double *)d_y.p,
                               (const uint8_t *)d_in.p, stage_y, inside ? stage_in : nullptr);
            if ((he = hipGetLastError()) != hipSuccess) { set_last_error("k_craft_eval_rows_out", he); return EPH_ERR_HIP; }
            EPH_HIP(hipStreamSynchronize(s));
            const auto c0 = std::chrono::steady_clock::now();
            std::memcpy(out_y + (size_t)e0 * 6 * n, host_y, sizeof(double) * (size_t)me * 6 * n);
            if (inside) std::memcpy(inside + (size_t)e0 * n, host_in, (size_t)me * n);
            if (trace) {
                float ms = 0.0f;
                EPH_HIP(hipEventElapsedTime(&ms, b->ev0, b->ev1));
                kernel_ms += ms;
                copy_ms += std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - c0).count();
            }
        }
        idle.disarm();
        if (trace)
            fprintf(stderr, "craft_eval: m %lld n %lld passes %lld kernel_ms %.4f host_copy_ms %.4f\n", (long long)m, (long long)n,
                    (long long)((m + per_pass - 1) / per_pass), kernel_ms, copy_ms);
        return EPH_OK;
    } catch (const std::bad_alloc &) { return EPH_ERR_OUT_OF_MEMORY; } catch (...) { return EPH_ERR_HIP; }
}

}  // extern "C"
#pragma GCC visibility pop
