// craft_eval.hip -- where is every craft of a batch at epoch T, relative to body B: the batch-wide evaluator of the knot slabs a
// sweep leaves on the device (eph_craft_batch_eval). Reads the batch; changes nothing in it.
//
// Mirrors (paths relative to the reference repository root):
//   RelativeTrajectory::state_vector (reference first, `?`, one subtraction per component)   ephemeris/src/trajectory.rs:326-334
// over CubicHermiteSpline::state_vector and UniformSpline::state_vector, which are trajectory_eval.h's.
#include <algorithm>
#include <cstring>

#include "craft_batch.h"

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
    KnotSlabs slabs;
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
    if (col >= a.slabs.n) return;
    const long long n = a.slabs.n;
    const long long craft = a.slabs.craft_of(col);
    const KnotColumn knots = a.slabs.column(col, craft);
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
    EPH_GUARD_BEGIN
        if (!b || m < 0 || (per_craft != 0 && per_craft != 1) || (m > 0 && !at) || (m > 0 && b->n > 0 && !out_y) ||
            reference_body < -1 || reference_body >= b->eph->n_bodies)
            return EPH_ERR_BAD_ARGUMENT;
        if (m == 0 || b->n == 0) return EPH_OK;
        const size_t n = (size_t)b->n;
        const auto table_lock = table_lock_if(b->eph, reference_body >= 0);
        EPH_HIP(hipSetDevice(b->device));
        PassTrace trace("EPH_TRACE_CRAFT_EVAL", b);     // the call's kernel time and copy time (scripts/craft_eval_timing.py)
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
        const BodyTable table = body_table(b->eph);
        if (!per_craft) {
            EPH_HIP(hipMemcpyAsync(d_at.p, at, sizeof(double) * (size_t)m, hipMemcpyHostToDevice, s));
            if (shared_ref)
                EPH_LAUNCH("k_craft_eval_reference", k_craft_eval_reference, dim3((unsigned)((m + 63) / 64)), dim3(64), s, (long long)m,
                           d_at.p, (int)reference_body, table.bodies, table.coeffs, table.ncoef, d_ref.p, d_ref_ok.p);
        }
        const bool dealt = !b->h_slot.empty();          // the slabs' columns are lane positions (craft_sort)
        CraftEvalArgs a{};
        a.slabs = knot_slabs(b);
        a.per_craft = per_craft; a.body = reference_body;
        a.table = table;
        a.out_y = d_y.p; a.inside = d_in.p;
        double *stage_y = static_cast<double *>(stage.dev());
        uint8_t *stage_in = reinterpret_cast<uint8_t *>(stage_y + y_count);
        const double *host_y = stage.host_of(stage_y);
        const uint8_t *host_in = stage.host_of(stage_in);
        const dim3 grid((unsigned)((n + 255) / 256)), block(256);
        for (long long e0 = 0; e0 < m; e0 += per_pass) {
            const long long me = std::min<long long>(per_pass, m - e0);
            if (per_craft) EPH_HIP(hipMemcpyAsync(d_at.p, at + (size_t)e0 * n, sizeof(double) * (size_t)me * n, hipMemcpyHostToDevice, s));
            a.m = me;
            a.at = per_craft ? d_at.p : d_at.p + e0;
            a.ref = shared_ref ? d_ref.p + 6 * e0 : nullptr;
            a.ref_ok = shared_ref ? d_ref_ok.p + e0 : nullptr;
            if ((st = trace.kernel_begin())) return st;
            EPH_LAUNCH("k_craft_eval", k_craft_eval, grid, block, s, a);
            if ((st = trace.kernel_end())) return st;
            EPH_LAUNCH("k_craft_eval_rows_out", k_craft_eval_rows_out, grid, block, s, me, (long long)n,
                       dealt ? (const int *)b->slot_of.p : nullptr, (const double *)d_y.p, (const uint8_t *)d_in.p, stage_y,
                       inside ? stage_in : nullptr);
            EPH_HIP(hipStreamSynchronize(s));
            trace.copy_begin();
            std::memcpy(out_y + (size_t)e0 * 6 * n, host_y, sizeof(double) * (size_t)me * 6 * n);
            if (inside) std::memcpy(inside + (size_t)e0 * n, host_in, (size_t)me * n);
            if ((st = trace.copy_end())) return st;
        }
        idle.disarm();
        trace.report("craft_eval", "m", (long long)m, "n", (long long)n, (long long)((m + per_pass - 1) / per_pass));
        return EPH_OK;
    EPH_GUARD_END
}

}  // extern "C"
#pragma GCC visibility pop
