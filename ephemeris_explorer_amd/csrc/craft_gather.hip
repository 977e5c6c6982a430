// craft_gather.hip -- eph_craft_batch_gather: a new batch whose craft are chosen craft of existing batches, bit for bit (the app's
// fleet changes while it flies: ephemeris_explorer/src/ui/windows/spawner.rs:136,367,408, ui/windows/body.rs:184-207; paths relative
// to the reference repository root). Removing, adding, splitting, merging, permuting and duplicating are special cases;
// eph_craft_batch_clone (craft.hip) is the identity case.
// The checks and the plan are gather_plan.h (a pure host value). The order of work follows from the deal: (1) the per-craft SoA arrays
// are gathered into craft order, (2) the output is dealt to the lanes from them by the creation rule (craft_sort), (3) the knot slabs
// move with both column maps known, the event slabs in craft order on both sides. One set of launches per source batch.
#include <algorithm>
#include <cstring>
#include <memory>
#include <shared_mutex>
#include <string>
#include <vector>

#include "craft_events.h"
#include "gather_plan.h"

namespace eph {

struct CraftScalars {          // the per-craft SoA arrays of one batch
    long long n;
    double *time, *y, *next_h, *klast, *kfirst, *last_knot, *t_start;
    unsigned *n_attempts, *rk_i, *steps;
    int *cur_seg, *status, *nknots;
    int *ev_seg, *ntr, *nap, *ev_status;      // events on
};
static CraftScalars craft_scalars(const eph_craft_batch *b) {
    return {b->n, b->time.p, b->y.p, b->next_h.p, b->klast.p, b->kfirst.p, b->last_knot.p, b->t_start.p, b->n_attempts.p, b->rk_i.p,
            b->steps.p, b->cur_seg.p, b->status.p, b->nknots.p, b->ev_seg.p, b->ntr.p, b->nap.p, b->ev_status.p};
}
// one lane per output craft of this source: craft out_of[l] of the output is craft craft_of[l] of the source. The 6-row arrays go as
// rows with the craft index fastest. cur_seg is relative to the craft's slice of the timeline CSR and ev_seg to its knots: both carry
// over unchanged.
__global__ void __launch_bounds__(256) k_gather_scalars(long long n_items, const long long *__restrict__ out_of,
                                                        const long long *__restrict__ craft_of, const CraftScalars s, const CraftScalars d,
                                                        int events) {
    const long long l = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (l >= n_items) return;
    const long long o = out_of[l], c = craft_of[l];
    d.time[o] = s.time[c];
    d.next_h[o] = s.next_h[c];
    d.last_knot[o] = s.last_knot[c];
    d.t_start[o] = s.t_start[c];
#pragma unroll
    for (int r = 0; r < 6; ++r) {
        d.y[r * d.n + o] = s.y[r * s.n + c];
        d.klast[r * d.n + o] = s.klast[r * s.n + c];
        d.kfirst[r * d.n + o] = s.kfirst[r * s.n + c];
    }
    d.n_attempts[o] = s.n_attempts[c];
    d.rk_i[o] = s.rk_i[c];
    d.steps[o] = s.steps[c];
    d.cur_seg[o] = s.cur_seg[c];
    d.status[o] = s.status[c];
    d.nknots[o] = s.nknots[c];
    if (events) {
        d.ev_seg[o] = s.ev_seg[c];
        d.ntr[o] = s.ntr[c];
        d.nap[o] = s.nap[c];
        d.ev_status[o] = s.ev_status[c];
    }
}
// The knot slabs: lane (blockIdx.x, threadIdx.x) owns output column lane_out[l], whose knots are column lane_src[l] of the source;
// the lanes are in output-column order, so a row's writes are coalesced, and its reads are wherever neighbouring output columns come
// from neighbouring source columns (identity, an ordered selection, a concatenation). Rows k < nknots of the craft only; blockIdx.y
// takes `rows` of them and threadIdx.y strides through those, so that a few long columns spread over the chip as many short ones do.
__global__ void __launch_bounds__(64) k_gather_knots(long long n_lanes, const long long *__restrict__ lane_out,
                                                     const long long *__restrict__ lane_src, const KnotSlabs src, const KnotSlabs dst,
                                                     double *__restrict__ dst_t, double *__restrict__ dst_y, int rows) {
    const long long l = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (l >= n_lanes) return;
    const long long oc = lane_out[l], sc = lane_src[l];
    const int nk = min(min(max(dst.nknots[dst.craft_of(oc)], 0), dst.max_knots), src.max_knots);
    const int k0 = (int)blockIdx.y * rows, k1 = min(k0 + rows, nk);
#pragma unroll 4
    for (int k = k0 + (int)threadIdx.y; k < k1; k += (int)blockDim.y) {
        const double t = src.knot_t[(long long)k * src.n + sc];
        double v[6];
#pragma unroll
        for (int r = 0; r < 6; ++r) v[r] = src.knot_y[((long long)k * 6 + r) * src.n + sc];
        dst_t[(long long)k * dst.n + oc] = t;
#pragma unroll
        for (int r = 0; r < 6; ++r) dst_y[((long long)k * 6 + r) * dst.n + oc] = v[r];
    }
}
// The event slabs, in craft order on both sides (craft_events.hip indexes them by craft): rows k < ntr of the transition columns and
// k < nap of the apsis columns; blockIdx.y takes `rows` of each.
__global__ void __launch_bounds__(256) k_gather_events(long long n_items, const long long *__restrict__ out_of,
                                                       const long long *__restrict__ craft_of, const EventArgs s, const EventArgs d, int rows) {
    const long long l = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (l >= n_items) return;
    const long long o = out_of[l], c = craft_of[l];
    const int ntr = min(min(max(s.ntr[c], 0), s.max_tr), d.max_tr), nap = min(min(max(s.nap[c], 0), s.max_ap), d.max_ap);
    const int k0 = (int)blockIdx.y * rows;
    for (int k = k0; k < min(k0 + rows, ntr); ++k) {
        d.tr_time[(long long)k * d.n_craft + o] = s.tr_time[(long long)k * s.n_craft + c];
        d.tr_body[(long long)k * d.n_craft + o] = s.tr_body[(long long)k * s.n_craft + c];
    }
    for (int k = k0; k < min(k0 + rows, nap); ++k) {
        d.ap_time[(long long)k * d.n_craft + o] = s.ap_time[(long long)k * s.n_craft + c];
        d.ap_dist[(long long)k * d.n_craft + o] = s.ap_dist[(long long)k * s.n_craft + c];
        d.ap_body[(long long)k * d.n_craft + o] = s.ap_body[(long long)k * s.n_craft + c];
        d.ap_kind[(long long)k * d.n_craft + o] = s.ap_kind[(long long)k * s.n_craft + c];
    }
}

// the coefficient table as bytes that depend on its values alone (padding zeroed): what gather_plan compares as "the method"
static ErkCoeffs canonical_method(const ErkCoeffs &rk) {
    ErkCoeffs c;
    std::memset(&c, 0, sizeof(c));
    c.stages = rk.stages; c.order = rk.order; c.order_embedded = rk.order_embedded; c.fsal = rk.fsal; c.has_embedded = rk.has_embedded;
    c.nystrom = rk.nystrom;
    std::memcpy(c.A, rk.A, sizeof(c.A)); std::memcpy(c.B, rk.B, sizeof(c.B)); std::memcpy(c.C, rk.C, sizeof(c.C));
    std::memcpy(c.E, rk.E, sizeof(c.E)); std::memcpy(c.A2, rk.A2, sizeof(c.A2)); std::memcpy(c.B2, rk.B2, sizeof(c.B2));
    std::memcpy(c.E2, rk.E2, sizeof(c.E2));
    return c;
}

// d_idx: four arrays of n_out entries -- output craft, source craft, then (gather_slabs) output column, source column -- in which
// source s owns [base[s], base[s] + items[s].size())
struct GatherWork {
    eph_craft_batch *out;
    eph_craft_batch *const *sources;
    const GatherPlan<SegmentDev> *plan;
    std::vector<long long> base;
    DevBuf<long long> d_idx;
    PassTrace trace_scalars, trace_slabs;     // EPH_TRACE_GATHER=1: the kernel time of step 1 and of step 3 (scripts/craft_gather_timing.py)
    GatherWork(eph_craft_batch *o, eph_craft_batch *const *s, const GatherPlan<SegmentDev> *p)
        : out(o), sources(s), plan(p), trace_scalars("EPH_TRACE_GATHER", o), trace_slabs("EPH_TRACE_GATHER", o) {}
};

// step 1: the per-craft arrays into craft order
static int gather_scalars(GatherWork &w) {
    eph_craft_batch *c = w.out;
    const size_t n = (size_t)c->n;
    PinnedStage stage(2 * n * sizeof(long long));
    if (stage.status()) return stage.status();
    StreamIdleOnExit idle(c->stream);
    long long *h = static_cast<long long *>(stage.host());
    for (size_t s = 0; s < w.plan->items.size(); ++s) {
        long long l = w.base[s];
        for (const GatherItem &it : w.plan->items[s]) { h[l] = it.out; h[n + (size_t)l] = it.craft; ++l; }
    }
    EPH_HIP(hipMemcpyAsync(w.d_idx.p, h, 2 * n * sizeof(long long), hipMemcpyHostToDevice, c->stream));
    int st;
    if ((st = w.trace_scalars.kernel_begin())) return st;
    const CraftScalars d = craft_scalars(c);
    for (size_t s = 0; s < w.plan->items.size(); ++s) {
        const long long m = (long long)w.plan->items[s].size();
        if (m == 0) continue;
        EPH_LAUNCH("k_gather_scalars", k_gather_scalars, dim3((unsigned)((m + 255) / 256)), dim3(256), c->stream, m, w.d_idx.p + w.base[s],
                   w.d_idx.p + n + w.base[s], craft_scalars(w.sources[s]), d, c->events ? 1 : 0);
    }
    if ((st = w.trace_scalars.kernel_end())) return st;
    EPH_HIP(hipStreamSynchronize(c->stream));
    idle.disarm();
    w.trace_scalars.copy_begin();
    return w.trace_scalars.copy_end();
}

// step 3: the slabs, with the output's deal known
static int gather_slabs(GatherWork &w) {
    eph_craft_batch *c = w.out;
    const size_t n = (size_t)c->n;
    PinnedStage stage(2 * n * sizeof(long long));
    if (stage.status()) return stage.status();
    StreamIdleOnExit idle(c->stream);
    long long *h = static_cast<long long *>(stage.host());
    const bool dealt = !c->h_slot.empty();
    std::vector<std::pair<long long, long long>> lanes;
    for (size_t s = 0; s < w.plan->items.size(); ++s) {
        lanes.clear();
        for (const GatherItem &it : w.plan->items[s]) lanes.emplace_back(dealt ? (long long)c->h_slot[(size_t)it.out] : it.out, it.col);
        if (dealt) std::sort(lanes.begin(), lanes.end());          // (undealt: the items are in output order already)
        long long l = w.base[s];
        for (const auto &p : lanes) { h[l] = p.first; h[n + (size_t)l] = p.second; ++l; }
    }
    EPH_HIP(hipMemcpyAsync(w.d_idx.p + 2 * n, h, 2 * n * sizeof(long long), hipMemcpyHostToDevice, c->stream));
    int st;
    if ((st = w.trace_slabs.kernel_begin())) return st;
    const KnotSlabs dst = knot_slabs(c);
    const EventArgs dev = c->events ? event_args(c) : EventArgs{};
    for (size_t s = 0; s < w.plan->items.size(); ++s) {
        const long long m = (long long)w.plan->items[s].size();
        if (m == 0) continue;
        const eph_craft_batch *b = w.sources[s];
        // columns by row chunks: enough blocks (of one wave) to fill the chip whatever the shape -- a block is cx columns wide and
        // 64 / cx rows deep, cx = 64 unless the source gives fewer columns
        unsigned cx = 64;
        while (cx > 1 && (long long)cx / 2 >= m) cx /= 2;
        const unsigned ry = 64 / cx;
        const long long bx = (m + cx - 1) / cx;
        const long long want = std::max<long long>(1, (8192 + bx - 1) / bx);
        const int depth = std::min(b->max_knots, c->max_knots);
        const long long chunks = std::min<long long>(std::min<long long>(want, 65535), std::max<long long>(1, (depth + (int)ry - 1) / (int)ry));
        const int rows = (int)((depth + chunks - 1) / chunks);
        EPH_LAUNCH("k_gather_knots", k_gather_knots, dim3((unsigned)bx, (unsigned)((depth + rows - 1) / rows)), dim3(cx, ry), c->stream, m,
                   w.d_idx.p + 2 * n + w.base[s], w.d_idx.p + 3 * n + w.base[s], knot_slabs(b), dst, c->knot_t.p, c->knot_y.p, rows);
        if (c->events) {
            const int edepth = std::max(std::min(b->max_tr, c->max_tr), std::min(b->max_ap, c->max_ap));
            const long long ebx = (m + 255) / 256;
            const long long echunks = std::min<long long>(std::max<long long>(1, (2048 + ebx - 1) / ebx), std::max(edepth, 1));
            const int erows = (int)((edepth + echunks - 1) / echunks);
            EPH_LAUNCH("k_gather_events", k_gather_events, dim3((unsigned)ebx, (unsigned)((edepth + erows - 1) / std::max(erows, 1))), dim3(256),
                       c->stream, m, w.d_idx.p + w.base[s], w.d_idx.p + n + w.base[s], event_args(b), dev, erows);
        }
    }
    if ((st = w.trace_slabs.kernel_end())) return st;
    EPH_HIP(hipStreamSynchronize(c->stream));
    idle.disarm();
    w.trace_slabs.copy_begin();
    return w.trace_slabs.copy_end();
}

}  // namespace eph

using namespace eph;

#pragma GCC visibility push(default)
extern "C" {

int32_t eph_craft_batch_gather(int32_t n_sources, eph_craft_batch *const *sources, int64_t n_out, const int32_t *source_of,
                               const int64_t *craft_of, eph_craft_batch **out) {
    EPH_GUARD_BEGIN
        if (out) *out = nullptr;
        // ---- everything that can be refused without a device ----
        std::string error;
        int st = gather_check_arguments(n_sources, reinterpret_cast<const void *const *>(sources), n_out, source_of, craft_of, out, error);
        if (st) { set_last_error_text(error); return st; }
        std::vector<GatherSource<SegmentDev>> src((size_t)n_sources);
        std::vector<ErkCoeffs> methods((size_t)n_sources);
        for (int s = 0; s < n_sources; ++s) {
            const eph_craft_batch *b = sources[s];
            GatherSource<SegmentDev> &g = src[(size_t)s];
            methods[(size_t)s] = canonical_method(b->rk);
            g.ephemeris = b->eph; g.method = &methods[(size_t)s]; g.method_bytes = sizeof(ErkCoeffs);
            g.params = b->params; g.pair_variant = b->pv; g.body_order = &b->body_order; g.retry = b->retry; g.events = b->events;
            g.n = b->n; g.max_knots = b->max_knots; g.max_tr = b->max_tr; g.max_ap = b->max_ap;
            g.slot = &b->h_slot; g.seg_off = &b->h_seg_off; g.segs = &b->h_segs;
        }
        const GatherPlan<SegmentDev> plan = gather_plan(src, n_out, source_of, craft_of);
        if (plan.status) { set_last_error_text(plan.error); return plan.status; }
        if ((st = check_device())) return st;
        // ---- the sources at rest; their sphere radii live on the device ----
        const eph_craft_batch *b0 = sources[0];
        EPH_HIP(hipSetDevice(b0->device));
        for (int s = 0; s < n_sources; ++s) EPH_HIP(hipStreamSynchronize(sources[s]->stream));
        const size_t nb = (size_t)std::max(b0->eph->n_bodies, 0);
        if (plan.events && n_sources > 1) {
            std::vector<std::vector<double>> soi((size_t)n_sources, std::vector<double>(nb));
            std::vector<const std::vector<double> *> view;
            for (int s = 0; s < n_sources; ++s) {
                if (nb) EPH_HIP(hipMemcpy(soi[(size_t)s].data(), sources[s]->soi.p, sizeof(double) * nb, hipMemcpyDeviceToHost));
                view.push_back(&soi[(size_t)s]);
            }
            const int differs = gather_soi_agree(view);
            if (differs >= 0) {
                set_last_error_text("gather: source " + std::to_string(differs) + " differs from source 0 in its soi radii");
                return EPH_ERR_BAD_ARGUMENT;
            }
        }
        // ---- built aside in a fresh batch; `out` is written on success only ----
        std::shared_lock<std::shared_mutex> table_lock(b0->eph->mu);       // (the deal to the lanes reads the table)
        std::unique_ptr<eph_craft_batch> c;
        if ((st = craft_batch_shell(*b0, n_out, plan.max_knots, c))) return st;       // source 0's settings, but the plan's:
        c->events = plan.events; c->max_tr = plan.max_tr; c->max_ap = plan.max_ap; c->retry = plan.retry;
        // `heterogeneous` only picks the queue form for an undealt batch. Set conservatively, not recomputed: true when a source says
        // so of its own craft or when the craft come from several batches, whose time scales nobody has compared.
        c->heterogeneous = n_sources > 1;
        for (int s = 0; s < n_sources; ++s) c->heterogeneous = c->heterogeneous || sources[s]->heterogeneous;
        const size_t n = (size_t)n_out;
        GatherWork w(c.get(), sources, &plan);
        if ((st = alloc_state(c.get(), n_out, plan.max_knots, plan.segs.size())) || (st = w.d_idx.alloc(4 * std::max<size_t>(n, 1))) ||
            (plan.events && (st = alloc_events(c.get(), plan.max_tr, plan.max_ap))))
            return st;
        {
            StreamIdleOnExit idle(c->stream);
            if (plan.events) EPH_HIP(hipMemcpyAsync(c->soi.p, b0->soi.p, sizeof(double) * c->soi.count, hipMemcpyDeviceToDevice, c->stream));
            if ((st = copy_buf(b0->bodies_ordered, c->bodies_ordered, c->stream))) return st;
            if ((st = copy_buf(b0->body_order_dev, c->body_order_dev, c->stream))) return st;
            EPH_HIP(hipMemcpy(c->rk_dev.p, &c->rk, sizeof(ErkCoeffs), hipMemcpyHostToDevice));
            EPH_HIP(hipMemcpy(c->seg_off.p, plan.seg_off.data(), sizeof(long long) * (n + 1), hipMemcpyHostToDevice));
            if (!plan.segs.empty())
                EPH_HIP(hipMemcpy(c->segs.p, plan.segs.data(), sizeof(SegmentDev) * plan.segs.size(), hipMemcpyHostToDevice));
            EPH_HIP(hipStreamSynchronize(c->stream));
            idle.disarm();
        }
        if (n > 0) {
            long long at = 0;
            for (const std::vector<GatherItem> &items : plan.items) { w.base.push_back(at); at += (long long)items.size(); }
            if ((st = gather_scalars(w))) return st;
            if ((st = craft_sort(c.get(), false))) return st;      // the creation rule, on the gathered current time and state
            if ((st = gather_slabs(w))) return st;
        }
        w.trace_scalars.report("gather_scalars", "craft", (long long)n_out, "sources", (long long)n_sources, 1);
        w.trace_slabs.report("gather_slabs", "craft", (long long)n_out, "sources", (long long)n_sources, 1);
        c->h_seg_off = plan.seg_off;
        c->h_segs = plan.segs;
        *out = c.release();
        return EPH_OK;
    EPH_GUARD_END
}

}  // extern "C"
#pragma GCC visibility pop
