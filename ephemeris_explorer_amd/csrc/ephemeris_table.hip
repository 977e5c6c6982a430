// ephemeris_table.hip -- the LIVE device table behind an eph_ephemeris (ephemeris_table.h): its one writer (plan, upload aside,
// commit), and the eph_ephemeris_* entry points that create, grow, truncate, query and ship it.
//
// Mirrors (paths relative to the reference repository root):
//   UniformSpline::{append, prepend, clear_before, clear_after, contains}   ephemeris/src/trajectory.rs:437-441,515-549
//   CelestialTrajectory::merge                          ephemeris_explorer/src/dynamics/celestial.rs:198-204,220-226
//   Bodies::is_valid_at, GravitationalBody.trajectory   ephemeris_explorer/src/dynamics/spacecraft.rs:52-74,199-201
#include <algorithm>
#include <cmath>
#include <cstring>
#include <memory>
#include <mutex>

#include "ephemeris_table.h"

namespace eph {

// the reciprocal of every body's spline interval, formed once, on the device the sweep kernels run on: the table entry carries it
// to spline_locate_fast and locate_spec, in every form of the sweep
__global__ void k_body_reciprocals(int n, BodyEntry *bodies) {
    const int b = blockIdx.x * blockDim.x + threadIdx.x;
    if (b >= n) return;
    const double iv = bodies[b].interval;
    // +0.0 = "take the plain IEEE lookup": the interval outside the guarded range of the shared-reciprocal division, or more than
    // 2^31 - 1 segments (the sweep's speculative lookup converts the segment count in 32 bits)
    bodies[b].rinv = in_range_div(iv) && (unsigned long long)bodies[b].npoly < 0x80000000ull ? rcp_refined(iv) : 0.0;
}

}  // namespace eph

using namespace eph;

// ---- the device table behind an eph_ephemeris ---------------------------------------------------------------------------
// one polynomial -> one zero-padded row of 8 x 3 doubles (rows >= ncoef stay +0.0: craft_rhs runs Horner over all kDiv rows)
static void eph_fill_row(const Polynomial &p, double *row, int *nc) {
    std::memset(row, 0, sizeof(double) * kDiv * 3);
    std::memcpy(row, &p.c[0][0], sizeof(double) * 3 * (size_t)std::min(std::max(p.ncoef, 0), kDiv));
    *nc = p.ncoef;
}
// What a writer is about to do to the host splines, decided before anything is touched: per body the counts (the plan's input)
// and the spline's start afterwards; `add` holds the incoming polynomials (null: a clear), which go behind (direction > 0) or in
// front. Nothing here changes the handle.
struct TableEdit {
    std::vector<BodyUpdate> up;
    std::vector<double> start;
    const std::vector<UniformSpline> *add = nullptr;
    int direction = 0;
    explicit TableEdit(const eph_ephemeris *e) : up(e->splines.size()), start(e->splines.size()) {
        for (size_t b = 0; b < start.size(); ++b) start[b] = e->splines[b].start;
    }
    void adds(const std::vector<UniformSpline> &ys, int dir) {
        add = &ys; direction = dir;
        for (size_t b = 0; b < up.size(); ++b) {
            (dir > 0 ? up[b].add_back : up[b].add_front) = (long long)ys[b].polynomials.size();
            if (dir < 0) start[b] = ys[b].start;
        }
    }
    // polynomial i of body b's spline as it will be: an incoming one, or one of the kept range of the host spline
    const Polynomial &at(const eph_ephemeris *e, size_t b, long long i) const {
        const BodyUpdate &u = up[b];
        const long long kept = (long long)e->splines[b].polynomials.size() - u.drop_front - u.drop_back;
        if (i < u.add_front) return (*add)[b].polynomials[(size_t)i];
        if (i >= u.add_front + kept) return (*add)[b].polynomials[(size_t)(i - u.add_front - kept)];
        return e->splines[b].polynomials[(size_t)(i - u.add_front + u.drop_front)];
    }
};
// one row range of the plan -> device rows of `coeffs` / `ncoef` (the table's own, or fresh ones nobody reads yet)
static int eph_upload_rows(const eph_ephemeris *e, const TableEdit &ed, const RowUpload &r, double *coeffs, int *ncoef) {
    const size_t count = (size_t)r.count;
    std::vector<double> co(count * kDiv * 3);
    std::vector<int> nc(count);
    for (size_t k = 0; k < count; ++k) eph_fill_row(ed.at(e, (size_t)r.body, r.first + (long long)k), &co[k * kDiv * 3], &nc[k]);
    EPH_HIP(hipMemcpy(coeffs + (size_t)r.row * kDiv * 3, co.data(), sizeof(double) * co.size(), hipMemcpyHostToDevice));
    EPH_HIP(hipMemcpy(ncoef + r.row, nc.data(), sizeof(int) * nc.size(), hipMemcpyHostToDevice));
    return EPH_OK;
}
// the entries of the table as it will be -> bodies_next (+ the refined reciprocals of the intervals, formed on the device like the
// sweep kernels would); complete on the device when this returns
static int eph_upload_bodies(eph_ephemeris *e, const TableEdit &ed, const std::vector<BodyRegion> &layout, const double *coeffs) {
    const int nb = e->n_bodies;
    if (!nb) return EPH_OK;
    std::vector<BodyEntry> host((size_t)nb);
    for (int b = 0; b < nb; ++b) {
        BodyEntry &be = host[(size_t)b];
        be.start = ed.start[(size_t)b]; be.interval = e->splines[(size_t)b].interval; be.mu = e->gm[(size_t)b];
        be.npoly = layout[(size_t)b].npoly;
        be.span = be.interval * (double)be.npoly;                // interval.scaled(len): the product UniformSpline::span() forms
        be.coeff_off = layout[(size_t)b].first_row();
        be.rinv = 0.0; be.rows = coeffs + (size_t)be.coeff_off * kDiv * 3;
    }
    EPH_HIP(hipMemcpy(e->bodies_next.p, host.data(), sizeof(BodyEntry) * (size_t)nb, hipMemcpyHostToDevice));
    EPH_LAUNCH("k_body_reciprocals", k_body_reciprocals, dim3((nb + 63) / 64), dim3(64), nullptr, nb, e->bodies_next.p);
    EPH_HIP(hipStreamSynchronize(nullptr));
    return EPH_OK;
}
// THE writer (ephemeris_table.h): plan from counts, do everything that can fail where no reader looks, commit. The caller holds the
// exclusive lock and has validated `ed`; any error return leaves the handle exactly as it was.
static int eph_write(eph_ephemeris *e, const TableEdit &ed) {
    const bool live = e->coeffs.p != nullptr;                    // (a table being created has no rows yet, and stays revision 0)
    TablePlan plan;
    plan.fits = false;
    if (live) plan = follow(e->layout, ed.up);
    const bool afresh = !plan.fits;
    DevBuf<double> co;
    DevBuf<int> nc;
    int st;
    if (afresh) {     // every body's region gets room for as many polynomials again, in buffers of their own
        std::vector<long long> npoly;
        std::vector<char> grows_front;
        counts_after(e->layout, ed.up, &npoly, &grows_front);
        plan = lay_out_afresh(npoly, grows_front);
        if ((st = co.alloc((size_t)std::max<long long>(plan.total, 1) * kDiv * 3)) || (st = nc.alloc((size_t)std::max<long long>(plan.total, 1)))) return st;
        const size_t nb = (size_t)std::max(e->n_bodies, 1);
        if (!live && ((st = e->bodies.alloc(nb)) || (st = e->bodies_next.alloc(nb)))) return st;
    }
    double *coeffs = afresh ? co.p : e->coeffs.p;
    int *ncoef = afresh ? nc.p : e->ncoef.p;
    for (const RowUpload &r : plan.uploads)
        if ((st = eph_upload_rows(e, ed, r, coeffs, ncoef))) return st;
    if ((st = eph_upload_bodies(e, ed, plan.regions, coeffs))) return st;
    // ---- commit: the insertions first (all bodies or none, host.h), then nothing that can fail
    if (ed.add) splines_splice(e->splines, *ed.add, ed.direction);
    for (size_t b = 0; b < e->splines.size(); ++b) {
        std::deque<Polynomial> &x = e->splines[b].polynomials;
        const BodyUpdate &u = ed.up[b];
        const auto kept_end = x.end() - (std::ptrdiff_t)u.add_back;
        x.erase(kept_end - (std::ptrdiff_t)u.drop_back, kept_end);       // (Polynomial is trivially copyable: closing the gap cannot throw)
        const auto kept_begin = x.begin() + (std::ptrdiff_t)u.add_front;
        x.erase(kept_begin, kept_begin + (std::ptrdiff_t)u.drop_front);
        e->splines[b].start = ed.start[b];
    }
    if (afresh) { e->coeffs.swap(co); e->ncoef.swap(nc); }
    e->bodies.swap(e->bodies_next);
    e->layout = std::move(plan.regions);
    if (live) e->revision += 1;
    return EPH_OK;
}

#pragma GCC visibility push(default)
extern "C" {

int32_t eph_ephemeris_create(const eph_solution *s, const double *mu, eph_ephemeris **out) {
    EPH_GUARD_BEGIN
        if (!s || !mu || !out) return EPH_ERR_BAD_ARGUMENT;
        int st = check_device();
        if (st) return st;
        std::unique_ptr<eph_ephemeris> e(new eph_ephemeris());
        EPH_HIP(hipGetDevice(&e->device));
        const int nb = (int)s->s.splines.size();
        e->n_bodies = nb;
        e->splines = s->s.splines;
        for (const UniformSpline &u : e->splines)
            if (u.ghost) return EPH_ERR_BAD_ARGUMENT;             // (only inside a propagator; never in a Solution handed out)
        e->gm.assign(mu, mu + nb);
        e->layout.assign((size_t)nb, BodyRegion{});              // no rows yet: the first write lays the table out
        for (int b = 0; b < nb; ++b) e->layout[(size_t)b].npoly = (long long)e->splines[(size_t)b].polynomials.size();
        if ((st = eph_write(e.get(), TableEdit(e.get())))) return st;
        *out = e.release();
        return EPH_OK;
    EPH_GUARD_END
}
void eph_ephemeris_destroy(eph_ephemeris *e) { delete e; }

// UniformSpline::append (direction > 0) / prepend (< 0) for every body  trajectory.rs:515-534; the asserts become EPH_ERR_BAD_ARGUMENT
// with the table untouched
int32_t eph_ephemeris_append(eph_ephemeris *e, const eph_solution *tail, int32_t direction) {
    EPH_GUARD_BEGIN
        if (!e || !tail || direction == 0) return EPH_ERR_BAD_ARGUMENT;
        std::unique_lock<std::shared_mutex> lock(e->mu);
        if (!splines_contiguous(e->splines, tail->s.splines, direction, true)) return EPH_ERR_BAD_ARGUMENT;
        EPH_HIP(hipSetDevice(e->device));
        TableEdit ed(e);
        ed.adds(tail->s.splines, direction > 0 ? 1 : -1);
        return eph_write(e, ed);
    EPH_GUARD_END
}
// UniformSpline::clear_before (after = 0, trajectory.rs:536-542) / clear_after (after != 0, :544-549) on body's spline or on all (body < 0)
int32_t eph_ephemeris_clear(eph_ephemeris *e, int32_t body, double at, int32_t after) {
    EPH_GUARD_BEGIN
        if (!e || body >= e->n_bodies) return EPH_ERR_BAD_ARGUMENT;
        std::unique_lock<std::shared_mutex> lock(e->mu);
        EPH_HIP(hipSetDevice(e->device));
        TableEdit ed(e);
        for (size_t b = 0; b < e->splines.size(); ++b) {
            if (body >= 0 && (size_t)body != b) continue;
            const UniformSpline &u = e->splines[b];
            const uint64_t np = u.polynomials.size();
            uint64_t idx;
            if (after) {                                                               // truncate(idx)
                if (u.get_index_local(at - u.start, &idx) && idx < np) ed.up[b].drop_back = (long long)(np - idx);
            } else if (u.get_index_local_exclusive((at + u.interval) - u.start, &idx)) {   // drain(0..idx)
                ed.start[b] = u.start + u.interval * (double)idx;
                ed.up[b].drop_front = (long long)std::min(idx, np);
            }
        }
        return eph_write(e, ed);
    EPH_GUARD_END
}
// CelestialTrajectory::merge  ephemeris_explorer/src/dynamics/celestial.rs:198-204 (Forward: clear_after(propagated.start()) then
// append) and :220-226 (Backward: clear_before(propagated.end()) then prepend), body by body
int32_t eph_ephemeris_merge(eph_ephemeris *e, const eph_solution *propagated, int32_t direction) {
    EPH_GUARD_BEGIN
        if (!e || !propagated || direction == 0 || propagated->s.splines.size() != e->splines.size()) return EPH_ERR_BAD_ARGUMENT;
        std::unique_lock<std::shared_mutex> lock(e->mu);
        const size_t nb = e->splines.size();
        TableEdit ed(e);
        // the reference's asserts, evaluated on copies of the bounds first so that a refusal leaves the table untouched; what the
        // clear drops is counted on the way
        for (size_t b = 0; b < nb; ++b) {
            const UniformSpline &y = propagated->s.splines[b];
            const uint64_t np = e->splines[b].polynomials.size();
            UniformSpline x;
            x.start = e->splines[b].start; x.interval = e->splines[b].interval;
            x.ghost = np;                                          // bounds only: no polynomial is copied
            if (y.ghost || x.interval != y.interval) return EPH_ERR_BAD_ARGUMENT;
            if (direction > 0) {
                uint64_t idx;
                if (x.get_index_local(y.start - x.start, &idx) && idx < x.ghost) x.ghost = idx;       // clear_after
                if (x.end() != y.start) return EPH_ERR_BAD_ARGUMENT;
                ed.up[b].drop_back = (long long)(np - x.ghost);
            } else {
                uint64_t idx;
                if (x.get_index_local_exclusive((y.end() + x.interval) - x.start, &idx)) {             // clear_before
                    x.start += x.interval * (double)idx;
                    x.ghost -= std::min<uint64_t>(idx, x.ghost);
                }
                if (x.start != y.end()) return EPH_ERR_BAD_ARGUMENT;
                ed.up[b].drop_front = (long long)(np - x.ghost);
            }
        }
        EPH_HIP(hipSetDevice(e->device));
        ed.adds(propagated->s.splines, direction > 0 ? 1 : -1);
        return eph_write(e, ed);
    EPH_GUARD_END
}
int32_t eph_ephemeris_info(const eph_ephemeris *e, int32_t body, double *start, double *interval, int64_t *npoly, uint64_t *revision) {
    if (!e || body >= e->n_bodies) return EPH_ERR_BAD_ARGUMENT;
    std::shared_lock<std::shared_mutex> lock(e->mu);
    if (body >= 0) {
        const UniformSpline &u = e->splines[(size_t)body];
        if (start) *start = u.start;
        if (interval) *interval = u.interval;
        if (npoly) *npoly = (int64_t)u.polynomials.size();
    } else if (start || interval || npoly) return EPH_ERR_BAD_ARGUMENT;
    if (revision) *revision = e->revision;
    return EPH_OK;
}
// Bodies::is_valid_at  dynamics/spacecraft.rs:199-201: every body's trajectory.contains(t) (trajectory.rs:437-441:
// local.is_positive() && local <= span -- ftime's Duration::is_positive is f64::is_sign_positive, duration.rs:78-80: the sign BIT,
// so the start itself (+0.0) is contained)
int32_t eph_ephemeris_is_valid_at(const eph_ephemeris *e, double t, int32_t *flag) {
    if (!e || !flag) return EPH_ERR_BAD_ARGUMENT;
    std::shared_lock<std::shared_mutex> lock(e->mu);
    bool all = true;
    for (const UniformSpline &u : e->splines) {
        const double local = t - u.start;
        all = all && (!std::signbit(local) && local <= u.span());
    }
    *flag = all ? 1 : 0;
    return EPH_OK;
}
// One contiguous, position-independent image of the table (what rank 0 broadcasts to the other ranks of a sweep):
// header, per body {start, interval, mu, npoly}, then every polynomial's zero-padded row and coefficient count.
namespace {
struct EphImageHeader { uint64_t magic, n_bodies, n_polys, reserved; };
constexpr uint64_t kEphImageMagic = 0x3130485045485045ull;     // "EPHEPH01"
struct EphImageBody { double start, interval, mu; int64_t npoly; };
}
int32_t eph_ephemeris_export(const eph_ephemeris *e, void *buf, uint64_t capacity, uint64_t *bytes) {
    EPH_GUARD_BEGIN
        if (!e || !bytes) return EPH_ERR_BAD_ARGUMENT;
        std::shared_lock<std::shared_mutex> lock(e->mu);
        uint64_t polys = 0;
        for (const UniformSpline &u : e->splines) polys += u.polynomials.size();
        const uint64_t need = sizeof(EphImageHeader) + sizeof(EphImageBody) * e->splines.size() +
                              polys * (sizeof(double) * kDiv * 3 + sizeof(int64_t));
        *bytes = need;
        if (!buf || capacity < need) return EPH_ERR_BAD_ARGUMENT;
        char *w = static_cast<char *>(buf);
        const EphImageHeader h{kEphImageMagic, (uint64_t)e->splines.size(), polys, 0};
        std::memcpy(w, &h, sizeof(h)); w += sizeof(h);
        for (size_t b = 0; b < e->splines.size(); ++b) {
            const UniformSpline &u = e->splines[b];
            const EphImageBody ib{u.start, u.interval, e->gm[b], (int64_t)u.polynomials.size()};
            std::memcpy(w, &ib, sizeof(ib)); w += sizeof(ib);
        }
        for (const UniformSpline &u : e->splines)
            for (const Polynomial &p : u.polynomials) {
                double row[kDiv * 3];
                int nc;
                eph_fill_row(p, row, &nc);
                const int64_t nc64 = nc;
                std::memcpy(w, row, sizeof(row)); w += sizeof(row);
                std::memcpy(w, &nc64, sizeof(nc64)); w += sizeof(nc64);
            }
        return EPH_OK;
    EPH_GUARD_END
}
int32_t eph_ephemeris_import(const void *buf, uint64_t bytes, eph_ephemeris **out) {
    EPH_GUARD_BEGIN
        if (!buf || !out || bytes < sizeof(EphImageHeader)) return EPH_ERR_BAD_ARGUMENT;
        *out = nullptr;
        const char *r = static_cast<const char *>(buf);
        EphImageHeader h;
        std::memcpy(&h, r, sizeof(h)); r += sizeof(h);
        if (h.magic != kEphImageMagic || h.n_bodies > 0x7fffffffu) return EPH_ERR_BAD_ARGUMENT;
        const uint64_t need = sizeof(EphImageHeader) + sizeof(EphImageBody) * h.n_bodies + h.n_polys * (sizeof(double) * kDiv * 3 + sizeof(int64_t));
        if (h.n_polys > (1ull << 40) || bytes < need) return EPH_ERR_BAD_ARGUMENT;
        eph_solution sol;
        std::vector<double> mu((size_t)h.n_bodies);
        sol.s.splines.resize((size_t)h.n_bodies);
        std::vector<int64_t> np((size_t)h.n_bodies);
        uint64_t total = 0;
        for (size_t b = 0; b < (size_t)h.n_bodies; ++b) {
            EphImageBody ib;
            std::memcpy(&ib, r, sizeof(ib)); r += sizeof(ib);
            if (ib.npoly < 0) return EPH_ERR_BAD_ARGUMENT;
            sol.s.splines[b].start = ib.start; sol.s.splines[b].interval = ib.interval;
            mu[b] = ib.mu; np[b] = ib.npoly; total += (uint64_t)ib.npoly;
        }
        if (total != h.n_polys) return EPH_ERR_BAD_ARGUMENT;
        for (size_t b = 0; b < (size_t)h.n_bodies; ++b)
            for (int64_t k = 0; k < np[b]; ++k) {
                Polynomial p;
                int64_t nc64;
                std::memcpy(&p.c[0][0], r, sizeof(double) * kDiv * 3); r += sizeof(double) * kDiv * 3;
                std::memcpy(&nc64, r, sizeof(nc64)); r += sizeof(nc64);
                if (nc64 < 0 || nc64 > kDiv) return EPH_ERR_BAD_ARGUMENT;
                p.ncoef = (int32_t)nc64;
                sol.s.splines[b].polynomials.push_back(p);
            }
        return eph_ephemeris_create(&sol, mu.data(), out);
    EPH_GUARD_END
}

}  // extern "C"
#pragma GCC visibility pop
