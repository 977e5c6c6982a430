// ephemeris_table.hip -- the LIVE device table behind an eph_ephemeris (ephemeris_table.h): layout, incremental follow-up of the host
// splines, and the eph_ephemeris_* entry points that create, grow, truncate, query and ship it.
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

// the reciprocal of every body's spline interval, formed once where the sweep kernels would form it (same instructions as
// LaneBody::r): the table entry carries it to spline_locate_fast
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
// polynomials [first, first + count) of body b's host spline -> device rows starting at `row`
static int eph_upload_rows(eph_ephemeris *e, int b, size_t first, size_t count, long long row) {
    if (count == 0) return EPH_OK;
    std::vector<double> co(count * kDiv * 3);
    std::vector<int> nc(count);
    const UniformSpline &u = e->splines[(size_t)b];
    for (size_t k = 0; k < count; ++k) eph_fill_row(u.polynomials[first + k], &co[k * kDiv * 3], &nc[k]);
    EPH_HIP(hipMemcpy(e->coeffs.p + (size_t)row * kDiv * 3, co.data(), sizeof(double) * co.size(), hipMemcpyHostToDevice));
    EPH_HIP(hipMemcpy(e->ncoef.p + row, nc.data(), sizeof(int) * nc.size(), hipMemcpyHostToDevice));
    return EPH_OK;
}
// host_bodies -> the device table (+ the refined reciprocals of the intervals, formed on the device like the sweep kernels would)
static int eph_upload_bodies(eph_ephemeris *e) {
    const int nb = e->n_bodies;
    for (int b = 0; b < nb; ++b) {
        const UniformSpline &u = e->splines[(size_t)b];
        BodyEntry &be = e->host_bodies[(size_t)b];
        be.start = u.start; be.interval = u.interval; be.mu = e->gm[(size_t)b];
        be.npoly = (long long)u.polynomials.size();
        be.span = u.interval * (double)u.polynomials.size();     // interval.scaled(len): the product UniformSpline::span() forms
        be.rinv = 0.0; be.rows = e->coeffs.p + (size_t)be.coeff_off * kDiv * 3;
    }
    if (!nb) return EPH_OK;
    EPH_HIP(hipMemcpy(e->bodies.p, e->host_bodies.data(), sizeof(BodyEntry) * (size_t)nb, hipMemcpyHostToDevice));
    EPH_LAUNCH("k_body_reciprocals", k_body_reciprocals, dim3((nb + 63) / 64), dim3(64), nullptr, nb, e->bodies.p);
    EPH_HIP(hipStreamSynchronize(nullptr));
    return EPH_OK;
}
// lay the table out afresh from the host splines: every body's region gets room for as many polynomials again behind it (and in
// front, for a body that grows backwards)
static int eph_rebuild(eph_ephemeris *e) {
    const int nb = e->n_bodies;
    e->host_bodies.assign((size_t)std::max(nb, 0), BodyEntry{});
    e->base.assign((size_t)nb, 0);
    e->cap.assign((size_t)nb, 0);
    long long total = 0;
    for (int b = 0; b < nb; ++b) {
        const long long np = (long long)e->splines[(size_t)b].polynomials.size();
        const long long room = std::max<long long>(np, 32);
        const long long front = e->grows_front[(size_t)b] ? room : 0;
        e->base[(size_t)b] = total;
        e->cap[(size_t)b] = front + np + room;
        e->host_bodies[(size_t)b].coeff_off = total + front;
        total += e->cap[(size_t)b];
    }
    DevBuf<double> co;
    DevBuf<int> nc;
    int st;
    if ((st = co.alloc((size_t)std::max<long long>(total, 1) * kDiv * 3)) || (st = nc.alloc((size_t)std::max<long long>(total, 1)))) return st;
    std::swap(e->coeffs.p, co.p); std::swap(e->coeffs.count, co.count);
    std::swap(e->ncoef.p, nc.p); std::swap(e->ncoef.count, nc.count);
    if (!e->bodies.p && (st = e->bodies.alloc((size_t)std::max(nb, 1)))) return st;
    for (int b = 0; b < nb; ++b)
        if ((st = eph_upload_rows(e, b, 0, e->splines[(size_t)b].polynomials.size(), e->host_bodies[(size_t)b].coeff_off))) return st;
    return eph_upload_bodies(e);
}
// the device table after the host splines changed: `back[b]` / `front[b]` polynomials were added behind / in front of body b,
// `dropped_front[b]` removed from its front (clear_before); a truncation (clear_after) needs no row traffic at all
static int eph_follow(eph_ephemeris *e, const std::vector<long long> &front, const std::vector<long long> &back,
                      const std::vector<long long> &dropped_front) {
    const int nb = e->n_bodies;
    bool fits = true;
    for (int b = 0; b < nb && fits; ++b) {
        const BodyEntry &be = e->host_bodies[(size_t)b];
        const long long off = be.coeff_off - e->base[(size_t)b] + dropped_front[(size_t)b];
        const long long np = (long long)e->splines[(size_t)b].polynomials.size();     // already the new count
        if (front[(size_t)b] > off || off - front[(size_t)b] + np > e->cap[(size_t)b]) fits = false;
    }
    if (!fits) return eph_rebuild(e);
    int st;
    for (int b = 0; b < nb; ++b) {
        BodyEntry &be = e->host_bodies[(size_t)b];
        be.coeff_off += dropped_front[(size_t)b] - front[(size_t)b];
        const size_t np = e->splines[(size_t)b].polynomials.size();
        if ((st = eph_upload_rows(e, b, 0, (size_t)front[(size_t)b], be.coeff_off))) return st;
        if ((st = eph_upload_rows(e, b, np - (size_t)back[(size_t)b], (size_t)back[(size_t)b], be.coeff_off + (long long)np - back[(size_t)b]))) return st;
    }
    return eph_upload_bodies(e);
}

// The host splines have changed already when the device table follows them: if the incremental update fails half way (a copy, an
// allocation), the table is laid out afresh from the host copy once before the error is reported, so that the two do not stay apart.
static int eph_follow_or_rebuild(eph_ephemeris *e, const std::vector<long long> &front, const std::vector<long long> &back,
                                 const std::vector<long long> &dropped_front) {
    const int st = eph_follow(e, front, back, dropped_front);
    if (st == EPH_OK) return st;
    (void)hipGetLastError();
    return eph_rebuild(e) == EPH_OK ? EPH_OK : st;
}

// UniformSpline::append (direction > 0) / prepend of `y` on body b's host spline (trajectory.rs:515-534, asserts checked by the caller);
// counts the polynomials added behind / in front for eph_follow
static void eph_splice(eph_ephemeris *e, size_t b, const UniformSpline &y, int direction, std::vector<long long> &front,
                       std::vector<long long> &back) {
    UniformSpline &x = e->splines[b];
    if (direction > 0) {
        x.polynomials.insert(x.polynomials.end(), y.polynomials.begin(), y.polynomials.end());
        back[b] = (long long)y.polynomials.size();
    } else {
        x.start = y.start;
        x.polynomials.insert(x.polynomials.begin(), y.polynomials.begin(), y.polynomials.end());
        front[b] = (long long)y.polynomials.size();
        if (front[b]) e->grows_front[b] = 1;
    }
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
        e->grows_front.assign((size_t)nb, 0);
        if ((st = eph_rebuild(e.get()))) return st;
        *out = e.release();
        return EPH_OK;
    EPH_GUARD_END
}
void eph_ephemeris_destroy(eph_ephemeris *e) { delete e; }

// UniformSpline::append (direction > 0) / prepend (< 0) for every body  trajectory.rs:515-534; the asserts become EPH_ERR_BAD_ARGUMENT
// with the table untouched
int32_t eph_ephemeris_append(eph_ephemeris *e, const eph_solution *tail, int32_t direction) {
    EPH_GUARD_BEGIN
        if (!e || !tail || direction == 0 || tail->s.splines.size() != e->splines.size()) return EPH_ERR_BAD_ARGUMENT;
        std::unique_lock<std::shared_mutex> lock(e->mu);
        const size_t nb = e->splines.size();
        for (size_t b = 0; b < nb; ++b) {
            const UniformSpline &x = e->splines[b], &y = tail->s.splines[b];
            if (y.ghost || x.interval != y.interval) return EPH_ERR_BAD_ARGUMENT;
            if (direction > 0 ? (x.end() != y.start) : (x.start != y.end())) return EPH_ERR_BAD_ARGUMENT;
        }
        EPH_HIP(hipSetDevice(e->device));
        std::vector<long long> front(nb, 0), back(nb, 0), none(nb, 0);
        for (size_t b = 0; b < nb; ++b) eph_splice(e, b, tail->s.splines[b], direction, front, back);
        e->revision += 1;
        return eph_follow_or_rebuild(e, front, back, none);
    EPH_GUARD_END
}
// UniformSpline::clear_before (after = 0, trajectory.rs:536-542) / clear_after (after != 0, :544-549) on body's spline or on all (body < 0)
int32_t eph_ephemeris_clear(eph_ephemeris *e, int32_t body, double at, int32_t after) {
    EPH_GUARD_BEGIN
        if (!e || body >= e->n_bodies) return EPH_ERR_BAD_ARGUMENT;
        std::unique_lock<std::shared_mutex> lock(e->mu);
        EPH_HIP(hipSetDevice(e->device));
        const size_t nb = e->splines.size();
        std::vector<long long> none(nb, 0), dropped(nb, 0);
        for (size_t b = 0; b < nb; ++b) {
            if (body >= 0 && (size_t)body != b) continue;
            UniformSpline &u = e->splines[b];
            const size_t before = u.polynomials.size();
            if (after) u.clear_after(at);
            else { u.clear_before(at); dropped[b] = (long long)(before - u.polynomials.size()); }
        }
        e->revision += 1;
        return eph_follow_or_rebuild(e, none, none, dropped);
    EPH_GUARD_END
}
// CelestialTrajectory::merge  ephemeris_explorer/src/dynamics/celestial.rs:198-204 (Forward: clear_after(propagated.start()) then
// append) and :220-226 (Backward: clear_before(propagated.end()) then prepend), body by body
int32_t eph_ephemeris_merge(eph_ephemeris *e, const eph_solution *propagated, int32_t direction) {
    EPH_GUARD_BEGIN
        if (!e || !propagated || direction == 0 || propagated->s.splines.size() != e->splines.size()) return EPH_ERR_BAD_ARGUMENT;
        std::unique_lock<std::shared_mutex> lock(e->mu);
        const size_t nb = e->splines.size();
        // the reference's asserts, evaluated on copies of the bounds first so that a refusal leaves the table untouched
        for (size_t b = 0; b < nb; ++b) {
            const UniformSpline &y = propagated->s.splines[b];
            UniformSpline x;
            x.start = e->splines[b].start; x.interval = e->splines[b].interval;
            x.ghost = e->splines[b].polynomials.size();            // bounds only: no polynomial is copied
            if (y.ghost || x.interval != y.interval) return EPH_ERR_BAD_ARGUMENT;
            if (direction > 0) {
                uint64_t idx;
                if (x.get_index_local(y.start - x.start, &idx) && idx < x.ghost) x.ghost = idx;       // clear_after
                if (x.end() != y.start) return EPH_ERR_BAD_ARGUMENT;
            } else {
                uint64_t idx;
                if (x.get_index_local_exclusive((y.end() + x.interval) - x.start, &idx)) {             // clear_before
                    x.start += x.interval * (double)idx;
                    x.ghost -= std::min<uint64_t>(idx, x.ghost);
                }
                if (x.start != y.end()) return EPH_ERR_BAD_ARGUMENT;
            }
        }
        EPH_HIP(hipSetDevice(e->device));
        std::vector<long long> front(nb, 0), back(nb, 0), dropped(nb, 0);
        for (size_t b = 0; b < nb; ++b) {
            UniformSpline &x = e->splines[b];
            const UniformSpline &y = propagated->s.splines[b];
            if (direction > 0) x.clear_after(y.start);
            else {
                const size_t before = x.polynomials.size();
                x.clear_before(y.end());
                dropped[b] = (long long)(before - x.polynomials.size());
            }
            eph_splice(e, b, y, direction, front, back);
        }
        e->revision += 1;
        return eph_follow_or_rebuild(e, front, back, dropped);
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
