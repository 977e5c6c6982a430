// ephemeris_table.h -- struct eph_ephemeris, the LIVE device table of the massive bodies' piecewise-polynomial ephemeris, for the units
// that bind to one: ephemeris_table.hip (the only writer), the craft_*.hip units, evaluators.hip.
#pragma once
#include <cstdint>
#include <shared_mutex>
#include <vector>

#include "host.h"
#include "table_layout.h"
#include "trajectory_eval.h"

// The device-resident Vec<UniformSpline> of the massive bodies. LIVE, like the reference's: GravitationalBody.trajectory is
// Trajectory(Arc<RwLock<PredictionTrajectory>>) (ephemeris_explorer/src/dynamics/spacecraft.rs:52-74, dynamics/mod.rs:84-85), merged
// N-body snapshots grow it (dynamics/celestial.rs:198-204,220-226 -> UniformSpline::append / prepend / clear_*,
// ephemeris/src/trajectory.rs:515-549) and every spacecraft propagator holding the context sees the new extent at its next
// evaluation. Here: `splines` is the authoritative host copy (the reference's own operations, host.h), the device table follows it
// incrementally -- body b owns a region of rows of `coeffs` / `ncoef` with its polynomials somewhere inside (`layout`, table_layout.h),
// so an append uploads the new rows only and a clear moves two integers; a region that overflows re-lays the table with headroom
// proportional to its size (amortised O(1) per polynomial). `mu` is the RwLock: sweeps, plots and scans hold it shared for the
// whole (synchronous) call, the writers exclusively -- a writer never changes rows a kernel is reading.
//
// EVERY WRITER EITHER COMPLETES OR CHANGES NOTHING. Under the exclusive lock it validates, plans from counts alone
// (table_layout.h), does everything that can fail into memory no reader can see -- new rows into headroom outside every published
// [first_row, first_row + npoly), or into fresh `coeffs` / `ncoef` held in locals when the table is laid out afresh; the BodyEntry
// array, reciprocals and synchronisation included, into `bodies_next` -- and only then commits with operations that cannot fail
// half way: splice the host splines, swap the buffers (DevBuf::swap), store the layout, bump `revision`.
// The invariant: after any error return from a writer, the host splines, layout, device buffers, `bodies` pointer and `revision`
// are exactly what they were before the call.
// Only ephemeris_table.hip writes these members; every other unit reads bodies, coeffs, ncoef, n_bodies (and the host copy) under
// `mu`, taking `bodies.p` afresh on every call (the writers swap which of the two entry arrays is current).
struct eph_ephemeris {
    int device = 0;
    int n_bodies = 0;
    mutable std::shared_mutex mu;
    uint64_t revision = 0;                     // bumped by every append / merge / clear
    std::vector<eph::UniformSpline> splines;
    std::vector<double> gm;
    eph::DevBuf<eph::BodyEntry> bodies;        // what `layout` and `splines` say, as the kernels read it
    eph::DevBuf<eph::BodyEntry> bodies_next;   // where the next writer builds its entries before it swaps the two
    eph::DevBuf<double> coeffs;
    eph::DevBuf<int> ncoef;
    std::vector<eph::BodyRegion> layout;       // body b's region of rows and its polynomials' place in it
};

namespace eph {
inline BodyTable body_table(const eph_ephemeris *e) { return {e->bodies.p, e->coeffs.p, e->ncoef.p}; }   // what a kernel reads, under `mu`
// the read lock of a call that reads the table only when one of its requests names a body: held if `reads_a_body`
inline std::shared_lock<std::shared_mutex> table_lock_if(const eph_ephemeris *e, bool reads_a_body) {
    return reads_a_body ? std::shared_lock<std::shared_mutex>(e->mu) : std::shared_lock<std::shared_mutex>();
}
}  // namespace eph
