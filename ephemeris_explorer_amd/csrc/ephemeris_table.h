// ephemeris_table.h -- struct eph_ephemeris, the LIVE device table of the massive bodies' piecewise-polynomial ephemeris, for the units
// that bind to one: ephemeris_table.hip (the only writer), the craft_*.hip units, evaluators.hip.
#pragma once
#include <cstdint>
#include <shared_mutex>
#include <vector>

#include "host.h"
#include "trajectory_eval.h"

// The device-resident Vec<UniformSpline> of the massive bodies. LIVE, like the reference's: GravitationalBody.trajectory is
// Trajectory(Arc<RwLock<PredictionTrajectory>>) (ephemeris_explorer/src/dynamics/spacecraft.rs:52-74, dynamics/mod.rs:84-85), merged
// N-body snapshots grow it (dynamics/celestial.rs:198-204,220-226 -> UniformSpline::append / prepend / clear_*,
// ephemeris/src/trajectory.rs:515-549) and every spacecraft propagator holding the context sees the new extent at its next
// evaluation. Here: `splines` is the authoritative host copy (the reference's own operations, host.h), the device table follows it
// incrementally -- body b owns rows [base[b], base[b] + cap[b]) of `coeffs` / `ncoef` with its polynomials at coeff_off .. +npoly, so
// an append uploads the new rows only and a clear moves two integers; a region that overflows re-lays the table with headroom
// proportional to its size (amortised O(1) per polynomial). `mu` is the RwLock: sweeps, plots and scans hold it shared for the
// whole (synchronous) call, append / clear exclusively -- a writer never changes rows a kernel is reading.
// Only ephemeris_table.hip writes host_bodies, base, cap, coeffs, ncoef (eph_rebuild / eph_follow are file-local there); every
// other unit reads bodies, coeffs, ncoef, n_bodies (and the host copy) under `mu`.
struct eph_ephemeris {
    int device = 0;
    int n_bodies = 0;
    mutable std::shared_mutex mu;
    uint64_t revision = 0;                     // bumped by every append / clear
    std::vector<eph::UniformSpline> splines;
    std::vector<double> gm;
    eph::DevBuf<eph::BodyEntry> bodies;
    eph::DevBuf<double> coeffs;
    eph::DevBuf<int> ncoef;
    std::vector<eph::BodyEntry> host_bodies;   // what `bodies` holds (rinv: filled on the device only)
    std::vector<long long> base, cap;          // body b's region of rows
    std::vector<char> grows_front;             // body b has been prepended to: keep headroom in front as well
};

namespace eph {
inline BodyTable body_table(const eph_ephemeris *e) { return {e->bodies.p, e->coeffs.p, e->ncoef.p}; }   // what a kernel reads, under `mu`
// the read lock of a call that reads the table only when one of its requests names a body: held if `reads_a_body`
inline std::shared_lock<std::shared_mutex> table_lock_if(const eph_ephemeris *e, bool reads_a_body) {
    return reads_a_body ? std::shared_lock<std::shared_mutex>(e->mu) : std::shared_lock<std::shared_mutex>();
}
}  // namespace eph
