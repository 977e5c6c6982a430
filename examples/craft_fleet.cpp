// examples/craft_fleet.cpp -- a fleet whose ships are spawned and deleted between propagate legs while the others fly on, kept in ONE
// SpacecraftBatch: the app spawns ships (ephemeris_explorer/src/ui/windows/spawner.rs:136,367,408) and deletes them
// (ui/windows/body.rs:184-207) while every ship owns its propagator. Spawn = gather the fleet with a one-ship batch, delete = select
// the others (include/ephemeris_amd.hpp: SpacecraftBatch::concat / select over eph_craft_batch_gather). Every ship is also flown
// alone in a batch of its own through the same legs; at the end the digests (FNV-1a over the bits of status, state, next step size
// and every knot) must be equal ship by ship.
//
//   g++ -std=c++17 -Iinclude examples/craft_fleet.cpp -Lephemeris_explorer_amd -lephemeris_amd -Wl,-rpath,$PWD/ephemeris_explorer_amd -o craft_fleet
//   ./craft_fleet     (needs an MI355X; without a device the first compute call throws Error{EPH_ERR_NO_DEVICE}: exit 77)
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <memory>
#include <string>

#include "ephemeris_amd.hpp"

namespace ea = ephemeris_amd;

static uint64_t fnv(uint64_t h, const void *p, size_t bytes) {
    const unsigned char *c = static_cast<const unsigned char *>(p);
    for (size_t i = 0; i < bytes; ++i) h = (h ^ c[i]) * 1099511628211ull;
    return h;
}
static uint64_t digest(const ea::SpacecraftBatch &b, int64_t craft) {
    std::vector<double> t, next_h, kt;
    std::vector<ea::DVec3> pos, vel, kp, kv;
    std::vector<int32_t> nknots;
    const std::vector<int32_t> status = b.status(&nknots);
    b.state(t, pos, vel, &next_h);
    const size_t c = static_cast<size_t>(craft);
    b.knots(craft, nknots[c], kt, kp, kv);
    uint64_t h = 14695981039346656037ull;
    h = fnv(h, &status[c], sizeof(int32_t));
    h = fnv(h, &nknots[c], sizeof(int32_t));
    h = fnv(h, &t[c], sizeof(double));
    h = fnv(h, pos[c].data(), 3 * sizeof(double));
    h = fnv(h, vel[c].data(), 3 * sizeof(double));
    h = fnv(h, &next_h[c], sizeof(double));
    for (size_t k = 0; k < kt.size(); ++k) {
        h = fnv(h, &kt[k], sizeof(double));
        h = fnv(h, kp[k].data(), 3 * sizeof(double));
        h = fnv(h, kv[k].data(), 3 * sizeof(double));
    }
    return h;
}

int main() try {
    // Sun, Earth, Moon (the system of examples/propagate.cpp): 40 days of ephemeris
    const std::vector<double> mu = {132712440041.27942, 398600.43550702266, 4902.80011845755};
    const std::vector<ea::DVec3> y = {{130800.7436285839, 344339.3116943656, 136496.914202216},
                                      {-27204249.66910069, 132940582.438431, 57641619.74238631},
                                      {-27017766.52877057, 133253431.1006455, 57806029.23241135}};
    const std::vector<ea::DVec3> dy = {{-0.007799748521575531, -0.005561934613704532, -0.00225317087714714},
                                       {-29.75359910616436, -5.189518219844614, -2.251561710555783},
                                       {-30.64009897505477, -4.820684674596127, -2.032529075882219}};
    const double t0 = -252460800.0, dt = 21600.0, day = 86400.0;
    ea::NBodyPropagator massive(y, dy, mu, t0, dt, ea::Direction::Forward, {12, 3, 1}, {6, 7, 6});
    ea::StepError err = ea::StepError::None;
    ea::Solution splines = massive.propagate(t0 + 40.0 * day, &err);
    if (err != ea::StepError::None) { std::fprintf(stderr, "propagate: %s\n", ea::to_string(err)); return 1; }
    ea::Ephemeris bodies(splines, mu);
    const ea::AdaptiveParams params(1e-3);

    // the fleet and, ship by ship, the same ship alone; names[i] is the ship in slot i of the fleet
    std::vector<std::string> names;
    std::vector<std::unique_ptr<ea::SpacecraftBatch>> alone;
    auto ship = [](double along) {
        return ea::StateVector{{-27204249.668775786 + along, 132947582.43848978, 57641619.74241204},
                               {-22.207539106181895, -5.189518219791726, -2.2515617105336263}};
    };
    std::vector<ea::StateVector> first = {ship(0.0), ship(10.0), ship(20.0)};
    const ea::Burn burn{t0 + 0.25 * day, t0 + 0.25 * day + 300.0, {0.0, 0.0, 1e-3}, 1};
    const std::vector<std::vector<ea::Burn>> plans = {{burn}, {}, {burn}};
    ea::SpacecraftBatch fleet(bodies, t0, first, "Verner87", params, plans);
    for (size_t i = 0; i < first.size(); ++i) {
        names.push_back("ship-" + std::to_string(i));
        alone.push_back(std::make_unique<ea::SpacecraftBatch>(bodies, t0, std::vector<ea::StateVector>{first[i]}, "Verner87", params,
                                                               std::vector<std::vector<ea::Burn>>{plans[i]}));
    }
    auto fly = [&](double to) {
        fleet.step_to(to);
        for (auto &a : alone) a->step_to(to);
    };
    auto spawn = [&](double at, const ea::StateVector &sv, const std::string &name) {
        ea::SpacecraftBatch one(bodies, at, {sv}, "Verner87", params);
        fleet = ea::SpacecraftBatch::concat({&fleet, &one});
        names.push_back(name);
        alone.push_back(std::make_unique<ea::SpacecraftBatch>(bodies, at, std::vector<ea::StateVector>{sv}, "Verner87", params));
    };
    auto remove = [&](size_t slot) {
        std::vector<int64_t> keep;
        for (size_t i = 0; i < names.size(); ++i) if (i != slot) keep.push_back(static_cast<int64_t>(i));
        fleet = fleet.select(keep);
        names.erase(names.begin() + static_cast<std::ptrdiff_t>(slot));
        alone.erase(alone.begin() + static_cast<std::ptrdiff_t>(slot));
    };

    fly(t0 + 0.5 * day);
    spawn(t0 + 0.5 * day, ship(4000.0), "ship-3");             // a ship appears while three fly (one of them has burnt already)
    fly(t0 + 1.0 * day);
    remove(1);                                                  // ship-1 is deleted
    spawn(t0 + 1.0 * day, ship(-2500.0), "ship-4");
    fly(t0 + 1.5 * day);
    remove(0);
    fly(t0 + 2.0 * day);

    int mismatches = 0;
    for (size_t i = 0; i < names.size(); ++i) {
        const uint64_t in_fleet = digest(fleet, static_cast<int64_t>(i)), by_itself = digest(*alone[i], 0);
        std::printf("%s fleet %016llx alone %016llx%s\n", names[i].c_str(), (unsigned long long)in_fleet, (unsigned long long)by_itself,
                    in_fleet == by_itself ? "" : "  MISMATCH");
        mismatches += in_fleet != by_itself;
    }
    if (fleet.len() != static_cast<int64_t>(names.size())) { std::fprintf(stderr, "fleet size %lld\n", (long long)fleet.len()); return 1; }
    return mismatches ? 1 : 0;
} catch (const ea::Error &e) {
    std::fprintf(stderr, "%s\n", e.what());
    return e.status == EPH_ERR_NO_DEVICE ? 77 : 1;
}
