// examples/craft_restart.cpp -- a flight plan is edited and every ship of a batch is re-propagated from where its plan diverges, in
// place on the device: FlightPlan::restart_propagator + apply_flight_plan (ephemeris_explorer/src/flight_plan.rs:263-361) for a
// whole SpacecraftBatch (include/ephemeris_amd.hpp: SpacecraftBatch::restart over eph_craft_batch_restart).
//
//   g++ -std=c++17 -Iinclude examples/craft_restart.cpp -Lephemeris_explorer_amd -lephemeris_amd -Wl,-rpath,$PWD/ephemeris_explorer_amd -o craft_restart
//   ./craft_restart     (needs an MI355X; without a device the first compute call throws Error{EPH_ERR_NO_DEVICE}: exit 77)
//
// Values are printed as hex floats: the GPU test compares them bit for bit with the Python calls'.
#include <cstdio>

#include "ephemeris_amd.hpp"

namespace ea = ephemeris_amd;

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

    // three ships in low Earth orbit, 10 km apart, each with one 5-minute burn in the Earth's TNB frame half a day in
    std::vector<ea::StateVector> ships;
    for (int i = 0; i < 3; ++i)
        ships.push_back({{-27204249.668775786 + 10.0 * i, 132947582.43848978, 57641619.74241204}, {-22.207539106181895, -5.189518219791726, -2.2515617105336263}});
    const ea::Burn burn{t0 + 0.5 * day, t0 + 0.5 * day + 300.0, {0.0, 0.0, 1e-3}, 1};
    const std::vector<std::vector<ea::Burn>> plan(3, {burn});
    ea::SpacecraftBatch batch(bodies, t0, ships, "Verner87", ea::AdaptiveParams(1e-3), plan);
    batch.step_to(t0 + 2.0 * day);

    // the edits: ship 0's burn 1 % stronger, ship 1's plan unchanged, ship 2 gets a second, inertial burn on day 1.5
    std::vector<std::vector<ea::Burn>> edited = plan;
    edited[0][0].acceleration[2] *= 1.01;
    edited[2].push_back({t0 + 1.5 * day, t0 + 1.5 * day + 120.0, {1e-3, 0.0, 0.0}, -1});
    std::vector<double> epoch;
    const std::vector<int32_t> outcome = batch.restart(edited, &epoch);
    for (size_t c = 0; c < ships.size(); ++c) std::printf("restart craft %zu outcome=%d epoch %a\n", c, (int)outcome[c], epoch[c]);

    // the plan's end: three days
    batch.step_to(t0 + 3.0 * day);
    std::vector<double> t, next_h;
    std::vector<ea::DVec3> pos, vel;
    batch.state(t, pos, vel, &next_h);
    std::vector<int32_t> nknots;
    const std::vector<int32_t> status = batch.status(&nknots);
    for (size_t c = 0; c < ships.size(); ++c)
        std::printf("state craft %zu status=%d knots=%d %a %a %a %a %a %a %a %a\n", c, (int)status[c], (int)nknots[c], t[c], pos[c][0], pos[c][1],
                    pos[c][2], vel[c][0], vel[c][1], vel[c][2], next_h[c]);
    return 0;
} catch (const ea::Error &e) {
    std::fprintf(stderr, "%s\n", e.what());
    return e.status == EPH_ERR_NO_DEVICE ? 77 : 1;
}
