// examples/craft_separation.cpp -- the app's target plotting (setup_target_plotting, ephemeris_explorer/src/analysis.rs:308-371:
// RelativeTrajectory::closest_separation_between + PlotSeparation) for ships that live in a SpacecraftBatch: the knots are read where
// the batch keeps them, on the device (include/ephemeris_amd.hpp: SpacecraftBatch::closest_separation over
// eph_craft_batch_closest_separation).
//
//   g++ -std=c++17 -Iinclude examples/craft_separation.cpp -Lephemeris_explorer_amd -lephemeris_amd -Wl,-rpath,$PWD/ephemeris_explorer_amd -o craft_separation
//   ./craft_separation  (needs an MI355X; without a device the first compute call throws Error{EPH_ERR_NO_DEVICE}: exit 77)
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

    // three ships in low Earth orbit, 10 km apart, two days
    std::vector<ea::StateVector> ships;
    for (int i = 0; i < 3; ++i)
        ships.push_back({{-27204249.668775786 + 10.0 * i, 132947582.43848978, 57641619.74241204}, {-22.207539106181895, -5.189518219791726, -2.2515617105336263}});
    ea::SpacecraftBatch batch(bodies, t0, ships, "Verner87", ea::AdaptiveParams(1e-3));
    batch.step_to(t0 + 2.0 * day);

    // the app's call: the whole plot window, precision 0.001, at most 1000 iterations, distance_squared_at
    eph_separation_request rq{};
    rq.source_body = -1; rq.target_body = 2;                                         // every ship against the Moon
    rq.left = t0; rq.right = t0 + 2.0 * day;
    rq.precision = 0.001; rq.max_iterations = 1000; rq.metric = 0;
    auto print = [](const char *what, size_t p, const ea::SpacecraftBatch::Separation &s) {
        std::printf("%s %zu: status %d, found %d, time %a, distance %a km, %d iterations\n", what, p, (int)s.status, (int)s.found, s.time, s.distance,
                    (int)s.iterations);
    };
    const std::vector<ea::SpacecraftBatch::Separation> moon = batch.closest_separation(std::vector<eph_separation_request>(ships.size(), rq));
    for (size_t p = 0; p < moon.size(); ++p) print("ship against the Moon", p, moon[p]);
    // ship 0 against the Earth over the second day, by distance_at; ships 1 and 2 against ship 0
    std::vector<eph_separation_request> mixed(3, rq);
    mixed[0].target_body = 1; mixed[0].left = t0 + 1.0 * day; mixed[0].metric = 1;
    mixed[1].target_body = -1;
    mixed[2].target_body = -1;
    const std::vector<ea::SpacecraftBatch::Separation> m = batch.closest_separation(mixed, {0, 1, 2}, {-1, 0, 0});
    for (size_t p = 0; p < m.size(); ++p) print("mixed request", p, m[p]);
    return 0;
} catch (const ea::Error &e) {
    std::fprintf(stderr, "%s\n", e.what());
    return e.status == EPH_ERR_NO_DEVICE ? 77 : 1;
}
