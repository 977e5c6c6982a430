// examples/craft_eval.cpp -- where is every craft of a batch at epoch T, relative to body B: EvaluateTrajectory::state_vector on
// RelativeTrajectory<&SpacecraftTrajectory, &Trajectory> (ephemeris/src/trajectory.rs:188-335) for a whole SpacecraftBatch in one call
// (include/ephemeris_amd.hpp: SpacecraftBatch::state_vectors_at over eph_craft_batch_eval).
//
//   g++ -std=c++17 -Iinclude examples/craft_eval.cpp -Lephemeris_explorer_amd -lephemeris_amd -Wl,-rpath,$PWD/ephemeris_explorer_amd -o craft_eval
//   ./craft_eval        (needs an MI355X; without a device the first compute call throws Error{EPH_ERR_NO_DEVICE}: exit 77)
//
// Values are printed as hex floats: the GPU test compares them bit for bit with the Python call's.
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

    // the same epochs for every ship: before the start (None), the start (knot 0 itself), inside, after the end (None)
    const std::vector<double> at = {t0 - 1.0, t0, t0 + 0.5 * day, t0 + 1.25 * day, t0 + 3.0 * day};
    for (int32_t reference : {-1, 1, 2}) {
        std::vector<ea::StateVector> sv;
        std::vector<uint8_t> inside;
        batch.state_vectors_at(at, sv, inside, reference);
        for (size_t e = 0; e < at.size(); ++e)
            for (size_t c = 0; c < ships.size(); ++c) {
                const ea::StateVector &s = sv[e * ships.size() + c];
                std::printf("ref %d epoch %zu craft %zu inside=%d %a %a %a %a %a %a\n", (int)reference, e, c, (int)inside[e * ships.size() + c], s.position[0],
                            s.position[1], s.position[2], s.velocity[0], s.velocity[1], s.velocity[2]);
            }
    }
    // every ship its own epoch: its own newest knot, relative to the Earth
    std::vector<double> own;
    for (int64_t c = 0; c < batch.len(); ++c) own.push_back(batch.trajectory(c).t.back());
    std::vector<ea::StateVector> sv;
    std::vector<uint8_t> inside;
    batch.state_vectors_at(own, sv, inside, 1, true);
    for (size_t c = 0; c < own.size(); ++c)
        std::printf("own craft %zu at %a inside=%d %a %a %a %a %a %a\n", c, own[c], (int)inside[c], sv[c].position[0], sv[c].position[1], sv[c].position[2],
                    sv[c].velocity[0], sv[c].velocity[1], sv[c].velocity[2]);
    return 0;
} catch (const ea::Error &e) {
    std::fprintf(stderr, "%s\n", e.what());
    return e.status == EPH_ERR_NO_DEVICE ? 77 : 1;
}
