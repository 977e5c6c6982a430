// examples/craft_plot.cpp -- the app's per-frame plot sampler (compute_plot_points_parallel + PlotPoints::new, ephemeris_explorer/src/
// ui/world/plot.rs:93-149,272-374) for ships that live in a SpacecraftBatch: the knots are read where the batch keeps them, on the
// device (include/ephemeris_amd.hpp: SpacecraftBatch::plot_points over eph_craft_batch_plot_points).
//
//   g++ -std=c++17 -Iinclude examples/craft_plot.cpp -Lephemeris_explorer_amd -lephemeris_amd -Wl,-rpath,$PWD/ephemeris_explorer_amd -o craft_plot
//   ./craft_plot        (needs an MI355X; without a device the first compute call throws Error{EPH_ERR_NO_DEVICE}: exit 77)
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

    // two views: far from the system with the identity grid, and near the Earth with a rotated, shifted floating-origin grid
    eph_plot_view far{}, near{};
    far.camera_position[0] = 1.2e8; far.camera_position[1] = -3.0e8; far.camera_position[2] = 2.0e8;
    far.grid_matrix3[0] = far.grid_matrix3[4] = far.grid_matrix3[8] = 1.0;
    far.current = t0 + 1.0 * day;
    near.camera_position[0] = 5.0e3; near.camera_position[1] = 2.0e4; near.camera_position[2] = -3.0e4;
    const double rot[9] = {0.36, -0.8, 0.48, 0.48, 0.6, 0.64, -0.8, 0.0, 0.6};      // column major
    for (int i = 0; i < 9; ++i) near.grid_matrix3[i] = rot[i];
    near.grid_translation[0] = 10.0; near.grid_translation[1] = -20.0; near.grid_translation[2] = 5.0;
    near.current = t0 + 0.25 * day;

    // every ship relative to the Earth over the two days; then ship 0 three ways: inertial, relative to the Moon, from `current` on
    const double res = 0.000290888 * 0.7853982;                                      // threshold * ARC_MINUTE * fov
    eph_plot_request rq{};
    rq.source_body = -1; rq.reference_body = 1;
    rq.start = t0; rq.end = t0 + 2.0 * day;
    rq.enabled = 1; rq.tan2_angular_resolution = res; rq.max_points = 2000;
    const std::vector<eph_plot_request> per_ship(ships.size(), rq);
    std::vector<eph_plot_request> ship0(3, rq);
    ship0[0].reference_body = -1;
    ship0[1].reference_body = 2;
    ship0[2].bound = 1;
    int view_no = 0;
    for (const eph_plot_view *view : {&far, &near}) {
        const std::vector<ea::SpacecraftBatch::PlotPoints> a = batch.plot_points(*view, per_ship);
        for (size_t p = 0; p < a.size(); ++p)
            std::printf("view %d ship %zu relative to body 1: status %d, %zu points, %a .. %a\n", view_no, p, (int)a[p].status, a[p].t.size(),
                        a[p].t.empty() ? 0.0 : a[p].t.front(), a[p].t.empty() ? 0.0 : a[p].t.back());
        const std::vector<ea::SpacecraftBatch::PlotPoints> c = batch.plot_points(*view, ship0, {0, 0, 0});
        for (size_t p = 0; p < c.size(); ++p)
            std::printf("view %d ship 0 request %zu: status %d, %zu points, first point %a %a %a\n", view_no, p, (int)c[p].status, c[p].t.size(),
                        c[p].xyz.empty() ? 0.0 : (double)c[p].xyz[0], c[p].xyz.empty() ? 0.0 : (double)c[p].xyz[1], c[p].xyz.empty() ? 0.0 : (double)c[p].xyz[2]);
        ++view_no;
    }
    return 0;
} catch (const ea::Error &e) {
    std::fprintf(stderr, "%s\n", e.what());
    return e.status == EPH_ERR_NO_DEVICE ? 77 : 1;
}
