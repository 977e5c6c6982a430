// examples/craft_markers.cpp -- the markers the app draws on, and picks from, a ship's plots (plot_manoeuvre_markers,
// plot_transition_markers, plot_apsis_markers, plot_bounds_markers, ephemeris_explorer/src/ui/world/tooltip.rs:84-245) for ships that
// live in a SpacecraftBatch: the plots of plot_segments, then for every plot the burn starts, SOI transitions, apsides and trajectory
// bounds inside its points, each with its distance from the plot's reference body and, for a burn, its TNB frame, evaluated on the
// device (include/ephemeris_amd.hpp: SpacecraftBatch::plot_markers over eph_craft_batch_plot_markers).
//
//   g++ -std=c++17 -Iinclude examples/craft_markers.cpp -Lephemeris_explorer_amd -lephemeris_amd -Wl,-rpath,$PWD/ephemeris_explorer_amd -o craft_markers
//   ./craft_markers  (needs an MI355X; without a device the first compute call throws Error{EPH_ERR_NO_DEVICE}: exit 77)
#include <cstdio>
#include <limits>

#include "ephemeris_amd.hpp"

namespace ea = ephemeris_amd;

int main() try {
    // the ten-body system of 1950-01-01 (Sun, the planets without Pluto, the Moon), QuinlanTremaine12 at 6 h: 230 days of ephemeris
    const char *const names[] = {"Sun", "Mercury", "Venus", "Earth", "Moon", "Mars", "Jupiter", "Saturn", "Uranus", "Neptune"};
    const std::vector<double> mu = {132712440041.27942, 22031.868551400003, 324858.592, 398600.43550702266, 4902.80011845755,
                                    42828.37362069909, 126712764.09999998, 37940584.8418, 5794556.3999999985, 6836527.100580399};
    const std::vector<ea::DVec3> y = {{130800.7436285839, 344339.3116943656, 136496.914202216},
                                      {48133224.97480647, 15233814.30014003, 3103329.958033448},
                                      {14233458.68580109, 98077616.63667394, 43195421.34399015},
                                      {-27204249.66910069, 132940582.438431, 57641619.74238631},
                                      {-27017766.52877057, 133253431.1006455, 57806029.23241135},
                                      {-208641466.9300484, 121298867.4908876, 61280235.09125485},
                                      {509752196.3414811, -512177335.8792, -231997361.2135479},
                                      {-1347351964.270596, 324851963.108166, 192024573.4070957},
                                      {-185586918.6536981, 2589909686.998426, 1136951196.569068},
                                      {-4352063774.898198, -1204009697.462287, -384499507.7396315}};
    const std::vector<ea::DVec3> dy = {{-0.007799748521575531, -0.005561934613704532, -0.00225317087714714},
                                       {-23.83420388027612, 42.24930079748117, 25.03952233448571},
                                       {-34.84686019789481, 3.212829613104719, 3.65143578319356},
                                       {-29.75359910616436, -5.189518219844614, -2.251561710555783},
                                       {-30.64009897505477, -4.820684674596127, -2.032529075882219},
                                       {-12.26550420899615, -16.73901959824886, -7.344170605831738},
                                       {9.52328775043255, 8.720782096040281, 3.50619007704306},
                                       {-3.100666034691074, -8.67293836760191, -3.447937093437607},
                                       {-6.84728583073883, -0.7355466074119503, -0.2251124007726725},
                                       {1.477609548428571, -4.788772477859187, -1.996856698322491}};
    const double t0 = -252460800.0, dt = 21600.0, day = 86400.0;
    ea::NBodyPropagator massive(y, dy, mu, t0, dt, ea::Direction::Forward, {12, 2, 10, 3, 1, 12, 25, 25, 25, 25}, {6, 7, 7, 7, 6, 7, 7, 6, 6, 5});
    ea::StepError err = ea::StepError::None;
    ea::Solution splines = massive.propagate(t0 + 230.0 * day, &err);
    if (err != ea::StepError::None) { std::fprintf(stderr, "propagate: %s\n", ea::to_string(err)); return 1; }
    ea::Ephemeris bodies(splines, mu);

    // the Mars-transfer ship: craft 0 flies all four burns, craft 1 leaves out the capture burn at Mars
    const ea::StateVector ship{{-27204249.668775786, 132947582.43848978, 57641619.74241204}, {-22.253599106181895, -5.189518219791726, -2.2515617105336263}};
    const std::vector<ea::Burn> plan = {{t0 + 915.0, t0 + 915.0 + 315.0, {0.0, 0.0, 0.01}, 3},
                                        {t0 + 2590.0, t0 + 2590.0 + 390.0, {0.00997, -0.00231, 0.0003}, 0},
                                        {t0 + 5026345.0, t0 + 5026345.0 + 60.0, {0.00051, -0.0001, -0.00653}, 5},
                                        {t0 + 17941445.0, t0 + 17941445.0 + 310.0, {-0.01, 0.0, 0.0}, 5}};
    ea::SpacecraftBatch batch(bodies, t0, {ship, ship}, "Verner87", ea::AdaptiveParams(1e-3),
                              {plan, std::vector<ea::Burn>(plan.begin(), plan.end() - 1)}, 20000);
    // sphere radii (load/mod.rs:283-307) and the static hierarchy (analysis.rs:101-124) at the epoch: the Moon is in the Earth's sphere
    batch.enable_events({std::numeric_limits<double>::infinity(), 97728.63717065519, 613523.176359236, 909153.0740387321, 68800.06030265747,
                         630324.3830536032, 47019685.971106865, 53501395.921809934, 51106231.493024185, 87311188.4006872},
                        16, 8192);                                                    // (the ship's orbits have many apsides)
    const std::vector<int32_t> parent = {-1, 0, 0, 0, 3, 0, 0, 0, 0, 0};
    batch.step_to(t0 + 215.0 * day);

    eph_plot_view view{};
    view.camera_position[0] = 1.2e8; view.camera_position[1] = -3.0e8; view.camera_position[2] = 2.0e8;
    view.grid_matrix3[0] = view.grid_matrix3[4] = view.grid_matrix3[8] = 1.0;
    view.current = t0 + 30.0 * day;
    eph_orbit_plot_config config{};
    config.start = t0; config.end = t0 + 400.0 * day;
    config.enabled = 1; config.reference_body = -1;                                   // OrbitPlotReference::Primary
    config.tan2_angular_resolution = 0.000290888 * 0.7853982;
    config.max_points_per_segment = 4000;
    const ea::SpacecraftBatch::PlotSegments plots = batch.plot_segments(view, {config, config}, parent);
    const std::vector<int64_t> craft_of_entry = {0, 1};
    std::vector<int64_t> craft;                                                       // the craft of every plot
    for (const eph_plot_segment &g : plots.segments) craft.push_back(craft_of_entry[static_cast<size_t>(g.plot)]);
    const ea::SpacecraftBatch::PlotMarkers marks = batch.plot_markers(ea::SpacecraftBatch::marker_requests(plots), craft);
    for (size_t s = 0; s < plots.segments.size(); ++s) {
        const eph_plot_segment &g = plots.segments[s];
        const int64_t m0 = marks.first[s], m1 = marks.first[s + 1];
        int64_t apsides = 0;
        for (int64_t m = m0; m < m1; ++m) apsides += marks.markers[static_cast<size_t>(m)].kind == 2 || marks.markers[static_cast<size_t>(m)].kind == 3;
        std::printf("ship %lld: %s %s%s%s, relative to %s: %lld markers, %lld of them apsides\n", static_cast<long long>(g.plot), names[g.soi_body],
                    ea::SpacecraftBatch::segment_kind(g.kind), g.is_burn ? " Burn" : "", g.overlapping ? " (overlapping)" : "",
                    names[g.reference_body], static_cast<long long>(m1 - m0), static_cast<long long>(apsides));
        int64_t shown = 0;
        for (int64_t m = m0; m < m1; ++m) {
            const eph_plot_marker &k = marks.markers[static_cast<size_t>(m)];
            if ((k.kind == 2 || k.kind == 3) && ++shown > 2) continue;               // (a low orbit has dozens: the first two)
            std::printf("    %-10s %-8s day %8.3f", ea::SpacecraftBatch::marker_kind(k.kind), k.body >= 0 ? names[k.body] : "", (k.time - t0) / day);
            if (k.status & 1) std::printf("  %.1f km", k.distance);
            if (k.kind == 0 && (k.status & 2)) std::printf("  prograde (%.3f, %.3f, %.3f)", k.frame[0], k.frame[1], k.frame[2]);
            std::printf("\n");
        }
    }
    return 0;
} catch (const ea::Error &e) {
    std::fprintf(stderr, "%s\n", e.what());
    return e.status == EPH_ERR_NO_DEVICE ? 77 : 1;
}
