// examples/convergence.cpp -- the reference's own convergence test (ephemeris/tests/solar_system_convergence.rs:225-285) on the
// device, through include/ephemeris_amd.hpp: a doubling sweep of step sizes on the compensated state Double<DVec3>
// (NBodyIntegration(.., compensated = true)), the answer being the largest step whose solution at the bound stays within 10 m and
// 1 m/s of the run with half the first step.
//
//   g++ -std=c++17 -Iinclude examples/convergence.cpp -Lephemeris_explorer_amd -lephemeris_amd -Wl,-rpath,$PWD/ephemeris_explorer_amd -o convergence
//   ./convergence tests/golden/systems/full_solar_system_2433282.5 [method = QuinlanTremaine12] [days = 365] [h0 = 75]
//   (needs an MI355X; without a device the first compute call throws Error{EPH_ERR_NO_DEVICE}: exit 77)
//
// The reference's answers on its 34-body system over 366 days, and this library's on the committed 32-body one over 365:
// QuinlanTremaine12 -> 600 s, Stormer13 -> 300 s, BlanesMoan14A -> 600 s (pass the method as the second argument; at 32 bodies
// every run of a sweep is a single launch, the BlanesMoan14A sweep about 16 s in all).
#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <fstream>
#include <sstream>
#include <string>

#include "ephemeris_amd.hpp"

namespace ea = ephemeris_amd;

namespace {

// state.json of a system directory: {"bodies": [{"name", "mu", "position": [x, y, z], "velocity": [x, y, z]}, ...]} -- the three keys
// are looked up in order, body after body (a reader for this example, not a JSON parser)
struct System {
    std::vector<double> mu;
    std::vector<ea::DVec3> y, dy;
};
bool number_after(const std::string &text, size_t &at, double &out) {
    at = text.find_first_of("-+0123456789.", at);
    if (at == std::string::npos) return false;
    char *end = nullptr;
    out = std::strtod(text.c_str() + at, &end);
    if (end == text.c_str() + at) return false;
    at = (size_t)(end - text.c_str());
    return true;
}
bool load_system(const std::string &directory, System &s) {
    std::ifstream in(directory + "/state.json");
    if (!in) return false;
    std::stringstream buf;
    buf << in.rdbuf();
    const std::string text = buf.str();
    size_t at = text.find("\"bodies\"");
    while (at != std::string::npos && (at = text.find("\"mu\"", at)) != std::string::npos) {
        double mu = 0.0;
        ea::DVec3 p{}, v{};
        at += 4;
        if (!number_after(text, at, mu)) return false;
        if ((at = text.find("\"position\"", at)) == std::string::npos) return false;
        at += 10;
        for (double &c : p) if (!number_after(text, at, c)) return false;
        if ((at = text.find("\"velocity\"", at)) == std::string::npos) return false;
        at += 10;
        for (double &c : v) if (!number_after(text, at, c)) return false;
        s.mu.push_back(mu);
        s.y.push_back(p);
        s.dy.push_back(v);
    }
    return !s.mu.empty();
}

struct State {
    double end = 0.0;
    std::vector<ea::DVec3> y, dy;
};
// Integration::solve with EveryStepSolout (integration/src/lib.rs:506-529): advance until time >= bound
bool solve(const System &s, double t0, double bound, const char *method, double h, State &out) {
    ea::NBodyIntegration integration(s.y, s.dy, s.mu, t0, h, method, true);
    integration.set_bound(bound);
    const ea::StepError e = integration.advance(int64_t{1} << 40);     // BoundReached on the step after the last
    if (e != ea::StepError::BoundReached) {
        std::fprintf(stderr, "Integration error: %s\n", ea::to_string(e));
        return false;
    }
    out.end = integration.state(out.y, out.dy);
    return true;
}
double length(const ea::DVec3 &a, const ea::DVec3 &b) {                // (a - b).length()
    const double x = a[0] - b[0], y = a[1] - b[1], z = a[2] - b[2];
    return std::sqrt(x * x + y * y + z * z);
}

}  // namespace

int main(int argc, char **argv) try {
    if (argc < 2) {
        std::fprintf(stderr, "usage: %s SYSTEM_DIRECTORY [method] [days] [h0 seconds]\n", argv[0]);
        return 2;
    }
    const char *method = argc > 2 ? argv[2] : "QuinlanTremaine12";
    const double days = argc > 3 ? std::atof(argv[3]) : 365.0, h0 = argc > 4 ? std::atof(argv[4]) : 75.0;
    System s;
    if (!load_system(argv[1], s)) {
        std::fprintf(stderr, "no bodies in %s/state.json\n", argv[1]);
        return 2;
    }
    const double t0 = 0.0, bound = t0 + days * 86400.0;
    std::printf("%zu bodies, %s<Double>, %.0f days, %d device(s)\n", s.mu.size(), method, days, (int)ea::device_count());

    State truth, state;
    if (!solve(s, t0, bound, method, h0 / 2.0, truth)) return 1;
    std::vector<double> hs;
    for (double h = h0;; h *= 2.0) {
        if (!solve(s, t0, bound, method, h, state)) return 1;
        double ey = 0.0, edy = 0.0;
        for (size_t i = 0; i < s.mu.size(); ++i) {
            ey = std::fmax(length(state.y[i], truth.y[i]) * 1e3, ey);    // f64::max
            edy = std::fmax(length(state.dy[i], truth.dy[i]) * 1e3, edy);
        }
        if (std::fabs(bound - state.end) != 0.0) {
            std::fprintf(stderr, "Overstepped integration bounds\n");
            return 1;
        }
        std::printf("h = %6.0f s: %.6g m, %.6g m/s\n", h, ey, edy);
        hs.push_back(h);
        if (ey > 10.0 || edy > 1.0) break;
    }
    const double converged = hs[hs.size() >= 2 ? hs.size() - 2 : 0];   // results.get(results.len().saturating_sub(2))
    std::printf("converged at h = %.0f s (%g min)\n", converged, converged / 60.0);
    return 0;
} catch (const ea::Error &e) {
    std::fprintf(stderr, "%s\n", e.what());
    return e.status == EPH_ERR_NO_DEVICE ? 77 : 1;
}
