// craft_attempt.inc -- one attempt of the embedded pair, included TEXTUALLY by the sweep kernels of craft_sweep.hip (parts 1 and 2: the
// static k_craft_propagate and the queue form k_craft_queue; part 3: those two and k_craft_wave). Textual on purpose: routed through
// a function the same code gets a measurably worse register allocation (444 SGPR-spill reloads against 8 in the static kernel, 4 % in
// the queue kernel; the ten controller lines of part 3 alone, as a function: 80 -> 96 B of scratch in the 13-stage static kernel).
// In scope at the include site: a (CraftArgs), EPH_RK (the method table: a.rk or *rkp), sg, time, h, rk_i, y[6], template parameters
// S / FSAL / NYS, and the stage derivatives k_s = (velocity half, acceleration half) behind KV_GET / KV_PUT and ka[S][3] (see
// craft_sweep.hip "stage storage": the velocity halves live in LDS). Every component's chain of additions is the reference's, in the
// reference's order -- the loops over d are merely split in two. EPH_ATTEMPT_PART 1: the stages (ERK::advance, explicit.rs:72-106, or
// the ERKNG form) -> `bool ok`; part 2: the solution update and the error estimate (RKEmbedded::error) -> `double e[6]`; part 3: the
// error norm and the step-size controller, from e[6], `lower` and next_h -> `double err`, next_h updated.
#if EPH_ATTEMPT_PART == 1
            // ERK::advance  explicit.rs:72-106
            bool ok = true;
#pragma unroll
            for (int s = 0; s < S; ++s) {
                if (FSAL && s == 0 && rk_i > 0) {
#pragma unroll
                    for (int d = 0; d < 3; ++d) {
                        const double t = ka[0][d]; ka[0][d] = ka[S - 1][d]; ka[S - 1][d] = t;
                        if (!NYS) { const double u = KV_GET(0, d); KV_PUT(0, d, KV_GET(S - 1, d)); KV_PUT(S - 1, d, u); }
                    }
                    continue;
                }
                if (!ok) continue;
                const double ti = time + h * EPH_RK.C[s];
                double yi[6];
                if (NYS) {
                    const double hc = h * EPH_RK.C[s];
#pragma unroll
                    for (int d = 0; d < 3; ++d) { yi[d] = y[d] + y[3 + d] * hc; yi[3 + d] = y[3 + d]; }
#pragma unroll
                    for (int j = 0; j < s; ++j) {
                        const double hhap = h * h * EPH_RK.A[s][j], hav = h * EPH_RK.A2[s & 7][j & 7];
#pragma unroll
                        for (int d = 0; d < 3; ++d) {
                            yi[d] = yi[d] + ka[j][d] * hhap;
                            yi[3 + d] = yi[3 + d] + ka[j][d] * hav;
                        }
                    }
                    double out[6];
                    ok = craft_rhs<false>(a, sg, ti, yi, out, nullptr);
                    // an Err leaves dk[s] as `self.dk[s].zero()` made it (explicit_generalized.rs:109-111); it can only be read again
                    // through the FSAL swap, i.e. as the last stage
#pragma unroll
                    for (int d = 0; d < 3; ++d) ka[s][d] = (FSAL && s == S - 1 && !ok) ? 0.0 : out[3 + d];
                    continue;
                }
#pragma unroll
                for (int d = 0; d < 6; ++d) yi[d] = y[d];
#pragma unroll
                for (int j = 0; j < s; ++j) {
                    const double ha = h * EPH_RK.A[s][j];
#pragma unroll
                    for (int d = 0; d < 3; ++d) {
                        yi[d] = yi[d] + KV_GET(j, d) * ha;
                        yi[3 + d] = yi[3 + d] + ka[j][d] * ha;
                    }
                }
                double out[6];
                ok = craft_rhs<false>(a, sg, ti, yi, out, nullptr);
                // an Err leaves k[s] as `self.k[s].zero()` made it (explicit.rs:92); only the last stage of an FSAL pair is ever
                // read again before it is recomputed
                const bool zeroed = FSAL && s == S - 1 && !ok;
#pragma unroll
                for (int d = 0; d < 3; ++d) {
                    KV_PUT(s, d, zeroed ? 0.0 : out[d]);          // dy.position = y.velocity  spacecraft.rs:303-305
                    ka[s][d] = zeroed ? 0.0 : out[3 + d];
                }
            }
#elif EPH_ATTEMPT_PART == 2
            double e[6] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
            if (NYS) {
#pragma unroll
                for (int d = 0; d < 3; ++d) y[d] = y[d] + y[3 + d] * h;
#pragma unroll
                for (int s = 0; s < S; ++s) {
                    const double hhbp = h * h * EPH_RK.B[s], hbv = h * EPH_RK.B2[s & 7];
#pragma unroll
                    for (int d = 0; d < 3; ++d) {
                        y[d] = y[d] + ka[s][d] * hhbp;
                        y[3 + d] = y[3 + d] + ka[s][d] * hbv;
                    }
                }
#pragma unroll
                for (int s = 0; s < S; ++s) {
                    const double hhep = h * h * EPH_RK.E[s], hev = h * EPH_RK.E2[s & 7];
#pragma unroll
                    for (int d = 0; d < 3; ++d) {
                        e[d] = e[d] + ka[s][d] * hhep;
                        e[3 + d] = e[3 + d] + ka[s][d] * hev;
                    }
                }
            } else {
                // one pass over the stages for both sums (each component's chain of additions is its own): every velocity half is
                // read from LDS once
#pragma unroll
                for (int s = 0; s < S; ++s) {
                    const double hb = h * EPH_RK.B[s];
                    const double he = h * EPH_RK.E[s];                 // RKEmbedded::error
#pragma unroll
                    for (int d = 0; d < 3; ++d) {
                        const double kv = KV_GET(s, d);
                        y[d] = y[d] + kv * hb;
                        y[3 + d] = y[3 + d] + ka[s][d] * hb;
                        e[d] = e[d] + kv * he;
                        e[3 + d] = e[3 + d] + ka[s][d] * he;
                    }
                }
            }
#else
            // AbsTol::err_over_tol
            const double pm = fmax(fabs(e[0] / a.tol_pos), fmax(fabs(e[1] / a.tol_pos), fabs(e[2] / a.tol_pos)));
            const double vm = fmax(fabs(e[3] / a.tol_vel), fmax(fabs(e[4] / a.tol_vel), fabs(e[5] / a.tol_vel)));
            const double err = fmax(pm, vm);
            // IController::step  mod.rs:225-243
            const double m = a.fac * cr_pow(err, -(1.0 / (double)lower));
            const double c = m < a.fac_min ? a.fac_min : (m > a.fac_max ? a.fac_max : m);
            const double nh = next_h * c;
            next_h = nh > a.h_max ? a.h_max : nh;
#endif
