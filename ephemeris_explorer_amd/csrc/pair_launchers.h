// pair_launchers.h -- what one evaluation order's translation units export to each other and, through pair_table() (pair_table.hip),
// to dispatch.cpp. INCLUDED INSIDE namespace eph::pv<k> (pair_ns.h).
int accel_wave(hipStream_t s, int bpw, int n, int npad, const Body4 *pos, const double *acc_init, double *acc_out, int lo, int hi,
               const KickDrift &kd);                                                                        // step_wave.hip
int accel_wg(hipStream_t s, int wb, int n, int npad, const Body4 *pos, const double *acc_init, double *acc_out, int lo, int hi,
             const KickDrift &kd);                                                                          // step_wg.hip
int lm_step_wave(hipStream_t s, int bpw, const LmArgs &a);                                                 // step_wave.hip
int lm_step_wg(hipStream_t s, int wb, const LmArgs &a);                                                    // step_wg.hip
int lm_persistent(hipStream_t s, const LmArgs &a, int64_t nsteps);                                         // step_wave.hip
int lm_small(hipStream_t s, const LmArgs &a, int64_t nsteps);                                              // step_small.hip
int lm_small_many(hipStream_t s, const LmArgs *argv_dev, int count, int L, int64_t nsteps);                // step_small.hip
int lm_double_small(hipStream_t s, const LmDoubleArgs &d, int64_t nsteps);                                 // step_double_small.hip
int srkn_small(hipStream_t s, const SrknSmallArgs &a, int64_t nsteps);                                     // step_srkn_small.hip
int srkn_double_small(hipStream_t s, const SrknSmallArgs &a, int64_t nsteps);                              // step_srkn_small.hip
int srkn_small_many(hipStream_t s, const SrknGangArgs *argv_dev, int count);                               // step_srkn_small.hip
int srkn_double_small_many(hipStream_t s, const SrknGangArgs *argv_dev, int count);                        // step_srkn_small.hip
int lm_startup_small(hipStream_t s, const LmStartupArgs &a, bool compensated);                             // step_srkn_small.hip
int lm_startup_small_many(hipStream_t s, const LmStartupArgs *argv_dev, int count);                        // step_srkn_small.hip
int lm_step_fast(hipStream_t s, const LmArgs &a, double *partial, int S, int unroll, bool approx, float *posf, int f32_stage,
                 int conv_lo, int conv_cnt, unsigned *tickets);                                             // fast.hip
int craft_launch(hipStream_t s, const CraftArgs &a, const CraftLaunch &how);                               // craft_sweep.hip
int debug_wg_cycles(long long *out8);       // step_small.hip; reached through the hooks' table only (pair_debug.hip)
const PairKernels *pair_table();                                                                           // pair_table.hip
