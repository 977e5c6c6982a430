// nbody.cpp -- NBodyIntegration: `M::new(FixedMethodParams{h}).integrate(NBodyProblem{..})` on the device.
//
// Mirrors, call for call:
//   LinearMultistepIntegrator::advance          integration/src/multistep/mod.rs:194-224
//   ELM2::{advance, advance_with}               integration/src/multistep/second_order/mod.rs:90-153
//   SubstepperIntegrator::advance               integration/src/multistep/mod.rs:97-108
//   FixedRungeKuttaIntegrator::advance + SRKN   integration/src/runge_kutta/mod.rs:106-126, nystrom/symplectic.rs:69-102
// The host replays the reference's scalar bookkeeping (time, bound, step counters) with the reference's f64
// operations; all vector arithmetic runs in the HIP kernels of step_wg.hip / step_wave.hip / step_small.hip / step_srkn_small.hip / fast.hip / solout.hip.
#include <cassert>
#include <cmath>
#include <cstdlib>
#include <cstring>

#include <mutex>

#include "host.h"
#include "double_state.h"
#include "method_name.h"

namespace eph {

namespace {
thread_local uint64_t g_launches = 0;    // test hook: launches queued by advance / advance_many on this thread (eph_internal.h)
}
void count_launches(uint64_t n) { g_launches += n; }
uint64_t launches_counted() { return g_launches; }

NBodyIntegration::~NBodyIntegration() {
    if (stream_) {
        (void)hipSetDevice(device_);
        (void)hipStreamSynchronize(stream_);
        if (ev0_) (void)hipEventDestroy(ev0_);
        if (ev1_) (void)hipEventDestroy(ev1_);
        for (auto *v : {&ev_pending_, &ev_free_})
            for (auto &e : *v) { (void)hipEventDestroy(e.first); (void)hipEventDestroy(e.second); }
        if (gang_ev_) (void)hipEventDestroy(gang_ev_);
        // (the pinned arrays of gang_, startup_ and srkn_gang_ go with the members, behind this wait for the last copy out of them)
        if (gang_copy_ev_) { (void)hipEventSynchronize(gang_copy_ev_); (void)hipEventDestroy(gang_copy_ev_); }
        (void)hipStreamDestroy(stream_);
    }
}

int NBodyIntegration::alloc_buffers() {
    npad_ = ((n_ + 63) / 64) * 64;
    if (npad_ < 64) npad_ = 64;
    return for_each_buffer(*this, [&](auto buf, size_t count, Buf kind) -> int {
        if (kind == Buf::lazy) return EPH_OK;
        auto &b = buf(*this);
        if (const int st = b.alloc(count)) return st;
        if (kind == Buf::state) EPH_HIP(hipMemsetAsync(b.p, 0, sizeof(*b.p) * b.count, stream_));   // (Double::new(x): error +0.0)
        return EPH_OK;
    });
}

int NBodyIntegration::open_device() {
    EPH_HIP(hipStreamCreateWithFlags(&stream_, hipStreamNonBlocking));
    EPH_HIP(hipEventCreate(&ev0_));
    EPH_HIP(hipEventCreate(&ev1_));
    return alloc_buffers();
}

int NBodyIntegration::create(int n, const double *pos, const double *vel, const double *mu, double t0, double h,
                             const char *method_in, std::unique_ptr<NBodyIntegration> *out) {
    if (n < 0 || !method_in || !out || (n > 0 && (!pos || !vel || !mu))) return EPH_ERR_BAD_ARGUMENT;
    int st = check_device();
    if (st) return st;
    std::unique_ptr<NBodyIntegration> o(new NBodyIntegration());
    o->n_ = n;
    // "Name" or "Name<Double>" (method_name.h); the coefficient tables know base names only
    char base[64];
    if (!parse_method_name(method_in, base, sizeof(base), &o->compensated_)) return EPH_ERR_BAD_ARGUMENT;
    const char *method = base;
    if (find_elm2(method, &o->lm_)) {
        // LinearMultistep::new + Substepper::<4, BlanesMoan6B>::new   multistep/mod.rs:54-57,120-128; methods.rs:37-40
        o->is_multistep_ = true;
        o->L_ = o->lm_.order;
        o->substeps_ = 4;
        if (!find_srkn("BlanesMoan6B", &o->rk_)) return EPH_ERR_UNSUPPORTED;
        o->h_sub_ = h * (1.0 / 4.0);   // params.h * Ratio::from_recip(SUBSTEPS)
    } else if (find_srkn(method, &o->rk_)) {
        o->is_multistep_ = false;
        o->L_ = 1;
        o->substeps_ = 1;
        o->h_sub_ = h;
    } else {
        return EPH_ERR_BAD_ARGUMENT;
    }
    o->h_ = h;
    o->time_ = t0;
    o->bound_ = INFINITY;   // nbody.rs:111
    o->pv_ = default_pair_variant();
    EPH_HIP(hipGetDevice(&o->device_));
    if ((st = o->open_device())) return st;
    o->lo_ = 0;
    o->hi_ = n;
    if (n > 0) {
        hipStream_t s = o->stream_;
        EPH_HIP(hipMemcpyAsync(o->mu_.p, mu, sizeof(double) * n, hipMemcpyHostToDevice, s));
        EPH_HIP(hipMemcpyAsync(o->stage_.p, pos, sizeof(double) * 3 * n, hipMemcpyHostToDevice, s));
        if ((st = launch_aos_to_soa(s, n, o->npad_, o->stage_.p, o->Yslot(0)))) return st;
        EPH_HIP(hipStreamSynchronize(s));   // stage_ is reused below
        EPH_HIP(hipMemcpyAsync(o->stage_.p, vel, sizeof(double) * 3 * n, hipMemcpyHostToDevice, s));
        if ((st = launch_aos_to_soa(s, n, o->npad_, o->stage_.p, o->V_.p))) return st;
        if ((st = launch_pack(s, n, o->npad_, o->Yslot(0), o->mu_.p, o->P_[0].p))) return st;
        if ((st = launch_pack(s, n, o->npad_, o->Yslot(0), o->mu_.p, o->P_[1].p))) return st;
        EPH_HIP(hipStreamSynchronize(s));
    }
    *out = std::move(o);
    return EPH_OK;
}

int NBodyIntegration::clone(std::unique_ptr<NBodyIntegration> *out) {
    EPH_HIP(hipSetDevice(device_));
    EPH_HIP(hipStreamSynchronize(stream_));
    std::unique_ptr<NBodyIntegration> o(new NBodyIntegration());
    // the bookkeeping in one assignment: a failed handle stays marked in its copies, a sharded one's clone shares the ranks
    static_cast<NBodyBook &>(*o) = *this;
    int st = o->open_device();
    if (st) return st;
    // the state buffers (on a <Double> handle the error parts among them: the clone continues bit-identically)
    st = for_each_buffer(*this, [&](auto buf, size_t, Buf kind) -> int {
        if (kind != Buf::state) return EPH_OK;
        auto &from = buf(*this), &to = buf(*o);
        EPH_HIP(hipMemcpyAsync(to.p, from.p, sizeof(*from.p) * from.count, hipMemcpyDeviceToDevice, o->stream_));
        return EPH_OK;
    });
    if (st) return st;
    EPH_HIP(hipStreamSynchronize(o->stream_));
    *out = std::move(o);
    return EPH_OK;
}

// Target partition: rank r owns bodies [r*slice, (r+1)*slice) with slice = npad/world. From here on
// only the owned bodies' history, velocities and accelerations are kept current on this rank; the packed
// positions of ALL bodies are, through one all-gather after every kernel that publishes positions.
int NBodyIntegration::shard_refusal() const {
    if (!compensated_) return EPH_OK;
    set_last_error_text("a <Double> handle is not sharded: the error parts of the state have no exchange");
    return EPH_ERR_UNSUPPORTED;
}
int NBodyIntegration::set_shard(std::shared_ptr<Exchange> x) {
    if (!x || xch_) return EPH_ERR_BAD_ARGUMENT;          // a handle is sharded once, while every body is current
    if (const int st = shard_refusal()) return st;
    if (n_ <= kSmallN) return EPH_ERR_UNSUPPORTED;        // one-workgroup systems: replicas only
    if (npad_ % (x->world() * kTile) != 0) {
        set_last_error_text("sharding needs the padded body count to be a multiple of 64 * world");
        return EPH_ERR_BAD_ARGUMENT;
    }
    slice_ = npad_ / x->world();
    lo_ = x->rank() * slice_;
    hi_ = lo_ + slice_ < n_ ? lo_ + slice_ : n_;
    if (hi_ < lo_) hi_ = lo_;
    xch_ = std::move(x);
    return EPH_OK;
}
int NBodyIntegration::gather_packed(Body4 *buf) {
    return xch_ ? xch_->all_gather_inplace(buf, sizeof(Body4) * (size_t)slice_, stream_) : EPH_OK;
}
int NBodyIntegration::gather_stage() {
    return xch_ ? xch_->all_gather_inplace(stage_.p, sizeof(double) * 3 * (size_t)slice_, stream_) : EPH_OK;
}

int NBodyIntegration::sync() {
    EPH_HIP(hipSetDevice(device_));
    EPH_HIP(hipStreamSynchronize(stream_));
    return xch_ ? xch_->poll_error() : EPH_OK;          // a peer that never delivered (peer.hip) surfaces here
}

// FixedRungeKuttaIntegrator::advance (runge_kutta/mod.rs:112-125) with SRKN::advance (symplectic.rs:69-102)
int NBodyIntegration::srkn_step(double h, double *y_slot) {
    if (time_ >= bound_) return EPH_BOUND_REACHED;
    if (time_ + h == time_) return EPH_STEP_SIZE_UNDERFLOW;
    int st;
    for (int s = 0; s < rk_.stages && compensated_; ++s)
        if ((st = srkn_stage_double(h * rk_.B[s], h * rk_.A[s], y_slot, YE_.p + (y_slot - Y_.p), !rk_.fsal || s > 0 || starter_i_ == 0))) return st;
    for (int s = 0; s < rk_.stages && !compensated_; ++s) {
        // *dy = *dy + *ddy * (h * C::B[s]);  *y = *y + *dy * (h * C::A[s])
        const KickDrift kd{V_.p, y_slot, h * rk_.B[s], h * rk_.A[s], P_[pp_ ^ 1].p};
        if (!rk_.fsal || s > 0 || starter_i_ == 0) {
            // problem.ode.eval(t_stage, &problem.state.y, self.ddy.zero()) and the stage update behind it, one launch
            if ((st = queued(launch_accel(pv_, stream_, n_, npad_, P_[pp_].p, nullptr, ASR_.p, force_kind(), lo_, hi_, &kd)))) return st;
            evals_++;
        } else if ((st = queued(launch_kick_drift(stream_, n_, npad_, ASR_.p, V_.p, y_slot, kd.hb, kd.ha, mu_.p, P_[pp_ ^ 1].p)))) {
            return st;                                 // FSAL first stage: the acceleration is the previous step's last
        }
        if ((st = gather_packed(P_[pp_ ^ 1].p))) return st;
        pp_ ^= 1;
    }
    time_ = time_ + h;
    starter_i_ += 1;
    return EPH_OK;
}

// One SRKN stage on Double: the force-only launch (values) when the stage evaluates, then the compensated kick and drift
int NBodyIntegration::srkn_stage_double(double hb, double ha, double *y_slot, double *ye_slot, bool eval) {
    int st;
    if (eval) {
        if ((st = queued(launch_accel(pv_, stream_, n_, npad_, P_[pp_].p, nullptr, ASR_.p, force_kind(), lo_, hi_)))) return st;
        evals_++;
    }                                                  // (FSAL first stage: the acceleration is the previous step's last)
    const KickDriftDouble kd{ASR_.p, V_.p, VE_.p, y_slot, ye_slot, hb, ha, P_[pp_ ^ 1].p};
    if ((st = queued(launch_kick_drift_double(stream_, n_, npad_, kd)))) return st;
    pp_ ^= 1;
    return EPH_OK;
}

// LinearMultistepIntegrator::advance while `starter.step_count() < ORDER`   multistep/mod.rs:211-218
//   first call only : lm.advance_with(problem, no-op)   -> current_ddy = f(y0)
//   every call      : lm.advance_with(problem, starter) -> ring.front = (state, current_ddy); 4 sub-steps;
//                                                           current_ddy = f(y)
// Ring convention here: slot cur_ holds the newest level (Y and A); the level under construction is built in
// place in the slot that will become the new front.
int NBodyIntegration::startup_macro_step() {
    if (time_ >= bound_) return EPH_BOUND_REACHED;
    if (time_ + h_ == time_) return EPH_STEP_SIZE_UNDERFLOW;
    int st;
    if (starter_i_ / (uint32_t)substeps_ == 0) {
        if ((st = queued(launch_accel(pv_, stream_, n_, npad_, P_[pp_].p, nullptr, Aslot(cur_), force_kind(), lo_, hi_)))) return st;
        evals_++;
    }
    const int nslot = (cur_ + L_ - 1) % L_;
    if ((st = queued(launch_copy3(stream_, n_, npad_, Yslot(cur_), Yslot(nslot))))) return st;
    if (compensated_ && (st = queued(launch_copy3(stream_, n_, npad_, YEslot(cur_), YEslot(nslot))))) return st;   // clone_from copies the error parts
    cur_ = nslot;   // from here on the working state is the new front, as in the reference after the clone_from
    for (int s = 0; s < substeps_; ++s)
        if ((st = srkn_step(h_sub_, Yslot(nslot)))) return st;
    if ((st = queued(launch_accel(pv_, stream_, n_, npad_, P_[pp_].p, nullptr, Aslot(nslot), force_kind(), lo_, hi_)))) return st;
    evals_++;
    return EPH_OK;
}

// ---- The start-up in one launch (k_lm_startup_small) -------------------------------------------------------------------------
int64_t NBodyIntegration::startup_small_steps(int64_t want, double *t_after) const {
    if (!is_multistep_ || started() || n_ < 1 || n_ > kGangMaxN || sharded() || (path_ != 0 && path_ != 2)) return 0;
    if (starter_i_ % (uint32_t)substeps_ != 0) return 0;               // a macro step abandoned between two substeps
    const int64_t m = std::min(want, startup_left());
    double t = time_;
    for (int64_t d = 0; d < m; ++d) {
        if (t >= bound_ || t + h_ == t) return 0;                       // startup_macro_step's two tests
        for (int s = 0; s < substeps_; ++s) {
            if (t >= bound_ || t + h_sub_ == t) return 0;               // srkn_step's
            t = t + h_sub_;
        }
    }
    if (t_after) *t_after = t;
    return m > 0 ? m : 0;
}
// what a launch of the single-workgroup SRKN stage loop takes from the handle, for steps of size h (the substeps of the start-up, the
// steps of an SRKN method): Y / YE are the ring's base, which is slot 0 -- the SRKN working position, and where the start-up kernel's
// ring begins
void NBodyIntegration::fill_srkn_args(SrknSmallArgs &a, double h) const {
    a.n = n_; a.npad = npad_;
    a.stages = rk_.stages; a.fsal = rk_.fsal ? 1 : 0;
    a.starter_i = starter_i_;
    a.pos[0] = P_[pp_].p; a.pos[1] = P_[pp_ ^ 1].p;
    a.Y = Y_.p; a.V = V_.p; a.ASR = ASR_.p;
    a.YE = compensated_ ? YE_.p : nullptr; a.VE = compensated_ ? VE_.p : nullptr;
    for (int s = 0; s < rk_.stages; ++s) { a.hb[s] = h * rk_.B[s]; a.ha[s] = h * rk_.A[s]; }
    a.samp = samp_;
}
void NBodyIntegration::fill_startup_args(LmStartupArgs &g, int64_t m) const {
    g = LmStartupArgs{};
    fill_srkn_args(g.s, h_sub_);
    g.A = A_.p;
    g.L = L_; g.cur = cur_;
    g.m = (int)m; g.substeps = substeps_;
}
void NBodyIntegration::commit_startup(int64_t m, double t_after) {
    const uint64_t steps = (uint64_t)m * (uint64_t)substeps_;
    // the first force evaluation and the FSAL table's first stage of the very first substep; per substep the other stages; per macro
    // step the closing force
    evals_ += (starter_i_ == 0 ? 1 + (rk_.fsal ? 1 : 0) : 0) + steps * srkn_step_evals() + (uint64_t)m;
    if ((steps * (uint64_t)rk_.stages) & 1) pp_ ^= 1;                  // every stage swaps the packed position buffers
    turn_ring(m);
    starter_i_ += (uint32_t)steps;
    time_ = t_after;
}
int NBodyIntegration::startup_batch(int64_t m, double t_after) {
    LmStartupArgs g;
    fill_startup_args(g, m);
    if (const int st = launch_lm_startup_small(pv_, stream_, g, compensated_)) return st;
    count_launches(1);
    commit_startup(m, t_after);
    return EPH_OK;
}

// The k-fold replay of `time = time + h` below reproduces the reference's bits of `problem.time`; the two tests inside it
// almost never fire. When they provably cannot -- no bound, and |h| far above the spacing of doubles at any |t| the k steps
// can reach -- the answer is k without the loop, and the replay that updates time_ can run AFTER the launch, under the kernel
// (lm_batch). It matters for gangs: 256 systems x 100 000 steps is 77 M dependent additions (three passes: gang_ready,
// advance, the update) that the device sat waiting for -- the "gang of 256 steps 1.31 us against 0.78 alone" of round 3
// (profiles/r04_small_kernel_evidence.md: every workgroup of the gang took 0.89 us per step; the rest was this loop).
bool NBodyIntegration::steps_certain(int64_t k) const {
    if (!(bound_ == INFINITY) || !std::isfinite(time_) || !std::isfinite(h_) || h_ == 0.0 || k < 0) return false;
    const double reach = (std::fabs(time_) + (double)k * std::fabs(h_)) * 1.000001;   // |t| stays below this (k <= 2^30 roundings of 2^-53)
    // t + h == t needs |h| <= ulp(t) / 2 <= 2^-53 |t|
    return std::isfinite(reach) && std::fabs(h_) > reach * 4.440892098500626e-16;
}

int64_t NBodyIntegration::steps_available(int64_t k, int *status_after) const {
    if (steps_certain(k)) { *status_after = EPH_OK; return k; }
    double t = time_;
    int64_t s = 0;
    *status_after = EPH_OK;
    for (; s < k; ++s) {
        if (t >= bound_) { *status_after = EPH_BOUND_REACHED; break; }
        if (t + h_ == t) { *status_after = EPH_STEP_SIZE_UNDERFLOW; break; }
        t = t + h_;
    }
    return s;
}

// Every pending pair has BOTH events recorded (TimingGuard::close pushes a pair only behind its closing record). A pair whose query fails
// (a device error in between) is skipped and recycled with the others: the list is always emptied, so one bad interval can neither
// stop the accumulation nor fill the list until every later batch fails (advisor, round 4).
int NBodyIntegration::resolve_timing() {
    int st = EPH_OK;
    for (auto &e : ev_pending_) {
        float ms = 0;
        if (hipEventSynchronize(e.second) == hipSuccess && hipEventElapsedTime(&ms, e.first, e.second) == hipSuccess) {
            kernel_ms_ += ms;
        } else {
            set_last_error("timing events", hipGetLastError());
            st = EPH_ERR_HIP;
        }
    }
    ev_free_.insert(ev_free_.end(), ev_pending_.begin(), ev_pending_.end());
    ev_pending_.clear();
    return st;
}

// One timed interval on a handle's stream (enable_timing): a pair of events around a batch's launches, read later (host.h). What
// holds for the two event lists, stated here once:
//   * a pair joins the pending list only behind its closing record (close): resolve_timing relies on both events being recorded;
//   * every return between open and a successful close -- a failed opening record too -- hands the pair back to the free list;
//   * the pending list is resolved when 1024 pairs wait (a failed interval is dropped there, not returned here).
struct NBodyIntegration::TimingGuard {
    NBodyIntegration &ig;
    std::pair<hipEvent_t, hipEvent_t> ev{nullptr, nullptr};   // null: not open (this batch is not timed), or closed
    ~TimingGuard() { if (ev.second) ig.ev_free_.push_back(ev); }
    int open() {
        if (!ig.timing_) return EPH_OK;
        if (ig.ev_pending_.size() >= 1024) (void)ig.resolve_timing();
        if (!ig.ev_free_.empty()) { ev = ig.ev_free_.back(); ig.ev_free_.pop_back(); }
        else { EPH_HIP(hipEventCreate(&ev.first)); EPH_HIP(hipEventCreate(&ev.second)); }
        if (hipEventRecord(ev.first, ig.stream_) == hipSuccess) return EPH_OK;
        set_last_error("hipEventRecord", hipGetLastError());
        return EPH_ERR_HIP;
    }
    int close() {
        if (!ev.second) return EPH_OK;
        EPH_HIP(hipEventRecord(ev.second, ig.stream_));
        ig.ev_pending_.push_back(ev);
        ev = {nullptr, nullptr};
        return EPH_OK;
    }
};

// what every steady batch's launches take from the handle: sizes, rings, weights, step sizes, the force kernel's kind
void NBodyIntegration::fill_lm_args(LmArgs &a) const {
    a.n = n_; a.npad = npad_; a.L = L_;
    a.Y = Y_.p; a.A = A_.p; a.V = V_.p;
    for (int j = 0; j < L_; ++j) { a.wa[j] = lm_.wa[j]; a.wb[j] = lm_.wb[j]; a.cw[j] = lm_.cw[j]; }
    a.h = h_;
    a.hh = h_ * h_ * lm_.inv_beta_d;     // h * h * Ratio::from_recip(C::BETA_D)
    a.hc = h_ * lm_.inv_cowell_d;        // h * Ratio::from_recip(Self::BETA_D)
    a.kind = force_kind();
}
void NBodyIntegration::point_lm_args(LmArgs &a) const {
    a.cur = cur_;
    a.pos_cur = P_[pp_].p;
    a.pos_next = P_[pp_ ^ 1].p;
}
void NBodyIntegration::next_level(LmArgs &a) {
    pp_ ^= 1;
    cur_ = (cur_ + L_ - 1) % L_;
    point_lm_args(a);
}

// The frame of a batch of k steps, stated once for lm_batch, lm_batch_double and srkn_batch: a timed interval around the launches that
// queue(launches) makes (it returns a status and says how many they were), then the k-fold `problem.time = problem.time + h` -- AFTER
// the launches are queued, so that it runs under the kernel (steps_certain). A handle's own batches only: a gang's members never come
// through here (gang_frame below: fill_gang_args / commit_gang).
template <typename Queue>
int NBodyIntegration::batch_frame(int64_t k, Queue &&queue) {
    int st;
    TimingGuard timing{*this};
    if ((st = timing.open())) return st;
    uint64_t launches = 0;
    if ((st = queue(launches))) return st;
    if (timing_) kernel_launches_ += launches;
    count_launches(launches);
    if ((st = timing.close())) return st;
    for (int64_t s = 0; s < k; ++s) time_ = time_ + h_;
    return EPH_OK;
}

// k x ELM2::advance on Double. At most 32 bodies (and not path 1): ONE launch of the single-workgroup kernel. Otherwise, per step,
// the predictor of the next level, the force-only launch on its values, Cowell's velocity -- the last two element-wise pieces of
// step s and the predictor of step s + 1 in one launch (double_step.hip).
int NBodyIntegration::lm_batch_double(int64_t k) {
    LmDoubleArgs d{};
    LmArgs &a = d.a;
    fill_lm_args(a);
    a.lo = 0; a.hi = n_;
    d.YE = YE_.p; d.VE = VE_.p;
    if (path_ == 2 && n_ > kGangMaxN) {
        set_last_error_text("a <Double> handle takes the single-workgroup kernel up to 32 bodies");
        return EPH_ERR_UNSUPPORTED;
    }
    const bool persistent = n_ <= kGangMaxN && path_ != 1;
    const int st = batch_frame(k, [&](uint64_t &launches) -> int {
        int st;
        point_lm_args(a);
        if (persistent) {
            if ((st = launch_lm_double_small(pv_, stream_, d, k))) return st;
            turn_ring(k);
            launches = 1;
            return EPH_OK;
        }
        a.do_predict = 1;
        d.do_cowell = 0;
        if ((st = queued(launch_lm_double_step(stream_, d)))) return st;   // the first step's predictor alone
        for (int64_t s = 1; s <= k; ++s) {
            next_level(a);
            if ((st = queued(launch_accel(pv_, stream_, n_, npad_, P_[pp_].p, nullptr, Aslot(cur_), force_kind(), 0, n_)))) return st;
            a.do_predict = s < k;
            d.do_cowell = 1;
            if ((st = launch_lm_double_step(stream_, d))) return st;
        }
        launches = (uint64_t)k;
        return EPH_OK;
    });
    if (st) return st;
    lm_i_ += (uint32_t)k;
    evals_ += (uint64_t)k;
    return EPH_OK;
}

// k x ELM2::advance   second_order/mod.rs:90-131
int NBodyIntegration::lm_batch(int64_t k) {
    if (compensated_) return lm_batch_double(k);
    LmArgs a{};
    fill_lm_args(a);
    a.lo = lo_; a.hi = hi_;
    a.samp = samp_;
    int st;
    const bool fast = path_ == EPH_PATH_FAST || path_ == EPH_PATH_FAST_RSQ || path_ == EPH_PATH_F32_PAIRS;
    // on a target partition only the binary32 pair arithmetic runs (BASELINE configs[4] as stated); fast / fast-rsq stay single-device
    if (fast && (n_ <= kSmallN || (sharded() && path_ != EPH_PATH_F32_PAIRS))) return EPH_ERR_UNSUPPORTED;
    const bool f32_sharded = sharded() && path_ == EPH_PATH_F32_PAIRS;
    if (fast && !fast_partial_.p) {
        DevBuf<double> partial;
        if ((st = partial.alloc(fast_partial_doubles(npad_)))) return st;
        // the arrival tickets of the one-launch step start at 0 (the last arriver of every block puts its ticket back); the handle
        // takes the scratch only with that clear queued, so no later call steps on tickets that were never zeroed
        const size_t toff = fast_ticket_offset_doubles(npad_);
        EPH_HIP(hipMemsetAsync(partial.p + toff, 0, sizeof(double) * (fast_partial_doubles(npad_) - toff), stream_));
        fast_partial_.swap(partial);
    }
    if (path_ == EPH_PATH_F32_PAIRS && !posf_.p) {
        if ((st = posf_.alloc((size_t)4 * npad_))) return st;
    }
    const bool persistent = n_ <= kSmallN && path_ != 1 && path_ != 3 && !fast;
    if (path_ == 2 && n_ > kSmallN) return EPH_ERR_UNSUPPORTED;
    st = batch_frame(k, [&](uint64_t &launches) -> int {
        int st;
        point_lm_args(a);
        if (persistent) {
            if ((st = launch_lm_persistent(pv_, stream_, a, k))) return st;
            turn_ring(k);
            launches = 1;
            return EPH_OK;
        }
        // a handle that can neither take the single-workgroup kernels nor exchange positions leaves the prediction of the step
        // after the batch behind (host.h predicted_): one launch and one launch boundary less per call
        const bool leave_prediction = n_ > kSmallN && !sharded();
        if (!predicted_) {
            if ((st = queued(launch_lm_predict(stream_, a)))) return st;
            if ((st = gather_packed(a.pos_next))) return st;
        }
        predicted_ = false;
        for (int64_t s = 1; s <= k; ++s) {
            next_level(a);
            a.do_predict = s < k || leave_prediction;
            a.step = (uint32_t)s;
            if (f32_sharded) {
                // this rank's rows of the binary32 copy (16 B per body: SURVEY 8(e)'s f32x4), one all-gather of them, then the rank's
                // targets against all sources in the single-device slice order. The f64 packed positions of the OTHER ranks' bodies
                // are not needed between the steps of a batch (the batch's first prediction gathers them once, above).
                if ((st = queued(launch_lm_step_fast(pv_, stream_, a, fast_partial_.p, false, posf_.p, 1, lo_, slice_)))) return st;
                if ((st = xch_->all_gather_inplace(posf_.p, sizeof(float) * 4 * (size_t)slice_, stream_))) return st;
                if ((st = launch_lm_step_fast(pv_, stream_, a, fast_partial_.p, false, posf_.p, 2))) return st;
                continue;
            }
            if ((st = fast ? launch_lm_step_fast(pv_, stream_, a, fast_partial_.p, path_ == EPH_PATH_FAST_RSQ,
                                                 path_ == EPH_PATH_F32_PAIRS ? posf_.p : nullptr)
                           : launch_lm_step(pv_, stream_, a)))
                return st;
            if (s < k && (st = gather_packed(a.pos_next))) return st;
        }
        predicted_ = leave_prediction;
        launches = (uint64_t)k;
        return EPH_OK;
    });
    if (st) return st;
    lm_i_ += (uint32_t)k;
    evals_ += (uint64_t)k;
    return EPH_OK;
}

// k x srkn_step(h_, Yslot(0)) in ONE launch of the single-workgroup kernel (srkn_small_ready); the caller has established that
// neither of srkn_step's two tests fires in these k steps (steps_available)
int NBodyIntegration::srkn_batch(int64_t k) {
    SrknSmallArgs a{};
    fill_srkn_args(a, h_);
    const int st = batch_frame(k, [&](uint64_t &launches) -> int {
        launches = 1;
        return compensated_ ? launch_srkn_double_small(pv_, stream_, a, k) : launch_srkn_small(pv_, stream_, a, k);
    });
    if (st) return st;
    // the rest of the bookkeeping of k calls of srkn_step
    evals_ += (uint64_t)k * srkn_step_evals() + (rk_.fsal && starter_i_ == 0 ? 1 : 0);
    starter_i_ += (uint32_t)k;
    return EPH_OK;
}

int NBodyIntegration::advance(int64_t n_steps, int64_t *done_out) { return advance_from(0, n_steps, done_out); }

// (advance_many continues here behind a start-up gang: `done` of the call's n_steps are taken, *done_out counts from there on)
int NBodyIntegration::advance_from(int64_t done, int64_t n_steps, int64_t *done_out) {
    if (failed_) { if (done_out) *done_out = 0; return failed_; }     // a gang launch with this member failed once something was queued (gang_frame)
    EPH_HIP(hipSetDevice(device_));
    const int64_t done_before = done;
    int st = EPH_OK;
    const SampleArgs samp = samp_;
    while (done < n_steps) {
        // An SRKN method at no more than 32 bodies takes its steps in one launch. The kernel's sampling countdown starts at this
        // advance()'s first step, so a sampled call that comes round again -- more than 2^30 steps -- finishes step by step.
        const bool srkn_small = srkn_small_ready() && !(done > 0 && samp.period);
        if (!is_multistep_ && !srkn_small) {
            if ((st = srkn_step(h_, Yslot(0)))) break;
            done++;
            if ((st = queued(launch_sample(stream_, n_, npad_, Yslot(0), samp, (uint32_t)done), samp.period != nullptr))) break;
        } else if (is_multistep_ && !started()) {
            // The start-up's macro steps in one launch where they can be. The kernel's sampling countdown starts at this advance()'s
            // first step, as the SRKN kernel's above.
            double t_after = 0.0;
            const int64_t m = done > 0 && samp.period ? 0 : startup_small_steps(n_steps - done, &t_after);
            if (m > 0) {
                if ((st = startup_batch(m, t_after))) break;
                done += m;
                continue;
            }
            if ((st = startup_macro_step())) break;
            done++;
            if ((st = queued(launch_sample(stream_, n_, npad_, Yslot(cur_), samp, (uint32_t)done), samp.period != nullptr))) break;
        } else {
            // the batching regimes: the steps that can be taken, below 2^31 at a time (the single-workgroup kernels take a 32-bit
            // step index for sampling)
            int after = EPH_OK;
            const int64_t want = std::min<int64_t>(n_steps - done, (int64_t)1 << 30);
            const int64_t k = steps_available(want, &after);
            if (k > 0 && is_multistep_ && done > 0 && samp.period) {
                // Sampling phases are relative to the start of this advance(). Start-up and steady state in one sampled call
                // (rare): finish one step at a time, sampling between the batches
                samp_ = SampleArgs{};
                for (int64_t s = 0; s < k && !st; ++s) {
                    st = lm_batch(1);
                    if (!st) {
                        done++;
                        st = queued(launch_sample(stream_, n_, npad_, Yslot(cur_), samp, (uint32_t)done), samp.period != nullptr);
                    }
                }
                samp_ = samp;
                if (st) break;
            } else if (k > 0) {
                if ((st = srkn_small ? srkn_batch(k) : lm_batch(k))) break;
                done += k;
            }
            if (k < want) { st = after; break; }
        }
    }
    samp_ = SampleArgs{};
    if (done_out) *done_out = done - done_before;
    return st;
}

bool NBodyIntegration::gang_ready(int64_t k) const {
    if (compensated_ || !is_multistep_ || !started() || sharded() || n_ > kGangMaxN || n_ <= 0 || (path_ != 0 && path_ != 2)) return false;
    if (k <= 0 || k > ((int64_t)1 << 30)) return false;
    int after = EPH_OK;
    return steps_available(k, &after) == k;
}

// ---- The gangs of advance_many -------------------------------------------------------------------------------------------------
// One gang launch, stated once for the start-up gang (LmStartupArgs, k_lm_startup_small), the steady one (LmArgs, k_lm_small) and the
// symplectic one (SrknGangArgs, k_srkn_small_many): the
// members igs[0 .. count), all on the device of the lead igs[0], a workgroup each in ONE launch on the lead's stream. `ga` is the
// lead's argument array of the gang's kind. fill(host[i], i) writes member i's launch arguments and moves nothing; launch(device
// array) queues the kernel on the lead's stream; commit(i) is member i's host bookkeeping, which runs under the kernel. A `timed`
// frame whose lead has enable_timing() on brackets the launch with the lead's event pair and waits for it (the steady and the
// symplectic gang; the start-up gang is not timed: kernel_time counts steady-state kernels). Otherwise not synchronised: like eph_nbody_advance, the
// call only queues.
template <typename Args, typename Fill, typename Launch, typename Commit>
int NBodyIntegration::gang_frame(NBodyIntegration *const *igs, int count, GangArgs<Args> &ga, bool timed, Fill &&fill, Launch &&launch,
                                 Commit &&commit) {
    NBodyIntegration &lead = *igs[0];
    EPH_HIP(hipSetDevice(lead.device_));
    // everything that can fail for lack of resources happens BEFORE anything is queued and before any handle's bookkeeping moves
    if (const int st = ga.dev.reserve((size_t)count)) return st;
    if (!lead.gang_ev_) EPH_HIP(hipEventCreateWithFlags(&lead.gang_ev_, hipEventDisableTiming));
    if (!lead.gang_copy_ev_) EPH_HIP(hipEventCreateWithFlags(&lead.gang_copy_ev_, hipEventDisableTiming));
    // the previous gang's argument copy out of a pinned array (either kind's) must have completed before one is rewritten or freed
    EPH_HIP(hipEventSynchronize(lead.gang_copy_ev_));
    if (ga.host_count < (size_t)count) {
        if (ga.host) (void)hipHostFree(ga.host);
        ga.host = nullptr;
        ga.host_count = 0;
        const size_t want = (size_t)count + (size_t)count / 2;
        EPH_HIP(hipHostMalloc((void **)&ga.host, sizeof(Args) * want, hipHostMallocDefault));
        ga.host_count = want;
    }
    for (int i = 0; i < count; ++i) fill(ga.host[i], i);
    // From the first queued operation on, a failure marks every member failed (every later call returns the status) instead of
    // handing the handles back as if nothing had happened: their streams may be half joined, and behind the launch their bookkeeping
    // is ahead of a device state nobody vouches for.
    auto fail = [&](int status) {
        for (int i = 0; i < count; ++i) igs[i]->failed_ = status;
        return status;
    };
#define EPH_GANG_HIP(call) do { hipError_t e_ = (call); if (e_ != hipSuccess) { set_last_error(#call, e_); return fail(EPH_ERR_HIP); } } while (0)
    // the launch goes on the lead's stream, behind whatever the other members still have in flight on theirs
    for (int i = 1; i < count; ++i) {
        EPH_GANG_HIP(hipEventRecord(lead.gang_ev_, igs[i]->stream_));
        EPH_GANG_HIP(hipStreamWaitEvent(lead.stream_, lead.gang_ev_, 0));
    }
    EPH_GANG_HIP(hipMemcpyAsync(ga.dev.p, ga.host, sizeof(Args) * (size_t)count, hipMemcpyHostToDevice, lead.stream_));
    EPH_GANG_HIP(hipEventRecord(lead.gang_copy_ev_, lead.stream_));
    timed = timed && lead.timing_;
    if (timed) EPH_GANG_HIP(hipEventRecord(lead.ev0_, lead.stream_));
    if (const int st = launch(ga.dev.p)) return fail(st);
    count_launches(1);
    for (int i = 0; i < count; ++i) commit(i);                          // host bookkeeping under the kernel
    if (timed) {
        EPH_GANG_HIP(hipEventRecord(lead.ev1_, lead.stream_));
        EPH_GANG_HIP(hipEventSynchronize(lead.ev1_));
        float ms = 0;
        EPH_GANG_HIP(hipEventElapsedTime(&ms, lead.ev0_, lead.ev1_));
        lead.kernel_ms_ += ms;
    }
    // the members' streams go on behind the launch
    EPH_GANG_HIP(hipEventRecord(lead.gang_ev_, lead.stream_));
    for (int i = 1; i < count; ++i) EPH_GANG_HIP(hipStreamWaitEvent(igs[i]->stream_, lead.gang_ev_, 0));
#undef EPH_GANG_HIP
    return EPH_OK;
}

// The start-up macro steps of `count` members, m[i] of member i, in one gang launch; the caller has established each m[i] by
// startup_small_steps, which also gave t_after[i]
int NBodyIntegration::startup_gang(NBodyIntegration *const *igs, int count, const int64_t *m, const double *t_after) {
    for (int i = 0; i < count; ++i)
        if (m[i] < 1 || m[i] > igs[i]->startup_left()) return EPH_ERR_BAD_ARGUMENT;
    NBodyIntegration &lead = *igs[0];
    return gang_frame(igs, count, lead.startup_, false,
                      [&](LmStartupArgs &g, int i) { igs[i]->fill_startup_args(g, m[i]); },
                      [&](const LmStartupArgs *args) { return launch_lm_startup_small_many(lead.pv_, lead.stream_, args, count); },
                      [&](int i) { igs[i]->commit_startup(m[i], t_after[i]); });
}

// The steady gang's member: what advance(k) comes to on a handle that gang_ready(k) has accepted -- lm_batch's single-workgroup
// launch in batch_frame -- in two halves, the launch arguments (nothing moves) and the bookkeeping once the launch is queued
void NBodyIntegration::fill_gang_args(LmArgs &a) const {
    static const int dbg = [] { const char *e = getenv("EPH_DEBUG_SMALL"); return e ? atoi(e) : 0; }();   // tuning switches of k_lm_small
    a = LmArgs{};                                                       // (do_predict and step stay 0, as in lm_batch's one launch)
    fill_lm_args(a);
    a.lo = lo_; a.hi = hi_;
    a.samp = samp_;
    point_lm_args(a);
    a.wg_flags = dbg;
}
void NBodyIntegration::commit_gang(int64_t k) {
    turn_ring(k);
    lm_i_ += (uint32_t)k;
    evals_ += (uint64_t)k;
    if (timing_) kernel_launches_ += 1;                                 // every timed member counts the shared launch; the lead alone times it
    samp_ = SampleArgs{};
    for (int64_t s = 0; s < k; ++s) time_ = time_ + h_;                 // behind the launch, under the kernel (steps_certain)
}

// The SRKN gang's member: what srkn_batch(k) comes to -- one launch of the single-workgroup kernel in batch_frame -- in two halves,
// as the steady gang's above. The block carries the member's own k.
int64_t NBodyIntegration::srkn_gang_steps(int64_t k, int *status_after) const {
    *status_after = EPH_OK;
    if (!srkn_small_ready() || failed_ || k <= 0) return 0;
    return steps_available(std::min<int64_t>(k, (int64_t)1 << 30), status_after);
}
void NBodyIntegration::fill_srkn_gang_args(SrknGangArgs &g, int64_t k) const {
    g = SrknGangArgs{};
    fill_srkn_args(g.s, h_);
    g.nsteps = (long long)k;
    // the terms launch_srkn_small / launch_srkn_double_small hold their one block to: the gang's blocks are in device memory by the
    // time dispatch.cpp sees them, so they are held to them here, on the host twin
    assert(g.s.n >= 1 && g.s.n <= kGangMaxN && g.s.stages >= 1 && g.s.stages <= 32 && g.nsteps >= 1 && (!compensated_ || (g.s.YE && g.s.VE)));
}
void NBodyIntegration::commit_srkn_gang(int64_t k) {
    evals_ += (uint64_t)k * srkn_step_evals() + (rk_.fsal && starter_i_ == 0 ? 1 : 0);
    starter_i_ += (uint32_t)k;
    if (timing_) kernel_launches_ += 1;                                 // as commit_gang: the lead alone times the shared launch
    samp_ = SampleArgs{};
    for (int64_t s = 0; s < k; ++s) time_ = time_ + h_;                 // behind the launch, under the kernel (steps_certain)
}

// The symplectic members of an advance_many call. Round by round (one round unless k exceeds 2^30) the members that can take steps
// in one launch of the single-workgroup kernel split into the plain group and the `<Double>` group; a group of at least two is one
// gang_frame on its first member, everybody else finishes in its own advance_from. A sampled member joins a launch in the first
// round only (the kernel's countdown starts at the call's first step: advance_from's rule). status[i]: what advance(k) on member i
// would have returned. The return value is a frame's failure, which ends the call.
int NBodyIntegration::advance_many_srkn(NBodyIntegration *const *igs, int count, int64_t k, int *status) {
    std::vector<int64_t> done((size_t)count, 0);
    std::vector<char> open((size_t)count, 1), ganged((size_t)count, 0);
    std::vector<NBodyIntegration *> mem;
    std::vector<int> who, after;
    std::vector<int64_t> ks;
    std::vector<SampleArgs> samp;
    for (int left = count, round = 0; left > 0; ++round) {
        std::fill(ganged.begin(), ganged.end(), 0);
        for (int kind = 0; kind < 2; ++kind) {                          // plain, then `<Double>`
            mem.clear(); who.clear(); after.clear(); ks.clear(); samp.clear();
            for (int i = 0; i < count; ++i) {
                NBodyIntegration &ig = *igs[i];
                if (!open[(size_t)i] || (int)ig.compensated_ != kind) continue;
                int after_i = EPH_OK;
                const int64_t k_i = round > 0 && ig.samp_.period ? 0 : ig.srkn_gang_steps(k - done[(size_t)i], &after_i);
                if (k_i <= 0 || (!mem.empty() && !ig.shares_srkn_launch_with(*mem[0]))) continue;
                mem.push_back(&ig); who.push_back(i); after.push_back(after_i); ks.push_back(k_i); samp.push_back(ig.samp_);
            }
            if (mem.size() < 2) continue;
            NBodyIntegration &lead = *mem[0];
            const int n = (int)mem.size();
            const int st = gang_frame(mem.data(), n, lead.srkn_gang_, true,
                                      [&](SrknGangArgs &g, int j) { mem[(size_t)j]->fill_srkn_gang_args(g, ks[(size_t)j]); },
                                      [&](const SrknGangArgs *args) {
                                          return kind ? launch_srkn_double_small_many(lead.pv_, lead.stream_, args, n)
                                                      : launch_srkn_small_many(lead.pv_, lead.stream_, args, n);
                                      },
                                      [&](int j) { mem[(size_t)j]->commit_srkn_gang(ks[(size_t)j]); });
            if (st) return st;
            for (size_t j = 0; j < mem.size(); ++j) {
                const size_t i = (size_t)who[j];
                const int64_t want = std::min<int64_t>(k - done[i], (int64_t)1 << 30);
                done[i] += ks[j];
                ganged[i] = 1;
                if (ks[j] < want) status[i] = after[j];                 // its bound, or t + h == t: where its own advance(k) stops
                if (ks[j] < want || done[i] == k) { open[i] = 0; --left; }
                else mem[j]->samp_ = samp[j];                            // it goes round again: the call's schedule is still its own
            }
        }
        // whoever is not in a launch of this round finishes alone; what stays open took 2^30 steps in a launch and has more to take
        for (int i = 0; i < count; ++i) {
            if (!open[(size_t)i] || ganged[(size_t)i]) continue;
            status[i] = igs[i]->advance_from(done[(size_t)i], k, nullptr);
            open[(size_t)i] = 0;
            --left;
        }
    }
    return EPH_OK;
}

int NBodyIntegration::advance_many(NBodyIntegration *const *igs, int count, int64_t k) {
    if (count < 0 || (count > 0 && !igs) || k < 0) return EPH_ERR_BAD_ARGUMENT;
    if (count == 0 || k == 0) return EPH_OK;
    for (int i = 0; i < count; ++i) {
        if (!igs[i]) return EPH_ERR_BAD_ARGUMENT;
        for (int j = 0; j < i; ++j)
            if (igs[j] == igs[i]) return EPH_ERR_BAD_ARGUMENT;          // a system cannot be in the gang twice
    }
    // The symplectic members first, then the others as a call that consists of them alone; the first status in member order.
    std::vector<NBodyIntegration *> part[2];
    std::vector<int> who[2];
    for (int i = 0; i < count; ++i) {
        part[igs[i]->is_multistep_ ? 1 : 0].push_back(igs[i]);
        who[igs[i]->is_multistep_ ? 1 : 0].push_back(i);
    }
    std::vector<int> status((size_t)count, EPH_OK), sub;
    for (int p = 0; p < 2; ++p) {
        if (part[p].empty()) continue;
        sub.assign(part[p].size(), EPH_OK);
        const int st = p == 0 ? advance_many_srkn(part[p].data(), (int)part[p].size(), k, sub.data())
                              : advance_many_multistep(part[p].data(), (int)part[p].size(), k, sub.data());
        if (st) return st;
        for (size_t j = 0; j < sub.size(); ++j) status[(size_t)who[p][j]] = sub[j];
    }
    for (int i = 0; i < count; ++i)
        if (status[(size_t)i]) return status[(size_t)i];
    return EPH_OK;
}

int NBodyIntegration::advance_many_multistep(NBodyIntegration *const *igs, int count, int64_t k, int *status) {
    // 1. The start-up. Every plain member that can take macro steps in one launch (startup_small_steps) takes m_i = min(k, macro
    // steps left) of them; at least two that can share a launch do. Anyone else -- a <Double> member too -- does its start-up in
    // its own advance below.
    std::vector<int64_t> taken((size_t)count, 0);
    {
        std::vector<NBodyIntegration *> mem;
        std::vector<int> who;
        std::vector<int64_t> ms;
        std::vector<double> ts;
        for (int i = 0; i < count; ++i) {
            NBodyIntegration &ig = *igs[i];
            double t = 0.0;
            const int64_t m = ig.failed_ || ig.compensated_ ? 0 : ig.startup_small_steps(k, &t);
            if (m <= 0 || (!mem.empty() && !ig.shares_launch_with(*mem[0]))) continue;
            mem.push_back(&ig); who.push_back(i); ms.push_back(m); ts.push_back(t);
        }
        if (mem.size() >= 2) {
            if (const int st = startup_gang(mem.data(), (int)mem.size(), ms.data(), ts.data())) return st;
            for (size_t j = 0; j < mem.size(); ++j) taken[(size_t)who[j]] = ms[j];
        }
    }
    // 2. What is left of k: the steady gang, when it is the same positive number for every member, no member's sampling schedule
    // has started counting in the start-up launch, and every member is ready for that many steps in a launch shared with the lead.
    const int64_t left = k - taken[0];
    bool gang = count > 1 && left > 0;
    for (int i = 0; i < count && gang; ++i)
        gang = taken[(size_t)i] == taken[0] && !(taken[(size_t)i] > 0 && igs[i]->samp_.period) && igs[i]->gang_ready(left) &&
               igs[i]->shares_launch_with(*igs[0]);
    if (!gang) {
        // the plain meaning: each member finishes its own call (the first status other than EPH_OK is the call's: advance_many)
        for (int i = 0; i < count; ++i) {
            if (taken[(size_t)i] == k) { igs[i]->samp_ = SampleArgs{}; continue; }
            status[i] = igs[i]->advance_from(taken[(size_t)i], k, nullptr);
        }
        return EPH_OK;
    }
    for (int i = 0; i < count; ++i)
        if (igs[i]->failed_) return igs[i]->failed_;
    NBodyIntegration &lead = *igs[0];
    return gang_frame(igs, count, lead.gang_, true,
                      [&](LmArgs &a, int i) { igs[i]->fill_gang_args(a); },
                      [&](const LmArgs *args) { return launch_lm_small_many(lead.pv_, lead.stream_, args, count, lead.L_, left); },
                      [&](int i) { igs[i]->commit_gang(left); });
}

// The read-back of get_state and get_acc. One device: the transposition kernels write straight into a pinned, device-mapped staging
// buffer of this call's own (a second handle's read-back does not wait for ours) -- one synchronisation, no copy-engine submissions
// (the reference's Integration reads the state after every step: 115-119 -> 63 us per step at N = 4096 with this,
// scripts/time_boundary.py). Sharded: every rank contributes its bodies to stage_, array by array.
int NBodyIntegration::read_back(const double *a_dev, double *a, const double *b_dev, double *b) {
    const double *const dev[2] = {a_dev, b_dev};
    double *const host[2] = {a, b};
    const size_t nd = 3 * (size_t)n_;
    int st;
    if (!xch_) {
        PinnedStage stage(sizeof(double) * nd * ((a ? 1 : 0) + (b ? 1 : 0)));
        if (stage.status()) return stage.status();
        StreamIdleOnExit idle(stream_);
        double *d = static_cast<double *>(stage.dev());
        for (int i = 0; i < 2; ++i)
            if (host[i]) { if ((st = launch_soa_to_aos(stream_, n_, npad_, dev[i], d))) return st; d += nd; }
        EPH_HIP(hipStreamSynchronize(stream_));
        idle.disarm();
        const double *h = static_cast<const double *>(stage.host());
        for (int i = 0; i < 2; ++i)
            if (host[i]) { std::memcpy(host[i], h, sizeof(double) * nd); h += nd; }
        return EPH_OK;
    }
    for (int i = 0; i < 2; ++i) {
        if (!host[i]) continue;
        if ((st = launch_soa_to_aos(stream_, n_, npad_, dev[i], stage_.p))) return st;
        if ((st = gather_stage())) return st;
        EPH_HIP(hipMemcpyAsync(host[i], stage_.p, sizeof(double) * nd, hipMemcpyDeviceToHost, stream_));
        EPH_HIP(hipStreamSynchronize(stream_));
        if ((st = xch_->poll_error())) return st;          // a peer that never delivered: the gathered rows are not data
    }
    return EPH_OK;
}

int NBodyIntegration::get_state(double *pos, double *vel, double *t, uint32_t *sc) {
    EPH_HIP(hipSetDevice(device_));
    if (n_ > 0 && (pos || vel))
        if (const int st = read_back(Yslot(is_multistep_ ? cur_ : 0), pos, V_.p, vel)) return st;
    if (t) *t = time_;
    if (sc) *sc = step_count();
    return EPH_OK;
}

int NBodyIntegration::get_acc(double *acc) {
    EPH_HIP(hipSetDevice(device_));
    if (!acc) return EPH_ERR_BAD_ARGUMENT;
    return n_ == 0 ? (int)EPH_OK : read_back(is_multistep_ ? Aslot(cur_) : ASR_.p, acc, nullptr, nullptr);
}

// seam 1: SecondOrderODE::eval for NewtonianGravity, host buffers in and out.
// The call's device buffers are grow-only scratch kept per device between calls (round 5): six hipMalloc / hipFree pairs per call --
// each hipFree a device synchronisation -- were most of what a call cost at the app's sizes. Round 6: a POOL of scratch sets per
// device, one leased per call with its own stream, so concurrent callers (the reference evaluates the RHS from every integrator
// thread) neither wait for each other nor share a buffer; the mutex covers the free list only. The scratch is ordinary library
// memory (eph_release_cached_memory does not touch it; it is a few MB at N = 65 536, and as many sets exist as calls ever overlapped).
namespace {
// grow-only device block taken from the driver directly: it lives as long as the process, so it must not count as a live allocation
// of the library's block cache (mem.cpp releases the cache with the LAST counted allocation on a device)
template <typename T>
struct RawScratch {
    T *p = nullptr;
    size_t count = 0;
    int reserve(size_t n) {
        if (n <= count) return EPH_OK;
        if (p) (void)hipFree(p);
        p = nullptr; count = 0;
        const size_t want = n + n / 2;
        hipError_t e = hipMalloc((void **)&p, want * sizeof(T));
        if (e != hipSuccess) { p = nullptr; set_last_error("hipMalloc (seam 1 scratch)", e); return e == hipErrorOutOfMemory ? EPH_ERR_OUT_OF_MEMORY : EPH_ERR_HIP; }
        count = want;
        return EPH_OK;
    }
};
struct AccelScratch {
    RawScratch<Body4> P;
    RawScratch<double> soa, init, out;
    hipStream_t stream = nullptr;
};
constexpr int kAccelDevices = 64;
std::mutex g_accel_mu;
std::vector<AccelScratch *> g_accel_free[kAccelDevices];             // (live as long as the process: destroying device memory at exit is the driver's job)
struct AccelLease {                                                  // one scratch set of `device` for the life of the object
    int device;
    AccelScratch *x = nullptr;
    explicit AccelLease(int dev) : device(dev) {
        std::lock_guard<std::mutex> lk(g_accel_mu);
        auto &fl = g_accel_free[device];
        if (!fl.empty()) { x = fl.back(); fl.pop_back(); }
        else x = new AccelScratch();
    }
    ~AccelLease() {
        std::lock_guard<std::mutex> lk(g_accel_mu);
        g_accel_free[device].push_back(x);
    }
    AccelLease(const AccelLease &) = delete;
    AccelLease &operator=(const AccelLease &) = delete;
};
}  // namespace
int accel_eval_device(int n, const double *pos, const double *mu, double *acc) {
    if (n < 0 || (n > 0 && (!pos || !mu || !acc))) return EPH_ERR_BAD_ARGUMENT;
    int st = check_device();
    if (st) return st;
    if (n == 0) return EPH_OK;
    const int npad = ((n + 63) / 64) * 64;
    int device = 0;
    EPH_HIP(hipGetDevice(&device));
    if (device < 0 || device >= kAccelDevices) return EPH_ERR_BAD_ARGUMENT;
    AccelLease lease(device);
    AccelScratch *x = lease.x;
    if (!x->stream) EPH_HIP(hipStreamCreateWithFlags(&x->stream, hipStreamNonBlocking));
    hipStream_t s = x->stream;
    if ((st = x->P.reserve(npad)) || (st = x->soa.reserve((size_t)3 * npad)) || (st = x->init.reserve((size_t)3 * npad)) ||
        (st = x->out.reserve((size_t)3 * npad)))
        return st;
    // Host buffers cross the bus through a pinned, device-mapped staging buffer (mem.cpp): the kernels read the caller's numbers and
    // write the result THROUGH it, so a call is five launches and one synchronisation -- no copy-engine submissions (three pageable
    // hipMemcpy in and one out were ~40 us of a 69 us call at 32 bodies: 29 us now; N = 4096: 177 us with the per-call allocations
    // of round 4, 136 without them, 75-80 through the staging buffer -- of which the force kernel is 40)
    const size_t nd = (size_t)n;
    PinnedStage stage(sizeof(double) * 7 * nd);
    if (stage.status()) return stage.status();
    StreamIdleOnExit idle(s);                         // an error return below leaves only once nothing in flight uses stage / scratch
    double *h = static_cast<double *>(stage.host()), *d = static_cast<double *>(stage.dev());
    std::memcpy(h, mu, sizeof(double) * nd);
    std::memcpy(h + nd, pos, sizeof(double) * 3 * nd);
    std::memcpy(h + 4 * nd, acc, sizeof(double) * 3 * nd);
    if ((st = launch_aos_to_soa(s, n, npad, d + nd, x->soa.p))) return st;
    if ((st = launch_pack(s, n, npad, x->soa.p, d, x->P.p))) return st;
    if ((st = launch_aos_to_soa(s, n, npad, d + 4 * nd, x->init.p))) return st;
    if ((st = launch_accel(default_pair_variant(), s, n, npad, x->P.p, x->init.p, x->out.p))) return st;
    if ((st = launch_soa_to_aos(s, n, npad, x->out.p, d + 4 * nd))) return st;
    EPH_HIP(hipStreamSynchronize(s));
    idle.disarm();
    std::memcpy(acc, h + 4 * nd, sizeof(double) * 3 * nd);
    return EPH_OK;
}

}  // namespace eph
