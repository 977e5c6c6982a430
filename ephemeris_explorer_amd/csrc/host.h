// host.h -- host-side mirror of the reference's operator surface for the hot path (C++; the reference's host
// language, Rust, is not available in this image -- see DESIGN.md). Names follow the reference:
//   integration::{Method, Integrator, IntegratorState, Integration, StepError}   integration/src/lib.rs
//   integration::multistep::{LinearMultistepIntegrator, Substepper, ELM2}         integration/src/multistep/
//   integration::runge_kutta::{FixedRungeKuttaIntegrator, SRKN}                    integration/src/runge_kutta/
//   ephemeris::{NBodyPropagator, SplineInterpolators, UniformSpline, Polynomial}   ephemeris/src/
// All numerical state lives on the device; the host keeps the scalar bookkeeping the reference keeps
// (time, bound, step counters, sampling counters) and replays it with the reference's f64 operations.
#pragma once
#include <algorithm>
#include <cmath>
#include <cstdint>
#include <deque>
#include <memory>
#include <mutex>
#include <string>
#include <vector>

#include "eph_internal.h"

namespace eph {

// device blocks through the library's cache of large allocations (mem.cpp): dev_alloc reuses a cached block of exactly `bytes`
// (contents unspecified) or calls hipMalloc; dev_free caches blocks of >= 64 MiB (after a device synchronisation, as hipFree has)
// up to the cache's cap and frees the rest; release_cached_memory returns the cache to the driver (bytes released).
int dev_alloc(size_t bytes, void **out);
void dev_free(void *p, size_t bytes);
size_t release_cached_memory();
size_t cached_memory_bytes();
// test hook (eph_debug.h): the nth dev_alloc from now on this thread returns EPH_ERR_OUT_OF_MEMORY ("injected allocation failure")
// before it makes any HIP call, and disarms the countdown; 0 disarms it. Returns what was left of the previous countdown.
int debug_fail_alloc(int nth);
// A pinned, device-mapped staging buffer taken from the library's pool for the life of the object (mem.cpp; one per concurrent user,
// so handles driven from distinct threads do not wait for each other): a kernel stores through dev(), the host reads host() after
// synchronising the kernel's stream. The stream must be idle with respect to the buffer before the object is destroyed.
class PinnedStage {
public:
    explicit PinnedStage(size_t bytes);
    ~PinnedStage();
    PinnedStage(const PinnedStage &) = delete;
    PinnedStage &operator=(const PinnedStage &) = delete;
    int status() const { return status_; }
    void *host() const { return host_; }
    void *dev() const { return dev_; }
    template <typename T>                              // where the host reads what a kernel stored through device address `d`
    const T *host_of(const T *d) const {
        return reinterpret_cast<const T *>(static_cast<const char *>(host_) + (reinterpret_cast<const char *>(d) - static_cast<const char *>(dev_)));
    }

private:
    void *host_ = nullptr, *dev_ = nullptr;
    size_t bytes_ = 0;
    int status_ = EPH_OK;
};

// Declared AFTER a PinnedStage (or a scratch lease) whose buffer kernels on `s` use: an early error return leaves the scope only once
// the stream is idle, so no kernel still in flight writes a buffer that has gone back to the pool. disarm() after the happy path's own
// synchronisation.
struct StreamIdleOnExit {
    hipStream_t s;
    bool armed = true;
    explicit StreamIdleOnExit(hipStream_t stream) : s(stream) {}
    StreamIdleOnExit(const StreamIdleOnExit &) = delete;
    StreamIdleOnExit &operator=(const StreamIdleOnExit &) = delete;
    ~StreamIdleOnExit() { if (armed) (void)hipStreamSynchronize(s); }
    void disarm() { armed = false; }
};

template <typename T>
struct DevBuf {   // owning device allocation
    T *p = nullptr;
    size_t count = 0;
    DevBuf() = default;
    DevBuf(const DevBuf &) = delete;
    DevBuf &operator=(const DevBuf &) = delete;
    ~DevBuf() { release(); }
    void release() {
        if (p) dev_free(p, count * sizeof(T));
        p = nullptr;
        count = 0;
    }
    int alloc(size_t n) {
        release();
        if (n == 0) n = 1;
        void *q = nullptr;
        const int st = dev_alloc(n * sizeof(T), &q);
        if (st) return st;
        p = static_cast<T *>(q);
        count = n;
        return EPH_OK;
    }
    int reserve(size_t n) { return n <= count ? EPH_OK : alloc(n + n / 2); }   // grow-only scratch; contents are lost
    // cannot fail: how a handle takes over a buffer that was allocated and filled aside (the old one leaves with `o`)
    void swap(DevBuf &o) noexcept { std::swap(p, o.p); std::swap(count, o.count); }
};
// a fresh allocation holding src[0, count) (DevBuf::alloc makes an empty one one element long): a blocking copy on the null stream
template <typename T>
int upload(DevBuf<T> &dst, const T *src, size_t count) {
    const int st = dst.alloc(count);
    if (st) return st;
    if (count) EPH_HIP(hipMemcpy(dst.p, src, sizeof(T) * count, hipMemcpyHostToDevice));
    return EPH_OK;
}
// a fresh allocation of src's size with src's contents, copied on stream `s` (the caller synchronises); nothing for an empty src
template <typename T>
int copy_buf(const DevBuf<T> &src, DevBuf<T> &dst, hipStream_t s) {
    if (!src.p) return EPH_OK;
    if (const int st = dst.alloc(src.count)) return st;
    EPH_HIP(hipMemcpyAsync(dst.p, src.p, sizeof(T) * src.count, hipMemcpyDeviceToDevice, s));
    return EPH_OK;
}

// Direct-write transport of the exchange step (peer.hip): every rank owns a mailbox that its peers map through
// hipIpc and write into; no collective library involved.
constexpr int kPeerMaxWorld = 16;
constexpr size_t kPeerHandleBytes = 64;            // sizeof(hipIpcMemHandle_t)
class PeerTransport {
public:
    ~PeerTransport();
    // form: 0 = fine-grained mailbox, falling back to plain device memory when allocation or export fails | 1 = fine-grained
    // or fail | 2 = plain device memory
    static int create(int rank, int world, size_t slot_bytes, int form, std::shared_ptr<PeerTransport> *out);
    int form() const { return form_; }                        // 1 fine-grained | 2 plain device memory: what is live
    const std::string &fallback_reason() const { return fallback_reason_; }
    const void *handle() const { return handle_; }           // kPeerHandleBytes, to be passed to every peer
    int connect(const void *handles);                         // world x kPeerHandleBytes in rank order
    int all_gather_inplace(void *buf, size_t slice_bytes, hipStream_t s);
    int poll_error() const;                                   // EPH_ERR_COMM once a wait has timed out
    int rank() const { return rank_; }
    int world() const { return world_; }
    uint64_t epochs() const { return epoch_; }

private:
    PeerTransport() = default;
    int rank_ = 0, world_ = 1, device_ = 0, form_ = 0;
    std::string fallback_reason_;
    size_t slot_ = 0;
    void *base_[kPeerMaxWorld] = {};
    char handle_[kPeerHandleBytes] = {};
    bool connected_ = false;
    uint64_t epoch_ = 0;
    unsigned *status_ = nullptr, *status_dev_ = nullptr;
    unsigned long long timeout_ticks_ = 0;
    // exchanges of one transport are totally ordered on the device, whatever stream they are issued on (a handle
    // and its clones share the transport but not the stream): each launch waits for the previous one's event
    hipEvent_t order_ = nullptr;
    hipStream_t last_stream_ = nullptr;
    bool have_last_ = false;
};

// The exchange step of a target-partitioned run (shard.cpp): in-place all-gather of equal slices over the ranks.
class Exchange {
public:
    ~Exchange();
    static int create(int rank, int world, const void *unique_id, eph_exchange_fn fn, void *ctx,
                      std::shared_ptr<Exchange> *out);
    static int create_peer(std::shared_ptr<PeerTransport> t, std::shared_ptr<Exchange> *out);
    int all_gather_inplace(void *buf, size_t slice_bytes, hipStream_t s);
    int poll_error() const { return peer_ ? peer_->poll_error() : EPH_OK; }
    int rank() const { return rank_; }
    int world() const { return world_; }
    uint64_t gathers() const { return gathers_; }

private:
    Exchange() = default;
    int rank_ = 0, world_ = 1;
    void *comm_ = nullptr;          // ncclComm_t
    eph_exchange_fn fn_ = nullptr;
    void *ctx_ = nullptr;
    std::shared_ptr<PeerTransport> peer_;
    uint64_t gathers_ = 0;
};
int rccl_unique_id(void *out128);

// The scalar bookkeeping of an NBodyIntegration: what a clone takes from its source in ONE assignment (a member added here travels;
// one added to the class itself -- timing, sampling, the gang's members, anything per stream -- does not).
struct NBodyBook {
    int device_ = 0;
    int n_ = 0, npad_ = 0, L_ = 1;
    int lo_ = 0, hi_ = 0, slice_ = 0;         // owned targets [lo_, hi_); slice_ = npad_ / world when sharded
    std::shared_ptr<Exchange> xch_;           // (a clone of a sharded handle shares the ranks)
    bool is_multistep_ = false;
    bool compensated_ = false;                // a `<Double>` handle
    Elm2Coeffs lm_{};
    SrknCoeffs rk_{};
    int substeps_ = 1;
    double h_ = 0, h_sub_ = 0;
    double time_ = 0, bound_ = 0;
    uint32_t starter_i_ = 0, lm_i_ = 0;       // SRKN.i (inner RK steps), ELM2.i
    uint64_t evals_ = 0;
    int cur_ = 0, pp_ = 0;
    int path_ = 0;
    int pv_ = 0;                              // evaluation order of the point-mass term, fixed at creation (dispatch.cpp)
    // the last fused step of a batch left the NEXT step's predicted positions in P_[pp_ ^ 1] and in the ring slot the next step
    // takes (the oldest level's, dead by then): the next batch starts with its force evaluation instead of a predictor launch
    bool predicted_ = false;
    int failed_ = EPH_OK;                     // sticky: a gang launch this handle was a member of failed once something was queued
};

// The launch arguments of a gang, one T per member, on the handle that leads it: the device array the kernel reads, its pinned twin
// that the copy is made from (so advance_many need not wait for the copy) and the twin's capacity. The twin is rewritten, grown and
// freed only behind a wait for the owner's copy event (NBodyIntegration::gang_frame, ~NBodyIntegration).
template <typename T>
struct GangArgs {
    DevBuf<T> dev;
    T *host = nullptr;
    size_t host_count = 0;
    ~GangArgs() { if (host) (void)hipHostFree(host); }
};

// Integration<NBodyProblem<DVec3>, M>: problem + integrator   (integration/src/lib.rs:394-503,
// ephemeris/src/propagators/nbody.rs:41,93-121)
class NBodyIntegration : private NBodyBook {
public:
    ~NBodyIntegration();
    static int create(int n, const double *pos, const double *vel, const double *mu, double t0, double h,
                      const char *method, std::unique_ptr<NBodyIntegration> *out);
    int clone(std::unique_ptr<NBodyIntegration> *out);

    // n_steps x Integrator::advance; *done = steps actually taken
    int advance(int64_t n_steps, int64_t *done = nullptr);
    int get_state(double *pos, double *vel, double *t, uint32_t *step_count);
    int get_acc(double *acc);
    int sync();

    // IntegratorState
    uint32_t step_count() const { return is_multistep_ ? starter_i_ / (uint32_t)substeps_ + lm_i_ : starter_i_; }
    double step_size() const { return h_; }
    // ODEProblem
    double time() const { return time_; }
    double bound() const { return bound_; }
    void set_bound(double b) { bound_ = b; }
    int n() const { return n_; }
    bool started() const { return !is_multistep_ || starter_i_ / (uint32_t)substeps_ >= (uint32_t)lm_.order; }
    uint64_t evals() const { return evals_; }
    hipStream_t stream() const { return stream_; }
    int device() const { return device_; }
    int pair_variant() const { return pv_; }
    // a `<Double>` handle (double_state.h): Integration<ODEProblem<f64, SecondOrderState<Vec<Double<DVec3>>>, NewtonianGravity>, M>
    bool compensated() const { return compensated_; }
    void set_path(int p) { path_ = p; }
    int path() const { return path_; }
    // path 1 -> per-step launches with the one-wave-per-block force, 3 -> with the workgroup-specialised force
    int force_kind() const { return path_ == 1 ? 1 : (path_ == 3 ? 2 : 0); }
    void set_sampling(const SampleArgs &s) { samp_ = s; }   // consumed by the next advance() batch
    // target-partition the system over the ranks of `x`: this rank keeps bodies [lo, hi) current
    int set_shard(std::shared_ptr<Exchange> x);
    int shard_refusal() const;                // EPH_ERR_UNSUPPORTED with its text for a `<Double>` handle (before an exchange is made)
    bool sharded() const { return (bool)xch_; }
    int exchange_error() const { return xch_ ? xch_->poll_error() : EPH_OK; }   // EPH_ERR_COMM once a peer wait timed out
    int shard_lo() const { return lo_; }
    int shard_hi() const { return hi_; }
    uint64_t gathers() const { return xch_ ? xch_->gathers() : 0; }
    int shard_rank() const { return xch_ ? xch_->rank() : 0; }
    int shard_world() const { return xch_ ? xch_->world() : 1; }
    int shard_slice() const { return xch_ ? slice_ : n_; }          // bodies per rank (the last rank may own fewer)
    // in-place all-gather of equal slices of a device buffer over the ranks, on this handle's stream
    int gather_buffer(void *buf, size_t slice_bytes) {
        return xch_ ? xch_->all_gather_inplace(buf, slice_bytes, stream_) : EPH_OK;
    }
    // device view of the current positions, SoA [3][npad] (for on-device consumers: the interpolation-error scan)
    const double *positions_soa() { return Yslot(is_multistep_ ? cur_ : 0); }
    int npad() const { return npad_; }
    void enable_timing(bool on) { timing_ = on; }
    double kernel_ms() { (void)resolve_timing(); return kernel_ms_; }
    uint64_t kernel_launches() const { return kernel_launches_; }
    // how many of the next k advance() calls would succeed before BoundReached / StepSizeUnderflow
    int64_t steps_available(int64_t k, int *status_after) const;
    bool steps_certain(int64_t k) const;       // neither the bound nor the underflow test can fire in the next k steps (closed form)
    // `count` independent single-workgroup systems advanced by k steps in ONE launch (k_lm_small, one workgroup each):
    // the same as advance(k) on every one of them. Systems that do not qualify (more than kGangMaxN bodies, sharded, a
    // forced kernel path, a step that would fail) make the call fall back to that.
    // Members still in their start-up take its macro steps first, those of at least two plain members in ONE launch of
    // k_lm_startup_small (a workgroup each); what is left of k then runs as above when it is the same for every member.
    // Either launch is one gang_frame: every member fills its block of the lead's argument array, the lead launches, every member
    // commits its bookkeeping under the kernel (fill_startup_args / commit_startup, fill_gang_args / commit_gang). No member's
    // advance() runs for a ganged launch.
    // The symplectic members of the call are taken out first: those that srkn_gang_steps accepts, the plain ones and the `<Double>`
    // ones apart, share ONE launch of k_srkn_small_many per kind when there are at least two (fill_srkn_gang_args /
    // commit_srkn_gang), each with its own step count -- a member stops at its own bound and is left where its own advance(k)
    // leaves it. A kind with one member, and every symplectic member that does not qualify, keeps its own advance. The call's
    // status is the first other than EPH_OK in member order.
    static int advance_many(NBodyIntegration *const *igs, int count, int64_t k);
    bool gang_ready(int64_t k) const;          // advance(k) on this handle would be ONE launch of k_lm_small that takes all k steps
    // A symplectic handle as a member of the SRKN gang: how many of the next k steps (at most 2^30 of them) one launch of the
    // single-workgroup kernel takes -- steps_available -- and the status behind them; 0 where the handle keeps its own advance:
    // not srkn_small_ready(), failed, or not one step to take.
    int64_t srkn_gang_steps(int64_t k, int *status_after) const;
    bool srkn_gang_ready(int64_t k) const { int after = EPH_OK; return k > 0 && k <= ((int64_t)1 << 30) && srkn_gang_steps(k, &after) == k; }
    bool is_multistep() const { return is_multistep_; }
    // The one-launch start-up (k_lm_startup_small): how many of the next `want` steps it would take now -- min(want, macro steps
    // left) -- or 0 where the per-launch route has to run: started, not multistep, more than kGangMaxN bodies, sharded, a forced
    // per-launch path, between two substeps of an abandoned macro step, or one of the tests of startup_macro_step / srkn_step
    // firing in those macro steps (a dry run of `time = time + h_sub` in the reference's order; *t_after: the time it ends at).
    int64_t startup_small_steps(int64_t want, double *t_after = nullptr) const;
    int64_t startup_left() const { return started() ? 0 : (int64_t)lm_.order - (int64_t)(starter_i_ / (uint32_t)substeps_); }

private:
    NBodyIntegration() = default;
    int open_device();                        // the handle's stream, its two events and its buffers (create and clone)
    int alloc_buffers();
    int advance_from(int64_t done, int64_t n_steps, int64_t *done_out);   // advance(n_steps) whose first `done` steps are taken already
    int startup_macro_step();                 // one LinearMultistepIntegrator::advance in the start-up regime
    int startup_batch(int64_t m, double t_after);                  // m of them in one launch (startup_small_steps said so)
    void fill_startup_args(LmStartupArgs &g, int64_t m) const;
    void commit_startup(int64_t m, double t_after);                // the bookkeeping m calls of startup_macro_step would have left
    static int startup_gang(NBodyIntegration *const *igs, int count, const int64_t *m, const double *t_after);
    void fill_gang_args(LmArgs &a) const;     // the steady gang's member, for k steps that gang_ready(k) has accepted: its launch arguments,
    void commit_gang(int64_t k);              // and the bookkeeping advance(k) would have left
    // the SRKN gang's member, for k steps that srkn_gang_steps has accepted: srkn_batch(k) in the same two halves
    void fill_srkn_gang_args(SrknGangArgs &g, int64_t k) const;
    void commit_srkn_gang(int64_t k);
    // the symplectic members of an advance_many call (all of igs, in member order): status[i] = what advance(k) on member i returns
    static int advance_many_srkn(NBodyIntegration *const *igs, int count, int64_t k, int *status);
    // the members of an advance_many call that are not symplectic: the start-up gang and the steady gang
    static int advance_many_multistep(NBodyIntegration *const *igs, int count, int64_t k, int *status);
    // one launch for the members igs[0 .. count) on the stream of the lead igs[0], whose argument array `ga` is (nbody.cpp)
    template <typename Args, typename Fill, typename Launch, typename Commit>
    static int gang_frame(NBodyIntegration *const *igs, int count, GangArgs<Args> &ga, bool timed, Fill &&fill, Launch &&launch, Commit &&commit);
    // what the members of one gang launch share with its lead: the device, the ring length, the evaluation order
    bool shares_launch_with(const NBodyIntegration &lead) const { return device_ == lead.device_ && L_ == lead.L_ && pv_ == lead.pv_; }
    // (the SRKN gang's: its blocks carry their own tables, and a symplectic handle's ring is its one working slot)
    bool shares_srkn_launch_with(const NBodyIntegration &lead) const {
        return device_ == lead.device_ && pv_ == lead.pv_ && compensated_ == lead.compensated_;
    }
    int queued(int st, bool made = true) { if (!st && made && n_ > 0) count_launches(1); return st; }   // a launch that was made, for the hook's count
    int srkn_step(double h, double *y_slot);  // FixedRungeKuttaIntegrator::advance (SRKN)
    int srkn_batch(int64_t k);                // k of them in one launch of the single-workgroup kernel (step_srkn_small.hip)
    void fill_srkn_args(SrknSmallArgs &a, double h) const;         // that kernel's arguments, and the start-up kernel's share of them, for steps of h
    uint64_t srkn_step_evals() const { return (uint64_t)(rk_.fsal ? rk_.stages - 1 : rk_.stages); }   // force evaluations per SRKN step behind the first
    bool srkn_small_ready() const { return !is_multistep_ && n_ >= 1 && n_ <= kGangMaxN && !sharded() && (path_ == 0 || path_ == 2); }
    int lm_batch(int64_t k);                  // k steady-state ELM2::advance
    int lm_batch_double(int64_t k);           // the same on a `<Double>` handle
    template <typename Queue>
    int batch_frame(int64_t k, Queue &&queue);   // what a handle's own three batches share around their launches (nbody.cpp); a gang's: gang_frame
    void fill_lm_args(LmArgs &a) const;       // the fields of a batch's launch arguments that both set
    void point_lm_args(LmArgs &a) const;      // the level a step starts from: ring slot and the two packed position buffers
    void next_level(LmArgs &a);               // one step on: the ring turns, the position buffers swap
    void turn_ring(int64_t k) { cur_ = (int)(((int64_t)cur_ - k % L_ + L_) % L_); }   // k steps on in one launch: the newest level's slot
    int srkn_stage_double(double hb, double ha, double *y_slot, double *ye_slot, bool eval);
    double *YEslot(int s) { return YE_.p + (size_t)s * 3 * npad_; }
    double *Yslot(int s) { return Y_.p + (size_t)s * 3 * npad_; }
    double *Aslot(int s) { return A_.p + (size_t)s * 3 * npad_; }

    int gather_packed(Body4 *buf);            // all-gather the ranks' slices of a packed position buffer
    int gather_stage();                       // same for the AoS staging buffer (read_back)
    // up to two SoA [3][npad] device arrays to host AoS [n][3] (a null host pointer: not asked for); n_ > 0 and one of them asked for
    int read_back(const double *a_dev, double *a, const double *b_dev, double *b);

    hipStream_t stream_ = nullptr;
    hipEvent_t ev0_ = nullptr, ev1_ = nullptr;
    // enable_timing: every batch of steps is bracketed by a pair of events that is read LATER (kernel_ms(), or when 1024 pairs
    // wait): waiting for the closing event inside advance() made the call synchronous and cost a 20-step block 2 % of its time
    std::vector<std::pair<hipEvent_t, hipEvent_t>> ev_pending_, ev_free_;
    int resolve_timing();
    struct TimingGuard;                       // one such interval, opened and closed by a batch (nbody.cpp)
    bool timing_ = false;
    double kernel_ms_ = 0;
    uint64_t kernel_launches_ = 0;
    SampleArgs samp_{};

    // ---- The handle's device buffers, stated once ---------------------------------------------------------------------------------
    // for_each_buffer names every DevBuf member with its element count and its kind; alloc_buffers and the copy half of clone are
    // walks over it. A NEW BUFFER IS ADDED HERE AND TO THAT LIST AND NOWHERE ELSE. The error parts exist on a `<Double>` handle alone:
    // those of the y ring (same slots as Y_) and of the current velocity; the accelerations have none. The SRKN working position is
    // the ring slot under construction (slot 0 of an SRKN method), so its error part is that slot of YE_.
    DevBuf<Body4> P_[2];
    DevBuf<double> Y_, A_, V_, ASR_, mu_, stage_, YE_, VE_;
    DevBuf<double> fast_partial_;             // the fast paths' [S][3][npad] partial sums and arrival tickets
    DevBuf<float> posf_;                      // EPH_PATH_F32_PAIRS: the level's positions and mu as 4 floats per body
    GangArgs<LmArgs> gang_;                   // advance_many: the argument array of the steady gang this handle leads (its .dev is the buffer)
    GangArgs<LmStartupArgs> startup_;         // advance_many: the same for the start-up gang it leads
    GangArgs<SrknGangArgs> srkn_gang_;        // advance_many: the same for the SRKN gang it leads (plain or `<Double>`, as the handle is)
    // state: allocated at creation, zeroed, copied by clone | scratch: allocated at creation, contents nobody's | lazy: allocated where
    // it is first used (lm_batch, advance_many), neither zeroed nor copied
    enum class Buf { state, scratch, lazy };
    template <typename F>   // f(accessor: handle -> its member, element count on g, kind), in allocation order, until a status other than EPH_OK
    static int for_each_buffer(const NBodyIntegration &g, F &&f) {
        const size_t bodies = (size_t)g.npad_, vec = 3 * bodies, ring = (size_t)g.L_ * vec;
#define EPH_NBODY_BUF(member) [](NBodyIntegration &x) -> auto & { return x.member; }
        int st;
        (void)((st = f(EPH_NBODY_BUF(P_[0]), bodies, Buf::state)) || (st = f(EPH_NBODY_BUF(P_[1]), bodies, Buf::state)) ||
               (st = f(EPH_NBODY_BUF(Y_), ring, Buf::state)) || (st = f(EPH_NBODY_BUF(A_), ring, Buf::state)) ||
               (st = f(EPH_NBODY_BUF(V_), vec, Buf::state)) || (st = f(EPH_NBODY_BUF(ASR_), vec, Buf::state)) ||
               (st = f(EPH_NBODY_BUF(mu_), bodies, Buf::state)) || (st = f(EPH_NBODY_BUF(stage_), vec, Buf::scratch)) ||
               (g.compensated_ && ((st = f(EPH_NBODY_BUF(YE_), ring, Buf::state)) || (st = f(EPH_NBODY_BUF(VE_), vec, Buf::state)))) ||
               (st = f(EPH_NBODY_BUF(fast_partial_), fast_partial_doubles(g.npad_), Buf::lazy)) ||
               (st = f(EPH_NBODY_BUF(posf_), 4 * bodies, Buf::lazy)) ||
               (st = f(EPH_NBODY_BUF(gang_.dev), (size_t)0, Buf::lazy)) ||                 // (one LmArgs per system of the gang)
               (st = f(EPH_NBODY_BUF(startup_.dev), (size_t)0, Buf::lazy)) ||
               (st = f(EPH_NBODY_BUF(srkn_gang_.dev), (size_t)0, Buf::lazy)));
#undef EPH_NBODY_BUF
        return st;
    }

    // gang_frame on the lead: the event that joins the members' streams to the lead's and releases them behind the launch, and the one
    // behind the argument copy, which guards the pinned twins of gang_, startup_ and srkn_gang_ alike
    hipEvent_t gang_ev_ = nullptr, gang_copy_ev_ = nullptr;
};

// Polynomial<DVec3> (SmallVec<[DVec3; 8]>)   ephemeris/src/trajectory.rs:337-396
struct Polynomial {
    int32_t ncoef = 0;
    double c[kDiv][3] = {};
};

// UniformSpline<DVec3>   ephemeris/src/trajectory.rs:412-633
struct UniformSpline {
    double start = 0, interval = 0;
    std::deque<Polynomial> polynomials;
    // polynomials already pushed as far as the bounds are concerned but still resident on the device (only inside an
    // NBodyPropagator between fits and take_solution; 0 in every Solution handed out)
    uint64_t ghost = 0;
    uint64_t len() const { return (uint64_t)polynomials.size() + ghost; }
    double span() const { return interval * (double)len(); }   // interval.scaled(len)
    double end() const { return start + span(); }
    void push_back(const Polynomial &p) { polynomials.push_back(p); }
    void push_front(const Polynomial &p) {
        polynomials.push_front(p);
        start -= interval;
    }
    // get_index_local / get_index_local_exclusive  trajectory.rs:591-617 (`as usize` saturates; NaN -> 0). false = None
    static uint64_t to_usize(double x) {
        if (!(x > 0.0)) return 0;
        return x >= 18446744073709551616.0 ? ~0ull : (uint64_t)x;
    }
    bool get_index_local(double time, uint64_t *idx) const {
        if (std::signbit(time) || time >= span()) return false;
        *idx = to_usize(time / interval);
        return true;
    }
    bool get_index_local_exclusive(double time, uint64_t *idx) const {
        if (std::signbit(time) || time > span()) return false;
        const uint64_t c = to_usize(std::ceil(time / interval));
        *idx = c == 0 ? 0 : c - 1;                        // saturating_sub(1)
        return true;
    }
    void clear_before(double at) {                        // trajectory.rs:536-542
        uint64_t idx;
        if (!get_index_local_exclusive((at + interval) - start, &idx)) return;
        start += interval * (double)idx;
        const uint64_t k = std::min<uint64_t>(idx, polynomials.size());   // drain(0..idx) (idx <= len here)
        polynomials.erase(polynomials.begin(), polynomials.begin() + (std::ptrdiff_t)k);
    }
    void clear_after(double at) {                         // trajectory.rs:544-549
        uint64_t idx;
        if (!get_index_local(at - start, &idx)) return;
        if (idx < polynomials.size()) polynomials.resize((size_t)idx);       // truncate(idx)
    }
    bool between(double from, double to, UniformSpline *out) const {        // trajectory.rs:484-502
        if (polynomials.empty()) return false;
        uint64_t a, b;
        if (!get_index_local_exclusive(from - start, &a) || !get_index_local_exclusive(to - start, &b)) return false;
        out->start = start + interval * (double)a;
        out->interval = interval;
        out->polynomials.clear();
        for (uint64_t i = a; i < b + 1 && b + 1 != 0; ++i)                   // (start..end + 1).filter_map(get)
            if (i < polynomials.size()) out->polynomials.push_back(polynomials[(size_t)i]);
        return true;
    }
};

struct Solution {   // Vec<UniformSpline<DVec3>>
    std::vector<UniformSpline> splines;
};
// UniformSpline::append (direction > 0) / prepend (< 0) of ys[b] onto xs[b] for every body  trajectory.rs:515-534, in two halves so
// that a refusal or a failure leaves `xs` untouched (the reference would have panicked).
// The asserts: equal intervals and touching ends; `refuse_ghost`: ys must hold every polynomial its bounds count.
inline bool splines_contiguous(const std::vector<UniformSpline> &xs, const std::vector<UniformSpline> &ys, int direction, bool refuse_ghost) {
    if (direction == 0 || xs.size() != ys.size()) return false;
    for (size_t b = 0; b < xs.size(); ++b) {
        const UniformSpline &x = xs[b], &y = ys[b];
        if ((refuse_ghost && y.ghost) || x.interval != y.interval) return false;
        if (direction > 0 ? (x.end() != y.start) : (x.start != y.end())) return false;
    }
    return true;
}
// The splice, all bodies or none: an insertion at an end of a deque either succeeds or has no effect, so when body k throws the
// bodies before it give back what they received (erasing at an end does not throw) and the exception goes on.
inline void splines_splice(std::vector<UniformSpline> &xs, const std::vector<UniformSpline> &ys, int direction) {
    size_t b = 0;
    try {
        for (; b < xs.size(); ++b) {
            std::deque<Polynomial> &x = xs[b].polynomials;
            const std::deque<Polynomial> &y = ys[b].polynomials;
            x.insert(direction > 0 ? x.end() : x.begin(), y.begin(), y.end());
        }
    } catch (...) {
        while (b-- > 0) {
            std::deque<Polynomial> &x = xs[b].polynomials;
            const std::ptrdiff_t k = (std::ptrdiff_t)ys[b].polynomials.size();
            if (direction > 0) x.erase(x.end() - k, x.end());
            else x.erase(x.begin(), x.begin() + k);
        }
        throw;
    }
    if (direction < 0)
        for (size_t k = 0; k < xs.size(); ++k) xs[k].start = ys[k].start;
}

// SplineInterpolator   ephemeris/src/propagators/nbody.rs:309-323
struct SplineInterpolator {
    double last_sample_time = 0, sample_period = 0;   // Durations
    uint32_t len = 1;       // PolyonmialInterpolator.index
    uint32_t degree = 0;    // LeastSquaresFit.degree
    // derived: after how many `last_sample_time += delta` the `== sample_period` test fires (0 = never),
    // and how many additions have been made since the last reset
    uint32_t period_steps = 0, phase = 0;
    double time() const { return last_sample_time + sample_period * (double)(len > 0 ? len - 1 : 0); }
};

// NBodyPropagator<D, DVec3, M, SplineInterpolators<D, DVec3, LeastSquaresFit>>
class NBodyPropagator {
public:
    static int create(int n, const double *pos, const double *vel, const double *mu, double t0, double dt,
                      int direction, const char *method, const uint32_t *count, const uint32_t *degree,
                      std::unique_ptr<NBodyPropagator> *out);
    int clone(std::unique_ptr<NBodyPropagator> *out);
    int step_n(int64_t k);                    // k x IncrementalPropagator::step
    // step_n(k) on every propagator of `ps`, the start-up and the steady-state steps of all of them in shared launches (advance_many)
    static int step_n_many(NBodyPropagator *const *ps, int count, int64_t k);
    int step_to(double t);
    // ONE IncrementalPropagator::step, executed lazily: the reference's callers step in a loop and look at time() /
    // has_reached() after every step (ephemeris_explorer/src/prediction.rs:422-443). Everything those two return is a
    // function of the number of steps taken (sampling counters and spline bounds), not of the numerical state, so a
    // steady-state step only advances that bookkeeping on the host and is queued; the queue runs as one device batch when
    // somebody needs data (take_solution, clone, state, step_n / step_to) or it reaches kDeferMax steps.
    int step_deferred();
    int flush();
    // run the queued steps and bring the device-resident polynomials into the host splines: afterwards the host
    // Solution is complete (eph_prop_shard needs that before the sharded branch starts pushing newer windows)
    int settle() { const int st = flush(); return st ? st : materialize(); }
    double time() const;                      // DirectionalSolout::solution_time
    bool has_reached(double t) const;
    int take_solution(std::unique_ptr<Solution> *out);
    NBodyIntegration *integration() { return integ_.get(); }
    int64_t deferred() const { return deferred_; }

private:
    NBodyPropagator() = default;
    Solution new_solution() const;
    int run_batch(int64_t k);
    int batch_begin();                         // run_batch up to the integrator's advance: sampling schedule on the device
    int64_t steps_until_reached(double t, int64_t cap) const;
    double bound_of(const UniformSpline &s) const { return direction_ > 0 ? s.end() : s.start; }
    int ensure_log_capacity(const std::vector<uint64_t> &need);

    std::unique_ptr<NBodyIntegration> integ_;
    int direction_ = 1;
    double delta_ = 0;
    int64_t kmax_ = 1;          // steps per device batch (bounded by the sample-log budget)
    std::vector<SplineInterpolator> interp_;
    Solution solution_;
    // device-side sample logs: body b owns log[log_off_[b] .. log_off_[b] + log_cap_[b]) samples
    DevBuf<double> log_;
    std::vector<uint64_t> log_off_, log_cap_;
    DevBuf<uint32_t> d_period_, d_phase_;
    DevBuf<uint64_t> d_offset_;
    // run_batch scratch (grow-only, reused by every batch) and the sticky status of a batch that failed half-way
    DevBuf<uint64_t> d_first_, d_region_;
    DevBuf<uint8_t> d_deg_;
    DevBuf<double> d_co_, d_all_;
    DevBuf<int32_t> d_nc_;
    DevBuf<uint32_t> d_src_, d_cnt_;
    int failed_ = EPH_OK;
    int fit_and_push(int64_t done, hipStream_t s);
    // Fitted polynomials stay on the device until somebody takes the solution: a batch appends its windows (body-major)
    // to pend_co_ / pend_nc_ and only the bounds (UniformSpline::start, ::ghost) move on the host, with the reference's
    // own f64 operations. materialize() downloads them and performs the push_back / push_front of every window.
    // deferred steps (step_deferred): how many, and the bookkeeping as it will be once they have run
    static constexpr int64_t kDeferMax = 8192;
    int64_t deferred_ = 0;
    double sh_time_ = 0;                                  // integrator time
    std::vector<uint32_t> sh_phase_, sh_len_;             // SplineInterpolator counters
    std::vector<double> sh_start_;                        // spline starts
    std::vector<uint64_t> sh_npoly_;                      // spline lengths
    double bound_at(size_t b) const {                     // bound of spline b, deferred steps included
        const UniformSpline &s = solution_.splines[b];
        if (deferred_ == 0) return bound_of(s);
        return direction_ > 0 ? sh_start_[b] + s.interval * (double)sh_npoly_[b] : sh_start_[b];
    }
    DevBuf<double> pend_co_;                  // [pend_cap_][kDiv][3]
    DevBuf<int32_t> pend_nc_;
    size_t pend_count_ = 0, pend_cap_ = 0;
    // device-side budget of the pending list (196 B per window): beyond it the list is spilled to the host splines
    // (materialize) instead of growing; a failed device allocation does the same instead of failing the run
    static constexpr size_t kPendMaxWindows = (size_t)1 << 23;   // 1.6 GB
    std::vector<std::vector<uint32_t>> pend_batches_;   // per batch: windows per body
    int reserve_pending(size_t extra, hipStream_t s);
    int materialize();
};

}  // namespace eph
struct eph_nbody {      // the C ABI's opaque Integration handle (a view when it belongs to a propagator)
    std::unique_ptr<eph::NBodyIntegration> own;
    eph::NBodyIntegration *p = nullptr;
    // a view's propagator: eph_prop_step queues steps on the host (NBodyPropagator::step_deferred), so every eph_nbody_*
    // call through the view runs that queue first -- the view never shows a state the propagator's callers have moved past
    eph::NBodyPropagator *owner = nullptr;
    int settle() const { return owner ? owner->flush() : 0; }
};
struct eph_solution {   // the C ABI's opaque Vec<UniformSpline<DVec3>>
    eph::Solution s;
};
namespace eph {

// device evaluation of one UniformSpline at many epochs
int spline_eval_device(const UniformSpline &s, int64_t m, const double *at, double *pos, double *vel, uint8_t *inside);
int least_squares_fit_device(int degree, int backward, int64_t nwin, const double *samples, double *coeffs,
                             int32_t *ncoef);
int accel_eval_device(int n, const double *pos, const double *mu, double *acc);

}  // namespace eph
