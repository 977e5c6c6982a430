"""ephemeris_explorer_amd -- MI355X-native ephemeris propagator (one hot path of Canleskis/ephemeris-explorer).

Python view of the C ABI in include/ephemeris_amd.h (libephemeris_amd.so, hand-written HIP for gfx950). The class
and method names mirror the reference's operator surface (paths relative to the reference repository):

    NBodyIntegration   = M::new(FixedMethodParams::new(h)).integrate(NBodyProblem{..})   integration/src/lib.rs
    NBodyPropagator    = ephemeris::NBodyPropagator<D, DVec3, M, SplineInterpolators<..>>   ephemeris/src/propagators/nbody.rs
    Solution           = Vec<UniformSpline<DVec3>>                                          ephemeris/src/trajectory.rs

There is NO CPU fallback: if the shared library is missing or no HIP device is visible, every compute call
raises. (The CPU oracle lives in oracle/ and is test infrastructure only; this package never imports it.)
"""
import ctypes as C

import numpy as np

from . import systems  # noqa: F401  (state.json / ephemeris.json / ships readers)
from ._abi import (ABI_SYMBOLS, EXCHANGE_FN, LIB_PATH, AdaptiveParams, MarkerRequest, OrbitPlotConfig, PlotMarker,  # noqa: F401  (the package's names)
                   PlotRequest, PlotSegment, PlotView, SeparationRequest, _dp, _fp, _i32p, _i64p, _lib, _u8p, _u32p, hip_runtime)

FORWARD, BACKWARD = 1, -1
PATH_FAST = 4
PATH_FAST_RSQ = 5
PATH_F32_PAIRS = 6   # OPT-IN mixed precision: f32 pair arithmetic, f64 accumulation and integrator (include/ephemeris_amd.h)

OK = 0
STEP_SIZE_UNDERFLOW, MAX_ITERATIONS_REACHED, BOUND_REACHED, EVAL_FAILED, SOLOUT_EXIT = 1, 2, 3, 4, 5
ERR_BAD_ARGUMENT, ERR_NO_DEVICE, ERR_HIP, ERR_UNSUPPORTED, ERR_OUT_OF_MEMORY = -1, -2, -3, -4, -5
KNOTS_FULL = 6


class EphemerisError(RuntimeError):
    """A library / device failure (negative status)."""

    def __init__(self, status, where=""):
        self.status = status
        msg = _lib().eph_status_string(status).decode()
        detail = _lib().eph_last_error().decode()
        super().__init__(f"{where}: {msg}" + (f" [{detail}]" if detail else ""))


class StepError(Exception):
    """integration::StepError / NBodyPropagatorError (positive status): errors the reference returns as values."""

    NAMES = {1: "StepSizeUnderflow", 2: "MaxIterationsReached", 3: "BoundReached", 4: "EvalFailed", 5: "Solout"}

    def __init__(self, status):
        self.status = status
        super().__init__(self.NAMES.get(status, str(status)))


def _check(st, where):
    if st < 0:
        raise EphemerisError(st, where)
    return st


def _call(name, *args):
    """THE call into the library: eph_<name>(*args), a negative status raised as EphemerisError, the status returned."""
    return _check(getattr(_lib(), name)(*args), name)


def _step(name, *args):
    """_call for the functions that step an integration: a positive status is the StepError the reference returns as Err."""
    st = _call(name, *args)
    if st:
        raise StepError(st)


def _contiguous(name, message, *args):
    """_call for append / prepend / merge: EPH_ERR_BAD_ARGUMENT is the reference's assert_eq! on the splines' ends
    (UniformSpline::append / prepend, trajectory.rs:517-518,530-531) and raises ValueError(message), the object untouched."""
    st = getattr(_lib(), name)(*args)
    if st == ERR_BAD_ARGUMENT:
        raise ValueError(message)
    _check(st, name)


def _new_handle(name, *args):
    """_call for the functions that leave a new object in their last parameter (eph_* **out) -> its handle."""
    h = C.c_void_p()
    _call(name, *args, C.byref(h))
    return h


def _f64(a):
    return np.ascontiguousarray(a, dtype=np.float64)


def _p(a, t=_dp):
    return a.ctypes.data_as(t)


def _p_or_null(a, t=_dp):
    return None if a is None else _p(a, t)


class _Handle:
    """An object of the library: `_L` the library, `_h` the handle, destroyed with the Python object unless it is borrowed
    from another one. A subclass names its eph_*_destroy in _DESTROY and binds the handle it creates with _bind()."""
    _DESTROY = None
    _owned = True

    def _bind(self, handle):
        self._L, self._h = _lib(), handle        # __del__ goes through self._L: module globals may be gone by then

    @classmethod
    def _adopt(cls, handle, owned=True, **attributes):
        """An existing handle as a `cls`, __init__ not run: `attributes` are the ones __init__ would have set."""
        self = object.__new__(cls)
        self._bind(handle)
        self._owned = owned
        vars(self).update(attributes)
        return self

    def _clone(self, name):
        """eph_*_clone -> a `cls` with a handle of its own and every other attribute of this one."""
        return self._adopt(_new_handle(name, self._h), **{k: v for k, v in vars(self).items() if k not in ("_L", "_h", "_owned")})

    def __del__(self):
        if self._owned and getattr(self, "_h", None):
            getattr(self._L, self._DESTROY)(self._h)
            self._h = None



def device_count():
    n = C.c_int32()
    _call("eph_device_count", C.byref(n))
    return n.value


def set_device(i):
    _call("eph_set_device", int(i))


def release_cached_memory():
    """Returns the library's cache of large device blocks to the driver (eph_release_cached_memory); bytes released."""
    b = C.c_uint64()
    _call("eph_release_cached_memory", C.byref(b))
    return int(b.value)


def device_name():
    buf = C.create_string_buffer(256)
    _call("eph_device_name", buf, 256)
    return buf.value.decode()


def srkn_coeffs(name):
    A, B = np.zeros(32), np.zeros(32)
    s, f = C.c_int32(), C.c_int32()
    _call("eph_srkn_coeffs", name.encode(), C.byref(s), C.byref(f), _p(A), _p(B))
    return A[: s.value].copy(), B[: s.value].copy(), bool(f.value)


def elm2_coeffs(name):
    wa, wb, cw = np.zeros(16), np.zeros(16), np.zeros(16)
    o = C.c_int32()
    ib, ic = C.c_double(), C.c_double()
    _call("eph_elm2_coeffs", name.encode(), C.byref(o), _p(wa), _p(wb), C.byref(ib), _p(cw), C.byref(ic))
    k = o.value
    return dict(order=k, w_alpha=wa[:k].copy(), w_beta=wb[:k].copy(), inv_beta_d=ib.value, cowell=cw[:k].copy(),
                inv_cowell_d=ic.value)


def accel_eval(pos, mu, acc=None):
    """SecondOrderODE::eval for NewtonianGravity: returns acc (+= the accelerations, reference summation order)."""
    pos, mu = _f64(pos), _f64(mu)
    acc = np.zeros_like(pos) if acc is None else _f64(acc).copy()
    _call("eph_accel_eval", len(mu), _p(pos), _p(mu), _p(acc))
    return acc


def least_squares_fit(degree, samples, backward=False):
    """LeastSquaresFit::interpolate on windows of 9 samples: samples [nwin, 9, 3] -> (coeffs [nwin, 8, 3], ncoef)."""
    samples = _f64(samples).reshape(-1, 9, 3)
    nwin = samples.shape[0]
    co = np.zeros((nwin, 8, 3))
    nc = np.zeros(nwin, dtype=np.int32)
    _call("eph_least_squares_fit", int(degree), int(bool(backward)), nwin, _p(samples), _p(co), _p(nc, _i32p))
    return co, nc


def pair_variant():
    """the evaluation order of the point-mass term new handles take (eph_pair_variant)"""
    return int(_lib().eph_pair_variant())


def set_pair_variant(k):
    """eph_set_pair_variant: the order (0..6, csrc/pair_term.h) for every handle created afterwards"""
    _call("eph_set_pair_variant", int(k))


def _shard_call(name, handle, rank, world, unique_id, exchange):
    cb = None
    if exchange is not None:
        def _tramp(ctx, buf, nbytes, r, w, stream):
            try:
                return int(exchange(buf, nbytes, r, w, stream) or 0)
            except Exception:                          # never unwind through the C frame
                import traceback
                traceback.print_exc()
                return 1
        cb = EXCHANGE_FN(_tramp)
    uid = None
    if unique_id is not None:
        if len(unique_id) != 128:
            raise ValueError("unique_id must be 128 bytes")
        uid = (C.c_char * 128).from_buffer_copy(bytes(unique_id))
    _call(name, handle, int(rank), int(world), uid, cb if cb else EXCHANGE_FN(0), None)
    return cb                                          # the caller keeps the trampoline alive with the handle


def advance_many(integrations, n_steps):
    """eph_nbody_advance_many: advance(n_steps) on every NBodyIntegration of the list, small systems in one launch."""
    arr = (C.c_void_p * len(integrations))(*[g._h for g in integrations])
    _step("eph_nbody_advance_many", arr, len(integrations), int(n_steps))


def step_n_many(propagators, n_steps):
    """eph_prop_step_n_many: step_n(n_steps) on every NBodyPropagator of the list, small systems in shared launches."""
    arr = (C.c_void_p * len(propagators))(*[p._h for p in propagators])
    _step("eph_prop_step_n_many", arr, len(propagators), int(n_steps))


class PeerTransport(_Handle):
    """eph_peer: the direct-write exchange (csrc/peer.hip). Create on every rank, pass `handle` (64 bytes) to every other
    rank, `connect(handles)` with all of them in rank order, then hand it to `NBodyIntegration.shard_peer` /
    `NBodyPropagator.shard_peer` (`parallel.peer_transport(dist)` does the hand-shake over torch.distributed)."""

    _DESTROY = "eph_peer_destroy"
    MEMORY = {"auto": 0, "fine": 1, "coarse": 2}

    def __init__(self, rank, world, slot_bytes=1 << 22, memory="auto"):
        self._bind(_new_handle("eph_peer_create_ex", int(rank), int(world), int(slot_bytes), self.MEMORY[memory]))
        self.rank, self.world = int(rank), int(world)
        f = C.c_int32()
        _call("eph_peer_memory_form", self._h, C.byref(f))
        self.memory = {1: "fine", 2: "coarse"}[f.value]          # what is live (auto may have fallen back)
        buf = (C.c_char * 64)()
        _call("eph_peer_handle", self._h, buf)
        self.handle = bytes(buf)

    def connect(self, handles):
        table = b"".join(bytes(h) for h in handles)
        if len(table) != 64 * self.world:
            raise ValueError("need one 64-byte handle per rank")
        _call("eph_peer_connect", self._h, (C.c_char * len(table)).from_buffer_copy(table))
        return self


def rccl_unique_id():
    """ncclGetUniqueId through the library (rank 0 calls it and distributes the 128 bytes)."""
    out = (C.c_char * 128)()
    _call("eph_rccl_unique_id", out)
    return bytes(out.raw)


class NBodyIntegration(_Handle):
    """Integration<NBodyProblem<DVec3>, M> (no solout). method: "QuinlanTremaine12", "Stormer13" or an SRKN name.
    compensated=True: the state is the reference's Double<DVec3> (every position and velocity component carries a running
    error term, ephemeris/tests/solar_system_convergence.rs:12-110) -- the method name goes out as "<method><Double>".
    state() returns the value parts; `.compensated` says which kind the handle is."""

    _DESTROY = "eph_nbody_destroy"
    DOUBLE_TAG = "<Double>"
    compensated = False                                    # (a handle adopted from a propagator is a plain one)

    def __init__(self, pos, vel, mu, t0, h, method="QuinlanTremaine12", compensated=False):
        pos, vel, mu = _f64(pos), _f64(vel), _f64(mu)
        self.n = len(mu)
        if compensated and not method.endswith(self.DOUBLE_TAG):
            method += self.DOUBLE_TAG
        self.compensated = method.endswith(self.DOUBLE_TAG)
        self._bind(_new_handle("eph_nbody_create", self.n, _p(pos), _p(vel), _p(mu), float(t0), float(h), method.encode()))

    def advance(self, n_steps=1):
        """n_steps x Integrator::advance; raises StepError like the reference returns Err."""
        _step("eph_nbody_advance", self._h, int(n_steps))

    def state(self):
        pos, vel = np.zeros((self.n, 3)), np.zeros((self.n, 3))
        t, sc = C.c_double(), C.c_uint32()
        _call("eph_nbody_get_state", self._h, _p(pos), _p(vel), C.byref(t), C.byref(sc))
        return pos, vel, t.value, sc.value

    def acc(self):
        a = np.zeros((self.n, 3))
        _call("eph_nbody_get_acc", self._h, _p(a))
        return a

    def set_bound(self, b):
        _call("eph_nbody_set_bound", self._h, float(b))

    def set_path(self, path):
        """0 auto | 1 wave kernel | 2 single workgroup | 3 workgroup kernel (all bit-identical to the reference order) |
        PATH_FAST = 4: opt-in slice-parallel sums, NOT the reference's summation order (include/ephemeris_amd.h)."""
        _call("eph_nbody_set_path", self._h, int(path))

    def enable_timing(self, on=True):
        _call("eph_nbody_enable_timing", self._h, int(on))

    def kernel_time(self):
        ms, n = C.c_double(), C.c_uint64()
        _call("eph_nbody_kernel_time", self._h, C.byref(ms), C.byref(n))
        return ms.value, n.value

    def sync(self):
        _call("eph_nbody_sync", self._h)

    def eval_count(self):
        n = C.c_uint64()
        _call("eph_nbody_eval_count", self._h, C.byref(n))
        return n.value

    def clone(self):
        return self._clone("eph_nbody_clone")

    def shard(self, rank, world, unique_id=None, exchange=None):
        """Partition the system by target body over `world` ranks (eph_nbody_shard). unique_id: the 128 bytes of
        rccl_unique_id() from rank 0 (RCCL transport), or exchange: callable(device_ptr, slice_bytes, rank, world,
        hip_stream) -> 0 performing the in-place all-gather (see parallel.host_staged_exchange)."""
        self._exchange_cb = _shard_call("eph_nbody_shard", self._h, rank, world, unique_id, exchange)
        return self

    def shard_peer(self, peer):
        """eph_nbody_shard_peer: the same partition with the direct-write transport (a connected PeerTransport)."""
        _call("eph_nbody_shard_peer", self._h, peer._h)
        self._peer = peer
        return self

    def shard_info(self):
        lo, hi, g = C.c_int32(), C.c_int32(), C.c_uint64()
        _call("eph_nbody_shard_info", self._h, C.byref(lo), C.byref(hi), C.byref(g))
        return lo.value, hi.value, g.value


class Solution(_Handle):
    """Vec<UniformSpline<DVec3>>"""
    _DESTROY = "eph_solution_destroy"

    def __init__(self, handle):
        self._bind(handle)
        n = C.c_int32()
        _call("eph_solution_bodies", handle, C.byref(n))
        self.n = n.value

    def info(self, body):
        s, i, n = C.c_double(), C.c_double(), C.c_int64()
        _call("eph_solution_info", self._h, body, C.byref(s), C.byref(i), C.byref(n))
        return s.value, i.value, n.value

    def coeffs(self, body):
        n = self.info(body)[2]
        co = np.zeros((max(n, 1), 8, 3))
        nc = np.zeros(max(n, 1), dtype=np.int32)
        _call("eph_solution_coeffs", self._h, body, _p(co), _p(nc, _i32p))
        return co[:n], nc[:n]

    def eval(self, body, at, with_velocity=True):
        """EvaluateTrajectory::state_vector / position at many epochs -> (pos, vel|None, inside)."""
        at = _f64(np.atleast_1d(at))
        m = len(at)
        pos = np.zeros((m, 3))
        vel = np.zeros((m, 3)) if with_velocity else None
        inside = np.zeros(m, dtype=np.uint8)
        _call("eph_solution_eval", self._h, body, m, _p(at), _p(pos), _p(vel) if with_velocity else None, _p(inside, _u8p))
        return pos, vel, inside.astype(bool)

    @classmethod
    def from_parts(cls, start, interval, polys):
        """Vec<UniformSpline> from per-body (start, interval) and a list per body of (coeffs[k][3]) polynomials (host
        only: no device needed)."""
        n = len(start)
        npoly = np.array([len(p) for p in polys], dtype=np.int64)
        tot = max(int(npoly.sum()), 1)
        co, nc, q = np.zeros((tot, 8, 3)), np.zeros(tot, dtype=np.int32), 0
        for body in polys:
            for poly in body:
                poly = np.asarray(poly, dtype=np.float64).reshape(-1, 3)
                co[q, :len(poly)] = poly
                nc[q] = len(poly)
                q += 1
        return cls._adopt(_new_handle("eph_solution_create", n, _p(_f64(start)), _p(_f64(interval)), _p(npoly, _i64p), _p(co),
                                      _p(nc, _i32p)), n=n)

    def clear_before(self, at, body=-1):
        _call("eph_solution_clear", self._h, int(body), float(at), 0)

    def clear_after(self, at, body=-1):
        _call("eph_solution_clear", self._h, int(body), float(at), 1)

    def between(self, start, end):
        """UniformSpline::between for every body -> Solution, or None where the reference returns None."""
        h = _new_handle("eph_solution_between", self._h, float(start), float(end))
        return Solution._adopt(h, n=self.n) if h.value else None

    def append(self, tail, direction=FORWARD):
        _contiguous("eph_solution_append", "splines are not contiguous (UniformSpline::append/prepend assert)", self._h, tail._h,
                    int(direction))


class NBodyPropagator(_Handle):
    """NBodyPropagator<D, DVec3, M, SplineInterpolators<D, DVec3, LeastSquaresFit>> on the device."""
    _DESTROY = "eph_prop_destroy"

    def __init__(self, pos, vel, mu, t0, dt, direction, count, degree, method="QuinlanTremaine12"):
        pos, vel, mu = _f64(pos), _f64(vel), _f64(mu)
        count = np.ascontiguousarray(count, dtype=np.uint32)
        degree = np.ascontiguousarray(degree, dtype=np.uint32)
        self.n = len(mu)
        self._bind(_new_handle("eph_prop_create", self.n, _p(pos), _p(vel), _p(mu), float(t0), float(dt), int(direction),
                               method.encode(), _p(count, _u32p), _p(degree, _u32p)))

    @classmethod
    def from_system(cls, system, direction=FORWARD, method="QuinlanTremaine12"):
        """CelestialTrajectory::<D>::new_propagator (ephemeris_explorer/src/dynamics/celestial.rs:156-186)."""
        return cls(system.pos, system.vel, system.mu, system.epoch, system.dt, direction, system.count, system.degree,
                   method)

    def shard(self, rank, world, unique_id=None, exchange=None):
        """eph_prop_shard: partition the propagator's system by target body over the ranks (right after creation, on
        every rank); arguments as NBodyIntegration.shard."""
        self._exchange_cb = _shard_call("eph_prop_shard", self._h, rank, world, unique_id, exchange)
        return self

    def shard_peer(self, peer):
        """eph_prop_shard_peer: eph_prop_shard with the direct-write transport (a connected PeerTransport)."""
        _call("eph_prop_shard_peer", self._h, peer._h)
        self._peer = peer
        return self

    def step(self):
        _step("eph_prop_step", self._h)

    def step_n(self, n):
        _step("eph_prop_step_n", self._h, int(n))

    def step_to(self, t):
        _step("eph_prop_step_to", self._h, float(t))

    def time(self):
        t = C.c_double()
        _call("eph_prop_time", self._h, C.byref(t))
        return t.value

    def has_reached(self, t):
        f = C.c_int32()
        _call("eph_prop_has_reached", self._h, float(t), C.byref(f))
        return bool(f.value)

    def integrator_time(self):
        t = C.c_double()
        _call("eph_prop_integrator_time", self._h, C.byref(t))
        return t.value

    def state(self):
        pos, vel = np.zeros((self.n, 3)), np.zeros((self.n, 3))
        t, sc = C.c_double(), C.c_uint32()
        _call("eph_prop_get_state", self._h, _p(pos), _p(vel), C.byref(t), C.byref(sc))
        return pos, vel, t.value, sc.value

    def take_solution(self):
        return Solution._adopt(_new_handle("eph_prop_take_solution", self._h), n=self.n)

    def propagate(self, to):
        h = C.c_void_p()
        _step("eph_prop_propagate", self._h, float(to), C.byref(h))
        return Solution._adopt(h, n=self.n)

    def integration(self):
        """the NBodyIntegration inside (borrowed)"""
        return NBodyIntegration._adopt(C.c_void_p(self._L.eph_prop_integrator(self._h)), owned=False, n=self.n)

    def clone(self):
        return self._clone("eph_prop_clone")


class Ephemeris(_Handle):
    """Device-resident table of the massive bodies' UniformSplines (what `Bodies` holds in the app)."""
    _DESTROY = "eph_ephemeris_destroy"

    def __init__(self, solution, mu):
        mu = _f64(mu)
        self._bind(_new_handle("eph_ephemeris_create", solution._h, _p(mu)))
        self.n_bodies = len(mu)

    # ---- the table is LIVE, like the reference's Arc<RwLock<PredictionTrajectory>> (dynamics/mod.rs:84-85): every batch bound to
    # it sees the new extent at its next call
    def append(self, tail, direction=FORWARD):
        """UniformSpline::append (FORWARD) / prepend (BACKWARD) for every body (trajectory.rs:515-534); raises ValueError where the
        reference's assert_eq! would panic, the table untouched."""
        _contiguous("eph_ephemeris_append", "eph_ephemeris_append: not contiguous (trajectory.rs:517-518,530-531)", self._h, tail._h,
                    int(direction))
        return self

    def merge(self, propagated, direction=FORWARD):
        """PredictionTarget::merge for the bodies (dynamics/celestial.rs:198-204 Forward, :220-226 Backward)."""
        _contiguous("eph_ephemeris_merge", "eph_ephemeris_merge: not contiguous (trajectory.rs:517-518,530-531)", self._h,
                    propagated._h, int(direction))
        return self

    def clear_before(self, at, body=-1):
        _call("eph_ephemeris_clear", self._h, int(body), float(at), 0)
        return self

    def clear_after(self, at, body=-1):
        _call("eph_ephemeris_clear", self._h, int(body), float(at), 1)
        return self

    def info(self, body):
        """(start, interval, npoly) of one body's spline as it is now"""
        s_, iv, npoly = C.c_double(), C.c_double(), C.c_int64()
        _call("eph_ephemeris_info", self._h, int(body), C.byref(s_), C.byref(iv), C.byref(npoly), None)
        return s_.value, iv.value, npoly.value

    @property
    def revision(self):
        r = C.c_uint64()
        _call("eph_ephemeris_info", self._h, -1, None, None, None, C.byref(r))
        return r.value

    def is_valid_at(self, t):
        """Bodies::is_valid_at (dynamics/spacecraft.rs:206-208)"""
        f = C.c_int32()
        _call("eph_ephemeris_is_valid_at", self._h, float(t), C.byref(f))
        return bool(f.value)

    def export_image(self):
        """One contiguous image of the table (numpy uint8): what rank 0 broadcasts (parallel.broadcast_ephemeris)."""
        need = C.c_uint64()
        self._L.eph_ephemeris_export(self._h, None, 0, C.byref(need))
        buf = np.empty(need.value, dtype=np.uint8)
        _call("eph_ephemeris_export", self._h, _p(buf, C.c_void_p), need.value, C.byref(need))
        return buf

    @classmethod
    def from_image(cls, image):
        image = np.ascontiguousarray(image, dtype=np.uint8)
        return cls._adopt(_new_handle("eph_ephemeris_import", _p(image, C.c_void_p), image.size),
                          n_bodies=int(np.frombuffer(image[8:16].tobytes(), dtype=np.uint64)[0]))

    def interpolation_errors(self, integration, n_steps):
        """debug.rs:182-238: advance `integration` (NBodyIntegration over the same bodies) up to n_steps steps, or to its
        bound, and return (max |position - spline position| per body in metres, steps taken)."""
        err = np.zeros(self.n_bodies)
        done = C.c_int64()
        _call("eph_ephemeris_interpolation_errors", self._h, integration._h, int(n_steps), _p(err), C.byref(done))
        return err, done.value


class SpacecraftBatch(_Handle):
    """n independent SpacecraftPropagator<[StateVector;1], ReferenceFrame, Bodies, <adaptive ERK pair>,
    CubicHermiteSplineSolout>, one device thread each. burns[i] = list of (start, end, acc[3], ref_body or -1)."""
    _DESTROY = "eph_craft_batch_destroy"

    def __init__(self, ephemeris, t0, pos, vel, method="Verner87", params=None, burns=None, max_knots=4096):
        self.ephemeris = ephemeris
        pos, vel = _f64(pos).reshape(-1, 3), _f64(vel).reshape(-1, 3)
        self.n = len(pos)
        t0 = _f64(np.broadcast_to(np.asarray(t0, dtype=np.float64), (self.n,)))
        self.params = params or AdaptiveParams.default()
        burns = burns if burns is not None else [[] for _ in range(self.n)]
        self._bind(_new_handle("eph_craft_batch_create", ephemeris._h, self.n, _p(t0), _p(pos), _p(vel), method.encode(),
                               C.byref(self.params), *_burn_csr(burns, self.n), int(max_knots)))

    def step_n(self, n_steps=1):
        """IncrementalPropagator::step n_steps times for every craft (one knot per step)."""
        _call("eph_craft_batch_step_n", self._h, int(n_steps))

    def clone(self):
        """SpacecraftPropagator: Clone -- a deep copy (state, knots, events) that can be resumed independently."""
        return self._clone("eph_craft_batch_clone")

    @classmethod
    def gather(cls, sources, source_of=None, craft_of=None):
        """A new batch whose craft i is craft craft_of[i] of sources[source_of[i]], as it is now, bit for bit
        (eph_craft_batch_gather): removing, adding, splitting, merging, permuting and duplicating ships are all this call. source_of
        None: every craft from the one source; craft_of None (and source_of None): all sources concatenated in order. The sources
        must share ephemeris, method, parameters, body order, a pending retry_failed and the event setup (ValueError names the first
        disagreement); they are not changed and stay independent of the result."""
        sources = list(sources)
        if not sources:
            raise ValueError("SpacecraftBatch.gather: at least one source batch")
        handles = (C.c_void_p * len(sources))(*[s._h for s in sources])
        co = None if craft_of is None else np.ascontiguousarray(craft_of, dtype=np.int64).reshape(-1)
        so = None if source_of is None else np.ascontiguousarray(source_of, dtype=np.int32).reshape(-1)
        if so is not None and (co is None or len(so) != len(co)):
            raise ValueError("SpacecraftBatch.gather: source_of needs a craft_of of the same length")
        n_out = sum(s.n for s in sources) if co is None else len(co)
        if co is not None and n_out == 0:            # an empty selection is still a selection: craft_of stays a pointer
            co = np.zeros(1, dtype=np.int64)
            so = None if so is None else np.zeros(1, dtype=np.int32)
        h = C.c_void_p()
        st = _lib().eph_craft_batch_gather(len(sources), handles, n_out, _p_or_null(so, _i32p), _p_or_null(co, _i64p), C.byref(h))
        if st == ERR_BAD_ARGUMENT:
            raise ValueError(_lib().eph_last_error().decode() or "SpacecraftBatch.gather: bad argument")
        _check(st, "eph_craft_batch_gather")
        first = sources[0]
        attributes = {k: v for k, v in vars(first).items() if k not in ("_L", "_h", "_owned")}
        attributes["n"] = int(n_out)
        return cls._adopt(h, **attributes)

    def select(self, indices):
        """The craft `indices` of this batch (in that order; an index may repeat), or those a boolean mask keeps, as a new batch."""
        idx = np.asarray(indices)
        if idx.dtype == bool:
            if idx.shape != (self.n,):
                raise ValueError("SpacecraftBatch.select: a mask has one entry per craft")
            idx = np.flatnonzero(idx)
        return type(self).gather([self], None, idx.astype(np.int64).reshape(-1))

    @classmethod
    def concat(cls, batches):
        """All craft of `batches`, in order, as one new batch."""
        return cls.gather(batches)

    def retry_failed(self):
        """Re-arm: the NEXT propagate / step_n steps the craft whose last step returned a StepError too -- the reference's next
        step() on a propagator that returned Err (how a stored ship propagator resumes once the ephemeris has grown)."""
        _call("eph_craft_batch_retry_failed", self._h)
        return self

    def propagate(self, t_end):
        """step_to(t_end) for every craft; per-craft outcomes in status()"""
        _call("eph_craft_batch_propagate", self._h, float(t_end))

    def status(self):
        st, nk = np.zeros(self.n, np.int32), np.zeros(self.n, np.int32)
        at, sp = np.zeros(self.n, np.uint32), np.zeros(self.n, np.uint32)
        _call("eph_craft_batch_status", self._h, _p(st, _i32p), _p(nk, _i32p), _p(at, _u32p), _p(sp, _u32p))
        return dict(status=st, nknots=nk, attempts=at, steps=sp)

    RECORD = np.dtype([("t", "f8"), ("pos", "f8", 3), ("vel", "f8", 3), ("next_h", "f8"), ("status", "i4"), ("nknots", "i4"),
                       ("attempts", "u4"), ("steps", "u4")])        # eph_craft_record

    def set_body_order(self, order):
        """The order in which the massive bodies' terms are added in the acceleration (eph_craft_batch_set_body_order):
        a permutation of range(n_bodies), or None for the table's order."""
        o = None if order is None else np.ascontiguousarray(order, dtype=np.int32)
        _call("eph_craft_batch_set_body_order", self._h, _p_or_null(o, _i32p))
        return self

    def summary(self, out=None):
        """status() and state() in one device-packed record array (eph_craft_batch_summary): fields t, pos, vel, next_h,
        status, nknots, attempts, steps. `out`: a record array of n entries to fill (one the caller keeps between sweeps
        has its pages mapped already: the copy into a fresh 21 MB allocation pays a page fault per 4 KB)."""
        rec = np.empty(self.n, dtype=self.RECORD) if out is None else out
        assert rec.itemsize == 80 and rec.shape == (self.n,) and rec.flags.c_contiguous
        _call("eph_craft_batch_summary", self._h, rec.ctypes.data_as(C.c_void_p))
        return rec

    def state(self):
        t, h = np.zeros(self.n), np.zeros(self.n)
        p, v = np.zeros((self.n, 3)), np.zeros((self.n, 3))
        _call("eph_craft_batch_state", self._h, _p(t), _p(p), _p(v), _p(h))
        return dict(t=t, pos=p, vel=v, next_h=h)

    def knots(self, craft, nknots=None):
        nk = int(self.status()["nknots"][craft]) if nknots is None else int(nknots)
        t, p, v = np.zeros(nk), np.zeros((nk, 3)), np.zeros((nk, 3))
        _call("eph_craft_batch_knots", self._h, int(craft), _p(t), _p(p), _p(v))
        return t, p, v

    def knot_slabs(self, first_knot=0, n_knots=None):
        """All craft at once: (t[k][craft], y[k][6][craft]) for knots first_knot .. first_knot + n_knots - 1; entries
        at or beyond a craft's nknots are unspecified (use status()["nknots"])."""
        if n_knots is None:
            n_knots = int(self.status()["nknots"].max()) - first_knot
        t = np.zeros((n_knots, self.n))
        y = np.zeros((n_knots, 6, self.n))
        _call("eph_craft_batch_knot_slabs", self._h, int(first_knot), int(n_knots), _p(t), _p(y))
        return t, y

    def eval(self, at, reference_body=-1, raw=False):
        """Where is every craft at the epochs `at`, relative to body `reference_body` of the ephemeris (table order; -1 =
        inertial): EvaluateTrajectory::state_vector on every craft's knots, on the device (eph_craft_batch_eval).
        `at` of shape (m,): the same epochs for every craft; (m, n): every craft its own. Returns
        (pos[m, n, 3], vel[m, n, 3], inside[m, n]); raw=True: (y[m, 6, n], inside[m, n]), the device layout, no transpose.
        Entries the reference answers None (outside the craft's knots or the body's spline) are zero with inside False."""
        at = _f64(at)
        if at.ndim == 0:
            at = at.reshape(1)
        if at.ndim not in (1, 2) or (at.ndim == 2 and at.shape[1] != self.n):
            raise ValueError("SpacecraftBatch.eval: `at` has shape (m,) or (m, n)")
        m = at.shape[0]
        y = np.zeros((m, 6, self.n))
        inside = np.zeros((m, self.n), dtype=np.uint8)
        _call("eph_craft_batch_eval", self._h, m, _p(at), 1 if at.ndim == 2 else 0, int(reference_body), _p(y), _p(inside, _u8p))
        inside = inside.astype(bool)
        if raw:
            return y, inside
        return (np.ascontiguousarray(y[:, :3].transpose(0, 2, 1)), np.ascontiguousarray(y[:, 3:].transpose(0, 2, 1)), inside)

    def plot_points(self, view, requests, craft=None):
        """The adaptive plot sampler on the batch's own knots (eph_craft_batch_plot_points): plot p draws craft craft[p]
        (None: plot p is craft p), read from the knot slabs on the device. view and requests as in plot_points(), the
        requests without source_body / knots (the source is the craft); one dict may be given for all plots.
        -> list of (status, failed_at, t[k], xyz[k, 3] float32), what plot_points() returns for the craft's knots."""
        requests, (crafts,) = _per_request("SpacecraftBatch.plot_points: one craft per request", self.n, requests, craft)
        n = len(requests)
        arr, cap = _plot_requests(requests, craft_source=True)
        out = _PlotOut(n, cap)
        _call("eph_craft_batch_plot_points", self._h, C.byref(_plot_view(view)), n, arr, _p_or_null(crafts, _i64p), *out.args())
        return out.rows(n)

    SEGMENT = np.dtype([("plot", "i8"), ("transition", "i4"), ("timeline_segment", "i4"), ("soi_body", "i4"), ("reference_body", "i4"),
                        ("kind", "i4"), ("is_burn", "i4"), ("overlapping", "i4"), ("start", "f8"), ("end", "f8")], align=True)  # eph_plot_segment

    def plot_segments(self, view, configs, body_parent, craft=None):
        """setup_segment_plotting (ephemeris_explorer/src/analysis.rs:159-296) on the device, ending in the sampler of
        plot_points() (eph_craft_batch_plot_segments): entry p splits craft craft[p] (None: entry p is craft p) at its SOI
        transitions and at the boundaries of its timeline, as the batch holds them now (events must be enabled).
        configs: list of dict(start, end, bound=0, enabled=1, tan2_angular_resolution, max_points_per_segment,
        reference_body=-1 (Primary) | body), or one dict for all entries; body_parent: soi_parents(system).
        -> (segments, plots): segments a record array (SEGMENT: plot, transition, timeline_segment, soi_body, reference_body,
        kind, is_burn, overlapping, start, end) in spawn order, entry by entry; plots[s] what plot_points() returns for
        segment s, or None with view=None (records only). Sizes with the records-only call, then fills."""
        configs, (crafts,) = _per_request("SpacecraftBatch.plot_segments: one craft per config", self.n, configs, craft)
        n = len(configs)
        arr = (OrbitPlotConfig * max(n, 1))()
        cap = 1
        for i, c in enumerate(configs):
            arr[i] = OrbitPlotConfig(float(c["start"]), float(c["end"]), int(c.get("bound", 0)), int(c.get("enabled", 1)),
                                     float(c["tan2_angular_resolution"]), int(c["max_points_per_segment"]), int(c.get("reference_body", -1)))
            cap = max(cap, int(c["max_points_per_segment"]))
        parents = np.ascontiguousarray(body_parent, dtype=np.int32).ravel()
        first = np.zeros(n + 1, dtype=np.int64)
        head = (self._h, n, arr, _p_or_null(crafts, _i64p), _p(parents, _i32p))
        st = _lib().eph_craft_batch_plot_segments(*head, 0, None, _p(first, _i64p), None, 0, None, None, None, None, None)
        total = int(first[n])
        if st != ERR_BAD_ARGUMENT or total == 0:        # (a sizing call that is refused has written the total it needs)
            _check(st, "eph_craft_batch_plot_segments")
        segments = np.zeros(total, dtype=self.SEGMENT)
        if total == 0:
            return segments, (None if view is None else [])
        records = segments.ctypes.data_as(C.POINTER(PlotSegment))
        if view is None:
            _call("eph_craft_batch_plot_segments", *head, total, records, _p(first, _i64p), None, 0, None, None, None, None, None)
            return segments, None
        out = _PlotOut(total, cap)
        _call("eph_craft_batch_plot_segments", *head, total, records, _p(first, _i64p), C.byref(_plot_view(view)), *out.args())
        return segments, out.rows(total)

    MARKER = np.dtype([("request", "i8"), ("kind", "i4"), ("index", "i4"), ("body", "i4"), ("status", "i4"), ("time", "f8"),
                       ("position", "f8", 3), ("distance", "f8"), ("apsis_distance", "f8"), ("frame", "f8", 9)], align=True)  # eph_plot_marker

    def plot_markers(self, requests, craft=None):
        """The event markers of the batch's plots (eph_craft_batch_plot_markers; the app's plot_*_markers and *_marker_picking,
        ephemeris_explorer/src/ui/world/tooltip.rs:84-245, picking.rs:256-447): request r asks, for one plot of craft craft[r]
        (None: request r is craft r), for every burn start, SOI transition, apsis and trajectory bound of that craft inside the
        plot's points. requests: list of dict(reference_body=-1, kinds, first, last), or one dict for all -- marker_requests()
        builds them from the output of plot_segments(). -> (markers, first): markers a record array (MARKER: request, kind,
        index, body, status, time, position, distance, apsis_distance, frame) request by request, manoeuvres, transitions,
        apsides, Start, End; first[r] .. first[r + 1] the records of request r. Sizes with the records-free call, then fills."""
        requests, (crafts,) = _per_request("SpacecraftBatch.plot_markers: one craft per request", self.n, requests, craft)
        n = len(requests)
        arr = (MarkerRequest * max(n, 1))()
        for i, q in enumerate(requests):
            arr[i] = MarkerRequest(int(q.get("reference_body", -1)), int(q["kinds"]), float(q["first"]), float(q["last"]))
        first = np.zeros(n + 1, dtype=np.int64)
        head = (self._h, n, arr, _p_or_null(crafts, _i64p))
        st = _lib().eph_craft_batch_plot_markers(*head, 0, None, _p(first, _i64p))
        total = int(first[n])
        if st != ERR_BAD_ARGUMENT or total == 0:        # (a sizing call that is refused has written the total it needs)
            _check(st, "eph_craft_batch_plot_markers")
        markers = np.zeros(total, dtype=self.MARKER)
        if total:
            _call("eph_craft_batch_plot_markers", *head, total, markers.ctypes.data_as(C.POINTER(PlotMarker)), _p(first, _i64p))
        return markers, first

    def closest_separation(self, requests, craft=None, target_craft=None):
        """The closest-separation search of target plotting on the batch's own knots (eph_craft_batch_closest_separation):
        request p searches craft craft[p] (None: request p is craft p) against body requests[p]["target_body"] of the live
        table or craft target_craft[p] of this batch (exactly one of the two >= 0; target_craft None: bodies only).
        requests: list of dict(target_body, left, right, precision, max_iterations, metric), or one dict for all.
        -> list of dict(found, time, distance, iterations, status, failed_at), what closest_separation() returns for the
        knots of the two craft."""
        requests, (crafts, targets) = _per_request("SpacecraftBatch.closest_separation: one craft (and one target craft) per request",
                                                   self.n, requests, craft, target_craft)
        n = len(requests)
        out = _SeparationOut(n)
        _call("eph_craft_batch_closest_separation", self._h, n, _separation_requests(requests, craft_source=True),
              _p_or_null(crafts, _i64p), _p_or_null(targets, _i64p), *out.args())
        return out.rows(n)

    UNSELECTED = np.iinfo(np.int32).min     # restart(): the outcome entry of a craft `which` did not select (never written)

    def restart(self, burns, plan_end=None, params=None, which=None):
        """Flight-plan restart in place (eph_craft_batch_restart): every selected craft continues from the knot where its new
        flight plan `burns` (the constructor's per-craft lists) diverges from the old one, as the app's new propagator would.
        plan_end: FlightPlan.end, a scalar or one per craft (None: +inf). params: new AdaptiveParams for the whole batch
        (only with which=None). which: a boolean mask or craft indices (None: all). Returns (restart_epoch[n], outcome[n]);
        an unselected craft's entries are NaN and UNSELECTED."""
        if len(burns) != self.n:
            raise ValueError("SpacecraftBatch.restart: one burn list per craft")
        pe = None if plan_end is None else _f64(np.broadcast_to(np.asarray(plan_end, dtype=np.float64), (self.n,)))
        sel = None
        if which is not None:
            w = np.asarray(which)
            sel = np.zeros(self.n, dtype=np.uint8)
            if w.dtype == bool:
                sel[:] = w.reshape(self.n)
            else:
                sel[w.astype(np.int64)] = 1
        epoch = np.full(self.n, np.nan)
        outcome = np.full(self.n, self.UNSELECTED, dtype=np.int32)
        _call("eph_craft_batch_restart", self._h, _p_or_null(sel, _u8p), *_burn_csr(burns, self.n), _p_or_null(pe),
              None if params is None else C.byref(params), _p(epoch), _p(outcome, _i32p))
        if params is not None:
            self.params = params
        return epoch, outcome

    def reset_knots(self):
        """Keep only the newest knot of every craft (as knot 0) and clear KNOTS_FULL: the drain point of a long run."""
        _call("eph_craft_batch_reset_knots", self._h)

    def reset_events(self):
        """Keep only the newest SOI transition of every craft, drop the apsides, clear EVENTS_FULL (after reading)."""
        _call("eph_craft_batch_reset_events", self._h)

    def enable_events(self, soi_radius, max_transitions=64, max_apsides=1024):
        """Switch to the app's SpacecraftSolout: SOI transitions + apsides per accepted step (call before propagate)."""
        r = _f64(soi_radius)
        _call("eph_craft_batch_enable_events", self._h, _p(r), int(max_transitions), int(max_apsides))
        return self

    def event_counts(self):
        ntr, nap, st = (np.zeros(self.n, dtype=np.int32) for _ in range(3))
        _call("eph_craft_batch_event_counts", self._h, _p(ntr, _i32p), _p(nap, _i32p), _p(st, _i32p))
        return ntr, nap, st

    def events(self, craft, counts=None):
        """(transitions: time[], body[]), (apsides: time[], distance[], body[], kind[]) of one craft."""
        ntr, nap, _ = counts if counts is not None else self.event_counts()
        a, b = max(int(ntr[craft]), 1), max(int(nap[craft]), 1)
        tt, tb = np.zeros(a), np.zeros(a, dtype=np.int32)
        at, ad, ab, ak = np.zeros(b), np.zeros(b), np.zeros(b, dtype=np.int32), np.zeros(b, dtype=np.int32)
        _call("eph_craft_batch_events", self._h, int(craft), _p(tt), _p(tb, _i32p), _p(at), _p(ad), _p(ab, _i32p), _p(ak, _i32p))
        k, m = int(ntr[craft]), int(nap[craft])
        return (tt[:k], tb[:k]), (at[:m], ad[:m], ab[:m], ak[:m])

    def kernel_ms(self):
        ms = C.c_double()
        _call("eph_craft_batch_kernel_time", self._h, C.byref(ms))
        return ms.value


def _burn_arrays(burns):
    n = len(burns)
    bs = _f64([b[0] for b in burns] or [0.0])
    be = _f64([b[1] for b in burns] or [0.0])
    ba = _f64([b[2] for b in burns] or [[0.0, 0.0, 0.0]])
    br = np.ascontiguousarray([b[3] for b in burns] or [0], dtype=np.int32)
    return n, bs, be, ba, br


def _burn_args(burns):
    """a list of burns as the C ABI takes it: count, start, end, acceleration, reference body"""
    n, bs, be, ba, br = _burn_arrays(burns)
    return n, _p(bs), _p(be), _p(ba), _p(br, _i32p)


def _burn_csr(burns, n):
    """n per-craft burn lists as the C ABI takes them: offsets[n + 1], then start / end / acceleration / reference body per burn"""
    off = np.zeros(n + 1, dtype=np.int64)
    flat = []
    for i, bl in enumerate(burns):
        flat.extend(bl)
        off[i + 1] = len(flat)
    return (_p(off, _i64p), *_burn_args(flat)[1:])


def _knot_arrays(knots):
    """a (t, pos, vel) knot triple, or None for no knots -> the C ABI's (count, t[k], pos[k][3], vel[k][3])"""
    if knots is None:
        knots = np.zeros(0), np.zeros((0, 3)), np.zeros((0, 3))
    t, pos, vel = _f64(knots[0]).ravel(), _f64(knots[1]).reshape(-1, 3), _f64(knots[2]).reshape(-1, 3)
    return len(t), _p(t), _p(pos), _p(vel)


def _per_request(mismatch, n_craft, requests, *craft_lists):
    """The conventions of the batch readers: one dict stands for all requests, and every optional craft index list has one
    entry per request (ValueError(mismatch) otherwise) -> (requests, the lists as int64 arrays or None)."""
    lists = [None if c is None else np.ascontiguousarray(c, dtype=np.int64).ravel() for c in craft_lists]
    if isinstance(requests, dict):
        requests = [requests] * (n_craft if lists[0] is None else len(lists[0]))
    if any(c is not None and len(c) != len(requests) for c in lists):
        raise ValueError(mismatch)
    return requests, lists


def timeline_divergence_time(old_burns, new_burns, before):
    """Timeline::divergence_time_before (spacecraft.rs:179-213) of new_burns against old_burns; burns are
    (start, end, acc[3], ref_body or -1). The epoch a flight plan restarts from (flight_plan.rs:263-303)."""
    out = C.c_double()
    _call("eph_timeline_divergence_time", *_burn_args(list(old_burns)), *_burn_args(list(new_burns)), float(before), C.byref(out))
    return out.value


def hermite_eval(t, pos, vel, at, with_velocity=True):
    """CubicHermiteSpline::state_vector at many epochs (device)."""
    t, pos, vel, at = _f64(t), _f64(pos), _f64(vel), _f64(np.atleast_1d(at))
    m = len(at)
    op, ov = np.zeros((m, 3)), np.zeros((m, 3))
    inside = np.zeros(m, dtype=np.uint8)
    _call("eph_hermite_eval", len(t), _p(t), _p(pos), _p(vel), m, _p(at), _p(op), _p(ov) if with_velocity else None, _p(inside, _u8p))
    return op, (ov if with_velocity else None), inside.astype(bool)


def _plot_view(view):
    """dict(camera_position, grid_matrix3 (3x3, columns = axes), grid_translation, cell_offset, current) -> PlotView"""
    v = PlotView()
    v.camera_position[:] = [float(x) for x in view["camera_position"]]
    m = np.asarray(view.get("grid_matrix3", np.eye(3)), dtype=np.float64)
    v.grid_matrix3[:] = [float(m[r, c]) for c in range(3) for r in range(3)]          # column major
    v.grid_translation[:] = [float(x) for x in view.get("grid_translation", (0.0, 0.0, 0.0))]
    v.cell_offset[:] = [float(x) for x in view.get("cell_offset", (0.0, 0.0, 0.0))]
    v.current = float(view["current"])
    return v


def plot_points(ephemeris, view, requests, knots=None):
    """compute_plot_points_parallel + PlotPoints::new (ephemeris_explorer/src/ui/world/plot.rs:93-149,272-374) for a batch
    of plots. view: dict(camera_position, grid_matrix3 (3x3, columns = axes), grid_translation, cell_offset, current);
    requests: list of dict(source_body | knots=(first, count), reference_body, start, end, bound, enabled,
    tan2_angular_resolution, max_points); knots: (t, pos, vel) arrays the hermite sources index into.
    -> list of (status, failed_at, t[k], xyz[k, 3] float32)."""
    n = len(requests)
    arr, cap = _plot_requests(requests)
    out = _PlotOut(n, cap)
    _call("eph_plot_points", ephemeris._h, C.byref(_plot_view(view)), n, arr, *_knot_arrays(knots), *out.args())
    return out.rows(n)


def _plot_requests(requests, craft_source=False):
    """-> (the eph_plot_request array, the point capacity the outputs need). craft_source: the batch's form, whose source is the
    craft itself."""
    arr = (PlotRequest * max(len(requests), 1))()
    cap = 1
    for i, r in enumerate(requests):
        if craft_source and ("source_body" in r or "knots" in r):
            raise ValueError("SpacecraftBatch.plot_points: the source is the craft (no source_body / knots)")
        first, count = r.get("knots", (0, 0))
        arr[i] = PlotRequest(int(r.get("source_body", -1)), int(r.get("reference_body", -1)), int(first), int(count),
                             float(r["start"]), float(r["end"]), int(r.get("bound", 0)), int(r.get("enabled", 1)),
                             float(r["tan2_angular_resolution"]), int(r["max_points"]))
        cap = max(cap, int(r["max_points"]))
    return arr, cap


class _PlotOut:
    """the point capacity and the five output arrays of the two plot calls"""

    def __init__(self, n, cap):
        m = max(n, 1)
        self.cap, self.t, self.xyz = cap, np.zeros((m, cap)), np.zeros((m, cap, 3), dtype=np.float32)
        self.count, self.status, self.failed_at = np.zeros(m, np.int64), np.zeros(m, np.int32), np.zeros(m)

    def args(self):
        return self.cap, _p(self.t), _p(self.xyz, _fp), _p(self.count, _i64p), _p(self.status, _i32p), _p(self.failed_at)

    def rows(self, n):
        return [(int(self.status[i]), float(self.failed_at[i]), self.t[i, :self.count[i]].copy(), self.xyz[i, :self.count[i]].copy())
                for i in range(n)]


SEGMENT_KINDS = ("Capture", "Escape", "Flyby", "Transit", "Orbit")      # PlotSegment, analysis.rs:144-151, by eph_plot_segment.kind


def segment_name(names, segment):
    """The Name setup_segment_plotting gives a plot (analysis.rs:212,245-290), e.g. "Mars Flyby Burn": names in table order,
    segment one record of SpacecraftBatch.plot_segments."""
    return f"{names[int(segment['soi_body'])]} {SEGMENT_KINDS[int(segment['kind'])]}" + (" Burn" if int(segment["is_burn"]) else "")


MARKER_KINDS = ("Manoeuvre", "Transition", "Periapsis", "Apoapsis", "Start", "End")
MARK_MANOEUVRES, MARK_TRANSITIONS, MARK_APSIDES, MARK_BOUNDS = 1, 2, 4, 8


def marker_requests(segments, plots):
    """The requests of SpacecraftBatch.plot_markers for the output of SpacecraftBatch.plot_segments(view, ...): one per record,
    relative to the record's reference body, between the epochs of the plot's first and last point; manoeuvres only on burn
    pieces (BurnPlotSegment), transitions only on plots that are not an overlapping copy, apsides and bounds on every plot;
    kinds = 0 for a plot without points. The craft of request s is the craft of entry segments["plot"][s]."""
    out = []
    for r, p in zip(segments, plots):
        t = p[2]
        if len(t) == 0:
            out.append({"reference_body": int(r["reference_body"]), "kinds": 0, "first": 0.0, "last": 0.0})
            continue
        kinds = MARK_APSIDES | MARK_BOUNDS | (MARK_MANOEUVRES if r["is_burn"] else 0) | (0 if r["overlapping"] else MARK_TRANSITIONS)
        out.append({"reference_body": int(r["reference_body"]), "kinds": kinds, "first": float(t[0]), "last": float(t[-1])})
    return out


def marker_name(names, marker):
    """What the app's tooltip calls a marker ("Mars Periapsis", "Sun Transition", "Start"): names the bodies' names in table
    order, marker one record of SpacecraftBatch.plot_markers. A manoeuvre is named after its frame's body ("Inertial" without)."""
    kind, body = MARKER_KINDS[int(marker["kind"])], int(marker["body"])
    if kind in ("Start", "End"):
        return kind
    return f"{names[body] if body >= 0 else 'Inertial'} {kind}"


def _separation_requests(requests, craft_source=False):
    """-> the eph_separation_request array. craft_source: the batch's form, whose source and target craft are its own."""
    arr = (SeparationRequest * max(len(requests), 1))()
    for i, r in enumerate(requests):
        if craft_source and ("source_body" in r or "source_knots" in r or "target_knots" in r):
            raise ValueError("SpacecraftBatch.closest_separation: source and target craft are the batch's (no source_body / knots)")
        sf, sc = r.get("source_knots", (0, 0))
        tf, tc = r.get("target_knots", (0, 0))
        arr[i] = SeparationRequest(int(r.get("source_body", -1)), int(r.get("target_body", -1)), int(sf), int(sc), int(tf), int(tc),
                                   float(r["left"]), float(r["right"]), float(r.get("precision", 0.001)),
                                   int(r.get("max_iterations", 1000)), int(r.get("metric", 0)))
    return arr


class _SeparationOut:
    """the six output arrays of the two closest-separation calls"""

    def __init__(self, n):
        m = max(n, 1)
        self.found, self.time, self.distance = np.zeros(m, np.uint8), np.zeros(m), np.zeros(m)
        self.iterations, self.status, self.failed_at = np.zeros(m, np.int32), np.zeros(m, np.int32), np.zeros(m)

    def args(self):
        return (_p(self.found, _u8p), _p(self.time), _p(self.distance), _p(self.iterations, _i32p), _p(self.status, _i32p),
                _p(self.failed_at))

    def rows(self, n):
        return [dict(found=bool(self.found[i]), time=float(self.time[i]), distance=float(self.distance[i]),
                     iterations=int(self.iterations[i]), status=int(self.status[i]), failed_at=float(self.failed_at[i]))
                for i in range(n)]


def closest_separation(ephemeris, requests, knots=None):
    """setup_target_plotting's search (ephemeris_explorer/src/analysis.rs:344-366): RelativeTrajectory::
    closest_separation_between + PlotSeparation.distance for a batch of (trajectory, target) pairs, on the device.
    requests: list of dict(source_body | source_knots=(first, count), target_body | target_knots=(first, count), left, right,
    precision=0.001, max_iterations=1000, metric=0 (distance_squared_at) | 1 (distance_at)); knots: (t, pos, vel) arrays the
    Hermite trajectories index into. -> list of dict(found, time, distance, iterations, status, failed_at)."""
    n = len(requests)
    out = _SeparationOut(n)
    _call("eph_closest_separation", ephemeris._h, n, _separation_requests(requests), *_knot_arrays(knots), *out.args())
    return out.rows(n)


def hermite_join(lhs, rhs):
    """SpacecraftPropagator::join(lhs, rhs) (ephemeris/src/propagators/spacecraft.rs:558-561) on (t, pos, vel) knot
    arrays -> the joined (t, pos, vel). Host only."""
    lhs, rhs = _knot_arrays(lhs), _knot_arrays(rhs)
    cap = lhs[0] + rhs[0]
    t, p, v = np.zeros(max(cap, 1)), np.zeros((max(cap, 1), 3)), np.zeros((max(cap, 1), 3))
    n = C.c_int64()
    _call("eph_hermite_join", *lhs, *rhs, cap, _p(t), _p(p), _p(v), C.byref(n))
    return t[:n.value].copy(), p[:n.value].copy(), v[:n.value].copy()


def transitions_join(lhs, rhs, at):
    """item.transitions.clear_after(at); item.transitions.extend(rhs) -- the SoiTransitions half of
    PredictionTarget::merge (ephemeris_explorer/src/dynamics/spacecraft.rs:838-839). lhs / rhs are (time, body) arrays;
    `at` is the merged solution's trajectory.start(). Host only."""
    lt, lb = _f64(lhs[0]).ravel(), np.ascontiguousarray(lhs[1], dtype=np.int32).ravel()
    rt, rb = _f64(rhs[0]).ravel(), np.ascontiguousarray(rhs[1], dtype=np.int32).ravel()
    cap = len(lt) + len(rt)
    t, b = np.zeros(max(cap, 1)), np.zeros(max(cap, 1), dtype=np.int32)
    n = C.c_int64()
    _call("eph_transitions_join", len(lt), _p(lt), _p(lb, _i32p), len(rt), _p(rt), _p(rb, _i32p), float(at), cap, _p(t),
          _p(b, _i32p), C.byref(n))
    return t[:n.value].copy(), b[:n.value].copy()


def apsides_join(lhs, rhs, at):
    """item.apsides.clear_after(at); item.apsides.extend(rhs) (ephemeris_explorer/src/dynamics/spacecraft.rs:836-837).
    lhs / rhs are (time, distance, kind, body) arrays. Host only."""
    def parts(x):
        return (_f64(x[0]).ravel(), _f64(x[1]).ravel(), np.ascontiguousarray(x[2], dtype=np.int32).ravel(),
                np.ascontiguousarray(x[3], dtype=np.int32).ravel())
    lt, ld, lk, lb = parts(lhs)
    rt, rd, rk, rb = parts(rhs)
    cap = len(lt) + len(rt)
    m = max(cap, 1)
    t, d, k, b = np.zeros(m), np.zeros(m), np.zeros(m, dtype=np.int32), np.zeros(m, dtype=np.int32)
    n = C.c_int64()
    _call("eph_apsides_join", len(lt), _p(lt), _p(ld), _p(lk, _i32p), _p(lb, _i32p), len(rt), _p(rt), _p(rd), _p(rk, _i32p),
          _p(rb, _i32p), float(at), cap, _p(t), _p(d), _p(k, _i32p), _p(b, _i32p), C.byref(n))
    return t[:n.value].copy(), d[:n.value].copy(), k[:n.value].copy(), b[:n.value].copy()


from .convergence import ConvergenceError, convergence, convergence_gang  # noqa: E402,F401  (needs NBodyIntegration above)
