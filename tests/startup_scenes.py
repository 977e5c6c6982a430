"""Scenes for k_lm_startup_small (csrc/step_srkn_small.hip): the multistep start-up of at most 32 bodies in one launch, alone and as
a gang. Shared by tests/test_startup_scenes.py (CPU: the conditions the scenes were planted for, on the C oracle alone) and
tests/test_gpu_startup_small.py (the device against the C oracle and against its own per-launch start-up, path 1). A plain module:
no fixtures, no GPU import.

What is planted, and for what:

  SIZES     1 (no pair at all), 2, 3; 16 | 17 (the row the chains walk grows from 16 to 32 doubles, the owner threads spill into a
            second wave); 31, 32. 33 is the first size that must stay on the per-launch route. Plummer spheres of
            workloads.plummer with the masses made distinct; the shipped systems of 3, 10 and 32 bodies beside them.
  massless  one body of mu == 0 among massive ones: its contributions are signed zeros in the ordered sums.
  backward  h < 0.
  PLAN      advance(1), advance(4), advance(L), advance(2 L + 5) on one handle: the start-up launches take m = 1, 4 and L - 5 macro
            steps, the second and third enter the ring at a slot other than its initial one with the FSAL carry of the launch
            before, and the first steady batch follows a partial start-up in the same call.
  bound     inside macro step 5's span, strictly between two substep times (BoundReached on a substep: the macro step is abandoned
            and every later call meets the same test); exactly on the boundary behind macro step 5 (BoundReached at macro step 6's
            own test); h = 2^-400 at t0 = 1 (StepSizeUnderflow from the first step).

`dry_run` restates the host's decision (NBodyIntegration::startup_small_steps, csrc/nbody.cpp): the tests of startup_macro_step and
srkn_step replayed over the macro steps a call wants, in the reference's order."""
import numpy as np

METHODS = {"QuinlanTremaine12": 12, "Stormer13": 13}          # method: L (ring length = start-up macro steps)
SUBSTEPS = 4                                                  # Substepper<4, BlanesMoan6B>
STAGES = 7                                                    # BlanesMoan6B, FSAL: 6 evaluations per substep after the first
SIZES = (1, 2, 3, 16, 17, 31, 32)
FIRST_PER_LAUNCH_SIZE = 33
H = 1.0 / 1024.0                                              # Plummer units (G = 1, total mass 1, scale radius 1)
SHIPPED = {"sun_earth_moon_2433282.5": 3, "simple_solar_system_2433282.5": 10, "full_solar_system_2433282.5": 32}
BOUND_REACHED, STEP_SIZE_UNDERFLOW = 3, 1                     # StepError values, as the oracle returns them (checked in the CPU test)


def plan(L):
    return (1, 4, L, 2 * L + 5)


def startup_evals(L):
    """right-hand-side evaluations of a whole start-up: the first, the FSAL table's first stage once, six per substep, one per macro step"""
    return 2 + L * (SUBSTEPS * (STAGES - 1) + 1)


def entry_slot(steps_taken, L):
    """ring slot of the newest level after `steps_taken` steps from a fresh handle (slot 0); every step moves the front one slot down"""
    return (-steps_taken) % L


class Scene:
    """one system: n bodies, a signed step, an optional bound"""

    def __init__(self, name, pos, vel, mu, h, t0=0.0, bound=None):
        self.name, self.pos, self.vel, self.mu = name, np.array(pos, dtype=np.float64), np.array(vel, dtype=np.float64), np.array(mu, dtype=np.float64)
        self.h, self.t0, self.bound, self.n = float(h), float(t0), bound, len(mu)

    def make(self, cls, method, **kw):
        """cls(pos, vel, mu, t0, h, method): orc.NBody or NBodyIntegration"""
        g = cls(self.pos, self.vel, self.mu, self.t0, self.h, method, **kw)
        if self.bound is not None:
            g.set_bound(self.bound)
        return g


def sphere(n, sign=1, massless=False, name=None):
    from ephemeris_explorer_amd.workloads import plummer
    pos, vel, mu = plummer(n)
    mu = mu * (1.0 + np.arange(n) / 7.0)                      # distinct: the two directed contributions of a pair cannot swap masses unseen
    if massless:
        mu[n // 2] = 0.0
    return Scene(name or f"plummer{n}{'+' if sign > 0 else '-'}{'-massless' if massless else ''}", pos, vel, mu, sign * H)


def shipped(name):
    from conftest import load_system
    s = load_system(name)
    return Scene(name.split("_2433")[0], s.pos, s.vel, s.mu, s.dt, t0=s.epoch)


def scenes():
    out = [sphere(n) for n in SIZES]
    out += [sphere(32, sign=-1), sphere(17, sign=-1, massless=True), sphere(3, massless=True)]
    out += [shipped(name) for name in SHIPPED]
    return out


def substep_times(t0, h, macro_steps):
    """problem.time at every substep boundary of the first `macro_steps` macro steps: time = time + h * (1 / 4), replayed"""
    hs, t, out = h * (1.0 / SUBSTEPS), t0, [t0]
    for _ in range(macro_steps * SUBSTEPS):
        t = t + hs
        out.append(t)
    return out


BOUND_MACRO_STEP = 5                                          # 1-based


def bound_scenes():
    """(scene, what fires): the bound inside macro step 5 between its second and third substep times; the bound exactly on the
    boundary behind macro step 5; the step that underflows at once"""
    ts = substep_times(0.0, H, BOUND_MACRO_STEP)
    a, b = ts[(BOUND_MACRO_STEP - 1) * SUBSTEPS + 1], ts[(BOUND_MACRO_STEP - 1) * SUBSTEPS + 2]
    inside, boundary, tiny = sphere(17, name="bound-inside"), sphere(17, name="bound-on-boundary"), sphere(17, name="underflow")
    inside.bound = 0.5 * (a + b)
    boundary.bound = ts[BOUND_MACRO_STEP * SUBSTEPS]
    tiny.h, tiny.t0 = 2.0 ** -400, 1.0
    return [(inside, BOUND_REACHED), (boundary, BOUND_REACHED), (tiny, STEP_SIZE_UNDERFLOW)]


INF = float("inf")


def dry_run(time, h, bound, substeps_taken, L, want):
    """the host's decision for a handle that qualifies by size and path: (m, time after) -- m = min(want, macro steps left) when
    none of the tests fires in those macro steps, 0 when one does, when the handle stands between two substeps, or is started"""
    if substeps_taken % SUBSTEPS or substeps_taken // SUBSTEPS >= L:
        return 0, time
    m, hs, t = min(want, L - substeps_taken // SUBSTEPS), h * (1.0 / SUBSTEPS), time
    for _ in range(m):
        if t >= bound or t + h == t:
            return 0, time
        for _ in range(SUBSTEPS):
            if t >= bound or t + hs == t:
                return 0, time
            t = t + hs
    return m, t


def status_of(handle, k):
    """advance(k) as a status: the oracle returns one, the product raises StepError with it"""
    try:
        return handle.advance(k) or 0
    except Exception as e:                                    # noqa: BLE001  (the product's StepError; anything else has no status)
        if not hasattr(e, "status"):
            raise
        return e.status


def record(h, acc=True, evals=True):
    """what is compared after every call: positions, velocities, accelerations, (time), (step count, evaluations)"""
    p, v, t, c = h.state()
    rec = dict(pos=np.array(p), vel=np.array(v), t=np.array([t]), steps=np.array([c], dtype=np.int64))
    if acc:
        rec["acc"] = np.array(h.acc())
    if evals:
        rec["evals"] = np.array([h.eval_count()], dtype=np.int64)
    return rec


def bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint64) if a.dtype == np.float64 else a


def assert_same(got, want, where):
    for key in want:
        g, w = got[key], want[key]
        assert g.shape == w.shape, f"{where}: {key}: {g.shape} against {w.shape}"
        diff = bits(g) != bits(w)
        if not diff.any():
            continue
        if g.ndim == 2:
            bad = np.flatnonzero(diff.any(axis=1))
            raise AssertionError(f"{where}: {key} of body {int(bad[0])} ({len(bad)} of {len(g)} bodies differ): {g[int(bad[0])]} against {w[int(bad[0])]}")
        raise AssertionError(f"{where}: {key} {g!r} against {w!r}")


def play(handle, calls, **what):
    """the calls on one handle: [(status, record)] after every call"""
    out = []
    for k in calls:
        st = status_of(handle, k)
        out.append((st, record(handle, **what)))
    return out


def assert_plays(got, want, where):
    assert len(got) == len(want), where
    for c, ((gs_, gr), (ws, wr)) in enumerate(zip(got, want)):
        assert gs_ == ws, f"{where}: call {c}: status {gs_} against {ws}"
        assert_same(gr, wr, f"{where}: after call {c}")
