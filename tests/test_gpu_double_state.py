"""-m gpu: the compensated integrator state, method "<M><Double>" (NBodyIntegration(..., compensated=True)), against the CPU
restatement of the reference's own convergence test (oracle/convergence_double.inc: the generic steppers on Double<DVec3>,
ephemeris/tests/solar_system_convergence.rs:12-216).

Every comparison is bit for bit (view(np.uint64)) on what the ABI returns: the VALUE parts of positions and velocities, the time
and the step count. No tolerance appears anywhere. The error parts cannot be read through the ABI; they are held indirectly:
y.value at step k + 1 depends on every error part at step k, so the cases compare after every single step.

BlanesMoan14A's convergence sweep is left to the CPU oracle (tests/test_convergence_pin.py): an SRKN stage is a launch of its own
on the device, 25 M launches for that sweep. The two multistep answers run here, each about 1.7 M steps in the single-workgroup
kernel."""
import numpy as np
import pytest

from conftest import load_system
from oracle import orc

pytestmark = pytest.mark.gpu

YEAR = 365 * 86400.0
INF = float("inf")


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def same(a, b):
    return np.array_equal(bits(a), bits(b))


def oracle_after(pos, vel, mu, t0, h, method, k):
    """(y values, dy values, time) after k steps of the restatement"""
    st, y, dy, end = orc.double_solve(pos, vel, mu, t0, INF, h, method, max_steps=k)
    assert st == 0
    return y[..., 0], dy[..., 0], end


def assert_state(g, want, count, what):
    p, v, t, c = g.state()
    assert c == count and t == want[2], (what, c, t, want[2])
    assert same(p, want[0]), (what, "positions", int((bits(p) != bits(want[0])).sum()))
    assert same(v, want[1]), (what, "velocities", int((bits(v) != bits(want[1])).sum()))


def step_by_step(gpu, pos, vel, mu, t0, h, method, steps, path=0):
    g = gpu.NBodyIntegration(pos, vel, mu, t0, h, method, compensated=True)
    assert g.compensated
    if path:
        g.set_path(path)
    for k in range(1, steps + 1):
        g.advance(1)
        assert_state(g, oracle_after(pos, vel, mu, t0, h, method, k), k, (method, len(mu), h, path, k))
    return g


@pytest.mark.parametrize("name,method,sign,steps", [("sun_earth_moon_2433282.5", "QuinlanTremaine12", 1, 40),
                                                    ("sun_earth_moon_2433282.5", "QuinlanTremaine12", -1, 20),
                                                    ("simple_solar_system_2433282.5", "Stormer13", 1, 30),
                                                    ("sun_earth_moon_2433282.5", "BlanesMoan14A", 1, 12)])
def test_every_step_equals_the_restatement(gpu, name, method, sign, steps):
    """start-up (ORDER macro steps of four BlanesMoan6B substeps) and steady steps, one advance(1) at a time"""
    s = load_system(name)
    step_by_step(gpu, s.pos, s.vel, s.mu, s.epoch, sign * s.dt, method, steps)


def test_srkn_method_on_65_bodies(gpu):
    from ephemeris_explorer_amd.workloads import plummer
    pos, vel, mu = plummer(65)
    step_by_step(gpu, pos, vel, mu, 0.0, 1.0 / 1024.0, "BlanesMoan6B", 6)


@pytest.fixture(scope="module")
def full():
    return load_system("full_solar_system_2433282.5")


def test_one_year_of_the_shipped_system_in_one_launch(gpu, full):
    """32 bodies -- the single-workgroup kernel's full width -- h = 600 s, bound = epoch + 365 d: 52 560 steps in one advance,
    which ends as the reference's solve does (BoundReached on the step after the last); the steady part was ONE launch."""
    s = full
    bound = s.epoch + YEAR
    g = gpu.NBodyIntegration(s.pos, s.vel, s.mu, s.epoch, 600.0, "QuinlanTremaine12", compensated=True)
    g.set_bound(bound)
    g.enable_timing()
    with pytest.raises(gpu.StepError) as e:
        g.advance(1 << 40)
    assert e.value.status == gpu.BOUND_REACHED
    st, y, dy, end = orc.double_solve(s.pos, s.vel, s.mu, s.epoch, bound, 600.0, "QuinlanTremaine12", native=True)
    assert st == 0 and end == bound
    assert_state(g, (y[..., 0], dy[..., 0], end), 52560, "one year")
    assert g.kernel_time()[1] == 1


@pytest.mark.parametrize("n", [31, 32, 33, 64, 65, 130])
def test_sizes_where_the_kernel_or_the_padding_changes(gpu, n):
    """12 start-up + 6 steady steps of QuinlanTremaine12; at most 32 bodies: the single-workgroup kernel (path 0, and 2) against
    the per-step launches (path 1) against the restatement; more bodies: the per-step launches, and path 2 is refused."""
    from ephemeris_explorer_amd.workloads import plummer
    pos, vel, mu = plummer(n)
    h = 1.0 / 1024.0
    want = {k: oracle_after(pos, vel, mu, 0.0, h, "QuinlanTremaine12", k) for k in (12, 15, 18)}
    for path in (0, 1, 2):
        g = gpu.NBodyIntegration(pos, vel, mu, 0.0, h, "QuinlanTremaine12", compensated=True)
        g.set_path(path)
        g.advance(12)
        assert_state(g, want[12], 12, (n, path))
        if path == 2 and n > 32:
            with pytest.raises(gpu.EphemerisError) as e:
                g.advance(3)
            assert e.value.status == gpu.ERR_UNSUPPORTED
            g.set_path(0)                              # ... and the handle is still usable
        g.advance(3)
        assert_state(g, want[15], 15, (n, path))
        g.advance(3)
        assert_state(g, want[18], 18, (n, path))


@pytest.mark.parametrize("n", [16, 17])
def test_row_lengths_and_a_ring_write_back_in_mid_rotation(gpu, n):
    """Stormer13 (L = 13). 16 bodies: rows of 16; 17 bodies: rows of 32 with fifteen zeros of padding, and the owner threads
    spill into a second wave. After the 13 start-up steps ONE launch of 31 steps: two full ring rotations and five steps, so the
    write-back runs at a rotation that is neither 0 nor L - 1."""
    from ephemeris_explorer_amd.workloads import plummer
    pos, vel, mu = plummer(n)
    h = 1.0 / 1024.0
    g = gpu.NBodyIntegration(pos, vel, mu, 0.0, h, "Stormer13", compensated=True)
    g.advance(13)
    g.advance(31)
    assert_state(g, oracle_after(pos, vel, mu, 0.0, h, "Stormer13", 44), 44, ("Stormer13", n))


def test_split_advances_clones_and_a_plain_neighbour(gpu, full):
    s = full
    args = (s.pos, s.vel, s.mu, s.epoch, s.dt, "QuinlanTremaine12")
    a = gpu.NBodyIntegration(*args, compensated=True)
    b = gpu.NBodyIntegration(*args, compensated=True)
    plain = gpu.NBodyIntegration(*args)                # created beside the tagged ones: its usual bits
    assert not plain.compensated
    a.advance(7); a.advance(5)
    b.advance(12)
    assert_state(a, b.state()[:3], 12, "7 + 5 == 12")
    a.advance(8)
    c = a.clone()                                      # a deep copy that carries the error parts
    assert c.compensated
    a.advance(13); a.advance(7)
    c.advance(20)
    want = oracle_after(s.pos, s.vel, s.mu, s.epoch, s.dt, "QuinlanTremaine12", 40)
    assert_state(a, want, 40, "original")
    assert_state(c, want, 40, "clone taken at step 20")
    plain.advance(40)
    o = orc.NBody(s.pos, s.vel, s.mu, s.epoch, s.dt)
    assert o.advance(40) == 0
    op, ov, ot, oc = o.state()
    assert_state(plain, (op, ov, ot), oc, "plain handle")
    assert not same(plain.state()[0], a.state()[0])    # the compensation was live: the plain values differ
    assert gpu._lib().eph_abi_version() == 3


def test_advance_many_with_a_tagged_member(gpu, full):
    s = full
    args = (s.pos, s.vel, s.mu, s.epoch, s.dt, "QuinlanTremaine12")
    gang = [gpu.NBodyIntegration(*args), gpu.NBodyIntegration(*args, compensated=True), gpu.NBodyIntegration(*args)]
    gpu.advance_many(gang, 12)
    gpu.advance_many(gang, 9)
    assert_state(gang[1], oracle_after(s.pos, s.vel, s.mu, s.epoch, s.dt, "QuinlanTremaine12", 21), 21, "tagged member")
    o = orc.NBody(s.pos, s.vel, s.mu, s.epoch, s.dt)
    assert o.advance(21) == 0
    for g in (gang[0], gang[2]):
        assert_state(g, o.state()[:3], 21, "plain member")


def test_refusals_leave_the_handle_usable(gpu):
    s = load_system("sun_earth_moon_2433282.5")
    args = (s.pos, s.vel, s.mu, s.epoch, s.dt)
    L = gpu._lib()
    g = gpu.NBodyIntegration(*args, "QuinlanTremaine12", compensated=True)
    g.advance(14)
    for path in (3, 4, 5, 6):
        with pytest.raises(gpu.EphemerisError) as e:
            g.set_path(path)
        assert e.value.status == gpu.ERR_UNSUPPORTED and "<Double>" in L.eph_last_error().decode()
    with pytest.raises(gpu.EphemerisError) as e:
        g.shard(0, 1, exchange=lambda *a: 0)
    assert e.value.status == gpu.ERR_UNSUPPORTED and "<Double>" in L.eph_last_error().decode()
    with pytest.raises(gpu.EphemerisError) as e:
        gpu.NBodyPropagator(s.pos, s.vel, s.mu, s.epoch, s.dt, gpu.FORWARD, np.full(len(s.mu), 2, dtype=np.uint32),
                            np.full(len(s.mu), 3, dtype=np.uint32), method="QuinlanTremaine12<Double>")
    assert e.value.status == gpu.ERR_UNSUPPORTED
    for bad in ("QuinlanTremaine12<Float>", "QuinlanTremaine12<double>", "QuinlanTremaine12 <Double>", "QuinlanTremaine12<Double> ",
                "<Double>", "QuinlanTremaine12<Double><Double>"):
        with pytest.raises(gpu.EphemerisError) as e:
            gpu.NBodyIntegration(*args, bad)
        assert e.value.status == gpu.ERR_BAD_ARGUMENT, bad
    with pytest.raises(gpu.EphemerisError) as e:       # the coefficient getters know base names only
        gpu.elm2_coeffs("QuinlanTremaine12<Double>")
    assert e.value.status == gpu.ERR_BAD_ARGUMENT
    g.advance(6)
    assert_state(g, oracle_after(*args, "QuinlanTremaine12", 20), 20, "after the refusals")


@pytest.mark.parametrize("method,answer", [("QuinlanTremaine12", 600.0), ("Stormer13", 300.0)])
def test_reference_convergence_answers_on_the_device(gpu, full, method, answer):
    """assert_eq!(convergence::<M>(problem, 75 s)?, N min) (solar_system_convergence.rs:346-357) on the committed 32-body system
    with the 365-day year of tests/test_convergence_pin.py, and the sweep's shape as that test asserts it."""
    s = full
    h, rows = gpu.convergence(s.pos, s.vel, s.mu, s.epoch, s.epoch + YEAR, method, 75.0)
    print(method, h, rows)
    assert h == answer, rows
    assert np.array_equal(rows[:, 0], 75.0 * 2.0 ** np.arange(len(rows)))
    assert (rows[:-1, 1] <= 10.0).all() and (rows[:-1, 2] <= 1.0).all()
    assert rows[-1, 1] > 10.0 or rows[-1, 2] > 1.0
    assert rows[-1, 0] == 2.0 * h
