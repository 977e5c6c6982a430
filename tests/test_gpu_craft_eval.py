"""-m gpu: eph_craft_batch_eval -- where is every craft of a batch at epoch T, relative to body B -- against the CPU oracle.

The expected value of craft c at epoch t is orc.hermite_eval(*batch.knots(c), t) (the knots themselves are proven equal to
orc.Craft's by test_gpu_craft.py), minus orc.Solution.eval(body, t) done in numpy for the relative case; None there <->
inside == 0 here, whose six values are +0.0. Every comparison is on bit patterns; there is no tolerance anywhere."""
import ctypes as C
import subprocess

import numpy as np
import pytest

from conftest import ROOT, load_system
from craft_cases import SHIP, bits, perturbed, simple_system  # noqa: F401  (the fixture)
from ephemeris_explorer_amd.systems import load_ship, parse_epoch
from oracle import orc

pytestmark = pytest.mark.gpu



def shared_epochs(t0, t_end, knots0, seed):
    """the issue's epoch list, shuffled: 200 random ones over [t0, t_end], t0, knot epochs of craft 0 (at most 2000, evenly
    strided), craft 0's last knot, one second before t0, one day after t_end. Returns (epochs, the random ones)."""
    rng = np.random.default_rng(seed)
    rand = rng.uniform(t0, t_end, 200)
    stride = max(1, -(-len(knots0) // 2000))
    at = np.concatenate([rand, [t0], knots0[::stride], [knots0[-1]], [t0 - 1.0, t_end + 86400.0]])
    rng.shuffle(at)
    return at, rand


def knot_span(batch, nknots):
    """every craft's first and last knot epoch, from the knot slab (times only)"""
    slab_t = np.zeros((int(nknots.max()), batch.n))
    assert batch._L.eph_craft_batch_knot_slabs(batch._h, 0, int(nknots.max()), slab_t.ctypes.data_as(C.POINTER(C.c_double)), None) == 0
    return slab_t[0].copy(), slab_t[nknots - 1, np.arange(batch.n)]


def oracle_answers(batch, crafts, at):
    """(y[m, 6, len(crafts)], inside[m, len(crafts)]) from orc.hermite_eval on each craft's knots; at: (m,) or (m, len(crafts))"""
    at = np.asarray(at)
    m = at.shape[0]
    y = np.zeros((m, 6, len(crafts)))
    inside = np.zeros((m, len(crafts)), dtype=bool)
    for k, c in enumerate(crafts):
        kt, kp, kv = batch.knots(int(c))
        for e in range(m):
            r = orc.hermite_eval(kt, kp, kv, at[e] if at.ndim == 1 else at[e, k])
            if r is not None:
                y[e, :3, k], y[e, 3:, k], inside[e, k] = r[0], r[1], True
    return y, inside


def body_states(osol, body, at):
    """orc.Solution.eval(body, t) for every epoch: (y[m, 6], ok[m])"""
    y, ok = np.zeros((len(at), 6)), np.zeros(len(at), dtype=bool)
    for e, t in enumerate(at):
        r = osol.eval(body, t)
        if r is not None:
            y[e, :3], y[e, 3:], ok[e] = r[0], r[1], True
    return y, ok


def relative(y, inside, by, bok):
    """the numpy subtraction: None where either side is None (zeros), else one IEEE subtraction per component"""
    ok = inside & bok[:, None]
    out = np.where(ok[:, None, :], y - by[:, :, None], 0.0)
    return out, ok


def assert_same(got, want, what):
    gy, gi = got
    wy, wi = want
    assert np.array_equal(gi, wi), f"{what}: inside differs at {np.argwhere(gi != wi)[:5].tolist()}"
    diff = bits(gy) != bits(wy)
    assert not diff.any(), f"{what}: {int(diff.sum())} values differ, first at [epoch, component, craft] {np.argwhere(diff)[:5].tolist()}"


@pytest.fixture(scope="module")
def wave_case(gpu, simple_system):
    """4(a): the wave form (n <= 12 288): the Mars Transfer Ship with its four burns plus 191 perturbed copies to 1951-01-01"""
    s, sol, eph, osol = simple_system
    ship = load_ship(SHIP)
    n = 192
    pos, vel = perturbed(ship, n, 20261016)
    burns = ship.burn_tuples(s.names)
    end = parse_epoch("1951-01-01 00:00:00")
    batch = gpu.SpacecraftBatch(eph, ship.start, pos, vel, ship.integrator, gpu.AdaptiveParams.default(ship.tolerance), [burns] * n,
                                max_knots=20000)
    batch.propagate(end)
    st = batch.status()
    assert np.isin(st["status"], (0, gpu.KNOTS_FULL)).all() and st["status"][0] == 0
    kt0 = batch.knots(0)[0]
    at, rand = shared_epochs(ship.start, end, kt0, 41)
    want = oracle_answers(batch, np.arange(n), at)
    return dict(batch=batch, n=n, at=at, rand=rand, want=want, t0=ship.start, end=end, crafts=np.arange(n))


@pytest.fixture(scope="module")
def thread_case(gpu, simple_system):
    """4(b): the thread form with dealt lanes: 16 384 perturbed copies over the first 220 days (all four burns), max_knots = 4096"""
    s, sol, eph, osol = simple_system
    ship = load_ship(SHIP)
    n = 16384
    pos, vel = perturbed(ship, n, 20261017)
    burns = ship.burn_tuples(s.names)
    end = ship.start + 220 * 86400.0
    batch = gpu.SpacecraftBatch(eph, ship.start, pos, vel, ship.integrator, gpu.AdaptiveParams.default(ship.tolerance), [burns] * n,
                                max_knots=4096)
    batch.propagate(end)
    st = batch.status()
    assert np.isin(st["status"], (0, gpu.KNOTS_FULL)).all() and st["status"][0] == 0
    kt0 = batch.knots(0)[0]
    at, rand = shared_epochs(ship.start, end, kt0, 42)
    crafts = np.unique(np.concatenate([[0], np.random.default_rng(43).choice(n, 512, replace=False)]))[:512]
    want = oracle_answers(batch, crafts, at)
    first, last = knot_span(batch, st["nknots"])
    return dict(batch=batch, n=n, at=at, rand=rand, want=want, t0=ship.start, end=end, crafts=crafts, first=first, last=last)


def check_inertial_shared(case, last_knots):
    batch, at, crafts = case["batch"], case["at"], case["crafts"]
    y, inside = batch.eval(at, raw=True)
    wy, wi = case["want"]
    assert_same((y[:, :, crafts], inside[:, crafts]), (wy, wi), "shuffled epochs")
    assert int(inside[:, crafts].sum()) == int(wi.sum())
    assert (bits(y)[~np.broadcast_to(inside[:, None, :], y.shape)] == 0).all()        # a None entry is six +0.0
    # every random epoch inside [t0, min over craft of the last knot] is answered for EVERY craft: nothing silently left out
    common = np.isin(at, case["rand"][case["rand"] <= last_knots.min()])
    assert common.sum() > 0 and inside[common].all()
    # the same epochs ascending (the common case) give the same bits
    order = np.argsort(at, kind="stable")
    ys, ins = batch.eval(at[order], raw=True)
    assert np.array_equal(ins, inside[order]) and np.array_equal(bits(ys), bits(y[order]))
    return y, inside


def test_inertial_shared_epochs_wave_form(gpu, wave_case):
    b = wave_case["batch"]
    assert wave_case["n"] <= 12288
    last = np.array([b.knots(c)[0][-1] for c in range(wave_case["n"])])
    check_inertial_shared(wave_case, last)


def test_inertial_shared_epochs_thread_form_dealt_lanes(gpu, thread_case):
    assert thread_case["n"] > 12288
    y, inside = check_inertial_shared(thread_case, thread_case["last"])
    at = thread_case["at"]
    want_inside = (at[:, None] >= thread_case["first"][None, :]) & (at[:, None] <= thread_case["last"][None, :])
    assert np.array_equal(inside, want_inside)


def test_relative_to_a_body(gpu, simple_system, wave_case):
    s, sol, eph, osol = simple_system
    batch, at = wave_case["batch"], wave_case["at"]
    for name in ("Earth", "Mars"):
        body = s.names.index(name)
        by, bok = body_states(osol, body, at)
        assert bok.sum() >= len(at) - 1                     # the ephemeris starts at t0: only `t0 - 1 s` is outside it
        want = relative(*wave_case["want"], by, bok)
        assert_same(batch.eval(at, reference_body=body, raw=True), want, f"relative to {name}")
        order = np.argsort(at, kind="stable")
        assert_same(batch.eval(at[order], reference_body=body, raw=True), (want[0][order], want[1][order]), f"relative to {name}, ascending")
    # the (pos, vel, inside) view is the same numbers transposed
    p, v, ins = batch.eval(at[:7], reference_body=s.names.index("Earth"))
    y, ins2 = batch.eval(at[:7], reference_body=s.names.index("Earth"), raw=True)
    assert np.array_equal(ins, ins2) and np.array_equal(bits(p), bits(y[:, :3].transpose(0, 2, 1))) and np.array_equal(bits(v), bits(y[:, 3:].transpose(0, 2, 1)))


def test_relative_follows_the_live_table(gpu, simple_system):
    """clear_before on the reference body's spline: the epochs before its new start become None for every craft, while the inertial
    evaluation still answers them. An Ephemeris (and oracle copy) of the test's own."""
    s, sol, _, osol = simple_system
    eph = gpu.Ephemeris(sol, s.mu)
    mine = osol.clone()
    ship = load_ship(SHIP)
    n = 8
    pos, vel = perturbed(ship, n, 7)
    earth = s.names.index("Earth")
    start, interval, _ = mine.info(earth)
    assert start == ship.start
    end = start + 3 * interval                              # three polynomials of the Earth's spline (low orbit: ~215 knots a day)
    batch = gpu.SpacecraftBatch(eph, ship.start, pos, vel, "Verner87", max_knots=8192)
    batch.propagate(end)
    assert (batch.status()["status"] == 0).all()
    at = np.sort(np.random.default_rng(8).uniform(ship.start, end, 60))
    inertial = oracle_answers(batch, np.arange(n), at)
    assert inertial[1].all()
    assert_same(batch.eval(at, reference_body=earth, raw=True), relative(*inertial, *body_states(mine, earth, at)), "before the clear")
    cut = start + 1.5 * interval
    eph.clear_before(cut, earth)
    mine.clear_before(cut, earth)
    new_start = mine.info(earth)[0]
    assert cut <= new_start < end and eph.info(earth)[0] == new_start
    by, bok = body_states(mine, earth, at)
    assert 0 < bok.sum() < len(at) and np.array_equal(bok, at >= new_start)
    got = batch.eval(at, reference_body=earth, raw=True)
    assert_same(got, relative(*inertial, by, bok), "after the clear")
    assert not got[1][~bok].any()
    assert_same(batch.eval(at, raw=True), inertial, "inertial after the clear")
    mars = s.names.index("Mars")                            # another body's spline is untouched
    assert_same(batch.eval(at, reference_body=mars, raw=True), relative(*inertial, *body_states(mine, mars, at)), "Mars after the clear")


def per_craft_epochs(case, crafts, first, last, seed, m=16):
    rng = np.random.default_rng(seed)
    n = case["n"]
    at = np.empty((m + 1, n))
    at[:m] = np.minimum(first + rng.uniform(0.0, 1.0, size=(m, n)) * (last - first), last)
    at[m] = last
    return at


def test_per_craft_epochs(gpu, simple_system, wave_case, thread_case):
    s, sol, eph, osol = simple_system
    earth = s.names.index("Earth")
    b = wave_case["batch"]
    ends = np.array([b.knots(c)[0][[0, -1]] for c in range(wave_case["n"])])
    for case, first, last, seed in ((wave_case, ends[:, 0], ends[:, 1], 51), (thread_case, thread_case["first"], thread_case["last"], 52)):
        crafts = case["crafts"][:64] if case is thread_case else case["crafts"]
        at = per_craft_epochs(case, crafts, first, last, seed)
        want = oracle_answers(case["batch"], crafts, at[:, crafts])
        assert want[1].all()                                 # every epoch is inside its craft's own span
        y, inside = case["batch"].eval(at, raw=True)
        assert inside.all()
        assert_same((y[:, :, crafts], inside[:, crafts]), want, "per-craft epochs")
        assert np.array_equal(bits(y[-1, :, crafts[0]]), bits(np.concatenate([np.ravel(k[-1]) for k in case["batch"].knots(int(crafts[0]))[1:]])))
        # relative: every lane evaluates the body at its own epoch
        yr, ir = case["batch"].eval(at, reference_body=earth, raw=True)
        for k, c in enumerate(crafts):
            by, bok = body_states(osol, earth, at[:, c])
            wy, wi = relative(want[0][:, :, k:k + 1], want[1][:, k:k + 1], by, bok)
            assert_same((yr[:, :, c:c + 1], ir[:, c:c + 1]), (wy, wi), f"per-craft epochs relative to the Earth, craft {c}")


def test_drained_slab(gpu, simple_system):
    """after reset_knots() and a further propagate only the new slab's span is covered"""
    s, sol, eph, osol = simple_system
    ship = load_ship(SHIP)
    n = 8
    pos, vel = perturbed(ship, n, 9)
    batch = gpu.SpacecraftBatch(eph, ship.start, pos, vel, "Verner87", max_knots=100)
    batch.propagate(ship.start + 86400.0)
    assert (batch.status()["status"] == gpu.KNOTS_FULL).all()
    full = np.array([batch.knots(c)[0][-1] for c in range(n)])
    batch.reset_knots()
    batch.propagate(full.max() + 3600.0)
    assert (batch.status()["nknots"] > 1).all()
    first = np.array([batch.knots(c)[0][0] for c in range(n)])
    assert np.array_equal(first, full)                      # knot 0 is the drained slab's newest knot
    at = np.concatenate([np.random.default_rng(10).uniform(ship.start, full.max() + 7200.0, 200), first, [ship.start]])
    want = oracle_answers(batch, np.arange(n), at)
    got = batch.eval(at, raw=True)
    assert_same(got, want, "drained slab")
    assert not got[1][at[:, None] < first[None, :]].any() and 0 < got[1].sum() < got[1].size
    assert_same(batch.eval(np.sort(at), raw=True), oracle_answers(batch, np.arange(n), np.sort(at)), "drained slab, ascending")


def test_eval_does_not_disturb_the_batch(gpu, simple_system):
    from ephemeris_explorer_amd.systems import soi_radii
    s, sol, eph, osol = simple_system
    ship = load_ship(SHIP)
    n = 200
    pos, vel = perturbed(ship, n, 11)
    burns = [ship.burn_tuples(s.names)[:2]] * n
    mid, end = ship.start + 1.5 * 86400.0, ship.start + 3 * 86400.0
    a, b = (gpu.SpacecraftBatch(eph, ship.start, pos, vel, "Verner87", burns=burns, max_knots=2048).enable_events(soi_radii(s), 16, 512)
            for _ in range(2))
    a.propagate(mid)
    b.propagate(mid)
    at = np.linspace(ship.start - 10.0, mid + 10.0, 50)
    got = a.eval(at, reference_body=s.names.index("Earth"), raw=True)
    clone = a.clone()
    again = clone.eval(at, reference_body=s.names.index("Earth"), raw=True)
    assert np.array_equal(got[1], again[1]) and np.array_equal(bits(got[0]), bits(again[0]))
    a.eval(np.tile(at[:, None], (1, n)), raw=True)          # the per-craft form as well
    a.propagate(end)
    b.propagate(end)
    sa, sb = a.summary(), b.summary()
    assert sa.tobytes() == sb.tobytes()
    ta, ya = a.knot_slabs()
    tb, yb = b.knot_slabs()
    nk = sa["nknots"]
    live = np.arange(ta.shape[0])[:, None] < nk[None, :]
    assert np.array_equal(bits(ta)[live], bits(tb)[live])
    assert np.array_equal(bits(ya)[np.broadcast_to(live[:, None, :], ya.shape)], bits(yb)[np.broadcast_to(live[:, None, :], yb.shape)])
    assert all(np.array_equal(x, y) for x, y in zip(a.event_counts(), b.event_counts()))
    for c in (0, 1, n // 2, n - 1):
        (tta, tba), apa = a.events(c)
        (ttb, tbb), apb = b.events(c)
        assert np.array_equal(bits(tta), bits(ttb)) and np.array_equal(tba, tbb)
        assert all(np.array_equal(np.asarray(x).view(np.uint8), np.asarray(y).view(np.uint8)) for x, y in zip(apa, apb))


def test_refusals_and_empty_requests(gpu, simple_system):
    s, sol, eph, osol = simple_system
    ship = load_ship(SHIP)
    pos, vel = perturbed(ship, 4, 12)
    batch = gpu.SpacecraftBatch(eph, ship.start, pos, vel, "Verner87", max_knots=256)
    batch.propagate(ship.start + 3600.0)
    L, h = batch._L, batch._h
    dp, u8p = C.POINTER(C.c_double), C.POINTER(C.c_uint8)
    at = np.array([ship.start, ship.start + 60.0])
    poison = np.float64(-7.25)
    out = np.full(2 * 6 * 4, poison)
    inside = np.full(2 * 4, 0xA5, dtype=np.uint8)
    atp, op, ip = at.ctypes.data_as(dp), out.ctypes.data_as(dp), inside.ctypes.data_as(u8p)
    bad = gpu.ERR_BAD_ARGUMENT
    assert L.eph_craft_batch_eval(h, -1, atp, 0, -1, op, ip) == bad
    assert L.eph_craft_batch_eval(h, 2, None, 0, -1, op, ip) == bad
    assert L.eph_craft_batch_eval(h, 2, atp, 0, -1, None, ip) == bad
    assert L.eph_craft_batch_eval(h, 2, atp, 0, -2, op, ip) == bad
    assert L.eph_craft_batch_eval(h, 2, atp, 0, s.n, op, ip) == bad
    assert L.eph_craft_batch_eval(h, 2, atp, 2, -1, op, ip) == bad
    assert L.eph_craft_batch_eval(h, 2, atp, -1, -1, op, ip) == bad
    assert L.eph_craft_batch_eval(h, 0, None, 0, -1, None, None) == 0       # m == 0: EPH_OK, nothing written
    assert L.eph_craft_batch_eval(h, 0, atp, 1, s.n - 1, op, ip) == 0
    assert (out == poison).all() and (inside == 0xA5).all()
    assert L.eph_craft_batch_eval(h, 2, atp, 0, s.n - 1, op, None) == 0     # `inside` may be NULL
    assert (out != poison).all() and (inside == 0xA5).all()
    with pytest.raises(ValueError):
        batch.eval(np.zeros((2, 3)))
    y, ins = batch.eval(ship.start + 60.0, raw=True)                        # a scalar epoch is m = 1
    assert y.shape == (1, 6, 4) and ins.all()


def test_full_width_multi_pass(gpu):
    """the default sweep population (262 144 craft, 0.25 d) at 32 shared epochs relative to the Earth: 403 MB of results, more than
    one staging pass"""
    from ephemeris_explorer_amd.workloads import craft_population
    s = load_system("full_solar_system_2433282.5")
    ship = load_ship(SHIP)
    days = 0.25
    end_eph = s.epoch + 2 * 86400.0
    sol = gpu.NBodyPropagator.from_system(s).propagate(end_eph)
    eph = gpu.Ephemeris(sol, s.mu)
    o = orc.Propagator(s.pos, s.vel, s.mu, s.epoch, s.dt, 1, s.count, s.degree)
    assert o.step_to(end_eph) == 0
    osol = o.take_solution()
    n = 262144
    pos, vel, _ = craft_population("transfer", n, s, ship)
    t_end = ship.start + days * 86400.0
    batch = gpu.SpacecraftBatch(eph, ship.start, pos, vel, "Verner87", max_knots=int(1200 * days) + 64)
    batch.propagate(t_end)
    st = batch.status()
    assert (st["status"] == 0).all()
    m = 32
    assert m * n * 49 > 256 << 20
    at = np.linspace(ship.start - 60.0, t_end + 60.0, m)
    at[5] = ship.start
    earth = s.names.index("Earth")
    y, inside = batch.eval(at, reference_body=earth, raw=True)
    first, last = knot_span(batch, st["nknots"])
    assert np.array_equal(inside, (at[:, None] >= first[None, :]) & (at[:, None] <= last[None, :]))
    crafts = np.sort(np.random.default_rng(20261016).choice(n, 1000, replace=False))
    want = relative(*oracle_answers(batch, crafts, at), *body_states(osol, earth, at))
    assert_same((y[:, :, crafts], inside[:, crafts]), want, "full width")
    shuffled = np.random.default_rng(3).permutation(m)       # the binary-search path, multi-pass as well
    y2, in2 = batch.eval(at[shuffled], reference_body=earth, raw=True)
    assert np.array_equal(in2, inside[shuffled]) and np.array_equal(bits(y2), bits(y[shuffled]))


def test_cpp_example_prints_the_python_calls_bits(gpu, tmp_path):
    """examples/craft_eval.cpp (SpacecraftBatch::state_vectors_at of include/ephemeris_amd.hpp) builds against the library alone, runs,
    and prints the values SpacecraftBatch.eval returns for the same batch"""
    libdir = ROOT / "ephemeris_explorer_amd"
    exe = tmp_path / "craft_eval"
    subprocess.check_call(["g++", "-std=c++17", "-Wall", "-Wextra", "-pedantic", "-Werror", f"-I{ROOT / 'include'}",
                           str(ROOT / "examples" / "craft_eval.cpp"), f"-L{libdir}", "-lephemeris_amd", f"-Wl,-rpath,{libdir}", "-o", str(exe)])
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, (r.stdout, r.stderr)
    mu = [132712440041.27942, 398600.43550702266, 4902.80011845755]
    y = [[130800.7436285839, 344339.3116943656, 136496.914202216], [-27204249.66910069, 132940582.438431, 57641619.74238631],
         [-27017766.52877057, 133253431.1006455, 57806029.23241135]]
    dy = [[-0.007799748521575531, -0.005561934613704532, -0.00225317087714714], [-29.75359910616436, -5.189518219844614, -2.251561710555783],
          [-30.64009897505477, -4.820684674596127, -2.032529075882219]]
    t0, dt, day = -252460800.0, 21600.0, 86400.0
    sol = gpu.NBodyPropagator(y, dy, mu, t0, dt, gpu.FORWARD, [12, 3, 1], [6, 7, 6]).propagate(t0 + 40.0 * day)
    eph = gpu.Ephemeris(sol, mu)
    pos = np.array([[-27204249.668775786 + 10.0 * i, 132947582.43848978, 57641619.74241204] for i in range(3)])
    vel = np.array([[-22.207539106181895, -5.189518219791726, -2.2515617105336263]] * 3)
    batch = gpu.SpacecraftBatch(eph, t0, pos, vel, "Verner87", gpu.AdaptiveParams.default(1e-3))
    batch.propagate(t0 + 2.0 * day)
    at = np.array([t0 - 1.0, t0, t0 + 0.5 * day, t0 + 1.25 * day, t0 + 3.0 * day])
    lines = r.stdout.splitlines()
    shared = [ln.split() for ln in lines if ln.startswith("ref ")]
    assert len(shared) == 3 * len(at) * 3
    seen_inside = set()
    for reference in (-1, 1, 2):
        p, v, inside = batch.eval(at, reference_body=reference)
        for f in (f for f in shared if int(f[1]) == reference):
            e, c = int(f[3]), int(f[5])
            assert f[6] == f"inside={int(inside[e, c])}"
            seen_inside.add(f[6])
            printed = np.array([float.fromhex(x) for x in f[7:13]])
            assert np.array_equal(bits(printed), bits(np.concatenate([p[e, c], v[e, c]]))), (reference, e, c)
    assert seen_inside == {"inside=0", "inside=1"}
    own = [ln.split() for ln in lines if ln.startswith("own ")]
    assert len(own) == 3
    last = np.array([batch.knots(c)[0][-1] for c in range(3)])
    p, v, inside = batch.eval(np.tile(last, (1, 1)), reference_body=1)
    for f in own:
        c = int(f[2])
        assert float.fromhex(f[4]) == last[c] and f[5] == "inside=1" and inside[0, c]
        printed = np.array([float.fromhex(x) for x in f[6:12]])
        assert np.array_equal(bits(printed), bits(np.concatenate([p[0, c], v[0, c]])))
