"""-m gpu: k_lm_small (csrc/step_small.hip on the frame of csrc/small_frame.h) in all eight forms of an evaluation order -- L = 12 | 13, one
system | a gang, eight waves | four -- at the body counts where its thread roles change, against the C oracle, bit pattern against bit
pattern (the scenes and what each is planted for: tests/gang_scenes.py; that they still reach their edges: tests/test_gang_scenes.py).

    form                        launched by
    <L, false>                  every start of a handle alone (the desynchronising advances of every test here)
    <L, true>                   test_gang_of_every_edge_size, test_gang_was_one_launch, test_sampled_gang_edges[as-created]
    <L, true, true>             test_four_wave_gang_above_the_cu_count, test_sampled_gang_edges[padded], the first child of
                                test_forced_forms_in_a_child (a gang of 16)
    <L, false, true>            the first child of test_forced_forms_in_a_child (EPH_SMALL_FORM=4)
    <L, true> above the CUs     the second child of test_forced_forms_in_a_child (EPH_SMALL_FORM=8)

advance_many / step_n_many fall back to separate advances without a word, and the results are the same bits by design:
test_gang_was_one_launch watches a member that is not the lead in each kind of gang the other tests build (started members, clones
above the CU count, sampled propagators and their clones), so a gang that was not ONE launch fails there, and only there.
profiles/gang_edges.md: wall times, and the one-line changes to the kernel these tests were run against."""
import os
import subprocess
import sys

import pytest

import gang_scenes as gs
from conftest import ROOT
from oracle import orc

pytestmark = pytest.mark.gpu

SIGNS = {"forward": 1, "backward": -1}


@pytest.fixture(scope="module")
def oracle(gpu):
    """the oracle's runs, shared by the tests of this module, in the evaluation order the device uses"""
    orc.set_pair_variant(gpu.pair_variant())
    yield gs.Oracle()
    orc.set_pair_variant(0)


@pytest.fixture(scope="module")
def cus(gpu):
    """the CU count, read the way lm_small_many reads it: hipDeviceGetAttribute(hipDeviceAttributeMultiprocessorCount) of the
    current device, through the HIP runtime the library itself is bound to (what torch reports as multi_processor_count)"""
    import ctypes as C
    hip, dev, count = gpu.hip_runtime(), C.c_int(-1), C.c_int(0)
    MULTIPROCESSOR_COUNT = 63                              # hipDeviceAttributeMultiprocessorCount (hip_runtime_api.h)
    assert hip.hipGetDevice(C.byref(dev)) == 0 and hip.hipDeviceGetAttribute(C.byref(count), MULTIPROCESSOR_COUNT, dev) == 0
    assert 64 <= count.value <= 512, count.value           # (an MI355X has 256)
    return count.value


def sources(gpu):
    """every started member of the padded gangs: the edge sizes with both step signs, the two far-pair scenes"""
    return gs.edge_members(1) + gs.edge_members(-1) + gs.far_members(gs.range_exponent(gpu.pair_variant()))


@pytest.mark.parametrize("sign", list(SIGNS))
@pytest.mark.parametrize("method", list(gs.METHODS))
def test_gang_of_every_edge_size(gpu, oracle, method, sign):
    """one member per size of gs.SIZES in one gang (at most the CU count: the eight-wave gang form <L, true>), member i advanced
    alone by i % L steps first, then advance_many with k = 1, 5, L, L + 1, 2 L + 5: positions, velocities, time, step count and
    acc() of every member after every call are its own oracle's"""
    members = gs.edge_members(SIGNS[sign])
    _, got = gs.run_gang(members, method, gpu.NBodyIntegration, gpu.advance_many)
    gs.compare_gang(members, got, gs.expected_gang(members, method, oracle), f"gang of the edge sizes, {method}, {sign}")


def test_gang_was_one_launch(gpu, oracle, cus):
    """This pins TODAY'S observable of the existing ABI (gang_scenes.LaunchProbe; nothing is exported for it): in a gang a member that
    is not the lead and has timing on counts one launch and keeps its milliseconds EXACTLY, the lead's milliseconds are the shared
    launch's; in a gang made to fall back by a member that does not qualify (33 bodies) the same member times its own launch.
    Then the kinds of gang the other tests of this file build, which would pass on separate advances too: clones above the CU
    count, sampled propagators padded with clones -- a started member, a clone and the last handle were members of one launch in
    every call"""
    method, L = "QuinlanTremaine12", 12
    members = gs.edge_members(1)
    handles = [m.make(gpu.NBodyIntegration, method) for m in members]
    for i, h in enumerate(handles):
        h.advance(L + gs.desync_steps(i, L))
    lead, probe = gs.LaunchProbe(handles[0]), gs.LaunchProbe(handles[9])
    assert (probe.ms, probe.launches) == (0.0, 0)
    gpu.advance_many(handles, 7)
    assert probe.after_call() == (0.0, 1)
    lead_ms, lead_launches = lead.after_call()
    assert lead_ms > 0.0 and lead_launches == 1
    big = gs.Member("n33", *gs.random_system(33), gs.H).make(gpu.NBodyIntegration, method)
    big.advance(L)
    gpu.advance_many(handles + [big], 7)
    ms, launches = probe.after_call()
    assert ms > 0.0 and launches == 1                      # its own launch, timed by itself: the gang fell back
    assert big.state()[3] == L + 7
    for i, (m, h) in enumerate(zip(members, handles)):     # both calls did what they say
        assert gs.same_record(gs.integration_record(h), oracle.record(m, method, L + gs.desync_steps(i, L) + 14)) is None, m.name
    total = cus + 8
    gs.run_padded(members, method, total, gpu.NBodyIntegration, gpu.advance_many, probes=(1, len(members), total - 1))
    sampled = gs.sampled_members()
    gs.run_sampled(sampled, "Stormer13", gpu.NBodyPropagator, gpu.step_n_many, pad_to=total, probes=(1, len(sampled), total - 1))


@pytest.mark.parametrize("method", list(gs.METHODS))
def test_four_wave_gang_above_the_cu_count(gpu, oracle, cus, method):
    """CUs + 8 handles in one launch: lm_small_many takes the four-wave form <L, true, true> (two unordered pairs per thread). The
    30 sources (every edge size with both step signs, both far-pair scenes) and clones of them advanced alone by 1, 2 or 3 steps:
    handles entered in the same state are equal bit for bit, and every handle is its oracle's after every call"""
    members, total = sources(gpu), cus + 8
    assert total >= 7 * len(members)                       # (every clone's entry state occurs at least twice)
    plan, got = gs.run_padded(members, method, total, gpu.NBodyIntegration, gpu.advance_many)
    gs.compare_padded(members, method, plan, got, oracle, f"gang of {total} > {cus} CUs, {method}")


@pytest.mark.parametrize("gang", ["as-created", "padded"])
@pytest.mark.parametrize("method", list(gs.METHODS))
def test_sampled_gang_edges(gpu, oracle, cus, method, gang):
    """step_n_many on propagators of 1, 3, 17, 24 and 32 bodies, forward and backward, counts [1, 2, 3, 7, 12] and degrees 2 .. 7 by
    body, each stepped alone by another count first: info, ncoef and coefficients of every body, time() and the state are
    orc.Propagator's. As created: ten workgroups, the eight-wave gang form; padded with clones of the 3-body propagator to
    CUs + 8: the four-wave form with sampling"""
    members, L = gs.sampled_members(), gs.METHODS[method]
    want, _ = gs.run_sampled(members, method, orc.Propagator)
    total = cus + 8 if gang == "padded" else 0
    got, clones = gs.run_sampled(members, method, gpu.NBodyPropagator, gpu.step_n_many, pad_to=total)
    gs.compare_sampled(members, got, want, f"sampled gang, {method}, {gang}")
    if clones:
        src = members[gs.PAD_SOURCE]
        alone = []
        for extra in (1, 2):                               # clones 1 and 2 (4 and 5) went 1 and 2 steps further alone
            o = src.make(orc.Propagator, method)
            assert o.step_n(src.entry_steps(L) + extra + sum(gs.SAMPLED_CALLS)) == 0
            alone.append(gs.sampled_record(o, src.n))
        expect = [want[gs.PAD_SOURCE], alone[0], alone[1]] * 2
        gs.compare_sampled([src] * 6, clones, expect, f"sampled gang, {method}, {gang}: clones of {src.name}")


CHILD = r'''
import sys
root, tests, form, cus, pair = sys.argv[1:6]
sys.path[:0] = [root, tests]
import ephemeris_explorer_amd as ea
import gang_scenes as gs
from oracle import orc
ea.set_pair_variant(int(pair))
orc.set_pair_variant(int(pair))
oracle = gs.Oracle()
far = gs.far_members(gs.range_exponent(int(pair)))
for method, L in gs.METHODS.items():
    if form == "4":
        for m in gs.edge_members(1) + gs.edge_members(-1) + far:          # <L, false, true>: every size alone
            g = m.make(ea.NBodyIntegration, method)
            g.advance(L + 7)
            diff = gs.same_record(gs.integration_record(g), oracle.record(m, method, L + 7))
            assert diff is None, f"four-wave form, one system, {method}: member {m.name}: {diff} differs from the oracle's"
        members = gs.edge_members(-1) + far                               # <L, true, true>: a gang of 16
        _, got = gs.run_gang(members, method, ea.NBodyIntegration, ea.advance_many)
        gs.compare_gang(members, got, gs.expected_gang(members, method, oracle), f"four-wave gang of 16, {method}")
    else:
        members, total = gs.edge_members(1) + gs.edge_members(-1) + far, int(cus) + 8
        plan, got = gs.run_padded(members, method, total, ea.NBodyIntegration, ea.advance_many)
        gs.compare_padded(members, method, plan, got, oracle, f"eight-wave gang of {total}, {method}")
print("ok")
'''


def test_forced_forms_in_a_child(gpu, cus):
    """EPH_SMALL_FORM is read once per process: a fresh child for each value, one at a time, the second only if the first passed.
    4: <L, false, true> -- every edge size with both step signs and both far-pair scenes alone, L + 7 steps -- and <L, true, true>
    on a gang of 16 (the sizes with the massless bodies, both far-pair scenes). 8: the eight-wave gang form on CUs + 8 workgroups,
    a grid that the default rule never gives it"""
    for form in ("4", "8"):
        env = dict(os.environ, EPH_SMALL_FORM=form)
        r = subprocess.run([sys.executable, "-c", CHILD, str(ROOT), str(ROOT / "tests"), form, str(cus), str(gpu.pair_variant())],
                           env=env, capture_output=True, text=True, timeout=300)
        if r.returncode != 0 or not r.stdout.strip().endswith("ok"):
            said = [line for line in r.stderr.splitlines() if line.startswith("AssertionError")]
            pytest.fail(f"{said[0] if said else f'EPH_SMALL_FORM={form}: the child ended with status {r.returncode}'}\n"
                        f"--- stdout ---\n{r.stdout[-1000:]}\n--- stderr ---\n{r.stderr[-3000:]}", pytrace=False)
