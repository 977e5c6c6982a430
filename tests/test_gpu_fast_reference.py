"""-m gpu: the three opt-in paths of the massive-body step (csrc/fast.hip) against a reference of the operation each one actually
performs. tests/test_gpu_fast.py pins determinism and closeness to the ORDERED path, scaled by the largest acceleration of the
system; a source dropped or doubled, a padding row leaking into one body, a wrong diagonal mask or slices combined in another order
pass there. Here:

EPH_PATH_FAST (4) promises bits (fast.hip's header): a_i = ((p_0 + p_1) + ... + p_{S-1}), p_s the in-order chain of the reference's
pair terms over slice s, the rest of the step being the ordered path's Cowell and predictor arithmetic. Held bit for bit, signs of
zeros included, to the oracle with orc_set_gravity_slices (state, velocity, acceleration) and to the numpy restatement evaluated at
the position the device returns (tests/fast_restatement.py; tests/test_fast_restatement.py holds the restatements together on the
CPU), with the partition (S, slice_len) the library reports for the process (eph_debug_fast_partition) -- the tests do not restate
the partition policy.

EPH_PATH_FAST_RSQ (5) and EPH_PATH_F32_PAIRS (6) promise no bits. Per body and component,
    |a_gpu - a_ref| <= K u sum_j |c_ij|
against np.longdouble sums of the exact terms of the returned positions (path 6: of their binary32 roundings). K counts the
first-order roundings of the kernels' own operations, at their worst; it is DERIVED, not measured:

  path 5, fast_slice_rsq, u = 2^-53. One term dx * sc, sc = (mu y)(y y):
    d = p_j - p_i                         1 rounding each                                             d:   1 u
    n2 = fma(dz, dz, fma(dy, dy, dx dx))  every d_c^2 carries 2 u, the convex sum keeps 2 u; + 3 roundings   n2:  5 u
    y0 = v_rsq_f64(n2), e = fma(-(n2 y0), y0, 1), c = fma(e, 3/8, 1/2) e, y = fma(y0, c, y0):
        the third-order correction leaves 5/16 e^3 ~ 2^-68 of the seed's 2^-23 (nothing); n2 y0 rounds once -> e off by u absolute,
        c by u / 2, y by u / 2 + its own rounding = 1.5 u; n2's 5 u arrive halved                     y:   4 u
    sc = (mu y)(y y)                      three y (12 u) + three multiplications                      sc: 15 u
    dx sc                                 + d's 1 u (the fma's rounding belongs to the chain)         term: 16 u -> K_term = 20
    the chain over a slice: at most slice_len roundings, each of a partial sum that sum|c| bounds; S more for the slices combined:
    K = 20 + slice_len + S
  path 6, f32_slice, u32 = 2^-24, inputs already binary32. One term dx * sc, sc = ((mu y) y) y:
    d: 1 u32; n2 (product, two fma): 5 u32; y = v_rsq_f32(n2), documented 1 ulp = 2 u32, + n2's halved 2.5 = 4.5 u32;
    sc: 3 * 4.5 + 3 multiplications = 16.5 u32; dx sc: 17.5 u32 -> K32_term = 20
    16 packed fma per half of a 32-source group accumulate in binary32 (16), the halves are added once (1); the binary64 chain behind
    them is 2^-29 of that:  K32 = 20 + 16 + 1 = 37
Such bounds are loose by design (88 to 172 u, 37 u32; a correct kernel sits at a few u). What makes them tests is the SENSITIVITY
condition, asserted on the reference before every comparison: for every target, the largest component of EVERY single term c_ij is
more than 8 bounds of that component, so a source dropped, doubled, mis-masked or replaced by a padding row cannot pass. plummer(n)
has it on path 5 (margins of 1e7); at binary32's resolution path 6 needs bodies no farther than a few units from one another:
equal masses on a jittered lattice (fast_restatement.jittered_lattice), no two coinciding in binary32 (asserted).

Sizes: the smallest at which each mechanism exists. 65: two blocks of targets, 63 of them padding, 4-source slices of which half are
empty, the diagonal and the padded slice in one wave; 127, 128, 129: the tile edge; 130; 705: 12-source slices, the last ragged
against n; 1100: 20-source slices; 2200: the first size class whose default slice count is below 64 (60, not a power of two). The
forms are chosen by environment variables read once per process: every form is a child process (tests/fast_reference_child.py), which
compares with the CPU itself and stops at its first failure; once a child has failed, hung or been killed, no test of this file
starts another."""
import os
import subprocess
import sys

import pytest

from conftest import ROOT

pytestmark = pytest.mark.gpu
CHILD = ROOT / "tests" / "fast_reference_child.py"
FORM_VARIABLES = ("EPH_FAST_SLICES", "EPH_FAST_UNROLL", "EPH_FAST_FUSED", "EPH_PAIR_VARIANT")


_failed = []            # the first child of this module that failed, hung or was killed: no later test starts another on the card


def child(batteries, timeout=240, **form):
    """one process per form; -> its `soak` lines"""
    assert not _failed, f"not started: an earlier child of this file failed ({_failed[0]})"
    env = {k: v for k, v in os.environ.items() if k not in FORM_VARIABLES}
    env.update({k: str(v) for k, v in form.items()})
    _failed.append(f"{' '.join(batteries)} {form}")          # (a timeout raises out of subprocess.run: it stays marked)
    r = subprocess.run([sys.executable, str(CHILD), *batteries], env=env, capture_output=True, text=True, timeout=timeout)
    print(f"--- {' '.join(batteries)} {form}")
    print(r.stdout, end="")                                  # (partitions, max ratios, digests: pytest -s shows them)
    assert r.returncode == 0 and r.stdout.strip().endswith("ok"), (form, r.stdout[-1500:], r.stderr[-3000:])
    _failed.clear()
    return [line for line in r.stdout.splitlines() if line.startswith("soak ")]


def test_path4_bit_for_bit_at_every_size_and_both_methods(gpu):
    """(a) n = 65, 127, 128, 129, 130, 705, 1100 (and 2200), QuinlanTremaine12 and Stormer13, default forms: after L + 1, L + 2 and
    L + 9 steps the acceleration is the slice-order sum of the returned position, state and acceleration are the oracle's"""
    child(["sizes_and_methods"])


def test_path4_every_evaluation_order_and_the_ieee_fall_back(gpu):
    """(a) orders 0-6 at n = 130 and 705; (c) at n = 130 and every order, operands outside the guarded ranges of pair_finish<true>,
    where fast_slice's ballot over range_key / mu_key / low_key must send the wave through the IEEE form: a light body 2^151 and 2^70
    away, a massless body with one of mu = 2^-210, a planar system -- signs of zeros included"""
    child(["orders", "exceptional"])


def test_path4_solout_clone_and_path_changes(gpu):
    """(b) n = 130: a propagator's splines over 60 steps (info, trimmed lengths, every coefficient), a clone taken five steady steps
    in, one handle through paths 0 -> 4 -> 0 -> 4 -- all against the oracle with the slices toggled the same way; (d) at the default
    forms (path 5 in two launches, path 6 in one)"""
    child(["solout_clone_paths", "bounds"])


def test_forced_slices_10_round_to_12(gpu):
    """EPH_FAST_SLICES=10: a slice count that is rounded (to 12) and is no power of two, three workgroups per block"""
    child(["forced_form"], EPH_FAST_SLICES=10)


@pytest.mark.parametrize("slices, unroll", [(8, 4), (64, 8)])
def test_forced_forms_and_the_soak_of_the_one_launch_hand_off(gpu, slices, unroll):
    """EPH_FAST_SLICES = 8 and 64 (2 and 16 workgroups per block of targets), the second with EPH_FAST_UNROLL=8, each in two launches
    (EPH_FAST_FUSED=0) and in one (1): (a) path 4 bit for bit at 65, 130, 705; (d) paths 5 and 6 inside their derived bounds at 65,
    130, 705 (1100 on path 5); (e) ADVICE round 6: 4000 steady steps of every path at n = 65 and 705, a digest of state and
    accelerations every 1000 -- identical between the one-launch form (k_fast_step: relaxed agent-scope ticket, no fence) and the
    two-launch form, between two runs of each, and for path 4 at n = 65 equal to the oracle after the first 1000. A determinism check
    where every block's ticket sees 2 or 16 arrivals per step; a difference or a hang is a finding to explain from the code."""
    digests = {}
    for fused in (0, 1):
        digests[fused] = child(["forced_form", "bounds", "soak"], EPH_FAST_SLICES=slices, EPH_FAST_UNROLL=unroll, EPH_FAST_FUSED=fused)
        assert len(digests[fused]) == 6                      # n = 65, 705 x paths 4, 5, 6
    assert digests[0] == digests[1]
