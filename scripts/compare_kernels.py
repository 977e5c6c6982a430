#!/usr/bin/env python3
"""Is the device code of two builds the same code? For every kernel (`.amdhsa_kernel` symbol) of two gfx950 assembly files, or of
every compiled-once .hip unit (or chosen per-order units) of two source trees, compares the kernel descriptor block and the instruction text between the
symbol's label and its `.Lfunc_end`, with `;` comments dropped and the function index in `.LBB<n>_` labels normalised (it changes
when a kernel changes file; nothing else should). For a refactor that moves kernels between units or code between functions.

    compare_kernels.py [-v] A.s B.s
    compare_kernels.py [-v] TREE_A TREE_B   # compiles SOURCES + HOOKS_SOURCES (*.hip) of each tree's build.py with its FLAGS
    compare_kernels.py [-v] --pair step_wg.hip [--pair ...] TREE_A TREE_B
                                            # instead: these per-order units (PAIR_SOURCES + PAIR_HOOKS_SOURCES; a tree whose
                                            # build.py has no PAIR_HOOKS_SOURCES has none of the latter), once per evaluation
                                            # order (-DEPH_PAIR_VARIANT=k, k < N_PAIR_VARIANTS); `--pair all`: every such unit.
                                            # A unit named with --pair that one tree does not have counts as empty there

Three verdicts per kernel:
    same       descriptor block and instruction text identical
    reordered  descriptor block (VGPRs, SGPRs, scratch, LDS) identical, and every floating-point arithmetic opcode (v_*_f64, v_*_f32
               other than compares and v_cndmask) and every global_load_* / global_store_* occurs equally often, the _e32 / _e64
               encoding suffix dropped; integer and address arithmetic, compares, moves, mask operations, waits, branches and labels
               may differ: the same arithmetic on the same memory traffic in the same registers, scheduled or addressed differently
    DIFF       anything else
-v prints, for every kernel that is not `same`, the descriptor lines and the opcode counts that differ.

Exit status 0: the same kernel names on both sides, every one `same` or `reordered`. No GPU needed."""
import re
from collections import Counter
import runpy
import subprocess
import sys
import tempfile
from concurrent.futures import ThreadPoolExecutor
from pathlib import Path


def normalise(lines):
    out = []
    for ln in lines:
        ln = re.sub(r"\.LBB\d+_", ".LBB_", ln.split(";", 1)[0]).strip()
        if ln:
            out.append(ln)
    return out


def kernels(path):
    """{kernel symbol: (normalised descriptor block, normalised instruction text)} of one assembly file"""
    lines = Path(path).read_text().split("\n")
    desc, at = {}, {}
    for i, ln in enumerate(lines):                          # `symbol:` at the start of a line, a comment may follow
        m = re.match(r"([A-Za-z_$][\w$.]*):", ln)
        if m:
            at.setdefault(m.group(1), i)
    for i, ln in enumerate(lines):
        m = re.match(r"\s*\.amdhsa_kernel\s+(\S+)", ln)
        if m:
            end = next(j for j in range(i, len(lines)) if lines[j].strip() == ".end_amdhsa_kernel")
            desc[m.group(1)] = normalise(lines[i:end + 1])
    out = {}
    for name, d in desc.items():
        end = next(j for j in range(at[name], len(lines)) if re.match(r"\.Lfunc_end\d+:", lines[j]))
        regs = [ln for ln in lines if re.match(rf"\s*\.set\s+{re.escape(name)}\.", ln)]      # the resource usage the descriptor refers to
        out[name] = (d + normalise(regs), normalise(lines[at[name] + 1:end]))
    return out


def opcodes(text):
    """opcode -> count over a kernel's normalised instruction text, the encoding suffix dropped"""
    return Counter(re.sub(r"_e(32|64)$", "", ln.split()[0]) for ln in text if not ln.endswith(":") and not ln.startswith("."))


def pinned(op):
    """the opcodes whose counts `reordered` holds equal: floating-point arithmetic and global memory traffic"""
    if op.startswith(("global_load_", "global_store_")):
        return True
    return op.startswith("v_") and bool(re.search(r"_f(32|64)(_|$)", op)) and not op.startswith(("v_cmp", "v_cndmask"))


def verdict(a, b):
    """a, b: (descriptor, text) of one kernel in the two builds"""
    if a == b:
        return "same"
    ca, cb = opcodes(a[1]), opcodes(b[1])
    if a[0] == b[0] and all(ca[op] == cb[op] for op in set(ca) | set(cb) if pinned(op)):
        return "reordered"
    return "DIFF"


def explain(a, b):
    for x, y in zip(a[0], b[0]):
        if x != y:
            print(f"        {x}  ->  {y}")
    ca, cb = opcodes(a[1]), opcodes(b[1])
    for op in sorted(set(ca) | set(cb)):
        if ca[op] != cb[op]:
            print(f"        {'*' if pinned(op) else ' '} {op:<28} {ca[op]:>5} -> {cb[op]:<5}")


def pair_units(tree):
    """the per-order units of a source tree"""
    b = runpy.run_path(str(Path(tree) / "ephemeris_explorer_amd" / "build.py"), run_name="build")
    return b["PAIR_SOURCES"] + b.get("PAIR_HOOKS_SOURCES", [])


def tree_kernels(tree, tmp, pair=()):
    """{kernel symbol: (unit, descriptor, text)} of the compiled-once .hip units of a source tree, or, with `pair`, of those
    per-order units in every evaluation order (their kernels live in one namespace per order, so the symbols stay apart)"""
    b = runpy.run_path(str(Path(tree) / "ephemeris_explorer_amd" / "build.py"), run_name="build")
    if pair:
        srcs = [s for s in pair_units(tree) if "all" in pair or s in pair]
        jobs = [(s, k) for s in srcs for k in range(b["N_PAIR_VARIANTS"])]
    else:
        jobs = [(s, None) for s in b["SOURCES"] + b["HOOKS_SOURCES"] if s.endswith(".hip")]

    def one(job):
        src, k = job
        unit = src if k is None else f"{src} pv{k}"
        out = Path(tmp) / (unit.replace(".hip", "").replace(" ", ".") + ".s")
        order = [] if k is None else [f"-DEPH_PAIR_VARIANT={k}"]
        subprocess.run([b["hipcc"](), *b["FLAGS"], *order, *b.get("SOURCE_FLAGS", {}).get(src, []), "--offload-device-only", "-S", "-x", "hip",
                        str(b["CSRC"] / src), "-o", str(out)],
                       check=True, stderr=subprocess.DEVNULL)
        return {name: (unit, *v) for name, v in kernels(out).items()}
    found = {}
    with ThreadPoolExecutor(8) as ex:
        for part in ex.map(one, jobs):
            assert not (set(part) & set(found)), "a kernel defined in two units"
            found.update(part)
    return found


def demangle(names):
    out = subprocess.run(["c++filt"], input="\n".join(names), capture_output=True, text=True).stdout.split("\n")
    return {n: re.sub(r"\(.*", "", d).replace("void ", "") for n, d in zip(names, out)}


def main(a, b, verbose=False, pair=()):
    if Path(a).is_dir():
        known = set(pair_units(a)) | set(pair_units(b)) | {"all"}
        assert set(pair) <= known, f"--pair takes per-order units of either tree: {sorted(known)}"
        with tempfile.TemporaryDirectory() as ta, tempfile.TemporaryDirectory() as tb:
            ka, kb = tree_kernels(a, ta, pair), tree_kernels(b, tb, pair)
    else:
        ka, kb = ({k: (Path(p).name, *v) for k, v in kernels(p).items()} for p in (a, b))
    short = demangle(sorted(set(ka) | set(kb)))
    bad = moved = reordered = 0
    for k in sorted(set(ka) | set(kb), key=lambda k: short[k]):
        if k not in ka or k not in kb:
            print(f"ONLY IN {'A' if k in ka else 'B'}  {short[k]}  ({(ka.get(k) or kb.get(k))[0]})")
            bad += 1
            continue
        v = verdict(ka[k][1:], kb[k][1:])
        bad += v == "DIFF"
        reordered += v == "reordered"
        moved += ka[k][0] != kb[k][0]
        print(f"{v:<9}  {short[k]:<44} {len(ka[k][2]):>6} -> {len(kb[k][2]):<6} lines  {ka[k][0]} -> {kb[k][0]}")
        if verbose and v != "same":
            explain(ka[k][1:], kb[k][1:])
    print(f"{len(set(ka) | set(kb))} kernels, {moved} in another unit, {reordered} reordered, {bad} different or missing")
    return 1 if bad else 0


if __name__ == "__main__":
    args, pair = [x for x in sys.argv[1:] if x != "-v"], []
    while "--pair" in args[:-1]:
        i = args.index("--pair")
        pair.append(args[i + 1])
        del args[i:i + 2]
    if len(args) != 2:
        sys.exit(__doc__)
    sys.exit(main(args[0], args[1], verbose="-v" in sys.argv[1:], pair=pair))
