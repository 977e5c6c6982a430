"""What the opt-in fast paths of the massive-body step (csrc/fast.hip) compute, restated in numpy. TEST INFRASTRUCTURE ONLY.

EPH_PATH_FAST promises, for the partition (S, slice_len) the library reports (hooks.fast_partition),
    a_i = ((p_0 + p_1) + ... + p_{S-1}),   p_s = ((0 + c(i, j0)) + c(i, j0 + 1)) + ...   (j over slice s, j != i, j < n)
with c(i, j) the reference's point-mass term of p_j - p_i in the selected evaluation order: IEEE add, multiply, divide and square
root only, so `sliced_gravity` below has the same bits. It is the third restatement (oracle/eph_oracle.c gravity_eval_sliced and
oracle/pyoracle.py gravity_sliced are the other two; tests/test_fast_restatement.py holds the three together).

EPH_PATH_FAST_RSQ and EPH_PATH_F32_PAIRS promise no bits. `exact_sums` gives what they approximate in np.longdouble, and
sum_j |c_ij| per body and component: the scale of a bound counted from their operations (tests/test_gpu_fast_reference.py)."""
import numpy as np

U64 = 2.0 ** -53
U32 = 2.0 ** -24


def same_bits(a, b):
    a, b = np.ascontiguousarray(a, np.float64), np.ascontiguousarray(b, np.float64)
    return a.shape == b.shape and np.array_equal(a.view(np.uint64), b.view(np.uint64))


def point_mass_term(dx, dy, dz, mu, variant):
    """(cx, cy, cz): the term of a mass mu seen along (dx, dy, dz) in evaluation order `variant` (eph_oracle.c point_mass_term);
    arrays of binary64, every operation a correctly rounded numpy ufunc"""
    n2 = dx * dx + dy * dy + dz * dz
    if variant == 4:
        p = n2 * np.sqrt(n2)
        return (dx * mu) / p, (dy * mu) / p, (dz * mu) / p
    if variant == 6:
        p = n2 * np.sqrt(n2)
        return (dx / p) * mu, (dy / p) * mu, (dz / p) * mu
    if variant == 5:
        s = mu / (n2 * np.sqrt(n2))
    elif variant == 1:
        r = np.sqrt(n2)
        s = mu * (1.0 / (r * r * r))
    elif variant == 2:
        r = 1.0 / np.sqrt(n2)
        s = mu * (r * r * r)
    elif variant == 3:
        s = mu * ((1.0 / n2) * (1.0 / np.sqrt(n2)))
    elif variant == 0:
        s = mu * (1.0 / (n2 * np.sqrt(n2)))
    else:
        raise ValueError(variant)
    return dx * s, dy * s, dz * s


def sliced_gravity(pos, mu, S, slice_len, variant=0):
    """[n, 3] accelerations in EPH_PATH_FAST's order: vectorised over the targets, the sources one after the other"""
    pos = np.ascontiguousarray(pos, np.float64)
    mu = np.ascontiguousarray(mu, np.float64)
    n = len(mu)
    x, y, z = pos[:, 0].copy(), pos[:, 1].copy(), pos[:, 2].copy()
    idx = np.arange(n)
    total = None
    with np.errstate(all="ignore"):
        for s in range(S):
            part = [np.zeros(n), np.zeros(n), np.zeros(n)]
            for j in range(s * slice_len, min((s + 1) * slice_len, n)):
                c = point_mass_term(x[j] - x, y[j] - y, z[j] - z, mu[j], variant)
                own = idx == j                          # the body itself is not a source (its term is NaN)
                for k in range(3):
                    part[k] = np.where(own, part[k], part[k] + c[k])
            total = part if total is None else [t + p for t, p in zip(total, part)]
    return np.stack(total, axis=1)


def ordered_pair(pos, mu, variant=0):
    """a two-body system's accelerations from the numpy term (each body has one source: no summation order to speak of)"""
    pos = np.ascontiguousarray(pos, np.float64)
    assert pos.shape == (2, 3)
    return sliced_gravity(pos, mu, 1, 2, variant)


def exact_terms(pos, mu):
    """c[i, j, :] in np.longdouble: mu_j (p_j - p_i) / |p_j - p_i|^3 of the given (binary64 or binary32) inputs, 0 on the diagonal"""
    p = np.asarray(pos).astype(np.longdouble)
    m = np.asarray(mu).astype(np.longdouble)
    d = p[None, :, :] - p[:, None, :]
    n2 = (d * d).sum(axis=2)
    np.fill_diagonal(n2, 1.0)
    c = d * (m[None, :] / (n2 * np.sqrt(n2)))[:, :, None]
    i = np.arange(len(m))
    c[i, i, :] = 0.0
    return c


def exact_sums(pos, mu):
    """(a_ref[n, 3], absum[n, 3], c[n, n, 3]) in np.longdouble: sum_j c_ij, sum_j |c_ij| and the terms themselves"""
    c = exact_terms(pos, mu)
    return c.sum(axis=1), np.abs(c).sum(axis=1), c


def sensitivity_margin(c, bound):
    """min over the pairs i != j of |c_ij[k]| / bound[i, k], k the largest component of c_ij: above 1, no single source can be
    dropped, doubled or replaced by a zero row without the body leaving its bound"""
    n = c.shape[0]
    a = np.abs(c)
    k = a.argmax(axis=2)
    big = np.take_along_axis(a, k[:, :, None], axis=2)[:, :, 0]
    b = np.take_along_axis(np.broadcast_to(bound[:, None, :], a.shape), k[:, :, None], axis=2)[:, :, 0]
    ratio = big / b
    ratio[np.arange(n), np.arange(n)] = np.inf
    return float(ratio.min())


def f32_emulation(pos, mu, S, slice_len, group=32):
    """EPH_PATH_F32_PAIRS' loop (csrc/fast.hip f32_slice) in numpy binary32 with the fused multiply-adds emulated in binary64 (a
    binary32 product is exact in binary64; the one rounding of sum-then-narrow differs from a true fma only by double rounding):
    NOT a bit-level restatement -- v_rsq_f32 is replaced by a correctly rounded 1/sqrt -- but the same operation count, to see on the
    CPU where the derived bound of the GPU test sits."""
    f = np.float32
    p32, m32 = np.asarray(pos).astype(f), np.asarray(mu).astype(f)
    n = len(m32)
    npad = (n + 63) // 64 * 64
    px = np.zeros((npad, 3), f)
    px[:n] = p32
    pm = np.zeros(npad, f)
    pm[:n] = m32
    fma = lambda a, b, c: (a.astype(np.float64) * b.astype(np.float64) + c.astype(np.float64)).astype(f)
    out = np.zeros((n, 3))
    with np.errstate(all="ignore"):
        for s in range(S):
            j0, j1 = s * slice_len, min((s + 1) * slice_len, npad)
            part = np.zeros((n, 3))
            for g0 in range(j0, j1, group):
                acc = [[np.zeros(n, f) for _ in range(3)] for _ in range(2)]
                for j in range(g0, g0 + group):
                    d = [px[j, k] - p32[:, k] for k in range(3)]
                    n2 = fma(d[2], d[2], fma(d[1], d[1], d[0] * d[0]))
                    yv = (1.0 / np.sqrt(n2.astype(np.float64))).astype(f)
                    sc = ((pm[j] * yv) * yv) * yv
                    sc = np.where(np.isnan(sc), f(0), np.clip(sc, f(0), f(3.0e38)))
                    h = acc[(j - g0) & 1]
                    for k in range(3):
                        h[k] = fma(d[k], sc, h[k])
                for k in range(3):
                    part[:, k] = part[:, k] + (acc[0][k] + acc[1][k]).astype(np.float64)
            out = out + part if s else part
    return out


def jittered_lattice(n, seed=5):
    """(pos, vel, mu) for EPH_PATH_F32_PAIRS: equal masses 1 / n on a cubic lattice of spacing 0.2, every coordinate moved by up to
    0.05, the bodies in shuffled order, at rest. Every pair is 0.1 to a few units apart: no term is small against the sum of the
    others' magnitudes (plummer's distant light bodies are, at binary32's resolution)."""
    rng = np.random.default_rng(seed)
    side = int(np.ceil(n ** (1.0 / 3.0)))
    g = np.stack(np.meshgrid(*[np.arange(side)] * 3, indexing="ij"), axis=-1).reshape(-1, 3).astype(np.float64)
    g = g[rng.permutation(len(g))[:n]]
    pos = (g - (side - 1) / 2.0) * 0.2 + rng.uniform(-0.05, 0.05, (n, 3))
    return pos, np.zeros((n, 3)), np.full(n, 1.0 / n)
