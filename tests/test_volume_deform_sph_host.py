"""CPU checks of xmipp_volume_deform_sph: the basis list and the basis functions against closed forms written here from the
mathematics, normalize_Robust against a numpy restatement of the stated readings, and the program's refusals, all before any device
is touched. The closed forms and the restatements are also what tests/test_gpu_volume_deform_sph.py compares the device against."""
import math
import os
import subprocess
from fractions import Fraction

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PROG = os.path.join(ROOT, "xmipp3_amd", "bin", "xmipp_volume_deform_sph")
XH_ERR_UNSUPPORTED = -5


@pytest.fixture(scope="module")
def xa():
    import __graft_entry__ as g
    g.build()
    assert os.path.exists(PROG)
    import xmipp3_amd
    return xmipp3_amd


# ---------------------------------------------------------------- the restatement: basis
def terms_ref(L1, L2):
    """for h = 0 .. L2, l = h, h + 2, ... <= L1, m = -h .. h: (l1 = l, n = h, l2 = h, m)"""
    return [(l, h, h, m) for h in range(L2 + 1) for l in range(h, L1 + 1, 2) for m in range(-h, h + 1)]


def radial_monomials(l, n):
    """R_l^n(r) = sqrt(2 l + 3) r^n P_k^(0, n + 1/2)(2 r^2 - 1), k = (l - n) / 2, as {power of r: coefficient / sqrt(2 l + 3)}, exact.
    P_k^(a, b)(x) = sum_s C(k + a, k - s) C(k + b, s) ((x - 1) / 2)^s ((x + 1) / 2)^(k - s), here with (x - 1) / 2 = r^2 - 1,
    (x + 1) / 2 = r^2."""
    k, b = (l - n) // 2, Fraction(2 * n + 1, 2)
    co = {}
    for s in range(k + 1):
        gb = Fraction(1)
        for i in range(s):
            gb *= (k + b - i) / Fraction(i + 1)                      # C(k + b, s), generalised
        w = math.comb(k, k - s) * gb
        for t in range(s + 1):                                       # (r^2 - 1)^s
            p = n + 2 * (t + k - s)
            co[p] = co.get(p, Fraction(0)) + w * math.comb(s, t) * (-1) ** (s - t)
    return co


def radial_ref(l, n, r):
    """(value, sum of the absolute monomials: the scale rounding errors are relative to)"""
    r = np.asarray(r, np.float64)
    v, a = np.zeros_like(r), np.zeros_like(r)
    for p, c in radial_monomials(l, n).items():
        t = float(c) * r ** p
        v, a = v + t, a + np.abs(t)
    f = math.sqrt(2 * l + 3)
    return f * v, f * a


_LEGENDRE = {  # P_l^m(c), s = sin(theta), without the Condon-Shortley phase
    (0, 0): lambda c, s: 1 + 0 * c, (1, 0): lambda c, s: c, (1, 1): lambda c, s: s,
    (2, 0): lambda c, s: (3 * c * c - 1) / 2, (2, 1): lambda c, s: 3 * c * s, (2, 2): lambda c, s: 3 * s * s,
    (3, 0): lambda c, s: (5 * c ** 3 - 3 * c) / 2, (3, 1): lambda c, s: 1.5 * (5 * c * c - 1) * s, (3, 2): lambda c, s: 15 * c * s * s,
    (3, 3): lambda c, s: 15 * s ** 3,
    (4, 0): lambda c, s: (35 * c ** 4 - 30 * c * c + 3) / 8, (4, 1): lambda c, s: 2.5 * (7 * c ** 3 - 3 * c) * s,
    (4, 2): lambda c, s: 7.5 * (7 * c * c - 1) * s * s, (4, 3): lambda c, s: 105 * c * s ** 3, (4, 4): lambda c, s: 105 * s ** 4,
}


def harmonic_ref(l, m, x, y, z):
    """the real solid harmonic rho^l Y_l^m at (x, y, z), rho their norm, from the spherical form
    Y_l^m = N P_l^|m|(cos theta) {sqrt 2 cos(m phi), 1, sqrt 2 sin(|m| phi)}, N^2 = (2 l + 1) / (4 pi) (l - |m|)! / (l + |m|)!;
    (value, scale). The one exception is (4, 0): the reference's sources, CPU and CUDA alike, evaluate the unit-sphere form
    35 z^4 - 30 z^2 + 3 at the scaled coordinates, and the library keeps that so that a coefficient file means the same field."""
    x, y, z = (np.asarray(a, np.float64) for a in (x, y, z))
    if (l, m) == (4, 0):
        k = 3.0 / 16.0 * math.sqrt(1 / math.pi)
        return k * (35 * z ** 4 - 30 * z * z + 3), k * (35 * z ** 4 + 30 * z * z + 3)
    rho = np.sqrt(x * x + y * y + z * z)
    safe = np.where(rho > 0, rho, 1.0)
    c = z / safe
    s = np.sqrt(x * x + y * y) / safe
    phi = np.arctan2(y, x)
    am = abs(m)
    N = math.sqrt((2 * l + 1) / (4 * math.pi) * math.factorial(l - am) / math.factorial(l + am))
    ang = 1.0 if m == 0 else math.sqrt(2) * (np.cos(am * phi) if m > 0 else np.sin(am * phi))
    v = N * _LEGENDRE[(l, am)](c, s) * ang * rho ** l
    if l > 0:
        v = np.where(rho > 0, v, 0.0)
    return v, math.sqrt((2 * l + 1) / (4 * math.pi)) * rho ** l


def zsh_ref(l1, n, l2, m, xr, yr, zr, r):
    R, _ = radial_ref(l1, n, r)
    Y, _ = harmonic_ref(l2, m, xr, yr, zr)
    return R * Y


# ---------------------------------------------------------------- the restatement: normalize_Robust
def partition_entropy(prob, mass):
    """base-10 entropy of the bins `prob` taken as a distribution of total mass `mass`; empty bins and an empty partition give 0"""
    if mass <= 1e-15:
        return 0.0
    q = prob[prob > 1e-15] / mass
    return -sum(t * math.log10(t) for t in q)


def normalize_robust_ref(v, clip=1.3284):
    """normalize_Robust with a zero background mask, restated from its description. The split is the maximum-entropy threshold
    (Kapur's criterion, which the reference's EntropySegmentation follows): over a 200-bin histogram, the first cut, among all but the
    last bin, at which the entropies of the two normalised partitions add up to the most. The readings of the issue: bins of
    (max - min) / 200 over [min, max], index floor((v - min) / step), the maximum in the last bin; a bin's value is min + i step;
    v <= t + 1e-6 is background; the median within a mask is the middle element of the sorted voxels (mean of the two middle ones
    for an even count); p99 = sorted[int(0.99 n)] of the foreground; (v - medianBg) / p99, clipped."""
    v = np.asarray(v, np.float64)
    flat = v.ravel()
    mn, mx = flat.min(), flat.max()
    step = (mx - mn) / 200
    idx = np.minimum(np.floor((flat - mn) / step).astype(np.int64), 199)
    prob = np.bincount(idx, minlength=200).astype(np.float64) / flat.size
    below = np.cumsum(prob)
    total = [partition_entropy(prob[:c + 1], below[c]) + partition_entropy(prob[c + 1:], 1 - below[c]) for c in range(199)]
    thr = mn + int(np.argmax(total)) * step          # argmax: the first maximum
    bgmask = flat <= thr + 1e-6
    bg, fg = np.sort(flat[bgmask]), np.sort(flat[~bgmask])
    nb = bg.size
    med = bg[nb // 2] if nb % 2 else 0.5 * (bg[nb // 2 - 1] + bg[nb // 2])
    p99 = fg[int(fg.size * 0.99)]
    out = (v - med) * (1 / p99)
    return np.clip(out, -clip, clip) if clip > 0 else out


def blobs(shape, seed, nblobs=5, noise=0.02):
    """a smooth seeded test volume: a few Gaussian blobs plus low noise"""
    rng = np.random.default_rng(seed)
    Z, Y, X = shape
    k, i, j = np.meshgrid(np.arange(Z) - Z // 2, np.arange(Y) - Y // 2, np.arange(X) - X // 2, indexing="ij")
    v = np.zeros(shape)
    for _ in range(nblobs):
        c = rng.uniform(-0.25, 0.25, 3) * np.array([Z, Y, X])
        s = rng.uniform(1.5, 3.0)
        v += rng.uniform(0.5, 1.0) * np.exp(-((k - c[0]) ** 2 + (i - c[1]) ** 2 + (j - c[2]) ** 2) / (2 * s * s))
    return v + noise * rng.standard_normal(shape)


# ---------------------------------------------------------------- tests
def test_term_count(xa):
    assert xa.vds_num_terms(3, 2) == 13
    assert xa.vds_num_terms(3, 0) == 2
    assert xa.vds_num_terms(5, 4) == len(terms_ref(5, 4)) == 45
    assert xa.vds_num_terms(2, 1) == 5


def test_term_list(xa):
    t = [tuple(r) for r in xa.vds_terms(3, 2).tolist()]
    assert t[:3] == [(0, 0, 0, 0), (2, 0, 0, 0), (1, 1, 1, -1)]
    for L1 in range(6):
        for L2 in range(5):
            assert [tuple(r) for r in xa.vds_terms(L1, L2).tolist()] == terms_ref(L1, L2)


@pytest.mark.parametrize("L1,L2", [(6, 0), (6, 2), (3, 5), (0, 5)])
def test_unsupported_degrees(xa, L1, L2):
    import ctypes as C
    n = C.c_int32()
    assert xa.lib().xh_vds_num_terms(L1, L2, C.byref(n)) == XH_ERR_UNSUPPORTED
    out = np.zeros((64, 4), np.int32)
    assert xa.lib().xh_vds_terms(L1, L2, out.ctypes.data_as(C.c_void_p)) == XH_ERR_UNSUPPORTED
    assert b"not supported" in xa.lib().xh_last_error()


def test_basis_values(xa):
    """Every supported (l1, n, l2, m) at 40 random points of the unit ball against the closed forms above, to 1e-14 relative. A
    radial polynomial has zeros inside the ball, where no evaluation keeps a bound relative to the value itself: the bound is
    relative to the term's size at the point, the sum of the absolute monomials of R times the sup of |Y_l| at that radius,
    which is what the rounding errors of either evaluation are proportional to. Where the value is at least a quarter of that size
    (no cancellation to speak of; 3507 of the 12 000 samples) the bound is also held relative to the value itself."""
    rng = np.random.default_rng(7)
    pts = rng.uniform(-1, 1, (400, 3))
    pts = pts[np.linalg.norm(pts, axis=1) < 1][:40]
    assert len(pts) == 40
    x, y, z = pts.T
    r = np.sqrt(x * x + y * y + z * z)
    checked, nwell, strict = 0, 0, 0.0
    for l1 in range(6):
        for n in range(l1 % 2, l1 + 1, 2):
            R, Ra = radial_ref(l1, n, r)
            for l2 in range(5):
                for m in range(-l2, l2 + 1):
                    Y, Ya = harmonic_ref(l2, m, x, y, z)
                    got = np.array([xa.vds_zsh(l1, n, l2, m, x[q], y[q], z[q], r[q]) for q in range(len(r))])
                    err = np.abs(got - R * Y) / (Ra * Ya)
                    assert err.max() <= 1e-14, (l1, n, l2, m, err.max())
                    well = np.abs(R * Y) >= 0.25 * Ra * Ya             # no cancellation to speak of: relative to the value itself
                    strict = max(strict, (np.abs(got - R * Y)[well] / np.abs(R * Y)[well]).max(initial=0.0))
                    nwell += int(well.sum())
                    checked += 1
    assert checked == 12 * 25
    print(f"basis values: {nwell} well-conditioned samples, largest error relative to the value {strict:.3g}")
    assert nwell > 1000 and strict <= 1e-14


def test_basis_orthogonality(xa):
    """Two different l2 = 1 terms integrate to 0 over the ball. Midpoint rule on a grid of step h = 1 / 20 that is symmetric under
    every sign flip. The product of two l2 = 1 terms of different m is odd in one coordinate, so the rule's sum cancels in pairs and
    its quadrature error is 0: what is left is rounding, n eps max|f| h^3. The terms' own size is pinned by test_basis_values (a
    cut-cell bound on the integral of a square at this step would be wider than the 5 / 7 it should confirm)."""
    h = 1.0 / 20
    c = (np.arange(-20, 20) + 0.5) * h
    z, y, x = np.meshgrid(c, c, c, indexing="ij")
    r = np.sqrt(x * x + y * y + z * z)
    inside = r < 1
    x, y, z, r = x[inside], y[inside], z[inside], r[inside]
    val = {m: np.array([xa.vds_zsh(1, 1, 1, m, x[q], y[q], z[q], r[q]) for q in range(r.size)]) for m in (-1, 0, 1)}
    fmax = 5 * 3 / (4 * math.pi)
    for a, b in ((-1, 1), (-1, 0), (0, 1)):
        assert abs(np.sum(val[a] * val[b]) * h ** 3) <= r.size * np.finfo(np.float64).eps * fmax * h ** 3
    assert all(np.sum(val[m] ** 2) * h ** 3 > 0.5 for m in (-1, 0, 1))      # the zeros above are not zeros of the terms


def test_normalize_robust(xa):
    """Pins the readings stated in normalize_robust_ref (xmippCore's compute_hist, index2val, binarize and masked median are not in
    the reference tree), not upstream."""
    v = blobs((20, 20, 20), seed=3)
    want = normalize_robust_ref(v)
    got = xa.vds_normalize_robust(v)
    assert np.abs(got - want).max() <= 1e-12
    tight = xa.vds_normalize_robust(v, clip=0.5)                # a clip that is reached
    assert np.abs(tight).max() == 0.5 and np.abs(tight - normalize_robust_ref(v, clip=0.5)).max() <= 1e-12
    unclipped = xa.vds_normalize_robust(v, clip=0)
    assert np.abs(unclipped - normalize_robust_ref(v, clip=0)).max() <= 1e-12 * np.abs(unclipped).max()
    with pytest.raises(xa.XhError, match="constant"):
        xa.vds_normalize_robust(np.full((20, 20, 20), 2.5))


def _run(args):
    return subprocess.run([PROG] + args, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=120)


def test_program_arguments(xa):
    r = _run(["-i", "a.vol"])
    assert r.returncode != 0
    assert "Parameter -r is mandatory" in r.stderr and "USAGE" in r.stderr
    for flag in ("-i", "-r", "-o", "--oroot", "--sigma", "--analyzeStrain", "--optimizeRadius", "--l1", "--l2", "--regularization", "--Rmax", "--thr"):
        assert flag in r.stderr
    for defaults in ("--oroot <=Volumes>", "--l1 <=3>", "--l2 <=2>", "--regularization <=0.00025>", "--Rmax <=-1>", "--thr <=-1>"):
        assert defaults in r.stderr
    r = _run(["-i", "a.vol", "-r", "b.vol", "--l1", "6"])
    assert r.returncode != 0
    assert "l1 = 6" in r.stderr and "not supported" in r.stderr
    r = _run(["-i", "a.vol", "-r", "b.vol", "--l2", "5"])
    assert r.returncode != 0 and "not supported" in r.stderr
