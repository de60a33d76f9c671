"""xmipp_volume_deform_sph on the device against an fp64 restatement of the reference's algorithm (reconstruction/volume_deform_sph.cpp
with the CUDA twin's displacement), kept in numpy here and in tests/test_volume_deform_sph_host.py (the basis, normalize_Robust).
Plus the search against the same search over the numpy cost, and the program end to end."""
import functools
import math
import os
import subprocess

import numpy as np
import pytest

from tests import xmipp_io
from tests.test_volume_deform_sph_host import blobs, terms_ref, zsh_ref

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PROG = os.path.join(ROOT, "xmipp3_amd", "bin", "xmipp_volume_deform_sph")
SHAPES = [(16, 16, 16), (17, 20, 18)]      # the second: odd, non-cubic, partial workgroups on every axis
LAMBDA = 0.00025


@pytest.fixture(scope="module")
def gpu():
    import torch
    import xmipp3_amd as xa
    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    return xa, xa.Context(0)


# ---------------------------------------------------------------- the restatement
def logical(shape):
    Z, Y, X = shape
    return np.meshgrid(np.arange(Z) - Z // 2, np.arange(Y) - Y // 2, np.arange(X) - X // 2, indexing="ij")


@functools.lru_cache(maxsize=None)
def basis(shape, L1, L2, Rmax):
    """Z_idx at every voxel [nterms, Z, Y, X]: 0 where r^2 >= Rmax^2 (strict inside), and at r = 0 for every term with l2 > 0"""
    if Rmax < 0:
        Rmax = float(shape[2] // 2)
    k, i, j = logical(shape)
    r2 = (k * k + i * i + j * j).astype(np.float64)
    inside = r2 < Rmax * Rmax
    iR = 1.0 / Rmax
    rr = np.sqrt(r2) * iR
    out = []
    for (l1, n, l2, m) in terms_ref(L1, L2):
        z = zsh_ref(l1, n, l2, m, j * iR, i * iR, k * iR, rr)
        out.append(np.where(inside & ((rr > 0) | (l2 == 0)), z, 0.0))
    return np.array(out)


def field(x, Zm):
    nt = Zm.shape[0]
    return [np.tensordot(x[d * nt:(d + 1) * nt], Zm, axes=1) for d in range(3)]


def sample(V, x, y, z):
    """interpolatedElement3D at logical positions, 0 outside the volume"""
    Z, Y, X = V.shape
    px, py, pz = x + X // 2, y + Y // 2, z + Z // 2
    x0, y0, z0 = np.floor(px), np.floor(py), np.floor(pz)
    ax, ay, az = px - x0, py - y0, pz - z0
    x0, y0, z0 = x0.astype(np.int64), y0.astype(np.int64), z0.astype(np.int64)

    def tap(zz, yy, xx):
        ok = (zz >= 0) & (zz < Z) & (yy >= 0) & (yy < Y) & (xx >= 0) & (xx < X)
        return np.where(ok, V[np.clip(zz, 0, Z - 1), np.clip(yy, 0, Y - 1), np.clip(xx, 0, X - 1)], 0.0)

    def lin(a, lo, hi):
        return lo + (hi - lo) * a
    dx00 = lin(ax, tap(z0, y0, x0), tap(z0, y0, x0 + 1))
    dx01 = lin(ax, tap(z0 + 1, y0, x0), tap(z0 + 1, y0, x0 + 1))
    dx10 = lin(ax, tap(z0, y0 + 1, x0), tap(z0, y0 + 1, x0 + 1))
    dx11 = lin(ax, tap(z0 + 1, y0 + 1, x0), tap(z0 + 1, y0 + 1, x0 + 1))
    return lin(az, lin(ay, dx00, dx10), lin(ay, dx01, dx11))


def cost_ref(I, R, x, Zm, lam=LAMBDA):
    """(cost, diff2, sumVD, modg) over every voxel of every pair"""
    k, i, j = logical(I.shape[1:])
    gx, gy, gz = field(np.asarray(x, np.float64), Zm)
    diff2 = sumVD = modg = 0.0
    for p in range(I.shape[0]):
        vI = sample(I[p], j + gx, i + gy, k + gz)
        diff2 += np.sum((R[p] - vI) ** 2)
        sumVD += np.sum(vI[vI >= 0])
        modg += np.sum(gx * gx + gy * gy + gz * gz)
    count = float(I.size)
    sumVI = np.sum(I[I >= 0])
    cost = math.sqrt(diff2 / count) + lam * (math.sqrt(modg / count) + abs(sumVI - sumVD) / sumVI)
    return np.array([cost, diff2, sumVD, modg])


def gauss_ref(v, sigma):
    def dig(n):
        q = np.arange(n)
        return np.where(q <= (n >> 1), q, q - n) / float(n)
    Z, Y, X = v.shape
    fz, fy, fx = dig(Z), dig(Y), dig(X)[:X // 2 + 1]
    w2 = fx[None, None, :] ** 2 + fy[None, :, None] ** 2 + fz[:, None, None] ** 2
    return np.fft.irfftn(np.fft.rfftn(v) * np.exp(-math.pi ** 2 * w2 * sigma * sigma), s=v.shape, axes=(0, 1, 2))


def strain_ref(G):
    """(LS, LR) of an already filtered field [3, Z, Y, X]: 0 on the 2-voxel border"""
    Z, Y, X = G.shape[1:]
    LS, LR = np.zeros((Z, Y, X)), np.zeros((Z, Y, X))
    c = (slice(2, Z - 2), slice(2, Y - 2), slice(2, X - 2))

    def d(V, axis):
        def sh(o):
            s = [slice(2, Z - 2), slice(2, Y - 2), slice(2, X - 2)]
            n = (Z, Y, X)[axis]
            s[axis] = slice(2 + o, n - 2 + o)
            return V[tuple(s)]
        return (sh(-2) - 8 * sh(-1) + 8 * sh(1) - sh(2)) / 12.0
    U = [[d(G[a], ax) for ax in (2, 1, 0)] for a in range(3)]        # U[a][b] = d g_a / d (x, y, z)[b]
    d00, d11, d22 = U[0][0], U[1][1], U[2][2]
    d01, d02, d12 = 0.5 * (U[0][1] + U[1][0]), 0.5 * (U[0][2] + U[2][0]), 0.5 * (U[1][2] + U[2][1])
    h01, h02, h12 = 0.5 * (U[0][1] - U[1][0]), 0.5 * (U[0][2] - U[2][0]), 0.5 * (U[1][2] - U[2][1])
    LS[c] = np.abs(d00 * (d11 * d22 - d12 * d12) - d01 * (d01 * d22 - d12 * d02) + d02 * (d01 * d12 - d11 * d02))
    w = np.sqrt(h01 * h01 + h02 * h02 + h12 * h12)
    LR[c] = np.where(w > 1e-6, w * 180.0 / math.pi, 0.0)
    return LS, LR, w


@functools.lru_cache(maxsize=None)
def pairs(shape, npairs=3):
    """normalised (input, reference) pairs on the clipped scale: the volumes, then their low passes at sigma 1 and 2"""
    import xmipp3_amd as xa
    VI, VR = blobs(shape, seed=11), blobs(shape, seed=11, noise=0.0) + 0.3 * blobs(shape, seed=12)
    I = [VI] + [gauss_ref(VI, s) for s in (1.0, 2.0)]
    R = [VR] + [gauss_ref(VR, s) for s in (1.0, 2.0)]
    I = np.array([xa.vds_normalize_robust(v) for v in I[:npairs]])
    R = np.array([xa.vds_normalize_robust(v) for v in R[:npairs]])
    return I, R


def random_x(Zm, seed, reach=2.0):
    """random coefficients scaled so that the largest displacement component is `reach` voxels"""
    x = np.random.default_rng(seed).standard_normal(3 * Zm.shape[0])
    return x * (reach / max(np.abs(g).max() for g in field(x, Zm)))


# ---------------------------------------------------------------- cost
@pytest.mark.parametrize("Rmax", [-1.0, 5.0, 40.0])
@pytest.mark.parametrize("degrees", [(0, 0), (1, 0), (3, 2), (5, 4)])      # (0, 0): the kernel with run-time degrees
@pytest.mark.parametrize("shape", SHAPES)
def test_cost_parity(gpu, shape, degrees, Rmax):
    """cost, diff2, sumVD and modg against the numpy restatement to 1e-9 relative, for 1 and 3 pairs, at random coefficients that
    push border samples outside the volume and at x = 0. The bound: sums of at most 3 * 6120 = 18 360 non-negative terms (2e-12);
    |g| errs by about 1e-13 voxel (a few ulps on coefficients of at most about 45), the volume's gradient is at most 2.66 per voxel
    after the clip, so a term errs by about 3e-13 against sums of order 0.1 to 1: a margin of 100 or more. Measured on an MI355X: at most
    3.1e-15 over the 72 cases of the three larger degrees."""
    xa, ctx = gpu
    L1, L2 = degrees
    Zm = basis(shape, L1, L2, Rmax)
    if Rmax == 5.0:      # r^2 = 25 exactly is outside
        k, i, j = logical(shape)
        for q in ((0, 3, 4), (0, 0, 5), (3, 4, 0)):
            at = (k == q[0]) & (i == q[1]) & (j == q[2])
            assert at.sum() == 1 and np.all(Zm[:, at] == 0)
    if Rmax == 40.0:
        assert np.all(Zm[0] != 0)      # the whole cube is inside
    h = xa.VolumeDeformSph(ctx, shape, L1, L2, Rmax, LAMBDA)
    assert h.nterms == Zm.shape[0]
    for npairs in (1, 3):
        I, R = pairs(shape)
        I, R = I[:npairs], R[:npairs]
        h.set_pairs(I, R)
        assert h.sumVI == pytest.approx(np.sum(I[I >= 0]), rel=1e-12)
        for x in (random_x(Zm, seed=5), np.zeros(3 * Zm.shape[0])):
            got, want = h.cost(x), cost_ref(I, R, x, Zm)
            rel = np.abs(got - want) / np.where(want != 0, np.abs(want), 1.0)
            print(f"shape {shape} degrees {degrees} Rmax {Rmax} pairs {npairs} |x|max {np.abs(x).max():.3g}: got {got} rel.err {rel}")
            assert np.all(np.abs(got - want) <= 1e-9 * np.abs(want)), (got, want)


def test_stage_prefix_kernel_matches_full(gpu):
    """Coefficients that are zero past the terms of (L1, 1) run the (L1, 1) instantiation. Against the restatement to 1e-9, and
    against the full (L1, 2) instantiation bit for bit: a last coefficient of 1e-300 forces the full kernel and changes nothing it
    computes (1e-300 Z is absorbed by any displacement above 1e-284 and moves a zero displacement by less than an ulp of the
    voxel's position), so the two calls differ only in which kernel ran. Powell compares costs across that switch at the start of a
    stage."""
    xa, ctx = gpu
    shape = SHAPES[1]
    Zm = basis(shape, 3, 2, -1.0)
    I, R = pairs(shape)
    h = xa.VolumeDeformSph(ctx, shape, 3, 2)
    h.set_pairs(I, R)
    x = random_x(Zm, seed=8)
    nt, n1 = Zm.shape[0], xa.vds_num_terms(3, 1)
    y = x.copy()
    for d in range(3):
        y[d * nt + n1:(d + 1) * nt] = 0
    prefix, want = h.cost(y), cost_ref(I, R, y, Zm)
    assert np.all(np.abs(prefix - want) <= 1e-9 * np.abs(want)), (prefix, want)
    y[3 * nt - 1] = 1e-300
    full = h.cost(y)
    print(f"prefix kernel {prefix} full kernel {full} difference {full - prefix}")
    assert np.array_equal(prefix.view(np.uint64), full.view(np.uint64))
    got, want = h.cost(x), cost_ref(I, R, x, Zm)
    assert np.all(np.abs(got - want) <= 1e-9 * np.abs(want)), (got, want)


def test_determinism(gpu):
    xa, ctx = gpu
    shape = SHAPES[1]
    Zm = basis(shape, 3, 2, -1.0)
    I, R = pairs(shape)
    h = xa.VolumeDeformSph(ctx, shape, 3, 2)
    h.set_pairs(I, R)
    xa_, xb = random_x(Zm, seed=1), random_x(Zm, seed=2, reach=0.5)
    first = h.cost(xa_)
    other = h.cost(xb)
    again = h.cost(xa_)
    assert not np.array_equal(first, other)
    assert np.array_equal(first.view(np.uint64), again.view(np.uint64))
    # Powell's returned minimum is the cost at the returned point, bit for bit
    x, fret, it, evals = h.refine_stage(0, np.zeros(3 * Zm.shape[0]))
    assert evals > 0 and it >= 1
    assert np.float64(fret).view(np.uint64) == h.cost(x)[:1].view(np.uint64)[0]


def test_apply(gpu):
    """VO and g against numpy to 1e-10 absolute on clipped-scale data; g exactly 0 outside Rmax"""
    xa, ctx = gpu
    shape = SHAPES[1]
    Zm = basis(shape, 3, 2, 5.0)
    raw = pairs(shape)[0][0]
    h = xa.VolumeDeformSph(ctx, shape, 3, 2, 5.0)
    x = random_x(Zm, seed=4)
    VO, G = h.apply(raw, x, field=True)
    gx, gy, gz = field(x, Zm)
    k, i, j = logical(shape)
    want = sample(raw, j + gx, i + gy, k + gz)
    assert np.abs(VO - want).max() <= 1e-10
    for got, w in zip(G, (gx, gy, gz)):
        assert np.abs(got - w).max() <= 1e-10
    outside = (k * k + i * i + j * j) >= 25
    assert outside.any() and np.all(G[:, outside] == 0)
    assert np.array_equal(h.apply(raw, x), VO)


@pytest.mark.parametrize("shape", SHAPES)
def test_gauss(gpu, shape):
    """the tolerance of the halves-restoration tests for the same transforms: 1e-12 of the largest value"""
    xa, ctx = gpu
    v = blobs(shape, seed=21)
    h = xa.VolumeDeformSph(ctx, shape, 1, 0)
    want = gauss_ref(v, 1.5)
    assert np.abs(h.gauss(v, 1.5) - want).max() <= 1e-12 * np.abs(want).max()


def test_strain(gpu):
    xa, ctx = gpu
    shape = SHAPES[0]
    Zm = basis(shape, 3, 2, 40.0)
    k, i, j = logical(shape)
    g = field(random_x(Zm, seed=6, reach=0.5), Zm)
    # a deformation plus a rigid rotation about z, so that the rotation stays away from the 1e-6 threshold
    G = np.array([g[0] - 0.05 * i, g[1] + 0.05 * j, g[2]])
    h = xa.VolumeDeformSph(ctx, shape, 3, 2, 40.0)
    Gf, LS, LR = h.strain(G)
    want = np.array([gauss_ref(G[c], 2.0) for c in range(3)])
    assert np.abs(Gf - want).max() <= 1e-12 * np.abs(want).max()
    eLS, eLR, w = strain_ref(Gf)
    assert np.abs(w - 1e-6).min() > 1e-3       # nowhere near the threshold: checked on the numpy side first
    border = np.ones(shape, bool)
    border[2:-2, 2:-2, 2:-2] = False
    assert np.all(LS[border] == 0) and np.all(LR[border] == 0)
    assert np.all(LR[~border] > 0)
    assert np.all(np.abs(LS - eLS) <= 1e-10 * np.abs(eLS) + 1e-12)
    assert np.all(np.abs(LR - eLR) <= 1e-10 * np.abs(eLR) + 1e-12)


# ---------------------------------------------------------------- past the grid caps
# k_vds_cost runs on min(ceil(nbox / 256), 8 CUs) workgroups of 256 and k_vds_apply / k_vds_gauss / k_vds_strain on as many for the N
# voxels; each walks the rest in a grid-stride loop. (81, 84, 82): N = 557 928, and the box of the ball of Rmax = -1 (41 voxels) is
# 81^3 = 531 441, both between one and two passes of 2048 threads per CU on 256 CUs: a second, partial pass, on a non-cubic volume
# with an odd dimension. The cost's 3 rows of 2048 partial sums take the final reduction through its strided loop (8 per thread).
# With Rmax = -1 the second pass of the cost holds the last 7153 voxels of the box, of which only the ball's pole (k = 40, about 250
# voxels) counts; with an Rmax that holds the whole volume every voxel of it does. k_vds_gauss loops over the half spectrum
# (285 768 elements) on the grid sized for N: that one still fits a single pass at this shape.
BIG = (81, 84, 82)
BIG_ALL = 80.0       # an Rmax that holds the whole volume: r^2 <= 40^2 + 42^2 + 41^2 = 5045 < 6400


def _past_caps(count):
    import torch
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    print(f"{BIG}: {count} elements on {cus} CUs, grid cap {256 * 8 * cus} threads")
    assert count > 256 * 8 * cus, f"{count} elements do not exceed the grid cap of {256 * 8 * cus} threads on {cus} CUs"
    return cus


@pytest.mark.parametrize("Rmax", [-1.0, BIG_ALL])
@pytest.mark.parametrize("degrees", [(3, 2), (0, 0)])      # a compile-time instantiation, and the kernel with run-time degrees
def test_cost_parity_past_the_cap(gpu, degrees, Rmax):
    """test_cost_parity at (81, 84, 82), to its 1e-9 relative. The bound restated for this size: the sums have at most 3 * 557 928,
    about 1.7 M, non-negative terms, so their worst-case linear rounding bound is 1.7e6 * 1.1e-16 = 2e-10, whatever the order. A
    sample errs by about 3e-13 as there: sumVD by at most 1.7e6 * 3e-13 = 5e-7 against 1e4 (5e-11), diff2, whose terms d^2 have an
    rms d of about 0.02, by at most 1.7e6 * 2 * 0.02 * 3e-13 = 2e-8 against 300 to 900 (7e-11). The two add up to under 3e-10: 1e-9
    holds with a margin of 3 over the worst case.
    Measured on an MI355X: at most 9.7e-15 over the 16 cases."""
    xa, ctx = gpu
    L1, L2 = degrees
    N = int(np.prod(BIG))
    nbox = 81 ** 3 if Rmax < 0 else N
    _past_caps(N)
    _past_caps(nbox)
    Zm = basis(BIG, L1, L2, Rmax)
    k, i, j = logical(BIG)
    inside = (k * k + i * i + j * j) < (41.0 if Rmax < 0 else Rmax) ** 2
    assert np.all(Zm[0][inside] != 0) and np.all(Zm[0][~inside] == 0)
    assert inside.all() == (Rmax == BIG_ALL)
    # the box the kernel loops over is the bounding box of the ball, clipped to the volume
    span = [int(np.ptp(np.nonzero(inside.any(axis=tuple(a for a in range(3) if a != ax)))[0])) + 1 for ax in range(3)]
    assert span[0] * span[1] * span[2] == nbox
    h = xa.VolumeDeformSph(ctx, BIG, L1, L2, Rmax, LAMBDA)
    assert h.nterms == Zm.shape[0]
    worst = 0.0
    for npairs in (1, 3):
        I, R = pairs(BIG)
        I, R = I[:npairs], R[:npairs]
        h.set_pairs(I, R)
        assert h.sumVI == pytest.approx(np.sum(I[I >= 0]), rel=1e-12)
        for x in (random_x(Zm, seed=5), np.zeros(3 * Zm.shape[0])):
            got, want = h.cost(x), cost_ref(I, R, x, Zm)
            rel = np.abs(got - want) / np.where(want != 0, np.abs(want), 1.0)
            worst = max(worst, rel.max())
            print(f"shape {BIG} degrees {degrees} Rmax {Rmax} pairs {npairs} |x|max {np.abs(x).max():.3g}: got {got} rel.err {rel}")
            assert np.all(np.abs(got - want) <= 1e-9 * np.abs(want)), (got, want)
    print(f"shape {BIG} degrees {degrees} Rmax {Rmax}: largest relative error {worst:.3e} (bound 1e-9)")


def test_determinism_past_the_cap(gpu):
    """the same coefficients twice give the same bits with 2048 partial sums in each of 3 rows: the final reduction's strided loop
    (more than 256 partials per row needs more than 32 CUs) and the grid-stride loop's second pass"""
    xa, ctx = gpu
    cus = _past_caps(81 ** 3)
    assert 8 * cus > 256, f"{8 * cus} partial sums per row do not take the final reduction past its first 256"
    Zm = basis(BIG, 3, 2, -1.0)
    I, R = pairs(BIG)
    h = xa.VolumeDeformSph(ctx, BIG, 3, 2)
    h.set_pairs(I, R)
    xa_, xb = random_x(Zm, seed=1), random_x(Zm, seed=2, reach=0.5)
    first = h.cost(xa_)
    other = h.cost(xb)
    again = h.cost(xa_)
    assert not np.array_equal(first, other)
    assert np.array_equal(first.view(np.uint64), again.view(np.uint64))


def test_apply_past_the_cap(gpu):
    """test_apply's bounds (1e-10 absolute on clipped-scale data; g exactly 0 outside Rmax) with Rmax = -1, the ball of 41 voxels.
    Measured on an MI355X: VO 1.4e-15, g 1.4e-15."""
    xa, ctx = gpu
    _past_caps(int(np.prod(BIG)))
    Zm = basis(BIG, 3, 2, -1.0)
    raw = pairs(BIG)[0][0]
    h = xa.VolumeDeformSph(ctx, BIG, 3, 2)
    x = random_x(Zm, seed=4)
    VO, G = h.apply(raw, x, field=True)
    gx, gy, gz = field(x, Zm)
    k, i, j = logical(BIG)
    want = sample(raw, j + gx, i + gy, k + gz)
    print(f"{BIG} apply: max |VO - numpy| {np.abs(VO - want).max():.3e}, max |g - numpy| {max(np.abs(got - w).max() for got, w in zip(G, (gx, gy, gz))):.3e}")
    assert np.abs(VO - want).max() <= 1e-10
    for got, w in zip(G, (gx, gy, gz)):
        assert np.abs(got - w).max() <= 1e-10
    assert np.abs(VO - raw).max() > 0.01       # the deformation moved something
    outside = (k * k + i * i + j * j) >= 41 * 41
    assert outside.any() and np.all(G[:, outside] == 0)
    assert np.array_equal(h.apply(raw, x), VO)


def test_gauss_past_the_cap(gpu):
    """test_gauss's 1e-12 of the largest value. Measured on an MI355X: 8.1e-16."""
    xa, ctx = gpu
    _past_caps(int(np.prod(BIG)))
    v = blobs(BIG, seed=21)
    h = xa.VolumeDeformSph(ctx, BIG, 1, 0)
    want = gauss_ref(v, 1.5)
    got = h.gauss(v, 1.5)
    print(f"{BIG} gauss: max |device - numpy| = {np.abs(got - want).max() / np.abs(want).max():.3e} of the largest value")
    assert np.abs(got - want).max() <= 1e-12 * np.abs(want).max()


def test_strain_past_the_cap(gpu):
    """test_strain's field and bounds on the whole of (81, 84, 82). Measured on an MI355X: filtered field 1.9e-15 of its largest
    value, LS and LR equal to the restatement bit for bit."""
    xa, ctx = gpu
    _past_caps(int(np.prod(BIG)))
    Zm = basis(BIG, 3, 2, BIG_ALL)
    k, i, j = logical(BIG)
    g = field(random_x(Zm, seed=6, reach=0.5), Zm)
    G = np.array([g[0] - 0.05 * i, g[1] + 0.05 * j, g[2]])
    h = xa.VolumeDeformSph(ctx, BIG, 3, 2, BIG_ALL)
    Gf, LS, LR = h.strain(G)
    want = np.array([gauss_ref(G[c], 2.0) for c in range(3)])
    eLS, eLR, w = strain_ref(Gf)
    assert np.abs(w - 1e-6).min() > 1e-3       # nowhere near the threshold: checked on the numpy side first
    border = np.ones(BIG, bool)
    border[2:-2, 2:-2, 2:-2] = False
    with np.errstate(all="ignore"):
        print(f"{BIG} strain: filtered field {np.abs(Gf - want).max() / np.abs(want).max():.3e} of the largest value, "
              f"LS {np.nanmax(np.abs(LS - eLS)[~border] / np.abs(eLS)[~border]):.3e}, LR {np.nanmax(np.abs(LR - eLR)[~border] / np.abs(eLR)[~border]):.3e} relative")
    assert np.abs(Gf - want).max() <= 1e-12 * np.abs(want).max()
    assert np.all(LS[border] == 0) and np.all(LR[border] == 0)
    assert np.all(LR[~border] > 0)
    assert np.all(np.abs(LS - eLS) <= 1e-10 * np.abs(eLS) + 1e-12)
    assert np.all(np.abs(LR - eLR) <= 1e-10 * np.abs(eLR) + 1e-12)


# ---------------------------------------------------------------- search
def test_stage_discipline(gpu):
    xa, ctx = gpu
    shape = SHAPES[0]
    I, R = pairs(shape)
    h = xa.VolumeDeformSph(ctx, shape, 3, 2)
    h.set_pairs(I[:1], R[:1])
    nt = h.nterms
    assert nt == 13
    x, _, _, _ = h.refine_stage(0, np.zeros(3 * nt))
    thirds = x.reshape(3, nt)
    assert np.any(thirds[:, :2] != 0) and np.all(thirds[:, 2:] == 0)
    x, _, _, _ = h.refine_stage(1, x)
    thirds = x.reshape(3, nt)
    assert np.any(thirds[:, 2:8] != 0) and np.all(thirds[:, 8:] == 0)


def staged_search_ref(I, R, Zm, L1, L2):
    """the program's loop over the numpy cost: per stage, Powell (xh_powell_minimize, ftol 0.01) over the variables whose step is 1"""
    import xmipp3_amd as xa
    nt = Zm.shape[0]
    x = np.zeros(3 * nt)
    cost = None
    for stage in range(L2 + 1):
        ns = xa.vds_num_terms(L1, stage)
        active = np.array([d * nt + q for d in range(3) for q in range(ns)])

        def f(p):
            y = x.copy()
            y[active] = p
            return cost_ref(I, R, y, Zm)[0]
        p, cost, _ = xa.powell_minimize(f, x[active], ftol=0.01)
        x[active] = p
    return x, cost


def test_search_quality(gpu):
    """VI is VR moved by one voxel along x; degrees (1, 1), lambda at its default. The search must lower the cost, and end no more
    than ftol = 0.01 relative above the same staged search run over the numpy cost (two correct runs may stop at different points
    of one valley, Powell's stopping tolerance apart). Measured on an MI355X: 0.0663764 at x = 0, the device search 0.0188844 in 239
    evaluations, the numpy search 0.0188844."""
    xa, ctx = gpu
    shape = SHAPES[0]
    VR = xa.vds_normalize_robust(blobs(shape, seed=31, noise=0.0))
    VI = np.roll(VR, 1, axis=2)
    I, R = VI[None], VR[None]
    Zm = basis(shape, 1, 1, -1.0)
    h = xa.VolumeDeformSph(ctx, shape, 1, 1)
    h.set_pairs(I, R)
    x, cost, evals = h.refine()
    start = h.cost(np.zeros(3 * h.nterms))[0]
    _, ref_cost = staged_search_ref(I, R, Zm, 1, 1)
    print(f"search quality: cost at 0 {start:.6g}, device search {cost:.6g} ({evals} evaluations), numpy search {ref_cost:.6g}")
    assert cost < start
    assert cost <= ref_cost * (1 + 0.01)


# ---------------------------------------------------------------- the program
def _read_mrc(path):
    hdr = np.fromfile(path, np.int32, 4)
    assert hdr[3] == 2
    return np.fromfile(path, np.float32, offset=1024).reshape(hdr[2], hdr[1], hdr[0])


def test_program_end_to_end(gpu, tmp_path):
    """--l1 2 --l2 1 has 5 terms by the issue's own basis list (h = 0: l = 0, 2; h = 1: l = 1, m = -1 .. 1), so line 2 of _clnm.txt
    holds 3 * 5 values."""
    xa, ctx = gpu
    shape = SHAPES[0]
    N = int(np.prod(shape))
    VR = blobs(shape, seed=41)
    VI = 0.5 * (VR + np.roll(VR, 1, axis=2)) + 0.1 * blobs(shape, seed=42)
    fi, fr, fo, root = (str(tmp_path / n) for n in ("vi.vol", "vr.vol", "out.vol", "fit"))
    xmipp_io.write_volume(fi, VI)
    xmipp_io.write_volume(fr, VR)
    r = subprocess.run([PROG, "-i", fi, "-r", fr, "-o", fo, "--oroot", root, "--l1", "2", "--l2", "1", "--sigma", "1", "--analyzeStrain"],
                       stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=300)
    assert r.returncode == 0, r.stderr
    for st in range(2):
        assert f"Basis Degrees: (2,{st})" in r.stdout
    assert "Deformation " in r.stdout
    lines = open(root + "_clnm.txt").read().split("\n")
    assert lines[0] == "2 1 8 "
    assert lines[1].endswith(" ")
    x = np.array([float(t) for t in lines[1].split()])
    assert x.size == 3 * 5 and np.any(x != 0)
    # the same pairs, through the library
    VI32, VR32 = xmipp_io.read_volume(fi).astype(np.float64), xmipp_io.read_volume(fr).astype(np.float64)
    h = xa.VolumeDeformSph(ctx, shape, 2, 1)
    I = np.array([xa.vds_normalize_robust(VI32), xa.vds_normalize_robust(h.gauss(VI32, 1.0))])
    R = np.array([xa.vds_normalize_robust(VR32), xa.vds_normalize_robust(h.gauss(VR32, 1.0))])
    h.set_pairs(I, R)
    # what 6 significant digits of every coefficient can move: |delta g| <= 5e-6 sum |c| |Z|
    Zm = basis(shape, 2, 1, -1.0)
    gabs = [np.tensordot(np.abs(x[d * 5:(d + 1) * 5]), np.abs(Zm), axes=1) for d in range(3)]
    dg = 5e-6 * np.sqrt(sum(g * g for g in gabs))
    deformation = math.sqrt(h.cost(x)[3] / (2 * N))
    written = float(open(root + "_deformation.txt").read())
    assert abs(written - deformation) <= 5e-6 * written + math.sqrt(np.sum(dg * dg) / N)
    VO = xmipp_io.read_volume(fo)
    assert VO.shape == shape
    want, G = h.apply(VI32, x, field=True)
    steep = max(np.abs(np.diff(VI32, axis=a)).max() for a in range(3))
    assert np.abs(VO - want).max() <= 3 * steep * dg.max() + 2.0 ** -23 * np.abs(want).max()
    for name in ("_PPPGx.vol", "_PPPGy.vol", "_PPPGz.vol"):
        assert xmipp_io.read_volume(root + name).shape == shape
    base = fo[:-len(".vol")]
    LS, LR = _read_mrc(base + "_strain.mrc"), _read_mrc(base + "_rotation.mrc")
    assert LS.shape == shape and LR.shape == shape
    Gf, eLS, eLR = h.strain(G)
    assert np.abs(xmipp_io.read_volume(root + "_PPPGx.vol") - Gf[0]).max() <= 3 * dg.max() + 2.0 ** -23 * np.abs(Gf[0]).max()
