"""GPU checks of the Zernike3D alignment (xh_asa, xmipp_angular_sph_alignment) against a numpy fp64 restatement of the reference CPU
program's arithmetic (reconstruction/angular_sph_alignment.cpp: deformVol, tranformImageSph, continuousSphCost, processImage), with the
deviations the library states: r^2 from the integer coordinates, R^-1 as the transpose of the Euler matrix. The basis is the closed forms
of tests/test_volume_deform_sph_host.py; the trilinear sampler, the low pass, the masked correlation and the CTF image are the helpers of the
volume-deformation and continuous-assignment tests; Euler matrices, LINEAR applyGeometry and CTF values come from the oracle.

The contract is discontinuous where a component of pos + g crosses an integer (the mask lookup truncates, the sampler takes a floor) and the
restatement asserts, for every case with a rotation or coefficients, that no voxel is within 1e-9 of such a place: with that, no voxel is
exempted from any comparison.

The sizes past 17, the RDef values, the degree pairs and the row count of the larger cases are named in tests/zernike_shapes.py, which
says what each is there for."""
import functools
import math
import os
import subprocess

import numpy as np
import pytest

from tests import xmipp_io
from tests import zernike_shapes as shapes
from tests.test_volume_deform_sph_host import blobs, terms_ref, zsh_ref

pytestmark = pytest.mark.gpu

from tests.test_gpu_continuous_assign2 import CTF, circular_mask, ctf_and_envelope, lowpass, masked_correlation  # noqa: E402
from tests.test_gpu_volume_deform_sph import sample  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PROG = os.path.join(ROOT, "xmipp3_amd", "bin", "xmipp_angular_sph_alignment")
SIZES = [16, 17]
TILED = SIZES + list(shapes.ASA_TILES)      # and the sizes with 7 workgroups per row, the last one partly idle
MARGIN = 1e-9


@pytest.fixture(scope="module")
def gpu():
    import torch
    import xmipp3_amd as xa
    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    return xa, xa.Context(0), torch


# ------------------------------------------------------------------ the restatement
@functools.lru_cache(maxsize=None)
def volume(D):
    return blobs((D, D, D), seed=21 + D).astype(np.float32)


def sphere_mask(D, R):
    k, i, j = np.meshgrid(*(np.arange(D) - D // 2,) * 3, indexing="ij")
    return ((k * k + i * i + j * j) <= R * R).astype(np.int32)            # BinaryCircularMask, INNER_MASK


class Restated:
    """continuousSphCost + tranformImageSph + deformVol for one set of program parameters"""

    def __init__(self, oracle, vol, L1, L2, mask3=None, RDef=-1.0, Rmax=-1.0, lam=0.01, max_shift=-1.0, max_angular_change=5.0, sampling=1.0,
                 max_resolution=4.0, phase_flipped=False):
        self.o, self.D = oracle, vol.shape[0]
        D = self.D
        self.V = vol.astype(np.float64)
        self.L1, self.L2 = L1, L2
        self.terms = terms_ref(L1, L2)
        self.vec = len(self.terms)
        self.nvars = 3 * self.vec + 8
        self.RDef = float(D // 2) if RDef < 0 else float(RDef)
        self.Rmax = float(D // 2) if Rmax < 0 else float(Rmax)
        self.mask3 = sphere_mask(D, self.RDef) if mask3 is None else np.asarray(mask3, np.int32)
        self.sumV = float(self.V[self.mask3 == 1].sum())
        self.mask2 = circular_mask(D, self.Rmax)
        self.lam, self.max_shift, self.max_ang, self.Ts = lam, max_shift, max_angular_change, sampling
        self.w1 = sampling / max_resolution
        self.phase_flipped = phase_flipped
        self.k, self.i, self.j = np.meshgrid(*(np.arange(D) - D // 2,) * 3, indexing="ij")
        self.r2 = (self.k * self.k + self.i * self.i + self.j * self.j).astype(np.float64)

    def out_of_bounds(self, x):
        t = x[3 * self.vec:]
        if not np.all(np.isfinite(x)):
            return True
        if self.max_shift > 0 and t[0] ** 2 + t[1] ** 2 > self.max_shift ** 2:
            return True
        return self.max_ang > 0 and max(abs(t[2]), abs(t[3]), abs(t[4])) > self.max_ang

    def displacement(self, px, py, pz, x):
        """g = sum c Z(pos / RDef) at the positions (px, py, pz) of the lattice's voxels; terms with l2 > 0 are off at r = 0"""
        vec, iR = self.vec, 1.0 / self.RDef
        rr = np.sqrt(self.r2) * iR
        gx, gy, gz = np.zeros_like(px), np.zeros_like(px), np.zeros_like(px)
        for idx, (l1, n, l2, m) in enumerate(self.terms):
            c = (x[idx], x[vec + idx], x[2 * vec + idx])
            if c == (0.0, 0.0, 0.0):
                continue
            z = np.where((rr > 0) | (l2 == 0), zsh_ref(l1, n, l2, m, px * iR, py * iR, pz * iR, rr), 0.0)
            gx, gy, gz = gx + c[0] * z, gy + c[1] * z, gz + c[2] * z
        return gx, gy, gz

    def deform(self, row, x, check=True):
        """deformVol -> (P_raw, sumVd, modg, count)"""
        D, vec = self.D, self.vec
        t = x[3 * vec:]
        R = self.o.euler_matrix(row.get("rot", 0.0) + t[2], row.get("tilt", 0.0) + t[3], row.get("psi", 0.0) + t[4]).T
        k, i, j = self.k, self.i, self.j
        px = R[0, 0] * j + R[0, 1] * i + R[0, 2] * k
        py = R[1, 0] * j + R[1, 1] * i + R[1, 2] * k
        pz = R[2, 0] * j + R[2, 1] * i + R[2, 2] * k
        inside = self.r2 < self.RDef * self.RDef
        gx, gy, gz = self.displacement(px, py, pz, x)
        sx, sy, sz = px + gx, py + gy, pz + gz
        moved = bool(np.any(x[:3 * vec] != 0)) or not np.array_equal(R, np.eye(3))
        if check and moved:
            # off the discontinuities: the truncation and the floor flip at the integers, which the volume's faces are, too
            for s in (sx, sy, sz):
                assert np.abs(s[inside] - np.rint(s[inside])).min() > MARGIN, "an input sits on a discontinuity of the contract"
                phys = s[inside] + D // 2
                for face in (-1.0, 0.0, D - 1.0, float(D)):
                    assert np.abs(phys - face).min() > MARGIN, "a sampled position sits on a face of the volume"
        mk, mi, mj = (np.trunc(np.clip(s, -1e6, 1e6)).astype(np.int64) + D // 2 for s in (sz, sy, sx))
        ok = (mk >= 0) & (mk < D) & (mi >= 0) & (mi < D) & (mj >= 0) & (mj < D)
        mval = np.where(ok, self.mask3[np.clip(mk, 0, D - 1), np.clip(mi, 0, D - 1), np.clip(mj, 0, D - 1)], 0)
        sel = inside & (mval == 1)
        v = np.where(sel, sample(self.V, sx, sy, sz), 0.0)
        P = np.zeros((D, D))
        for q in range(D):                       # the reference's k-outer loop: every column adds its voxels in ascending k
            P = P + v[q]
        g2 = np.where(sel, gx * gx + gy * gy + gz * gz, 0.0)
        sumVd, modg = float(v.sum()), float(g2.sum())
        return P, sumVd, modg, int(sel.sum())

    def ctf_image(self, row, t):
        kw = dict(row["ctf"])
        kw["DeltafU"] += t[5]
        kw["DeltafV"] += t[6]
        kw["azimuthal_angle"] += t[7]
        ctf, _ = ctf_and_envelope(self.o, kw, self.D, self.Ts)
        return np.abs(ctf) if self.phase_flipped else ctf

    def project(self, row, x, check=True):
        """P after the CTF and the low pass, and deformVol's sums"""
        P, sumVd, modg, count = self.deform(row, x, check)
        raw = P
        if row.get("ctf"):
            P = np.fft.irfft2(np.fft.rfft2(P) * self.ctf_image(row, x[3 * self.vec:]), s=P.shape)
        return raw, lowpass(P, self.w1), sumVd, modg, count

    def particle(self, If, row, x):
        t = x[3 * self.vec:]
        A = np.eye(3)
        A[0, 2] = row.get("shift_x", 0.0) + t[0]
        A[1, 2] = row.get("shift_y", 0.0) + t[1]
        if row.get("flip", 0):
            A[0, :] *= -1
        return np.where(self.mask2, self.o.apply_geometry2d(If, A, 1, False, False), 0.0)

    def cost(self, If, row, x, check=True):
        if self.out_of_bounds(x):
            return 1e38
        _, P, sumVd, modg, count = self.project(row, x, check)
        if count == 0:
            return 1e38
        corr = masked_correlation(self.particle(If, row, x), P, self.mask2)
        return -corr + self.lam * (math.sqrt(modg / count) + abs(self.sumV - sumVd) / self.sumV)


def coefficients(ref, seed, reach):
    """random coefficients scaled so that the largest displacement component over the unrotated ball is `reach` voxels; the pose variables stay 0"""
    x = np.zeros(ref.nvars)
    x[:3 * ref.vec] = np.random.default_rng(seed).standard_normal(3 * ref.vec)
    inside = ref.r2 < ref.RDef ** 2
    g = ref.displacement(ref.j.astype(np.float64), ref.i.astype(np.float64), ref.k.astype(np.float64), x)
    x[:3 * ref.vec] *= reach / max(np.abs(c[inside]).max() for c in g)
    return x


def handle(gpu, ref, vol, capacity=8, mask=None, **kw):
    xa, ctx, torch = gpu
    return xa.AngularSphAlignment(ctx, torch.from_numpy(vol).cuda(), mask=mask, capacity=capacity, l1=ref.L1, l2=ref.L2, RDef=kw.pop("RDef", -1.0),
                                  Rmax=kw.pop("Rmax", -1.0), **kw)


def make_particle(ref, row, x, seed, noise=0.05):
    """the restatement's own projection at (row, x) plus a little noise, as float32"""
    _, P, _, _, _ = ref.project(row, x, check=False)
    rng = np.random.default_rng(seed)
    return (P + noise * P.std() * rng.standard_normal(P.shape)).astype(np.float32)


GENERIC = dict(rot=37.3, tilt=61.7, psi=-23.9)


# ------------------------------------------------------------------ 1. the projection
def _check_projection(gpu, ref, vol, row, x, mask=None, exact=False, **kw):
    h = handle(gpu, ref, vol, mask=mask, **kw)
    img = np.zeros((1, ref.D, ref.D), np.float32)
    img[0, ref.D // 2, ref.D // 2] = 1
    h.load(img, [dict(row)])
    cost = h.cost([0], x[None])[0]
    Praw, _, _, sums = h.last(0)
    Praw = Praw.cpu().numpy()
    want, sumVd, modg, count = ref.deform(row, x)
    scale = np.abs(want).max()
    print(f"D {ref.D} ({ref.L1},{ref.L2}): max|P| {scale:.6g}, P error {np.abs(Praw - want).max():.3g}, sumVd {sums[0]:.12g} vs {sumVd:.12g}, "
          f"modg {sums[1]:.12g} vs {modg:.12g}, count {sums[2]:.0f} vs {count}")
    assert sums[2] == count
    if exact:
        assert np.array_equal(Praw, want)
    assert np.abs(Praw - want).max() <= 1e-10 * scale
    assert abs(sums[0] - sumVd) <= 1e-9 * abs(sumVd)
    assert abs(sums[1] - modg) <= 1e-9 * abs(modg)
    return cost, count


@pytest.mark.parametrize("D", SIZES)
def test_projection_identity_is_the_in_order_column_sum(gpu, oracle, D):
    vol = volume(D)
    ref = Restated(oracle, vol, 3, 2)
    _, count = _check_projection(gpu, ref, vol, {}, np.zeros(ref.nvars), exact=True)
    assert count == int((ref.r2 < ref.RDef ** 2).sum())


@pytest.mark.parametrize("degrees", [(3, 2), (5, 4)])
@pytest.mark.parametrize("D", TILED)
def test_projection_generic(gpu, oracle, D, degrees):
    vol = volume(D)
    ref = Restated(oracle, vol, *degrees)
    _check_projection(gpu, ref, vol, GENERIC, coefficients(ref, 5 + D, 1.5))


@pytest.mark.parametrize("D", TILED)
def test_projection_user_mask(gpu, oracle, D):
    vol = volume(D)
    k, i, j = np.meshgrid(*(np.arange(D) - D // 2,) * 3, indexing="ij")
    mask = ((np.abs(k) <= 4) & (np.abs(i) <= 3) & (np.abs(j) <= 5)).astype(np.int32)
    mask[(k + i + j) % 5 == 0] *= 2                     # values other than 1 are not the mask
    ref = Restated(oracle, vol, 3, 2, mask3=mask, RDef=5.0)
    _, count = _check_projection(gpu, ref, vol, GENERIC, coefficients(ref, 9 + D, 1.5), mask=mask, RDef=5.0)
    assert 0 < count < int((ref.r2 < 25).sum())


@pytest.mark.parametrize("D", TILED)
def test_projection_large_coefficients(gpu, oracle, D):
    vol = volume(D)
    ref = Restated(oracle, vol, 3, 2)
    x = coefficients(ref, 13 + D, 7.0)
    _, count = _check_projection(gpu, ref, vol, GENERIC, x)
    # the case is what it says: mask lookups outside the volume, samples with taps outside
    assert count < int((ref.r2 < ref.RDef ** 2).sum())


@pytest.mark.parametrize("D", SIZES)
def test_projection_empty_mask(gpu, oracle, D):
    vol = volume(D)
    ref = Restated(oracle, vol, 3, 2)
    x = np.zeros(ref.nvars)
    x[0] = 1000.0                                        # the constant term: every voxel leaves along x
    h = handle(gpu, ref, vol)
    h.load(np.ones((1, D, D), np.float32), [dict(GENERIC)])
    assert ref.deform(GENERIC, x, check=False)[3] == 0
    assert h.cost([0], x[None])[0] == 1e38
    Praw, _, _, sums = h.last(0)
    assert sums[2] == 0 and sums[0] == 0 and not Praw.any()


@pytest.mark.parametrize("D,RDef", shapes.ASA_RDEF)
def test_projection_rdef_off_the_default(gpu, oracle, D, RDef):
    """a non-integer RDef (|k| <= ceil(RDef) - 1), and two RDef beyond the volume, where the clip of kmin / kmax to the volume binds"""
    vol = volume(D)
    ref = Restated(oracle, vol, 3, 2, RDef=RDef)
    _, count = _check_projection(gpu, ref, vol, GENERIC, coefficients(ref, 9 + D, 1.5), RDef=RDef)
    ball = ref.r2 < RDef * RDef
    inside = int(ball.sum())
    kmin, kmax, B = shapes.k_range(D, RDef)
    print(f"D {D} RDef {RDef}: count {count} of {inside} voxels in the ball, k {kmin} .. {kmax}, ceil(RDef) - 1 = {B}")
    assert ball[np.abs(ref.k) == B].any() or kmax < B            # the plane |k| = ceil(RDef) - 1 holds voxels wherever the volume has it
    if RDef > D // 2:
        assert kmax < B and count < inside                       # voxels leave the volume
        assert ball[np.abs(ref.k) == D // 2].any()               # and the ball reaches the volume's first plane, k = -D / 2
    else:
        assert (kmin, kmax) == (-B, B) and count == inside


@pytest.mark.parametrize("degrees", shapes.PAIRS + [shapes.RUN_TIME])
def test_projection_every_instantiation(gpu, oracle, degrees):
    """the 19 compiled (L1, L2) pairs of the dispatch table, each unrolled on its own, and (0, 0), which the run-time form serves"""
    D = 17
    vol = volume(D)
    ref = Restated(oracle, vol, *degrees)
    _check_projection(gpu, ref, vol, GENERIC, coefficients(ref, 5 + D, 1.5))


def _raw(gpu, ref, vol, row, x):
    """P_raw and the sums of one row on a handle of ref's degrees"""
    h = handle(gpu, ref, vol)
    h.load(np.zeros((1, ref.D, ref.D), np.float32), [dict(row)])
    h.cost([0], x[None])
    Praw, _, _, sums = h.last(0)
    return Praw.cpu().numpy(), sums.copy()


@pytest.mark.parametrize("h2", range(5))
def test_projection_effective_l2(gpu, oracle, h2):
    """a (5, 4) handle whose coefficients stop at the terms of (5, h) runs the (5, h) instantiation: the restatement's values, and the
    bits of a (5, h) handle given the same coefficients. (Equal bits are necessary, not sufficient: the terms left out multiply
    coefficients that are exactly 0. The handle exposes no count of launches per instantiation.)"""
    D = 17
    vol = volume(D)
    ref = Restated(oracle, vol, 5, 4)
    small = Restated(oracle, vol, 5, h2)
    assert ref.terms[:small.vec] == small.terms
    x = coefficients(ref, 5 + D, 1.5)
    xs = np.zeros(small.nvars)
    for d in range(3):
        x[d * ref.vec + small.vec:(d + 1) * ref.vec] = 0.0
        xs[d * small.vec:(d + 1) * small.vec] = x[d * ref.vec:d * ref.vec + small.vec]
    assert np.all(x[:small.vec] != 0)
    _check_projection(gpu, ref, vol, GENERIC, x)
    P54, s54 = _raw(gpu, ref, vol, GENERIC, x)
    P5h, s5h = _raw(gpu, small, vol, GENERIC, xs)
    assert np.array_equal(P54, P5h) and np.array_equal(s54[:3], s5h[:3])


def test_projection_second_lap_of_the_totals(gpu):
    """D = 260: 265 workgroups per row, so k_asa_cost adds the partials in two laps. Identity pose, no coefficients, a volume of small
    integers: P_raw is the column sum over r^2 < 130^2 and sumVd, count are integers, all exact in any order of addition"""
    xa, ctx, torch = gpu
    D = shapes.LAP
    c = D // 2
    assert shapes.tiles(D) == 265 and shapes.laps(shapes.tiles(D)) == 2
    vol = np.random.default_rng(D).integers(-2, 5, (D, D, D)).astype(np.float32)
    q = np.arange(D) - c
    ij2 = (q * q)[:, None] + (q * q)[None, :]
    want, count = np.zeros((D, D)), 0
    for k in range(D):                                   # the reference's k-outer loop, from index vectors: no D^3 grids
        ball = ij2 + q[k] * q[k] < c * c
        want += np.where(ball, vol[k], 0.0)
        count += int(ball.sum())
    h = xa.AngularSphAlignment(ctx, torch.from_numpy(vol).cuda(), capacity=1, l1=3, l2=2)
    assert h.RDef == c
    img = np.zeros((1, D, D), np.float32)
    img[0, c, c] = 1
    h.load(img, [{}])
    cost = h.cost([0], np.zeros((1, h.nvars)))[0]
    Praw, _, _, sums = h.last(0)
    Praw = Praw.cpu().numpy()
    print(f"D {D}: count {sums[2]:.0f} vs {count}, sumVd {sums[0]:.0f} vs {want.sum():.0f}, modg {sums[1]}, cost {cost}")
    assert np.array_equal(Praw, want)
    assert sums[2] == count and sums[0] == want.sum() and sums[1] == 0.0
    assert want.reshape(-1)[256 * 256:].any()            # the partials of the second lap (the columns from 65536 on) are not zeros
    assert cost < 1e30


# ------------------------------------------------------------------ 2. the cost
COST_CASES = {
    "plain": dict(),
    "ctf": dict(ctf=True),
    "ctf_phase_flipped": dict(ctf=True, phase_flipped=True),
    "defocus_deltas": dict(ctf=True, defocus=(120.0, -80.0, 3.5)),
    "flip": dict(flip=1),
    "shift_out_of_frame": dict(shift=(6.3, -5.6)),
    "small_Rmax": dict(Rmax=5.0),
}


@pytest.mark.parametrize("case", sorted(COST_CASES))
@pytest.mark.parametrize("D", SIZES)
def test_cost(gpu, oracle, D, case):
    _check_cost(gpu, oracle, D, case)


@pytest.mark.parametrize("case", ["plain", "ctf", "flip", "shift_out_of_frame"])
@pytest.mark.parametrize("D", shapes.ASA_TILES)
def test_cost_seven_tiles(gpu, oracle, D, case):
    _check_cost(gpu, oracle, D, case)


def _check_cost(gpu, oracle, D, case):
    xa = gpu[0]
    c = COST_CASES[case]
    vol = volume(D)
    ref = Restated(oracle, vol, 3, 2, Rmax=c.get("Rmax", -1.0), phase_flipped=c.get("phase_flipped", False))
    row = dict(GENERIC, shift_x=0.6, shift_y=-0.4, flip=c.get("flip", 0))
    if c.get("ctf"):
        row["ctf"] = dict(CTF)
    x = coefficients(ref, 31 + D, 1.2)
    x[3 * ref.vec:3 * ref.vec + 5] = (0.7, -0.9, 1.1, -0.6, 0.8)
    if "shift" in c:
        x[3 * ref.vec:3 * ref.vec + 2] = c["shift"]
    if "defocus" in c:
        x[3 * ref.vec + 5:] = c["defocus"]
    x0 = np.zeros(ref.nvars)
    img = make_particle(ref, row, x0, seed=3 + D)
    h = handle(gpu, ref, vol, Rmax=c.get("Rmax", -1.0), phase_flipped=int(c.get("phase_flipped", False)))
    h.load(img[None], [dict(row, ctf=xa.api.ctf_params(**row["ctf"]) if row.get("ctf") else None)])
    got = h.cost([0], x[None])[0]
    If = lowpass(img, ref.w1)
    want = ref.cost(If, row, x)
    _, P, Ip, sums = h.last(0)
    _, Pw, _, _, _ = ref.project(row, x)
    Ipw = ref.particle(If, row, x)
    print(f"D {D} {case}: cost {got:.15g} vs {want:.15g} (difference {abs(got - want):.3g}), P error {np.abs(P.cpu().numpy() - Pw).max():.3g}, "
          f"particle error {np.abs(Ip.cpu().numpy() - Ipw).max():.3g}")
    assert abs(got - want) <= 1e-9
    assert np.abs(P.cpu().numpy() - Pw).max() <= 1e-10 * max(np.abs(Pw).max(), np.abs(ref.deform(row, x)[0]).max())
    assert np.abs(Ip.cpu().numpy() - Ipw).max() <= 1e-10 * np.abs(If).max()
    assert abs(sums[3] - masked_correlation(Ipw, Pw, ref.mask2)) <= 1e-9


def test_cost_barrier_rows_never_reach_the_device(gpu, oracle):
    D = 16
    vol = volume(D)
    ref = Restated(oracle, vol, 3, 2, max_shift=2.0)
    h = handle(gpu, ref, vol, max_shift=2.0)
    h.load(make_particle(ref, GENERIC, np.zeros(ref.nvars), seed=1)[None], [dict(GENERIC)])
    p = 3 * ref.vec
    rows = np.zeros((5, ref.nvars))
    rows[0, p], rows[0, p + 1] = 1.5, 1.5                # 4.5 > 2^2
    rows[1, p + 3] = 5.5                                 # an angle past --max_angular_change
    rows[2, 3] = np.nan
    rows[3, p + 6] = np.inf
    rows[4, p + 2] = -5.0000001
    for r in rows:
        assert ref.out_of_bounds(r)
    assert np.array_equal(h.cost([0] * 5, rows), np.full(5, 1e38))
    assert h.stats()["rows"] == 0 and h.stats()["steps"] == 0
    ok = np.zeros((1, ref.nvars))
    ok[0, p], ok[0, p + 4] = 1.2, 5.0                    # on the bounds: inside
    mixed = np.concatenate([rows[:2], ok, rows[2:]])
    c = h.cost([0] * 6, mixed)
    assert np.array_equal(c[[0, 1, 3, 4, 5]], np.full(5, 1e38)) and c[2] < 1
    assert h.stats()["rows"] == 1 and h.stats()["steps"] == 1


# ------------------------------------------------------------------ 3, 4. batch independence, seams, repeatability
def _mixed_rows(gpu, oracle, D):
    xa = gpu[0]
    vol = volume(D)
    ref = Restated(oracle, vol, 3, 2)
    rows = [dict(GENERIC), dict(rot=101.2, tilt=33.3, psi=77.1, shift_x=0.8, flip=1), dict(rot=-50.5, tilt=120.4, psi=10.2, ctf=dict(CTF))]
    zero = np.zeros(ref.nvars)
    imgs = np.array([make_particle(ref, r, zero, seed=40 + q) for q, r in enumerate(rows)])
    load = [dict(r, ctf=xa.api.ctf_params(**r["ctf"]) if r.get("ctf") else None) for r in rows]
    part = np.array([0, 1, 2, 0, 0, 2, 1], np.int32)
    X = np.array([coefficients(ref, 60 + q, 1.0 + 0.2 * q) for q in range(7)])
    X[0, :3 * ref.vec] = 0                               # a row of the (L1, 0) instantiation among rows of the full one
    X[4, 2:ref.vec] = X[4, ref.vec + 2:2 * ref.vec] = X[4, 2 * ref.vec + 2:3 * ref.vec] = 0
    for q in range(7):
        X[q, 3 * ref.vec:] = np.random.default_rng(80 + q).uniform(-1, 1, 8) * (1, 1, 2, 2, 2, 100, 100, 3)
    return vol, ref, imgs, load, part, X, rows


def _call(h, part, X):
    """one cost call over the rows (all in bounds): the costs, and the last() sums of the rows of its last device chunk {row: sums}"""
    cost = h.cost(part, X)
    m = len(part)
    first = ((m - 1) // h.capacity) * h.capacity
    return cost, {first + r: h.last(r)[3].copy() for r in range(m - first)}


@pytest.mark.parametrize("D", SIZES)
def test_batch_independence_and_repeatability(gpu, oracle, D):
    vol, ref, imgs, load, part, X, _ = _mixed_rows(gpu, oracle, D)
    handles = {}
    for capacity in (3, 7, 8):
        handles[capacity] = handle(gpu, ref, vol, capacity=capacity)
        handles[capacity].load(imgs, load)
    # each row alone
    cost0, sums0 = np.zeros(7), {}
    for q in range(7):
        c, s = _call(handles[8], part[q:q + 1], X[q:q + 1])
        cost0[q], sums0[q] = c[0], s[0]
    assert np.all(cost0 < 1) and len({c for c in cost0}) == 7
    for capacity, h in handles.items():
        cost, sums = _call(h, part, X)
        again, sums_again = _call(h, part, X)
        assert np.array_equal(cost, again) and all(np.array_equal(sums[r], sums_again[r]) for r in sums)      # the same call twice: the same bits
        assert np.array_equal(cost, cost0), capacity
        assert sorted(sums) == ([6] if capacity == 3 else list(range(7)))           # capacity 3: chunks of 3, 3, 1
        for r, v in sums.items():
            assert np.array_equal(v, sums0[r]), (capacity, r)
    # at capacity 3 the seams fall after rows 2 and 5: every row's sums, chunk by chunk
    for a in (0, 3, 6):
        cost, sums = _call(handles[3], part[a:a + 3], X[a:a + 3])
        assert np.array_equal(cost, cost0[a:a + 3])
        for r, v in sums.items():
            assert np.array_equal(v, sums0[a + r])


def test_six_hundred_rows_in_one_step(gpu, oracle):
    """grid.y = 600 in k_asa_project, 600 workgroups of k_asa_cost and 9600 lines in a transform: the mixed rows, cycled. Every row's
    cost and sums are the bits of the same row in a step of 7; 12 rows, the first and the last among them, against the restatement"""
    D, m = shapes.ASA_ROWS
    vol, ref, imgs, load, part7, X7, rows = _mixed_rows(gpu, oracle, D)
    # row 0 has no coefficients, so its rotation leaves the origin voxel at exactly (0, 0, 0), which the restatement's margin refuses:
    # the constant term moves it, and the row still runs the (L1, 0) instantiation
    X7[0, [0, ref.vec, 2 * ref.vec]] = (0.31, -0.27, 0.43)
    part, X = np.resize(part7, m), np.resize(X7, (m, ref.nvars))
    assert np.array_equal(X[597], X7[597 % 7]) and part[599] == part7[599 % 7]
    big, small = handle(gpu, ref, vol, capacity=m), handle(gpu, ref, vol, capacity=7)
    big.load(imgs, load)
    small.load(imgs, load)
    cost = big.cost(part, X)
    assert big.stats()["steps"] == 1 and big.stats()["rows"] == m
    sums = np.array([big.last(r)[3] for r in range(m)])
    cost7, sums7 = _call(small, part7, X7)
    assert np.array_equal(small.cost(part, X), cost) and small.stats()["steps"] == -(-m // 7)
    for r in range(m):
        assert cost[r] == cost7[r % 7] and np.array_equal(sums[r], sums7[r % 7]), r
    sampled = sorted({0, m - 1} | set(np.random.default_rng(m).choice(np.arange(1, m - 1), 10, replace=False).tolist()))
    assert len(sampled) == 12
    want = {}
    for r in sampled:
        q = r % 7
        if q not in want:
            want[q] = ref.cost(lowpass(imgs[part7[q]], ref.w1), rows[part7[q]], X7[q])
        print(f"row {r}: cost {cost[r]:.15g} vs {want[q]:.15g} (difference {abs(cost[r] - want[q]):.3g})")
        assert abs(cost[r] - want[q]) <= 1e-9


# ------------------------------------------------------------------ 5. the search
# The searches run at --regularization 1. cost = -corr + lambda (deformation + mass difference) >= -1 + lambda deformation, so a cost
# below 0 needs an rms displacement under 1 / lambda voxels: at lambda = 1 under one voxel, which cannot turn the contrast of an image
# low-passed at a period of 4 px, and the contrast-inverted particle stays at a positive cost. At the default 0.01 the contract itself
# lets it escape: the same staged Powell search over the numpy restatement ends at -0.787 (the device at -0.763) after 6236
# evaluations, with an rms displacement of 7 voxels that empties the centre of a volume of radius 8; at lambda = 1 the restated search
# ends at +0.510 for that particle and at -0.991 (from -0.967 at zero) for the one made from known coefficients.
SEARCH_LAMBDA = 1.0


def _search_inputs(gpu, oracle, D):
    xa = gpu[0]
    vol = volume(D)
    ref = Restated(oracle, vol, 2, 1, max_shift=3.0, lam=SEARCH_LAMBDA)
    known = coefficients(ref, 91, 1.0)
    rows = [dict(GENERIC, shift_x=0.3, shift_y=-0.2), dict(rot=101.2, tilt=33.3, psi=77.1, ctf=dict(CTF)), dict(rot=-50.5, tilt=120.4, psi=10.2)]
    truth = [known.copy(), np.zeros(ref.nvars), np.zeros(ref.nvars)]
    truth[0][3 * ref.vec] = 1.0                          # a 1-px shift on top of the known coefficients
    imgs = np.array([make_particle(ref, r, t, seed=70 + q, noise=0.02) for q, (r, t) in enumerate(zip(rows, truth))])
    imgs[2] = -imgs[2]                                   # contrast-inverted: its correlation is negative wherever the search goes
    load = [dict(r, ctf=xa.api.ctf_params(**r["ctf"]) if r.get("ctf") else None) for r in rows]
    return vol, ref, imgs, load


def test_refine_equals_powell_stage_by_stage(gpu, oracle):
    xa = gpu[0]
    vol, ref, imgs, load = _search_inputs(gpu, oracle, 16)
    h = handle(gpu, ref, vol, capacity=2, max_shift=3.0, lam=SEARCH_LAMBDA, optimize_deformation=1, optimize_alignment=1, optimize_defocus=1)
    h.load(imgs, load)
    X, cost, en, de, it, ev = h.refine()
    at_zero = h.cost([0, 1, 2], np.zeros((3, ref.nvars)))
    print("refine: cost", cost, "at zero", at_zero, "enabled", en, "deformation", de, "iterations", it, "evaluations", ev)
    for q in range(3):
        x, enabled, fret, evals = np.zeros(ref.nvars), 1, None, 0
        for stage in range(1, ref.L2 + 1):
            act = xa.asa_stage_active(ref.L1, ref.L2, stage, True, True, True)

            def f(p):
                nonlocal evals
                evals += 1
                xx = x.copy()
                xx[act] = p
                return h.cost([q], xx[None])[0]
            p, fret, _ = xa.powell_minimize(f, x[act])
            if fret > 0:
                enabled = -1
                x[:] = 0
            else:
                x[act] = p
        assert np.array_equal(X[q], x) and cost[q] == fret and en[q] == enabled and ev[q] == evals, q
        c = h.cost([q], x[None])[0]
        s = h.last(0)[3]
        assert de[q] == (math.sqrt(s[1] / s[2]) if c < 1e30 else 0.0)
    # the particle made from known coefficients and a 1-px shift improves on its start and stays enabled
    assert en[0] == 1 and cost[0] < at_zero[0] and cost[0] < 0
    # the contrast-inverted particle is disabled and its variables return to zero
    assert en[2] == -1 and not X[2].any() and cost[2] > 0 and de[2] == 0


# ------------------------------------------------------------------ 6. the program
def _run_program(tmp_path, xmd, out, odir, extra=()):
    os.makedirs(odir, exist_ok=True)
    cmd = [PROG, "-i", str(xmd), "-o", str(out), "--ref", str(tmp_path / "ref.vol"), "--odir", str(odir), "--l1", "2", "--l2", "1", "--max_shift", "3", "--regularization", str(SEARCH_LAMBDA),
           "--optimizeDeformation", "--optimizeAlignment"] + list(extra)
    r = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=300)
    assert r.returncode == 0, r.stderr
    return r


def _read_rows(path):
    """labels and rows of the program's output; sphCoefficients is the unquoted vector [ v0 v1 ... ]"""
    labels, rows = [], []
    for line in open(path):
        t = line.strip()
        if not t or t[0] == "#" or t.startswith("data_") or t == "loop_":
            continue
        if t[0] == "_":
            labels.append(t[1:])
            continue
        a, b = t.index("["), t.index("]")
        head, vec, tail = t[:a].split(), [float(v) for v in t[a + 1:b].split()], t[b + 1:].split()
        rows.append(head + [vec] + tail)
    return labels, rows


def test_program_end_to_end(gpu, oracle, tmp_path):
    D = 16
    vol, ref, imgs, load = _search_inputs(gpu, oracle, D)
    xa = gpu[0]
    # a fourth particle; particles 1 and 3 carry a CTF. A metadata table gives every row the same columns, so the two with a CTF and the
    # two without are two input files of one stack
    extra_row = dict(rot=12.5, tilt=85.1, psi=-130.3, shift_x=-0.4, flip=1, ctf=dict(CTF, DeltafU=18000.0, DeltafV=17500.0))
    imgs = np.concatenate([imgs, make_particle(ref, extra_row, np.zeros(ref.nvars), seed=75)[None]])
    load = load + [dict(extra_row, ctf=xa.api.ctf_params(**extra_row["ctf"]))]
    rows = [dict(GENERIC, shift_x=0.3, shift_y=-0.2), dict(rot=101.2, tilt=33.3, psi=77.1, ctf=dict(CTF)), dict(rot=-50.5, tilt=120.4, psi=10.2), extra_row]
    xmipp_io.write_volume(str(tmp_path / "ref.vol"), vol)
    xmipp_io.write_stack(str(tmp_path / "in.stk"), imgs)
    pose = ["image", "angleRot", "anglePsi", "angleTilt", "shiftX", "shiftY", "flip"]
    ctf_labels = {"ctfVoltage": "kV", "ctfDefocusU": "DeltafU", "ctfDefocusV": "DeltafV", "ctfDefocusAngle": "azimuthal_angle", "ctfSphericalAberration": "Cs",
                  "ctfChromaticAberration": "Ca", "ctfEnergyLoss": "espr", "ctfQ0": "Q0", "ctfConvergenceCone": "alpha",
                  "ctfLongitudinalDisplacement": "DeltaF", "ctfTransversalDisplacement": "DeltaR"}

    def table(ids, with_ctf):
        out = []
        for q in ids:
            r = rows[q]
            line = [f"{q + 1}@{tmp_path / 'in.stk'}", r["rot"], r["psi"], r["tilt"], r.get("shift_x", 0.0), r.get("shift_y", 0.0), r.get("flip", 0)]
            out.append(line + ([r["ctf"].get(v, 0.0) for v in ctf_labels.values()] if with_ctf else []))
        return out
    xmipp_io.write_xmd(str(tmp_path / "plain.xmd"), [("noname", pose, table([0, 2], False))])
    xmipp_io.write_xmd(str(tmp_path / "ctf.xmd"), [("noname", pose + list(ctf_labels), table([1, 3], True))])
    _run_program(tmp_path, tmp_path / "plain.xmd", tmp_path / "plain_out.xmd", tmp_path / "o1")
    _run_program(tmp_path, tmp_path / "ctf.xmd", tmp_path / "ctf_out.xmd", tmp_path / "o2")
    assert not os.path.exists(tmp_path / "o1" / "sphDone.xmd") and not os.path.exists(tmp_path / "o2" / "sphDone.xmd")
    # the library on the same inputs
    h = handle(gpu, ref, vol, capacity=64, max_shift=3.0, lam=SEARCH_LAMBDA, optimize_deformation=1, optimize_alignment=1)
    h.load(imgs, load)
    X, cost, en, de, _, _ = h.refine()
    assert set(en) == {1, -1}
    for name, ids in (("plain_out.xmd", [0, 2]), ("ctf_out.xmd", [1, 3])):
        labels, out = _read_rows(tmp_path / name)
        assert labels == ["image", "enabled", "angleRot", "angleTilt", "anglePsi", "shiftX", "shiftY", "flip", "sphDeformation", "sphCoefficients", "cost"]
        assert len(out) == 2
        col = {l: k for k, l in enumerate(labels)}
        for r, q in zip(out, ids):
            t = X[q][3 * ref.vec:]
            assert r[col["image"]] == f"{q + 1}@{tmp_path / 'in.stk'}"
            assert int(r[col["enabled"]]) == en[q] and int(r[col["flip"]]) == rows[q].get("flip", 0)
            want = {"angleRot": rows[q]["rot"] + t[2], "angleTilt": rows[q]["tilt"] + t[3], "anglePsi": rows[q]["psi"] + t[4],
                    "shiftX": rows[q].get("shift_x", 0.0) + t[0], "shiftY": rows[q].get("shift_y", 0.0) + t[1], "sphDeformation": de[q], "cost": -cost[q]}
            for l, v in want.items():
                assert abs(float(r[col[l]]) - v) <= 1e-6, (l, q)
            assert len(r[col["sphCoefficients"]]) == 3 * ref.vec + 8 == h.nvars
            assert np.abs(np.array(r[col["sphCoefficients"]]) - X[q]).max() <= 1e-6
    # --resume over a half-finished sphDone.xmd: only the missing image is processed, and the file is the same
    whole = open(tmp_path / "ctf_out.xmd").read()
    lines = whole.splitlines(keepends=True)
    os.makedirs(tmp_path / "o3")
    open(tmp_path / "o3" / "sphDone.xmd", "w").write("".join(lines[:-1]))
    _run_program(tmp_path, tmp_path / "ctf.xmd", tmp_path / "ctf_resumed.xmd", tmp_path / "o3", ["--resume"])
    assert open(tmp_path / "ctf_resumed.xmd").read() == whole
    # that the first image was skipped, not recomputed to the same text: a sphDone.xmd whose first row is altered keeps the alteration
    os.makedirs(tmp_path / "o4")
    altered = lines[-2].replace(lines[-2].split()[2], "123.456000", 1)
    open(tmp_path / "o4" / "sphDone.xmd", "w").write("".join(lines[:-2]) + altered)
    _run_program(tmp_path, tmp_path / "ctf.xmd", tmp_path / "ctf_resumed2.xmd", tmp_path / "o4", ["--resume"])
    again = open(tmp_path / "ctf_resumed2.xmd").read().splitlines(keepends=True)
    assert again[-2] == altered and again[-1] == lines[-1] and len(again) == len(lines)
