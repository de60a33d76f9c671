"""GPU checks of the Zernike3D ART reconstruction (xh_faz, xmipp_forward_art_zernike3d) against a numpy fp64 restatement, written here, of
the reference's arithmetic (reconstruction_adapt_cuda11/forward_art_zernike3d_gpu.cpp: preProcess, processImage, artModel;
reconstruction_cuda11/cuda_forward_art_zernike3d.cu: forwardKernel, splattingAtPos, backwardKernel, computeTV, computeDTV), with the
deviations the library states at the head of xh_faz.hip. The comparator is this restatement, as for the sibling programs: the reference's
float arithmetic is not reproduced, and the reference cannot be built here. The basis is the closed forms of
tests/test_volume_deform_sph_host.py; Euler matrices, LINEAR applyGeometry and CTF values come from the oracle.

Margins. The contract is discontinuous where a projected coordinate has fractional part 1/2 (the pixel is a rounding) and where
sumMw crosses 0 (Idiff and Iws switch on). The restatement asserts that no splatted voxel is within MARGIN = 1e-9 of the first, and,
whenever the volume is updated, that every pixel a backward tap can reach (the disc of radius RDef + max|g| + 1) has
sumMw >= 1e-9 max(sumMw). With both, no voxel and no pixel is exempted from a comparison of V. Idiff, Iws and the error are compared over
the pixels above that margin, a set that is asserted to be the whole image at D = 16, 17 with RDef = D / 2 and sigma = 2, and wherever
the error value is compared (compare_forward compares it only then; at D = 80 and 260 test_error_where_it_is_exact makes it so).

Tolerances. A pixel of P or W is a sum of at most ~2 D terms (the voxels of a column through the ball, spread over the pixels next to
it), each a product of a weight and gw = (1 - a)(1 - b) whose position carries a few ulp of the rotation, the basis and the sums of g:
relative to the plane's maximum that is at most 2 D x a few x 2.2e-16 < 1e-13 at D = 33 and < 1e-12 at D = 260, the largest size
here (tests/zernike_shapes.py lists the sizes past 33 and what each is there for), in whatever order the atomics arrive. The
transform pair adds a few ulp times log2 of the size. 1e-10 x the plane's maximum, the tolerance of the sibling tests, is three orders
above that bound; the volume after n updates is held to n x 1e-10 x max|V|, every update adding a quotient of two such planes. A case that
needs more has a cause to be found.

Repeatability. Two sweeps from the same state agree within the same tolerance. Bitwise equality is not asserted: P and W are added with
floating-point atomics, the order of arrival differs from run to run, and so do the last bits of the sums."""
import functools
import os
import subprocess

import numpy as np
import pytest

from tests import xmipp_io
from tests import zernike_shapes as shapes
from tests.test_volume_deform_sph_host import blobs, terms_ref, zsh_ref

pytestmark = pytest.mark.gpu

from tests.test_gpu_continuous_assign2 import CTF, ctf_and_envelope  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PROG = os.path.join(ROOT, "xmipp3_amd", "bin", "xmipp_forward_art_zernike3d")
SIZES = [16, 17, 33]
TILED = SIZES + list(shapes.FAZ_TILES)      # and the sizes with LDS tiles inside the image and across each of its edges
MARGIN = 1e-9
TOL = 1e-10
MIN_CTF = 0.05


@pytest.fixture(scope="module")
def gpu():
    import torch
    import xmipp3_amd as xa
    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    return xa, xa.Context(0), torch


# ------------------------------------------------------------------ the restatement
def round_half_away(x):
    return np.sign(x) * np.floor(np.abs(x) + 0.5)


def sphere(D, R):
    k, i, j = np.meshgrid(*(np.arange(D) - D // 2,) * 3, indexing="ij")
    return ((k * k + i * i + j * j) <= R * R).astype(np.int32)            # BinaryCircularMask, INNER_MASK


class Art:
    """steps 1-7 of the contract for one set of program parameters; the state is V, Dx, Dy, Dz, Dl1, Reg"""

    def __init__(self, oracle, D, L1=3, L2=2, V0=None, maskf=None, maskb=None, sigma=(2.0,), RDef=-1.0, step=1, lam=0.01, ltv=1e-4, ltk=1e-4,
                 ll1=1e-4, lst=1e-4, use_zernike=True, use_ctf=False, phase_flipped=False, sampling=1.0, sym=()):
        self.o, self.D, self.c = oracle, D, D // 2
        self.L1, self.L2, self.terms = L1, L2, terms_ref(L1, L2)
        self.vec = len(self.terms)
        self.RDef = float(D // 2) if RDef < 0 else float(RDef)
        self.sigma, self.step, self.lam, self.ltv, self.ltk, self.ll1, self.lst = [float(s) for s in sigma], step, lam, ltv, ltk, ll1, lst
        self.use_zernike, self.use_ctf, self.phase_flipped, self.Ts = use_zernike, use_ctf, phase_flipped, sampling
        self.sym = [np.eye(3)] + [np.asarray(s, np.float64).reshape(3, 3) for s in sym]
        self.k, self.i, self.j = np.meshgrid(*(np.arange(D) - D // 2,) * 3, indexing="ij")
        self.r2 = (self.k * self.k + self.i * self.i + self.j * self.j).astype(np.float64)
        self.maskf, self.maskb = self._mask(maskf), self._mask(maskb)
        self.V = np.zeros((D, D, D)) if V0 is None else np.array(V0, np.float64)
        self.Dx, self.Dy, self.Dz, self.Dl1, self.Reg = (np.zeros((D, D, D)) for _ in range(5))
        pk, pi, pj = self.k + self.c, self.i + self.c, self.j + self.c
        self.lattice = (pk % step == 0) & (pi % step == 0) & (pj % step == 0)

    def _mask(self, m):
        if m is None:
            return sphere(self.D, self.RDef)
        return np.where(self.r2 >= self.RDef ** 2, 0, np.asarray(m).astype(np.int32))      # a file's values, truncated, inside the ball

    # step 1 and the displacement
    def rotations(self, row):
        E = self.o.euler_matrix(row.get("rot", 0.0), row.get("tilt", 0.0), row.get("psi", 0.0))
        return [E @ S for S in self.sym]

    def displacement(self, coef):
        """g = sum c Z((j, i, k) / RDef) on the lattice; terms with l2 > 0 are off at r = 0"""
        z = np.zeros(self.r2.shape)
        if not self.use_zernike or coef is None:
            return z, z, z
        vec, iR = self.vec, 1.0 / self.RDef
        rr = np.sqrt(self.r2) * iR
        gx, gy, gz = z.copy(), z.copy(), z.copy()
        for idx, (l1, n, l2, m) in enumerate(self.terms):
            c = (coef[idx], coef[vec + idx], coef[2 * vec + idx])
            if c == (0.0, 0.0, 0.0):
                continue
            zs = np.where((rr > 0) | (l2 == 0), zsh_ref(l1, n, l2, m, self.j * iR, self.i * iR, self.k * iR, rr), 0.0)
            gx, gy, gz = gx + c[0] * zs, gy + c[1] * zs, gz + c[2] * zs
        return gx, gy, gz

    def positions(self, R, coef):
        gx, gy, gz = self.displacement(coef)
        rx, ry, rz = self.j + gx, self.i + gy, self.k + gz
        return R[0, 0] * rx + R[0, 1] * ry + R[0, 2] * rz, R[1, 0] * rx + R[1, 1] * ry + R[1, 2] * rz

    # step 2
    def splat(self, R, coef, check=True):
        D, c, S = self.D, self.c, len(self.sigma)
        px, py = self.positions(R, coef)
        P, W = np.zeros((S, D, D)), np.zeros((S, D, D))
        self.outside = 0
        for s in range(S):
            sel = self.lattice & (self.maskf != 0)
            if S > 1:
                sel &= self.maskf == self.sigma[s]
            x, y, w = px[sel], py[sel], self.V[sel]
            fin = np.isfinite(x) & np.isfinite(y)
            x, y, w = x[fin], y[fin], w[fin]
            if check and x.size:
                for q in (x, y):
                    assert np.abs(np.abs(q) % 1.0 - 0.5).min() > MARGIN, "a voxel projects onto a rounding boundary"
            ii, jj = round_half_away(y), round_half_away(x)
            ok = (ii >= -c) & (ii <= D - 1 - c) & (jj >= -c) & (jj <= D - 1 - c)
            self.outside += int((~ok).sum())
            ii, jj, x, y, w = ii[ok], jj[ok], x[ok], y[ok], w[ok]
            m = 1.0 / self.step
            a, b = m * np.abs(ii - y), m * np.abs(jj - x)
            gw = 1.0 - a - b + a * b
            at = (ii.astype(np.int64) + c, jj.astype(np.int64) + c)
            np.add.at(P[s], at, w * gw)
            np.add.at(W[s], at, gw * gw)
        return P, W

    # step 3
    def filter(self, P, W):
        D = self.D
        w2 = np.fft.fftfreq(D)[:, None] ** 2 + np.fft.rfftfreq(D)[None, :] ** 2
        Pf, Wf = np.empty_like(P), np.empty_like(W)
        for s, sg in enumerate(self.sigma):
            Pf[s] = np.fft.irfft2(np.fft.rfft2(P[s]) * np.exp(-2.0 * np.pi ** 2 * w2 * sg * sg), s=(D, D))
            Wf[s] = np.fft.irfft2(np.fft.rfft2(W[s]) * (1.0 / (4 * np.pi * sg * sg)) * np.exp(-np.pi ** 2 * w2 * sg * sg), s=(D, D))
        return Pf, Wf

    # step 4
    def particle(self, img, row):
        I = np.asarray(img, np.float32).astype(np.float64)
        if row.get("ctf") and self.use_ctf:
            ctf, _ = ctf_and_envelope(self.o, row["ctf"], self.D, self.Ts)
            if self.phase_flipped:
                ctf = np.abs(ctf)
            inv = np.where(np.abs(ctf) <= MIN_CTF, 0.0, 1.0 / np.where(ctf == 0, 1.0, ctf))
            I = np.fft.irfft2(np.fft.rfft2(I) * inv, s=I.shape)
        A = np.eye(3)
        A[0, 2], A[1, 2] = row.get("shift_x", 0.0), row.get("shift_y", 0.0)
        if row.get("flip", 0):
            A[0, :] *= -1
        if np.abs(A - np.eye(3)).max() <= 1e-6:
            return I
        return self.o.apply_geometry2d(I, A, 1, False, False)

    # step 5
    def residual(self, Is, Pf, Wf):
        S = len(self.sigma)
        cs = [sg * sg if S > 1 else 1.0 for sg in self.sigma]
        diff, sumMw = Is.copy(), np.zeros_like(Is)
        for s in range(S):
            diff = diff - cs[s] * Pf[s]
            sumMw = sumMw + cs[s] * cs[s] * Wf[s]
        on = sumMw > 0
        Idiff = np.where(on, self.lam * diff, 0.0)
        Iws = np.where(on, np.maximum(sumMw, 1.0), 0.0)
        return Idiff, Iws, diff, sumMw

    def forward(self, Is, R, coef, check=True):
        P, W = self.splat(R, coef, check)
        Pf, Wf = self.filter(P, W)
        Idiff, Iws, diff, sumMw = self.residual(Is, Pf, Wf)
        safe = np.abs(sumMw) >= MARGIN * np.abs(sumMw).max() if sumMw.any() else np.zeros(sumMw.shape, bool)
        on = safe & (sumMw > 0)
        err = float(np.sqrt((diff[on] ** 2).sum() / on.sum())) if on.any() else float("nan")
        return dict(P_raw=P, W_raw=W, P=Pf, W=Wf, Idiff=Idiff, Iws=Iws, diff=diff, sumMw=sumMw, safe=safe, error=err)

    # step 6, as written in computeTV and computeDTV
    def regulariser(self):
        V, m = self.V, self.maskb != 0
        inx, iny, inz = (np.zeros(V.shape, bool) for _ in range(3))
        inx[:, :, 1:-1], iny[:, 1:-1, :], inz[1:-1, :, :] = True, True, True
        gx, gy, gz = (np.zeros(V.shape) for _ in range(3))
        gx[:, :, 1:-1] = 0.5 * V[:, :, 2:] - V[:, :, :-2]
        gy[:, 1:-1, :] = 0.5 * V[:, 2:, :] - V[:, :-2, :]
        gz[1:-1, :, :] = 0.5 * V[2:, :, :] - V[:-2, :, :]
        mag = np.sqrt(gx * gx + gy * gy + gz * gz + 1e-5)
        self.Dx = np.where(m & inx, gx / mag, self.Dx)
        self.Dy = np.where(m & iny, gy / mag, self.Dy)
        self.Dz = np.where(m & inz, gz / mag, self.Dz)
        self.Dl1 = np.where(m & (V > 0), self.lst, self.Dl1)
        self.Dl1 = np.where(m & (V < 0), self.ll1 * V, self.Dl1)
        Dx, Dy, Dz = self.Dx, self.Dy, self.Dz
        gx, gy, gz, gx2, gy2, gz2 = (np.zeros(V.shape) for _ in range(6))
        gx[:, :, 1:-1] = 0.5 * Dx[:, :, 2:] - Dx[:, :, :-2]
        gy[:, 1:-1, :] = 0.5 * Dy[:, 2:, :] - Dy[:, :-2, :]
        gz[1:-1, :, :] = 0.5 * Dz[2:, :, :] - Dz[:-2, :, :]
        gx2[:, :, 1:-1] = 0.5 * Dz[:, :, 2:] * Dx[:, :, 2:] - Dx[:, :, :-2] * Dx[:, :, :-2]
        gy2[:, 1:-1, :] = 0.5 * Dy[:, 2:, :] * Dy[:, 2:, :] - Dy[:, :-2, :] * Dy[:, :-2, :]
        gz2[1:-1, :, :] = 0.5 * Dz[2:, :, :] * Dz[2:, :, :] - Dz[:-2, :, :] * Dz[:-2, :, :]
        div, div2 = gx + gy + gz, 2.0 * (gx2 + gy2 + gz2)
        self.Reg = np.where(m, -self.lam * (self.ltv * div + self.ltk * div2 + self.Dl1), self.Reg)

    def interp2(self, I, x, y):
        D, c = self.D, self.c
        x0, y0 = np.floor(x), np.floor(y)
        fx, fy = x - x0, y - y0
        x0, y0 = x0.astype(np.int64) + c, y0.astype(np.int64) + c

        def tap(yy, xx):
            ok = (xx >= 0) & (xx < D) & (yy >= 0) & (yy < D)
            return np.where(ok, I[np.clip(yy, 0, D - 1), np.clip(xx, 0, D - 1)], 0.0)
        d00, d01, d10, d11 = tap(y0, x0), tap(y0, x0 + 1), tap(y0 + 1, x0), tap(y0 + 1, x0 + 1)
        d0, d1 = d00 + (d01 - d00) * fx, d10 + (d11 - d10) * fx
        return d0 + (d1 - d0) * fy

    # step 7
    def backward(self, R, coef, f):
        m = self.maskb != 0
        g = self.displacement(coef)
        reach = self.RDef + float(np.sqrt(g[0] ** 2 + g[1] ** 2 + g[2] ** 2)[m].max()) + 1.0
        ii, jj = np.meshgrid(np.arange(self.D) - self.c, np.arange(self.D) - self.c, indexing="ij")
        disc = ii * ii + jj * jj <= reach * reach
        assert f["sumMw"][disc].min() >= MARGIN * f["sumMw"].max(), "a pixel a backward tap can reach has no safe weight"
        px, py = self.positions(R, coef)
        x, y = px[m], py[m]
        self.V[m] += self.interp2(f["Idiff"], x, y) / (self.interp2(f["Iws"], x, y) + 1e-5) + self.Reg[m]

    def update(self, Is, row, coef):
        """every presentation of one image -> the errors"""
        errors = []
        for R in self.rotations(row):
            f = self.forward(Is, R, coef)
            self.regulariser()
            self.backward(R, coef, f)
            errors.append(f["error"])
        return errors


# ------------------------------------------------------------------ inputs
@functools.lru_cache(maxsize=None)
def volume(D, seed=0):
    return blobs((D, D, D), seed=31 + D + seed)


def coefficients(ref, seed, reach):
    """random coefficients scaled so that the largest displacement component over the ball is `reach` voxels"""
    x = np.random.default_rng(seed).standard_normal(3 * ref.vec)
    inside = ref.r2 < ref.RDef ** 2
    g = ref.displacement(x)
    return x * (reach / max(np.abs(q[inside]).max() for q in g))


GENERIC = dict(rot=37.3, tilt=61.7, psi=-23.9)
POSES = [dict(rot=37.3, tilt=61.7, psi=-23.9), dict(rot=101.2, tilt=33.3, psi=77.1), dict(rot=-50.5, tilt=120.4, psi=10.2),
         dict(rot=12.5, tilt=85.1, psi=-130.3), dict(rot=163.9, tilt=142.6, psi=55.5), dict(rot=-99.1, tilt=17.2, psi=-61.8)]


def particle_image(ref, row, coef, seed):
    """a particle that is not the projection of the volume under test: the filtered projection of another blob volume plus noise"""
    other = Art(ref.o, ref.D, ref.L1, ref.L2, V0=volume(ref.D, seed=100), RDef=ref.RDef, use_zernike=ref.use_zernike)
    P, W = other.splat(ref.rotations(row)[0], coef, check=False)
    Pf, _ = other.filter(P[:1], W[:1])
    rng = np.random.default_rng(seed)
    return (Pf[0] + 0.1 * Pf[0].std() * rng.standard_normal(Pf[0].shape)).astype(np.float32)


def handle(gpu, ref, V0=None, maskf=None, maskb=None, sym=None):
    xa, ctx, _ = gpu
    return xa.ForwardArtZernike3D(ctx, ref.D, volume=V0, maskf=maskf, maskb=maskb, sigma=ref.sigma, sym=sym, RDef=ref.RDef, l1=ref.L1, l2=ref.L2,
                                  step=ref.step, lam=ref.lam, ltv=ref.ltv, ltk=ref.ltk, ll1=ref.ll1, lst=ref.lst, use_zernike=int(ref.use_zernike),
                                  use_ctf=int(ref.use_ctf), phase_flipped=int(ref.phase_flipped), sampling=ref.Ts)


def load_rows(gpu, rows):
    xa = gpu[0]
    return [dict(r, ctf=xa.api.ctf_params(**r["ctf"]) if r.get("ctf") else None) for r in rows]


def compare_forward(tag, got, want, whole):
    """raw and filtered planes, then Idiff, Iws and the error over the pixels above the margin"""
    out = {k: (v.cpu().numpy() if hasattr(v, "cpu") else v) for k, v in got.items()}
    for name in ("P_raw", "W_raw", "P", "W"):
        for s in range(want[name].shape[0]):
            scale = np.abs(want[name][s]).max()
            err = np.abs(out[name][s] - want[name][s]).max()
            print(f"{tag} {name}[{s}]: max {scale:.6g}, error {err:.3g}")
            assert err <= TOL * scale, (name, s)
    safe = want["safe"]
    if whole:
        assert safe.all(), "the pixels above the margin are not the whole image"
    for name in ("Idiff", "Iws"):
        scale = np.abs(want[name]).max()
        err = np.abs(out[name] - want[name])[safe].max() if safe.any() else 0.0
        print(f"{tag} {name}: max {scale:.6g}, error {err:.3g}, pixels compared {int(safe.sum())} of {safe.size}")
        assert err <= TOL * scale, name
    if safe.all():
        scale = max(np.abs(want["diff"]).max(), 1e-300)
        print(f"{tag} error: {out['error']:.15g} vs {want['error']:.15g}")
        assert abs(out["error"] - want["error"]) <= TOL * scale
    return out


def run_forward(gpu, ref, row, coef, img=None, V0=None, maskf=None, maskb=None, whole=False, tag=""):
    h = handle(gpu, ref, V0=V0, maskf=maskf, maskb=maskb)
    img = particle_image(ref, row, coef, seed=5) if img is None else img
    h.load(img[None], load_rows(gpu, [row]), None if coef is None else coef[None])
    want = ref.forward(ref.particle(img, row), ref.rotations(row)[0], coef)
    got = compare_forward(tag, h.forward(0), want, whole)
    assert np.array_equal(h.get_volume(), ref.V)                # forward does not update the volume
    return h, got, want


# ------------------------------------------------------------------ 1. the forward model
@pytest.mark.parametrize("D", SIZES)
def test_forward_exact(gpu, oracle, D):
    """identity rotation, no deformation, V of small integers, step 1: raw P is the in-mask column sum and W the in-mask count, bit for bit"""
    V0 = np.random.default_rng(D).integers(-3, 4, (D, D, D)).astype(np.float64)
    ref = Art(oracle, D, V0=V0, use_zernike=False)
    h = handle(gpu, ref, V0=V0)
    h.load(np.ones((1, D, D), np.float32), [{}])
    inside = ref.maskf != 0
    got = h.forward(0)
    nb = -(-D // 16)
    occupied = sum(bool(inside[16 * z:16 * z + 16, 16 * y:16 * y + 16, 16 * x:16 * x + 16].any()) for z in range(nb) for y in range(nb) for x in range(nb))
    assert h.nbricks == occupied and (occupied > 1) == (D > 16)
    assert np.array_equal(got["P_raw"][0].cpu().numpy(), np.where(inside, V0, 0.0).sum(axis=0))
    assert np.array_equal(got["W_raw"][0].cpu().numpy(), inside.sum(axis=0).astype(np.float64))
    want = ref.forward(np.ones((D, D)), np.eye(3), None)
    assert np.array_equal(want["P_raw"][0], np.where(inside, V0, 0.0).sum(axis=0))
    compare_forward(f"exact D {D}", got, want, whole=D in (16, 17))


def _flat(D, sigma=(2.0,), lam=0.01):
    """steps 3 and 5 alone: an Art without its D^3 grids, for filter() and residual()"""
    a = Art.__new__(Art)
    a.D, a.sigma, a.lam = D, [float(s) for s in sigma], lam
    return a


@pytest.mark.parametrize("D", shapes.FAZ_EXACT)
def test_error_where_it_is_exact(gpu, oracle, D):
    """a file mask of ones inside a ball that covers the cube (RDef = D), identity rotation, no deformation, V of small integers: raw P
    is the column sum and raw W is D in every pixel, bit for bit, every pixel is above the margin, and the error is compared. At D = 260
    k_faz_errors adds 265 partials in two laps and N = 67600; the expectation comes from the column sums and the 2-D steps alone"""
    xa, ctx, _ = gpu
    assert 3 * (D // 2) ** 2 < D * D
    rng = np.random.default_rng(D)
    V0 = rng.integers(-3, 4, (D, D, D)).astype(np.float64)
    img = rng.standard_normal((D, D)).astype(np.float32) * 10
    ones = np.ones((D, D, D), np.int32)
    flat = _flat(D)
    P, W = V0.sum(axis=0)[None], np.full((1, D, D), float(D))
    Pf, Wf = flat.filter(P, W)
    Idiff, Iws, diff, sumMw = flat.residual(img.astype(np.float64), Pf, Wf)
    safe = np.abs(sumMw) >= MARGIN * np.abs(sumMw).max()
    assert safe.all() and (sumMw > 0).all()
    on = safe & (sumMw > 0)
    want = dict(P_raw=P, W_raw=W, P=Pf, W=Wf, Idiff=Idiff, Iws=Iws, diff=diff, sumMw=sumMw, safe=safe, error=float(np.sqrt((diff[on] ** 2).sum() / on.sum())))
    if D < 100:                                                # the same through the whole restatement, where its grids are small
        ref = Art(oracle, D, V0=V0, maskf=ones, RDef=float(D), use_zernike=False)
        assert (ref.maskf == 1).all()
        full = ref.forward(ref.particle(img, {}), ref.rotations({})[0], None)
        for name in ("P_raw", "W_raw", "P", "W", "Idiff", "Iws"):
            assert np.array_equal(full[name], want[name]), name
        assert full["error"] == want["error"] and full["safe"].all()
    else:
        assert shapes.tiles(D) == 265 and shapes.laps(shapes.tiles(D)) == 2 and D * D > 65536
    h = xa.ForwardArtZernike3D(ctx, D, volume=V0, maskf=ones, sigma=flat.sigma, RDef=float(D), lam=flat.lam, use_zernike=0)
    assert h.nbricks == shapes.brick_grid(D) ** 3
    h.load(img[None], [{}])
    got = h.forward(0)
    assert np.array_equal(got["P_raw"].cpu().numpy(), P) and np.array_equal(got["W_raw"].cpu().numpy(), W)
    assert np.array_equal(got["particle"].cpu().numpy(), img.astype(np.float64))
    compare_forward(f"exact error D {D}", got, want, whole=True)
    # the same value through a sweep, whose partials lie at the first slot
    err = h.sweep(0, 1)
    print(f"exact error D {D}: sweep {err[0, 0]:.15g} vs {want['error']:.15g}")
    assert abs(err[0, 0] - want["error"]) <= TOL * np.abs(diff).max()


def test_load_seam(gpu, oracle):
    """16384 + 6 images of 32 x 32: two chunks of faz_load. The first holds no CTF and is not filtered: its images come back bit for bit
    (but the last, which is shifted). The second holds one CTF, so all six of its images pass through the transform pair"""
    D, n = shapes.SEAM_D, shapes.SEAM_N
    first = shapes.load_chunks(D, n)[0]
    assert first == 16384 and n - first == 6
    ref = Art(oracle, D, use_zernike=False, use_ctf=True)
    idx = np.arange(n)
    base = (blobs((1, D, D), seed=3 + D)[0] * 10).astype(np.float32)
    imgs = base[None] * (1 + (idx % 97) / 97.0)[:, None, None].astype(np.float32)
    imgs[idx, (idx // D) % D, idx % D] += (1 + idx / n).astype(np.float32)      # every image is distinct
    assert len({im.tobytes() for im in imgs[::61]}) == len(imgs[::61]) and len({im.tobytes() for im in imgs[first - 3:]}) == 9
    rows = [{} for _ in range(n)]
    rows[first - 1] = dict(shift_x=1.6, shift_y=-2.3)
    rows[first + 1] = dict(shift_x=-0.7, shift_y=1.2)
    rows[first + 2] = dict(flip=1)
    rows[first + 3] = dict(ctf=dict(CTF))
    h = handle(gpu, ref)
    h.load(imgs, load_rows(gpu, rows))

    def particle(i):
        return h.forward(i)["particle"].cpu().numpy()
    drawn = np.random.default_rng(n).choice(np.arange(2, first - 2), 12, replace=False).tolist()
    for i in [0, 1, first // 2 - 1, first - 2] + drawn:
        assert np.array_equal(particle(i), imgs[i].astype(np.float64)), i
    worst = 0.0
    for i in range(first - 1, n):
        got, want = particle(i), ref.particle(imgs[i], rows[i])
        err, scale = np.abs(got - want).max(), np.abs(want).max()
        worst = max(worst, err / scale)
        print(f"load seam image {i} {rows[i] and sorted(rows[i])}: max {scale:.6g}, error {err:.3g}")
        assert err <= TOL * scale, i
    print(f"load seam: worst relative error {worst:.3g}")
    assert not np.array_equal(particle(first), imgs[first].astype(np.float64))          # the chunk was filtered
    assert np.abs(particle(first) - imgs[first]).max() <= TOL * np.abs(imgs[first]).max()
    unfiltered = imgs[first + 3].astype(np.float64)
    assert np.abs(particle(first + 3) - unfiltered).max() > 1e-3 * np.abs(unfiltered).max()


@pytest.mark.parametrize("degrees", [(1, 0), (2, 1), (3, 2), (5, 4), (0, 0)])
@pytest.mark.parametrize("D", SIZES)
def test_forward_generic(gpu, oracle, D, degrees):
    """(0, 0) is served by the run-time form of the kernels"""
    ref = Art(oracle, D, *degrees, V0=volume(D))
    run_forward(gpu, ref, GENERIC, coefficients(ref, 5 + D, 1.5), V0=ref.V.copy(), whole=D in (16, 17), tag=f"generic D {D} {degrees}")


@pytest.mark.parametrize("D,degrees", [(65, (3, 2)), (65, (5, 4)), (80, (3, 2))])
def test_forward_generic_whole_tiles(gpu, oracle, D, degrees):
    """48 x 48 tiles that lie wholly inside the image (8 at D = 65, 23 at D = 80) and tiles across each of its edges
    (tests/test_zernike_shapes.py counts them for this case); at D = 80, 117 of the 125 bricks are listed"""
    ref = Art(oracle, D, *degrees, V0=volume(D))
    h, _, want = run_forward(gpu, ref, GENERIC, coefficients(ref, 5 + D, 1.5), V0=ref.V.copy(), tag=f"generic D {D} {degrees}")
    assert h.nbricks == len(shapes.bricks(ref.maskf)) == {65: 67, 80: 117}[D]
    assert int(want["safe"].sum()) == {(65, (3, 2)): 4208, (65, (5, 4)): 4205, (80, (3, 2)): 6377}[D, degrees]      # the pixels compared in Idiff, Iws


@pytest.mark.parametrize("degrees", shapes.PAIRS)
def test_forward_every_instantiation(gpu, oracle, degrees):
    """the 19 compiled (L1, L2) pairs of the dispatch table, each unrolled on its own"""
    D = 17
    ref = Art(oracle, D, *degrees, V0=volume(D))
    run_forward(gpu, ref, GENERIC, coefficients(ref, 5 + D, 1.5), V0=ref.V.copy(), whole=True, tag=f"pair D {D} {degrees}")


@pytest.mark.parametrize("D", TILED)
def test_forward_no_deformation(gpu, oracle, D):
    ref = Art(oracle, D, V0=volume(D), use_zernike=False)
    run_forward(gpu, ref, GENERIC, None, V0=ref.V.copy(), whole=D in (16, 17), tag=f"no deformation D {D}")


@pytest.mark.parametrize("D", SIZES)
def test_forward_effective_l2(gpu, oracle, D):
    """coefficients that stop at the terms of (3, 1) run the (3, 1) instantiation of a (3, 2) handle"""
    ref = Art(oracle, D, 3, 2, V0=volume(D))
    coef = coefficients(ref, 7 + D, 1.5)
    last = len(terms_ref(3, 1))
    for d in range(3):
        coef[d * ref.vec + last:(d + 1) * ref.vec] = 0.0
    run_forward(gpu, ref, GENERIC, coef, V0=ref.V.copy(), whole=D in (16, 17), tag=f"effective l2 D {D}")


@pytest.mark.parametrize("D", TILED)
def test_forward_step_2(gpu, oracle, D):
    ref = Art(oracle, D, V0=volume(D), step=2)
    _, got, want = run_forward(gpu, ref, GENERIC, coefficients(ref, 9 + D, 1.5), V0=ref.V.copy(), tag=f"step 2 D {D}")
    full = Art(oracle, D, V0=volume(D)).splat(ref.rotations(GENERIC)[0], coefficients(ref, 9 + D, 1.5))[1]
    assert 0 < want["W_raw"].sum() < 0.5 * full.sum()          # an eighth of the voxels, each with a wider footprint weight


@pytest.mark.parametrize("D", shapes.FAZ_TILES)
def test_forward_step_3(gpu, oracle, D):
    """a lattice that does not line up with the 16-voxel bricks: the first lattice plane of a brick is at offset 0, 2 or 1"""
    ref = Art(oracle, D, V0=volume(D), step=3)
    assert shapes.BRICK % 3 != 0 and {(b * shapes.BRICK) % 3 for b in range(shapes.brick_grid(D))} == {0, 1, 2}
    h, got, want = run_forward(gpu, ref, GENERIC, coefficients(ref, 9 + D, 1.5), V0=ref.V.copy(), tag=f"step 3 D {D}")
    assert h.nbricks == len(shapes.bricks(ref.maskf, 3))
    assert int(ref.lattice.sum()) == (-(-D // 3)) ** 3 and want["W_raw"].sum() > 0


@pytest.mark.parametrize("D", SIZES)
def test_forward_file_mask(gpu, oracle, D):
    """a mask as read from a file: values other than 1, and voxels outside the ball of RDef that the program zeroes"""
    k, i, j = np.meshgrid(*(np.arange(D) - D // 2,) * 3, indexing="ij")
    mask = ((np.abs(k) <= 6) & (np.abs(i) <= 5) & (np.abs(j) <= 7)).astype(np.int32) * 3
    mask[(k + i + j) % 5 == 0] = 0
    ref = Art(oracle, D, V0=volume(D), maskf=mask, RDef=7.0)
    assert ((mask != 0) & (ref.maskf == 0)).any() and (ref.maskf == 3).any()
    run_forward(gpu, ref, GENERIC, coefficients(ref, 11 + D, 1.2), V0=ref.V.copy(), maskf=mask, tag=f"file mask D {D}")


@pytest.mark.parametrize("D", TILED)
def test_forward_two_sigmas(gpu, oracle, D):
    """maskF holds both sigmas and one value that matches neither: those voxels are skipped"""
    k, i, j = np.meshgrid(*(np.arange(D) - D // 2,) * 3, indexing="ij")
    mask = np.where(k < -1, 2, np.where(k > 1, 3, 5)).astype(np.int32)
    ref = Art(oracle, D, V0=volume(D), maskf=mask, sigma=(2.0, 3.0))
    _, got, want = run_forward(gpu, ref, GENERIC, coefficients(ref, 13 + D, 1.5), V0=ref.V.copy(), maskf=mask, tag=f"two sigmas D {D}")
    one = Art(oracle, D, V0=volume(D)).splat(ref.rotations(GENERIC)[0], coefficients(ref, 13 + D, 1.5))[1]
    assert want["W_raw"][0].any() and want["W_raw"][1].any() and want["W_raw"].sum() < one.sum()


@pytest.mark.parametrize("D", TILED)
def test_forward_large_coefficients(gpu, oracle, D):
    """displacements of up to 9 voxels push voxels out of the 48 x 48 tile's centre, and out of the image"""
    ref = Art(oracle, D, V0=volume(D))
    coef = coefficients(ref, 17 + D, 9.0)
    _, got, want = run_forward(gpu, ref, GENERIC, coef, V0=ref.V.copy(), tag=f"large D {D}")
    assert ref.outside > 0


def test_forward_outside_the_tile(gpu, oracle):
    """a steep gradient of the displacement stretches a brick of 16 voxels over ~60 pixels: some of its voxels land in the image more than
    half a tile (24 pixels) away from the projection of the brick's centre, where the tile is placed, and go to the global planes directly"""
    D = 33
    ref = Art(oracle, D, 1, 1, V0=volume(D), RDef=16.0)
    coef = np.zeros(3 * ref.vec)
    grad = [idx for idx, t in enumerate(ref.terms) if t[0] == 1 and t[2] == 1]
    coef[grad[2]] = 40.0                                       # x grows with x
    R = ref.rotations(dict(rot=3.1, tilt=2.2, psi=1.3))[0]
    px, py = ref.positions(R, coef)
    brick = (ref.maskf != 0) & (ref.k + ref.c < 16) & (ref.i + ref.c < 16) & (ref.j + ref.c < 16)
    landed = brick & (np.abs(px) <= 16) & (np.abs(py) <= 16)
    centre = px[8, 8, 8]
    assert landed.any() and np.abs(px[landed] - centre).max() > 24 + 1
    run_forward(gpu, ref, dict(rot=3.1, tilt=2.2, psi=1.3), coef, V0=ref.V.copy(), tag="outside the tile")
    assert ref.outside > 0


@pytest.mark.parametrize("D", [16, 33])
def test_forward_empty_mask(gpu, oracle, D):
    ref = Art(oracle, D, V0=volume(D), maskf=np.zeros((D, D, D), np.int32))
    h = handle(gpu, ref, V0=ref.V.copy(), maskf=np.zeros((D, D, D), np.int32))
    assert h.nbricks == 0
    h.load(np.ones((1, D, D), np.float32), [dict(GENERIC)], np.zeros((1, 3 * ref.vec)))
    got = h.forward(0)
    for name in ("P_raw", "W_raw", "P", "W", "Idiff", "Iws"):
        assert not got[name].any(), name
    assert np.isnan(got["error"])                              # sqrt(0 / 0), as in the reference


# ------------------------------------------------------------------ 2. the particle
PARTICLE_CASES = {
    "plain": dict(),
    "shift": dict(shift_x=1.6, shift_y=-2.3),
    "flip": dict(flip=1, shift_x=0.6, shift_y=-0.4),
    "ctf": dict(ctf=True, shift_x=0.6),
    "ctf_off": dict(ctf=True, use_ctf=False, shift_x=0.6),
    "ctf_phase_flipped": dict(ctf=True, phase_flipped=True, flip=1),
}


@pytest.mark.parametrize("case", sorted(PARTICLE_CASES))
@pytest.mark.parametrize("D", [16, 17])
def test_particle_preparation(gpu, oracle, D, case):
    c = dict(PARTICLE_CASES[case])
    ref = Art(oracle, D, V0=volume(D), use_ctf=c.pop("use_ctf", True), phase_flipped=c.pop("phase_flipped", False), use_zernike=False)
    row = dict(GENERIC, **{k: v for k, v in c.items() if k != "ctf"})
    if c.get("ctf"):
        row["ctf"] = dict(CTF)
    img = (blobs((1, D, D), seed=3 + D)[0] * 10).astype(np.float32)
    h = handle(gpu, ref, V0=ref.V.copy())
    h.load(img[None], load_rows(gpu, [row]))
    got = h.forward(0)["particle"].cpu().numpy()
    want = ref.particle(img, row)
    plain = img.astype(np.float64)
    print(f"particle D {D} {case}: max {np.abs(want).max():.6g}, error {np.abs(got - want).max():.3g}")
    assert np.abs(got - want).max() <= TOL * np.abs(want).max()
    assert np.array_equal(got, plain) == (case in ("plain",))
    if case == "ctf_off":
        assert np.array_equal(want, Art(oracle, D, use_zernike=False).particle(img, dict(row, ctf=None)))
    if case == "ctf_phase_flipped":
        assert np.abs(want - Art(oracle, D, use_ctf=True, use_zernike=False).particle(img, row)).max() > 1e-3 * np.abs(want).max()


# ------------------------------------------------------------------ 3. updates
def _update_case(oracle, D, sym=(), n=6):
    """non-zero weights of every regulariser, maskB different from maskF, V with both signs and exact zeros; n images"""
    V0 = volume(D) - 0.2
    k, i, j = np.meshgrid(*(np.arange(D) - D // 2,) * 3, indexing="ij")
    V0[(k + 2 * i + 3 * j) % 4 == 0] = 0.0
    maskb = ((k * k + i * i + j * j) <= (D // 2 - 2) ** 2).astype(np.int32) * 2
    maskb[(np.abs(k) <= 1) & (np.abs(i) <= 1)] = 0
    ref = Art(oracle, D, 3, 2, V0=V0, maskb=maskb, lam=0.05, ltv=2e-2, ltk=3e-2, ll1=4e-2, lst=5e-2, sym=sym)
    assert (ref.V > 0).any() and (ref.V < 0).any() and (ref.V[ref.maskb != 0] == 0).any() and not np.array_equal(ref.maskb, ref.maskf)
    coefs = np.array([coefficients(ref, 40 + q, 1.0 + 0.1 * q) for q in range(n)])
    imgs = np.array([particle_image(ref, POSES[q], coefs[q], seed=60 + q) for q in range(n)])
    return ref, V0, maskb, coefs, imgs


@functools.lru_cache(maxsize=None)
def _swept(D):
    """the restatement of one sweep over 6 images, computed once: (V after every image, errors)"""
    from oracle import pyoracle
    pyoracle.lib()
    ref, V0, maskb, coefs, imgs = _update_case(pyoracle, D)
    states, errors = [], []
    for q in range(6):
        errors.append(ref.update(ref.particle(imgs[q], POSES[q]), POSES[q], coefs[q]))
        states.append(ref.V.copy())
    return V0, maskb, coefs, imgs, states, np.array(errors), ref


def _check_volume(tag, got, want, n):
    scale = np.abs(want).max()
    err = np.abs(got - want).max()
    print(f"{tag}: max|V| {scale:.6g}, error {err:.3g} after {n} updates")
    assert err <= n * TOL * scale


@pytest.mark.parametrize("D", SIZES)
def test_one_update(gpu, oracle, D):
    V0, maskb, coefs, imgs, states, errors, ref = _swept(D)
    h = handle(gpu, ref, V0=V0, maskb=maskb)
    h.load(imgs[:1], load_rows(gpu, POSES[:1]), coefs[:1])
    err = h.sweep()
    _check_volume(f"one update D {D}", h.get_volume(), states[0], 1)
    assert not np.array_equal(states[0], V0) and np.array_equal(states[0][maskb == 0], V0[maskb == 0])
    assert err.shape == (1, 1) and abs(err[0, 0] - errors[0, 0]) <= TOL * max(np.abs(imgs[0]).max(), 1.0)


@pytest.mark.parametrize("D", SIZES)
def test_sweep_of_six_and_repeatability(gpu, oracle, D):
    V0, maskb, coefs, imgs, states, errors, ref = _swept(D)
    vols = []
    for _ in range(2):                                          # two handles: the same state, the regulariser's fields included
        h = handle(gpu, ref, V0=V0, maskb=maskb)
        h.load(imgs, load_rows(gpu, POSES), coefs)
        e1 = h.sweep(0, 2)                                      # a sweep in two calls is the sweep
        e2 = h.sweep(2, 4)
        vols.append(h.get_volume())
        err = np.concatenate([e1, e2])
        print(f"sweep D {D}: errors {err[:, 0]} vs {errors[:, 0]}")
        assert np.abs(err - errors).max() <= TOL * np.abs(imgs).max()
    _check_volume(f"sweep D {D}", vols[0], states[5], 6)
    # stale Dl1 entries matter: without them the restatement ends elsewhere
    _check_volume(f"repeat D {D}", vols[1], vols[0], 6)


@pytest.mark.parametrize("D", shapes.FAZ_TILES)
def test_sweep_of_two_whole_tiles(gpu, oracle, D):
    """two updates where tiles lie inside the image and k_faz_back reads it over more than one brick's footprint: V after each update,
    and a second handle from the same state. The restatement asserts its margin and the backward disc's weights for both updates. The
    pixels above the margin are not the whole image at these sizes, so the error value is not compared (test_error_where_it_is_exact)"""
    ref, V0, maskb, coefs, imgs = _update_case(oracle, D, n=2)
    states = []
    for q in range(2):
        ref.update(ref.particle(imgs[q], POSES[q]), POSES[q], coefs[q])
        states.append(ref.V.copy())
    vols = []
    for _ in range(2):
        h = handle(gpu, ref, V0=V0, maskb=maskb)
        h.load(imgs, load_rows(gpu, POSES[:2]), coefs)
        for q in range(2):
            h.sweep(q, 1)
            vols.append(h.get_volume())
            if len(vols) <= 2:
                _check_volume(f"sweep of two D {D}, update {q + 1}", vols[-1], states[q], q + 1)
    assert not np.array_equal(states[1], states[0]) and np.array_equal(states[1][maskb == 0], V0[maskb == 0])
    _check_volume(f"repeat D {D}", vols[3], vols[1], 2)


def test_symmetry_c2(gpu, oracle):
    D = 16
    c2 = np.diag([-1.0, -1.0, 1.0])
    ref, V0, maskb, coefs, imgs = _update_case(oracle, D, sym=[c2])
    h = handle(gpu, ref, V0=V0, maskb=maskb, sym=[c2])
    assert h.per_image == 2
    h.load(imgs[:2], load_rows(gpu, POSES[:2]), coefs[:2])
    second = ref.forward(ref.particle(imgs[0], POSES[0]), ref.rotations(POSES[0])[1], coefs[0])
    compare_forward("c2 second presentation", h.forward(0, 1), second, whole=True)
    errors = [ref.update(ref.particle(imgs[q], POSES[q]), POSES[q], coefs[q]) for q in range(2)]
    err = h.sweep()
    _check_volume("c2", h.get_volume(), ref.V, 4)
    assert err.shape == (2, 2) and np.abs(err - np.array(errors)).max() <= TOL * np.abs(imgs).max()
    assert abs(errors[0][0] - errors[0][1]) > 1e-6              # the two presentations are two different projections


def test_volume_round_trip(gpu, oracle):
    D = 17
    ref = Art(oracle, D)
    h = handle(gpu, ref)
    assert not h.get_volume().any()
    V = np.random.default_rng(1).standard_normal((D, D, D))
    h.set_volume(V)
    assert np.array_equal(h.get_volume(), V)
    xa = gpu[0]
    with pytest.raises(xa.XhError, match="not supported"):
        xa.ForwardArtZernike3D(gpu[1], D, l1=6, l2=2)
    with pytest.raises(xa.XhError, match="loaded"):
        h.sweep(0, 1)


# ------------------------------------------------------------------ 4. the program
def _read_mrc(path):
    raw = open(path, "rb").read()
    h = np.frombuffer(raw[:1024], np.int32)
    assert h[3] == 2
    return np.frombuffer(raw[1024:], np.float32).reshape(h[2], h[1], h[0])


def test_program_end_to_end(gpu, oracle, tmp_path):
    xa = gpu[0]
    D = 16
    V0 = volume(D).astype(np.float32)
    ref = Art(oracle, D, 3, 2, V0=V0)
    coefs = np.array([coefficients(ref, 40 + q, 1.0 + 0.1 * q) for q in range(6)])
    rows = [dict(POSES[q], shift_x=0.3 * q, shift_y=-0.2 * q, flip=q % 2) for q in range(6)]
    imgs = np.array([particle_image(ref, rows[q], coefs[q], seed=80 + q) for q in range(6)])
    xmipp_io.write_volume(str(tmp_path / "ref.vol"), V0)
    xmipp_io.write_stack(str(tmp_path / "in.stk"), imgs)
    # rows as xmipp_angular_sph_alignment writes them: the vector unquoted, "[ v0 v1 ... ]"
    with open(tmp_path / "in.xmd", "w") as f:
        f.write("# XMIPP_STAR_1 * \n# \ndata_noname\nloop_\n _image\n _enabled\n _angleRot\n _angleTilt\n _anglePsi\n _shiftX\n _shiftY\n _flip\n _sphCoefficients\n _cost\n")
        for q, r in enumerate(rows):
            vec = "[ " + " ".join(repr(float(v)) for v in coefs[q]) + " ]"
            f.write(f" {q + 1}@{tmp_path / 'in.stk'} 1 {r['rot']!r} {r['tilt']!r} {r['psi']!r} {r['shift_x']!r} {r['shift_y']!r} {r['flip']} {vec} 0.5 \n")
    odir = tmp_path / "out"
    os.makedirs(odir)
    cmd = [PROG, "-i", str(tmp_path / "in.xmd"), "-o", "somewhere/refined.vol", "--odir", str(odir), "--ref", str(tmp_path / "ref.vol"), "--useZernike", "--l1", "3",
           "--l2", "2", "--niter", "2", "--debug_iter", "--save_iter", "3", "--onlyPositive", "-v", "2"]
    r = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=300)
    assert r.returncode == 0, r.stderr
    for name in ("refined.vol", "refined_iter1.mrc", "refined_iter2.mrc", "refined_partial.mrc"):
        assert os.path.exists(odir / name), name
    assert r.stdout.count("Error for image") == 12
    # the restatement in the program's order
    order = xa.faz_sort_orthogonal([r_["rot"] for r_ in rows], [r_["tilt"] for r_ in rows], 2)
    assert sorted(order) == list(range(6)) and not np.array_equal(order, np.arange(6))

    def iterate(art, times):
        partial = None
        for _ in range(times):
            for pos, q in enumerate(order):
                art.update(art.particle(imgs[q], rows[q]), rows[q], coefs[q])
                if xa.faz_save_schedule(6, 3)[pos]:
                    partial = np.maximum(art.V, 0.0)
        return partial
    first = None
    for it in range(2):
        partial = iterate(ref, 1)
        if it == 0:
            first = np.maximum(ref.V, 0.0)
    final = np.maximum(ref.V, 0.0)
    got = xmipp_io.read_volume(str(odir / "refined.vol"))
    assert got.dtype == np.float32 and os.path.getsize(odir / "refined.vol") < 4 * D ** 3 + 4096
    print(f"program: max|V| {np.abs(final).max():.6g}, error {np.abs(got - final).max():.3g}")
    assert np.abs(got - final).max() <= 1e-6 and (got >= 0).all() and (ref.V < 0).any()
    assert np.abs(_read_mrc(odir / "refined_iter1.mrc") - first).max() <= 1e-6
    assert np.array_equal(_read_mrc(odir / "refined_iter2.mrc"), got)
    assert np.abs(_read_mrc(odir / "refined_partial.mrc") - partial).max() <= 1e-6      # the last one written: after the 5th image of iteration 2
    # --resume continues from the file the first run wrote
    r = subprocess.run(cmd + ["--resume"], stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=300)
    assert r.returncode == 0, r.stderr
    resumed = Art(oracle, D, 3, 2, V0=got)
    iterate(resumed, 2)
    again = xmipp_io.read_volume(str(odir / "refined.vol"))
    assert np.abs(again - np.maximum(resumed.V, 0.0)).max() <= 1e-6
    assert np.abs(again - got).max() > 1e-4                     # it went on from there, it did not start over
