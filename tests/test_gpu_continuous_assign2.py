"""GPU checks of the continuous assignment (xh_ca2, xmipp_angular_continuous_assign2) against a restatement of the reference program's
arithmetic (reconstruction/angular_continuous_assign2.cpp: continuous2cost, tranformImage, processImage) composed here from the oracle's
projector, applyGeometry and Euler matrices plus numpy for the mask, the low pass and the masked correlation."""
import ctypes as C
import gc
import os
import subprocess

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

from tests import synth, xmipp_io  # noqa: E402

PROG = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "xmipp3_amd", "bin", "xmipp_angular_continuous_assign2")

VARS = 13


@pytest.fixture(scope="module")
def gpu():
    import torch
    import xmipp3_amd as xa
    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    return xa, xa.Context(0), torch


# ------------------------------------------------------------------ the restatement
def circular_mask(D, R):
    yy, xx = np.mgrid[0:D, 0:D]
    return ((yy - D // 2) ** 2 + (xx - D // 2) ** 2) <= R * R          # BinaryCircularMask, INNER_MASK, about the Xmipp origin


def lowpass(img, w1, raised_w=0.02):
    """FourierFilter LOWPASS, RAISED_COSINE (fourier_filter.cpp:423-432) applied as applyMaskSpace does"""
    D = img.shape[0]
    fy = np.fft.fftfreq(D)[:, None]
    fx = np.fft.rfftfreq(D)[None, :]
    w = np.sqrt(fx * fx + fy * fy)
    lp = np.where(w < w1, 1.0, np.where(w < w1 + raised_w, (1 + np.cos(np.pi / raised_w * (w - w1))) / 2, 0.0))
    return np.fft.irfft2(np.fft.rfft2(img.astype(np.float64)) * lp, s=img.shape)


def masked_correlation(x, y, mask):
    """correlationIndex(x, y, mask): the oracle's correlation_index over the masked pixels (0 when a sigma is below 1e-6)"""
    a, b = x[mask], y[mask]
    n = a.size
    ma, mb = a.sum() / n, b.sum() / n
    sa = np.sqrt(abs((a * a).sum() / n - ma * ma))
    sb = np.sqrt(abs((b * b).sum() / n - mb * mb))
    if sa < 1e-6 or sb < 1e-6:
        return 0.0
    return ((a - ma) * (b - mb)).sum() / (sa * sb * n)


def nr_bessj0(x):
    """the rational approximation of J0 that xmippCore's bessj0 is (Numerical Recipes), which the envelope is defined with"""
    x = np.asarray(x, np.float64)
    ax = np.abs(x)
    y = x * x
    a1 = 57568490574.0 + y * (-13362590354.0 + y * (651619640.7 + y * (-11214424.18 + y * (77392.33017 + y * (-184.9052456)))))
    a2 = 57568490411.0 + y * (1029532985.0 + y * (9494680.718 + y * (59272.64853 + y * (267.8532712 + y * 1.0))))
    small = a1 / a2
    axs = np.where(ax < 8.0, 8.0, ax)
    z = 8.0 / axs
    y = z * z
    xx = axs - 0.785398164
    b1 = 1.0 + y * (-0.1098628627e-2 + y * (0.2734510407e-4 + y * (-0.2073370639e-5 + y * 0.2093887211e-6)))
    b2 = -0.1562499995e-1 + y * (0.1430488765e-3 + y * (-0.6911147651e-5 + y * (0.7621095161e-6 - y * 0.934935152e-7)))
    large = np.sqrt(0.636619772 / axs) * (np.cos(xx) * b1 - z * np.sin(xx) * b2)
    return np.where(ax < 8.0, small, large)


def ctf_and_envelope(oracle, kw, D, Ts):
    """generateCTF (K = 1: the CTF with its damping) and generateEnvelope (ctf.h:1219-1241, 1271-1290, 424-496) on the half spectrum
    [D, D//2+1] at sampling Ts. The CTF values are the oracle's; the envelope is restated in numpy and checked against them."""
    p = oracle.ctf_params(**dict(kw, K=1.0))
    xh = D // 2 + 1
    fy = np.array([(i if i <= D // 2 else i - D) / D for i in range(D)])[:, None] / Ts       # FFT_IDX2DIGFREQ
    fx = (np.arange(xh) / D)[None, :] / Ts
    X, Y = np.broadcast_to(fx, (D, xh)), np.broadcast_to(fy, (D, xh))
    f = oracle.lib().xo_ctf_value_pure_nok
    ctf = np.array([[f(C.byref(p), float(X[i, j]), float(Y[i, j])) for j in range(xh)] for i in range(D)])
    # produceSideInfo (ctf.cpp:645-679)
    lam = 12.2643247 / np.sqrt(p.kV * 1e3 * (1.0 + 0.978466e-6 * p.kV * 1e3))
    Cs, Ca = p.Cs * 1e7, p.Ca * 1e7
    K1, K2 = np.pi * lam, np.pi / 2 * Cs * lam ** 3
    K3 = (0.25 * np.pi * Ca * lam * (p.espr / p.kV + 2 * p.ispr * 1e6)) ** 2 / np.log(2.0)
    K5, K6, K7 = np.pi * p.DeltaF * lam, np.pi ** 2 * p.alpha ** 2, Cs * lam ** 2
    u2 = X * X + Y * Y
    u = np.sqrt(u2)
    deltaf = -(p.DeltafU + p.DeltafV) / 2 - (p.DeltafU - p.DeltafV) / 2 * np.cos(2 * (np.arctan2(Y, X) - np.radians(p.azimuthal_angle)))
    deltaf = np.where((np.abs(X) < 1e-6) & (np.abs(Y) < 1e-6), 0.0, deltaf)
    xs = u * p.DeltaR
    sinc = np.where(xs == 0, 1.0, np.sin(np.pi * xs) / np.where(xs == 0, 1.0, np.pi * xs))
    aux = K7 * u2 * u + deltaf * u
    env = np.exp(-K3 * u2 * u2) * nr_bessj0(K5 * u2) * sinc * np.exp(-K6 * aux * aux) + p.envR0 + p.envR1 * u + p.envR2 * u2
    env = np.maximum(env, 0.0)
    arg = K1 * deltaf * u2 + K2 * u2 * u2
    mine = -(np.sqrt(1 - p.Q0 ** 2) * np.sin(arg) - p.Q0 * np.cos(arg)) * env
    assert np.abs(mine - ctf).max() <= 1e-11, "the numpy restatement of the CTF disagrees with the oracle's"
    return ctf, env


CTF = dict(kV=300.0, Cs=2.7, Ca=0.02, espr=1.0, Q0=0.07, DeltafU=15000.0, DeltafV=15400.0, azimuthal_angle=35.0, alpha=1e-4, DeltaF=20.0,
           DeltaR=0.3)


class Restated:
    """continuous2cost + tranformImage for one set of program parameters"""

    def __init__(self, oracle, vol, prm, l1, phase_flipped=False, same_defocus=False):
        self.phase_flipped, self.same_defocus = phase_flipped, same_defocus
        self.o = oracle
        self.D = vol.shape[0]
        self.prm = prm
        self.l1 = l1
        self.w1 = prm["sampling"] / prm["max_resolution"]
        self.fp = oracle.FP(vol, prm["padding"], self.w1, 3)
        R = prm["Rmax"] if prm["Rmax"] >= 0 else self.D // 2
        self.mask = circular_mask(self.D, R)

    def prepare(self, img, row=None):
        img = np.asarray(img, np.float32)
        If = lowpass(img, self.w1)
        if row is not None and row.get("ctf"):
            # L447-460: the spectrum times the envelope image at the input defocus
            _, env = ctf_and_envelope(self.o, row["ctf"], self.D, self.prm["sampling"])
            If = np.fft.irfft2(np.fft.rfft2(If) * env, s=If.shape)
        return If, float(np.std(img.astype(np.float64)))

    def ctf_image(self, row, x):
        if not row.get("ctf"):
            return None
        kw = dict(row["ctf"])
        kw["DeltafU"] = row["ctf"]["DeltafU"] + x[10]
        kw["DeltafV"] = kw["DeltafU"] if self.same_defocus else row["ctf"]["DeltafV"] + x[11]
        kw["azimuthal_angle"] = row["ctf"]["azimuthal_angle"] + x[12]
        ctf, _ = ctf_and_envelope(self.o, kw, self.D, self.prm["sampling"])
        return np.abs(ctf) if self.phase_flipped else ctf

    def out_of_bounds(self, row, sd, x):
        q = self.prm
        if q["max_shift"] > 0 and x[2] ** 2 + x[3] ** 2 > q["max_shift"] ** 2:
            return True
        if abs(x[4]) > q["max_scale"] or abs(x[5]) > q["max_scale"]:
            return True
        if max(abs(x[7]), abs(x[8]), abs(x[9])) > q["max_angular_change"]:
            return True
        if abs(x[0] - (row.get("gray_a", 1.0) if self.l1 else 1.0)) > q["max_gray_scale"]:
            return True
        if abs(x[1]) > q["max_gray_shift"] * sd:
            return True
        if abs(x[10]) > q["max_defocus_change"] or abs(x[11]) > q["max_defocus_change"]:
            return True
        return False

    def matrix(self, row, x):
        s2, s_2 = np.sin(x[6]) ** 2, np.sin(2 * x[6])
        A = np.eye(3)
        A[0, 0] = 1 + x[4] + (x[5] - x[4]) * s2
        A[0, 1] = A[1, 0] = 0.5 * (x[5] - x[4]) * s_2
        A[1, 1] = 1 + x[5] - (x[5] - x[4]) * s2
        A[0, 2] = row.get("shift_x", 0.0) + x[2]
        A[1, 2] = row.get("shift_y", 0.0) + x[3]
        if row.get("flip", 0):
            A[0, :] *= -1
        return A

    def images(self, If, row, x):
        P = self.fp.project(row.get("rot", 0.0) + x[7], row.get("tilt", 0.0) + x[8], row.get("psi", 0.0) + x[9], self.ctf_image(row, x))
        Ip = self.o.apply_geometry2d(If, self.matrix(row, x), 1, False, False)
        Ip = np.where(self.mask, Ip, 0.0)
        E = np.where(self.mask, (x[0] * P + x[1] - Ip) if self.l1 else (P - Ip), 0.0)
        return P, E, Ip

    def cost(self, If, sd, row, x):
        if self.out_of_bounds(row, sd, x):
            return 1e38
        P, E, Ip = self.images(If, row, x)
        if self.l1:
            return np.abs(E).sum() * (1.0 / self.mask.sum())
        return -masked_correlation(Ip, P, self.mask)


PRM = dict(max_shift=-1.0, max_scale=0.02, max_angular_change=5.0, max_defocus_change=500.0, max_resolution=4.0, max_gray_scale=0.05,
           max_gray_shift=0.05, sampling=1.0, Rmax=-1.0, padding=2.0)


def _particles(oracle, vol, n, rng, w1, flip, noise=0.05):
    """projections at random orientations, shifted, with a little noise; input rows a few degrees / a pixel away"""
    D = vol.shape[0]
    fp = oracle.FP(vol, 2.0, 0.5, 3)
    imgs, rows = [], []
    for _ in range(n):
        ang = synth.random_angles(1, rng)[0]
        ts = rng.uniform(-2, 2, 2)
        P = fp.project(*ang)
        A = np.eye(3)
        A[0, 2], A[1, 2] = -ts
        img = oracle.apply_geometry2d(P, A, 3, False, True)
        if flip:
            img = img[:, ::-1].copy()
        img = img + noise * P.std() * rng.standard_normal((D, D))
        imgs.append(img.astype(np.float32))
        rows.append(dict(rot=ang[0] + rng.uniform(-2, 2), tilt=ang[1] + rng.uniform(-2, 2), psi=ang[2] + rng.uniform(-2, 2),
                         shift_x=ts[0] + rng.uniform(-1, 1), shift_y=ts[1] + rng.uniform(-1, 1), flip=int(flip)))
    return np.stack(imgs), rows


def _random_rows(rng, prm, rows, sds, l1, n):
    """n rows inside the bounds, every family of variables moved"""
    idx = rng.integers(0, len(rows), n)
    X = np.zeros((n, VARS))
    for r, i in enumerate(idx):
        ga = rows[i].get("gray_a", 1.0) if l1 else 1.0
        X[r, 0] = ga + rng.uniform(-1, 1) * prm["max_gray_scale"] * 0.95
        X[r, 1] = rng.uniform(-1, 1) * prm["max_gray_shift"] * sds[i] * 0.95
        rad = prm["max_shift"] * 0.95 if prm["max_shift"] > 0 else 3.0
        t = rng.uniform(0, 2 * np.pi)
        X[r, 2:4] = rad * np.sqrt(rng.uniform()) * np.array([np.cos(t), np.sin(t)])
        X[r, 4:6] = rng.uniform(-1, 1, 2) * prm["max_scale"] * 0.95
        X[r, 6] = rng.uniform(-np.pi, np.pi)
        X[r, 7:10] = rng.uniform(-1, 1, 3) * prm["max_angular_change"] * 0.95
        if rows[i].get("ctf"):
            X[r, 10:12] = rng.uniform(-1, 1, 2) * prm["max_defocus_change"] * 0.95
            X[r, 12] = rng.uniform(-10, 10)
    return idx.astype(np.int32), X


def _outside_rows(prm, row, sd, l1):
    """one row just outside each bound of continuous2cost (L364-375)"""
    base = np.zeros(VARS)
    base[0] = row.get("gray_a", 1.0) if l1 else 1.0
    out = []
    eps = 1 + 1e-9
    for k, v in ((4, prm["max_scale"]), (5, -prm["max_scale"]), (7, prm["max_angular_change"]), (8, -prm["max_angular_change"]),
                 (9, prm["max_angular_change"]), (10, prm["max_defocus_change"]), (11, -prm["max_defocus_change"]),
                 (1, prm["max_gray_shift"] * sd), (1, -prm["max_gray_shift"] * sd)):
        x = base.copy()
        x[k] = v * eps
        out.append(x)
    for s in (1, -1):
        x = base.copy()
        x[0] += s * prm["max_gray_scale"] * eps
        out.append(x)
    if prm["max_shift"] > 0:
        x = base.copy()
        x[2] = prm["max_shift"] * np.cos(0.3) * eps
        x[3] = prm["max_shift"] * np.sin(0.3) * eps
        out.append(x)
    return np.stack(out)


def _device_rows(rows):
    """the rows as ContinuousAssign2.load takes them: the CTF as the library's structure"""
    from xmipp3_amd.api import ctf_params
    return [dict(r, ctf=ctf_params(**r["ctf"]) if r.get("ctf") else None) for r in rows]


# ------------------------------------------------------------------ check 3: cost parity
@pytest.mark.parametrize("l1", [False, True], ids=["corr", "l1"])
@pytest.mark.parametrize("flip", [False, True], ids=["noflip", "flip"])
@pytest.mark.parametrize("ctf", ["noctf", "ctf", "ctfflipped"])
@pytest.mark.parametrize("D", [32, 48, 45])
def test_cost_parity(gpu, oracle, D, ctf, flip, l1):
    """Device cost against the restatement: <= 1e-9 absolute for the correlation cost, <= 1e-9 mean|Ifiltered| for L1. Both sides are
    fp64 and differ in FFT algorithm and summation order only."""
    xa, ctx, torch = gpu
    rng = np.random.default_rng(1000 + D + 2 * flip + l1)
    prm = dict(PRM, max_shift=4.0)
    vol = synth.phantom(D, seed=11, nblobs=9).astype(np.float32)
    res = Restated(oracle, vol, prm, l1, phase_flipped=ctf == "ctfflipped")
    imgs, rows = _particles(oracle, vol, 4, rng, res.w1, flip)
    if ctf != "noctf":
        for k, r in enumerate(rows[:3]):            # the last particle has none: both kinds share a batch
            r["ctf"] = dict(CTF, DeltafU=CTF["DeltafU"] + 700.0 * k, azimuthal_angle=CTF["azimuthal_angle"] + 20.0 * k)
    if l1:
        for r in rows:
            r["gray_a"], r["gray_b"] = 1.0 + rng.uniform(-0.1, 0.1), rng.uniform(-0.01, 0.01)
    rows[0].update(scale_x=0.01, scale_y=-0.005, scale_angle=0.4)
    h = xa.ContinuousAssign2(ctx, torch.from_numpy(vol).cuda(), capacity=16, optimize_gray=int(l1), optimize_shift=1, optimize_angles=1,
                             optimize_scale=1, optimize_defocus=int(ctf != "noctf"), phase_flipped=int(ctf == "ctfflipped"), **prm)
    h.load(imgs, _device_rows(rows))
    prep = [res.prepare(im, r) for im, r in zip(imgs, rows)]
    for i, (If, sd) in enumerate(prep):
        got_If, got_sd = h.filtered(i)
        # fp64 both sides, different FFT algorithms: the relative bound test_gpu_fp.py holds the projector's transform to
        assert np.abs(got_If - If).max() <= 1e-11 * np.abs(If).max() and abs(got_sd - sd) <= 1e-12 * sd
    sds = [sd for _, sd in prep]
    idx, X = _random_rows(rng, prm, rows, sds, l1, 40)
    if ctf != "noctf":
        idx[0] = 0
        X[0, 10:13] = 0         # a row that leaves the defocus alone is served by the particle's resident CTF image (|.| when phase flipped)
    outside = _outside_rows(prm, rows[1], sds[1], l1)
    idx_all = np.concatenate([idx, np.full(len(outside), 1, np.int32)])
    X_all = np.concatenate([X, outside])
    got = h.cost(idx_all, X_all)
    exp = np.array([res.cost(prep[i][0], prep[i][1], rows[i], x) for i, x in zip(idx_all, X_all)])
    assert np.all(got[40:] == 1e38) and np.all(exp[40:] == 1e38)
    assert np.all(np.abs(exp[:40]) < 1e30)
    scale = np.mean([np.abs(If).mean() for If, _ in prep]) if l1 else 1.0
    err = np.abs(got[:40] - exp[:40]).max()
    print(f"cost parity D={D} {ctf} flip={flip} l1={l1}: max |device - restatement| = {err:.3e} (bound {1e-9 * scale:.3e})")
    assert err <= 1e-9 * scale
    # the same rows one by one, and in another order, are the same bits
    one = np.array([h.cost(idx_all[r:r + 1], X_all[r:r + 1])[0] for r in range(len(idx_all))])
    assert one.tobytes() == got.tobytes()
    perm = rng.permutation(len(idx_all))
    assert h.cost(idx_all[perm], X_all[perm]).tobytes() == got[perm].tobytes()
    h.close()


def test_identity_transform_and_empty_overlap(gpu, oracle):
    """A row whose A is the identity takes applyGeometry's copy; a particle shifted out of the box has zero variance under the mask and
    the correlation is 0, not NaN."""
    xa, ctx, torch = gpu
    D = 32
    vol = synth.phantom(D, seed=11, nblobs=9).astype(np.float32)
    res = Restated(oracle, vol, PRM, False)
    rng = np.random.default_rng(3)
    imgs, rows = _particles(oracle, vol, 2, rng, res.w1, False)
    rows[0].update(shift_x=0.0, shift_y=0.0)
    rows[1].update(shift_x=3.0 * D, shift_y=0.0)
    h = xa.ContinuousAssign2(ctx, torch.from_numpy(vol).cuda(), capacity=4, optimize_shift=1, **PRM)
    h.load(imgs, rows)
    x = np.zeros((2, VARS))
    x[:, 0] = 1
    got = h.cost([0, 1], x)
    If0, sd0 = res.prepare(imgs[0])
    assert abs(got[0] - res.cost(If0, sd0, rows[0], x[0])) <= 1e-9
    assert got[1] == 0.0 and res.cost(*res.prepare(imgs[1]), rows[1], x[1]) == 0.0
    h.close()


# ------------------------------------------------------------------ check 4: lockstep is the sequential search
def test_lockstep_refine_is_the_sequential_search(gpu, oracle):
    xa, ctx, torch = gpu
    D, n = 32, 37
    vol = synth.phantom(D, seed=11, nblobs=9).astype(np.float32)
    dvol = torch.from_numpy(vol).cuda()
    rng = np.random.default_rng(4)
    imgs, rows = _particles(oracle, vol, n, rng, 0.25, False)
    rows[5]["scale_x"] = 0.05            # outside --max_scale: not searched, disabled
    kw = dict(PRM, optimize_shift=1, optimize_angles=1)
    h = xa.ContinuousAssign2(ctx, dvol, capacity=16, **kw)
    h.load(imgs, rows)
    X, cost, it, ev, en = h.refine()
    st = h.stats()
    assert 0 < st["rows"] <= int(ev.sum()) and st["steps"] <= int(ev.sum())    # evaluations that the bounds decide never reach the device
    assert en[5] == -1 and cost[5] == -1 and it[5] == 0 and ev[5] == 0
    assert np.all(en[np.arange(n) != 5] == 1) and np.all(cost[np.arange(n) != 5] < 0)
    # (a) each particle alone in a fresh handle
    for i in range(n):
        h1 = xa.ContinuousAssign2(ctx, dvol, capacity=1, **kw)
        h1.load(imgs[i:i + 1], rows[i:i + 1])
        X1, c1, it1, ev1, en1 = h1.refine()
        h1.close()
        assert X1[0].tobytes() == X[i].tobytes(), (i, X1[0], X[i])
        assert c1.tobytes() == cost[i:i + 1].tobytes() and it1[0] == it[i] and ev1[0] == ev[i] and en1[0] == en[i]
    # (b) the sequential minimiser driven from Python over the handle's own cost, on the compacted variables
    active = [2, 3, 7, 8, 9]
    for i in (0, 17, 36):
        calls = [0]

        def f(xc, i=i):
            calls[0] += 1
            x = np.zeros(VARS)
            x[0] = 1
            x[active] = xc
            return h.cost([i], x[None])[0]
        p, fmin, its = xa.powell_minimize(f, np.zeros(5), np.ones(5), 0.01)
        assert p.tobytes() == X[i][active].tobytes(), (i, p, X[i][active])
        assert np.float64(fmin).tobytes() == cost[i:i + 1].tobytes() and its == it[i] and calls[0] == ev[i]
    h.close()


@pytest.mark.parametrize("same", [False, True], ids=["uv", "samedefocus"])
def test_defocus_search_in_lockstep(gpu, oracle, same):
    """--optimizeDefocus [--sameDefocus]: the compact vector is (shift, defocus U, [V,] angle); lockstep refine equals the sequential
    minimiser over the handle's own cost bit for bit, and an evaluation that leaves the defocus alone (served by the particle's resident
    CTF image) agrees with the restatement."""
    xa, ctx, torch = gpu
    D, n = 32, 6
    vol = synth.phantom(D, seed=11, nblobs=9).astype(np.float32)
    rng = np.random.default_rng(8)
    imgs, rows = _particles(oracle, vol, n, rng, 0.25, False)
    for k, r in enumerate(rows):
        r["ctf"] = dict(CTF, DeltafU=CTF["DeltafU"] + 300.0 * k)
    rows[4]["ctf"] = dict(CTF, DeltafU=100.0, DeltafV=150.0)          # the search may push U + dU below 0: disabled (L654-655)
    kw = dict(PRM, optimize_shift=1, optimize_defocus=1, same_defocus=int(same), max_defocus_change=500.0)
    h = xa.ContinuousAssign2(ctx, torch.from_numpy(vol).cuda(), capacity=4, **kw)
    h.load(imgs, _device_rows(rows))
    X, cost, it, ev, en = h.refine()
    active = [2, 3, 10, 12] if same else [2, 3, 10, 11, 12]
    if same:
        assert np.all(X[:, 11] == 0)
    for i in range(n):
        calls = [0]

        def f(xc, i=i):
            calls[0] += 1
            x = np.zeros(VARS)
            x[0] = 1
            x[active] = xc
            return h.cost([i], x[None])[0]
        p, fmin, its = xa.powell_minimize(f, np.zeros(len(active)), np.ones(len(active)), 0.01)
        assert np.float64(fmin).tobytes() == cost[i:i + 1].tobytes() and its == it[i] and calls[0] == ev[i]
        if en[i] == 1:
            assert p.tobytes() == X[i][active].tobytes()
        # the expected flag restates the library's own rule (:523, :654-655 with the reference's U + p(11)), not an independent source
        expect_disabled = fmin > 0 or rows[i]["ctf"]["DeltafU"] + p[2] < 0 or (not same and rows[i]["ctf"]["DeltafU"] + p[3] < 0)
        assert (en[i] == -1) == bool(expect_disabled)
    res = Restated(oracle, vol, kw, False, same_defocus=same)
    x = np.zeros((1, VARS))
    x[0, 0] = 1
    If, sd = res.prepare(imgs[0], rows[0])
    assert abs(h.cost([0], x)[0] - res.cost(If, sd, rows[0], x[0])) <= 1e-9
    h.close()


# ------------------------------------------------------------------ check 5: the search against the CPU
def _geodesic(oracle, a, b):
    M = oracle.euler_matrix(*a) @ oracle.euler_matrix(*b).T
    return np.degrees(np.arccos(np.clip((np.trace(M) - 1) / 2, -1, 1)))


def test_search_against_the_cpu(gpu, oracle):
    """40 noise-free particles at D = 32, started 2-3 degrees and 1-2 px away. The yardstick is the sequential minimiser over the restated
    cost on the CPU. The CPU search alone, rerun with relative noise of 1e-10 on every cost, ends within 3.0e-7 in cost and 4.9e-3 in
    the variables of itself; the device differs from the host by at most the 1e-9 of the parity check, so the device search must end
    within 1e-5 in cost and 0.05 (degrees, pixels) in every variable of the CPU search, for every particle."""
    xa, ctx, torch = gpu
    D, n = 32, 40
    vol = synth.phantom(D, seed=11, nblobs=9).astype(np.float32)
    res = Restated(oracle, vol, PRM, False)
    rng = np.random.default_rng(5)
    imgs, rows, truth = [], [], []
    for _ in range(n):
        true = synth.random_angles(1, rng)[0]
        ts = rng.uniform(-2, 2, 2)
        A = np.eye(3)
        A[0, 2], A[1, 2] = -ts
        imgs.append(oracle.apply_geometry2d(res.fp.project(*true), A, 3, False, True).astype(np.float32))
        dang = rng.uniform(2, 3, 3) * rng.choice([-1, 1], 3)
        dsh = rng.uniform(1, 2, 2) * rng.choice([-1, 1], 2)
        rows.append(dict(rot=true[0] + dang[0], tilt=true[1] + dang[1], psi=true[2] + dang[2], shift_x=ts[0] + dsh[0], shift_y=ts[1] + dsh[1]))
        truth.append((true, ts))
    imgs = np.stack(imgs)
    h = xa.ContinuousAssign2(ctx, torch.from_numpy(vol).cuda(), capacity=64, optimize_shift=1, optimize_angles=1, **PRM)
    h.load(imgs, rows)
    start = np.zeros((n, VARS))
    start[:, 0] = 1
    c0 = h.cost(np.arange(n), start)
    X, cost, it, ev, en = h.refine()
    active = [2, 3, 7, 8, 9]
    max_dc, max_dx, ang_better = 0.0, 0.0, 0
    for i in range(n):
        If, sd = res.prepare(imgs[i])

        def f(xc, i=i, If=If, sd=sd):
            x = np.zeros(VARS)
            x[0] = 1
            x[active] = xc
            return res.cost(If, sd, rows[i], x)
        p, fmin, _ = xa.powell_minimize(f, np.zeros(5), np.ones(5), 0.01)
        dc, dx = abs(cost[i] - fmin), np.abs(X[i][active] - p).max()
        max_dc, max_dx = max(max_dc, dc), max(max_dx, dx)
        true, ts = truth[i]
        old = np.array([rows[i]["shift_x"], rows[i]["shift_y"]])
        s0, s1 = np.hypot(*(old - ts)), np.hypot(*(old + X[i][2:4] - ts))
        a0 = np.array([rows[i]["rot"], rows[i]["tilt"], rows[i]["psi"]])
        g0, g1 = _geodesic(oracle, a0, true), _geodesic(oracle, a0 + X[i][7:10], true)
        ang_better += g1 < g0
        print(f"particle {i}: cost {c0[i]:.6f} -> {cost[i]:.6f} (cpu {fmin:.6f}, |d| {dc:.2e}) max|dvar| {dx:.2e} shift err {s0:.3f} -> {s1:.3f} "
              f"angle err {g0:.2f} -> {g1:.2f} evals {ev[i]} iters {it[i]}")
        assert en[i] == 1
        assert dc <= 1e-5 and dx <= 0.05
        assert cost[i] < c0[i]
        assert s1 < s0
    print(f"device-to-CPU maxima: cost {max_dc:.3e}, variables {max_dx:.3e}; angular error improved for {ang_better} of {n}; "
          f"evaluations per particle {ev.min()}..{ev.max()}, iterations {it.min()}..{it.max()}")
    h.close()


def correlation_masked(I1, I2):
    """correlationMasked (filters.cpp:1397-1452): means over the pixels of I1 at or above its standard deviation, sums over those above"""
    th = np.sqrt(abs((I1 * I1).sum() / I1.size - (I1.sum() / I1.size) ** 2))
    ge, gt = I1 >= th, I1 > th
    if not ge.any():
        return 0.0
    a1, a2 = I1[ge].sum() / ge.sum(), I2[ge].sum() / ge.sum()
    p1, p2 = I1[gt] - a1, I2[gt] - a2
    return (p1 * p2).sum() / np.sqrt((p1 * p1).sum() * (p2 * p2).sum())


def imed_distance(I1, I2):
    """imedDistance (filters.cpp:1269-1318) with its weights from their formula"""
    D = I1.shape[0]
    g = np.arange(-3, 4)
    w = np.exp(-0.5 * (g[:, None] ** 2 + g[None, :] ** 2)) / np.sqrt(2 * np.pi)
    d = I1 - I2
    mid = D // 2
    imed = 0.0
    for i in range(3, D - 3):
        for j in range(3, D - 3):
            if (i - mid) ** 2 + (j - mid) ** 2 > mid * mid:
                continue
            imed += (w * d[i - 3:i + 4, j - 3:j + 4]).sum() * d[i, j]
    return np.sqrt(imed)


# ------------------------------------------------------------------ check 6: outputs at the final variables, and apply
@pytest.mark.parametrize("l1", [False, True], ids=["corr", "l1"])
def test_outputs_at_the_final_variables(gpu, oracle, l1):
    xa, ctx, torch = gpu
    D = 32
    vol = synth.phantom(D, seed=11, nblobs=9).astype(np.float32)
    res = Restated(oracle, vol, PRM, l1)
    rng = np.random.default_rng(6)
    imgs, rows = _particles(oracle, vol, 3, rng, res.w1, False)
    h = xa.ContinuousAssign2(ctx, torch.from_numpy(vol).cuda(), capacity=8, optimize_gray=int(l1), optimize_shift=1, optimize_angles=1, **PRM)
    h.load(imgs, rows)
    X, cost, it, ev, en = h.refine()
    again = h.cost(np.arange(3), X)                  # one more evaluation at the returned variables precedes the outputs
    assert np.abs(again - cost).max() <= 1e-12       # Powell's minimum was evaluated at p + t xi, the returned p is p += t xi
    for i in range(3):
        P, E, Ip = (t.cpu().numpy() for t in h.last_images(i))
        If, sd = res.prepare(imgs[i])
        eP, eE, eIp = res.images(If, rows[i], X[i])
        for got, exp in ((P, eP), (E, eE), (Ip, eIp)):
            assert np.abs(got - exp).max() <= 1e-9 * np.abs(exp).max()
        got = h.measures(i)
        exp = (oracle.correlation_index(eP, eIp), correlation_masked(eP, eIp), imed_distance(eP, eIp))
        print(f"particle {i}: corrIdx, corrMask, imed device {got} restated {exp}")
        for g_, e_ in zip(got, exp):
            assert abs(g_ - e_) <= 1e-9
    # apply: the original images through the final transform (BSPLINE3), grey map inside the mask when grey values were optimised
    out = h.apply(imgs, X)
    for i in range(3):
        exp = oracle.apply_geometry2d(imgs[i].astype(np.float64), res.matrix(rows[i], X[i]), 3, False, False)
        if l1:
            exp = np.where(res.mask, (exp - X[i][1]) / X[i][0], 0.0)
        assert np.abs(out[i] - exp).max() <= 3e-7 * np.abs(exp).max()
    with pytest.raises(xa.XhError):
        h.last_images(3)
    h.close()


# ------------------------------------------------------------------ check 6b: every chunk seam of load and apply
def _seam_row(i):
    """a row whose every number is a function of the particle's index: neighbours differ, and so do particles one chunk (16 384,
    32 768) apart. Shifts on a quarter-pixel grid, so that the variables that cancel them are exact."""
    ctf = dict(CTF, DeltafU=12000.0 + (i * 7919) % 6000, azimuthal_angle=float((i * 37) % 180), Ca=0.015 + 0.001 * (i % 11), espr=0.8 + 0.05 * (i % 9),
               ispr=5e-10 * (i % 5), alpha=2e-5 * (1 + i % 4), DeltaF=10.0 + i % 13, DeltaR=0.1 + 0.05 * (i % 7))
    ctf["DeltafV"] = ctf["DeltafU"] + 100.0 + i % 300
    return dict(rot=float((i * 17) % 360), tilt=float((i * 29) % 180), psi=float((i * 41) % 360), shift_x=0.25 * ((i * 13) % 9 - 4),
                shift_y=0.25 * ((i * 7) % 11 - 5), flip=i % 2, ctf=ctf)


def _identity_variables(row):
    """the variables at which the final transform is the identity: they cancel the row's shift, and a flipped row's mirror by a scale
    of -2 along x (A[0][0] = -(1 + scaleX)); every entry of A comes out exact"""
    x = np.zeros(VARS)
    x[0] = 1
    x[2], x[3] = -row["shift_x"], -row["shift_y"]
    if row["flip"]:
        x[4] = -2.0
    return x


def test_every_chunk_seam_of_load_and_apply(gpu, oracle):
    """32 772 particles of 32 x 32 in one load: the load transforms them in chunks of 256 MB / (D^2 16 B) = 16 384 images and evaluates
    their CTF images in launches of 32 768 rows; apply works in chunks of 32 768. At the particles next to every seam the resident
    filtered image, the resident CTF image (a cost that leaves the defocus alone reads it), a cost that evaluates the CTF in its row, and
    the applied image are held to the bounds of test_cost_parity and test_outputs_at_the_final_variables; everywhere else apply
    gets the identity, which copies: one comparison of the whole output finds an image that went to another particle's place.
    Measured on an MI355X: filtered image 4.7e-16 of its largest value, its standard deviation 1.4e-15 relative, costs 3.3e-15 and
    3.4e-15, applied images 4.4e-8 of the largest value."""
    xa, ctx, torch = gpu
    D, n = 32, 32772
    seams = [0, 1, 16383, 16384, 16385, 32767, 32768, 32771]
    assert (256 << 20) // (D * D * 16) == 16384 and min(32768, (256 << 20) // (D * D * 8)) == 32768 and n > 32768 + 1
    prm = dict(PRM, max_shift=4.0)
    vol = synth.phantom(D, seed=11, nblobs=9).astype(np.float32)
    res = Restated(oracle, vol, prm, False)
    imgs = np.random.default_rng(n).standard_normal((n, D, D), dtype=np.float32)
    rows = [_seam_row(i) for i in range(n)]
    h = xa.ContinuousAssign2(ctx, torch.from_numpy(vol).cuda(), capacity=8, optimize_shift=1, optimize_angles=1, optimize_defocus=1, **prm)
    h.load(imgs, _device_rows(rows))
    # the resident filtered images
    prep = {i: res.prepare(imgs[i], rows[i]) for i in seams}
    err_If = err_sd = 0.0
    got_If = {i: h.filtered(i) for i in seams}
    for i in seams:
        err_If = max(err_If, np.abs(got_If[i][0] - prep[i][0]).max() / np.abs(prep[i][0]).max())
        err_sd = max(err_sd, abs(got_If[i][1] - prep[i][1]) / prep[i][1])
    print(f"seams: filtered image max {err_If:.3e} of its largest value (bound 1e-11), standard deviation {err_sd:.3e} relative (bound 1e-12)")
    for i in seams:
        assert np.abs(got_If[i][0] - prep[i][0]).max() <= 1e-11 * np.abs(prep[i][0]).max(), i
        assert abs(got_If[i][1] - prep[i][1]) <= 1e-12 * prep[i][1], i
    # costs: the particle's resident CTF image, then the CTF evaluated in the row
    x = np.zeros(VARS)
    x[0] = 1
    x[2:4] = 0.6, -0.35
    x[7:10] = 1.5, -0.8, 2.1
    moved = x.copy()
    moved[10:13] = 120.0, -80.0, 5.0
    for what, xs in (("resident CTF", x), ("CTF in the row", moved)):
        got = h.cost(seams, np.tile(xs, (len(seams), 1)))
        exp = np.array([res.cost(prep[i][0], prep[i][1], rows[i], xs) for i in seams])
        print(f"seams: cost with the {what}: device {got} max |device - restatement| = {np.abs(got - exp).max():.3e} (bound 1e-9)")
        assert np.all(np.abs(exp) < 1e30) and len(set(np.round(exp, 6))) == len(seams)      # every particle has a cost of its own
        assert np.abs(got - exp).max() <= 1e-9
    # apply: a transform at the seams, the identity everywhere else
    X = np.stack([_identity_variables(r) for r in rows])
    eye = np.eye(3)
    assert all(np.array_equal(res.matrix(rows[i], X[i]), eye) for i in range(n))
    for i in seams:
        X[i] = [1, 0, 0.7, -0.4, 0.01, -0.005, 0.4, 0, 0, 0, 0, 0, 0]
    out = h.apply(imgs, X)
    err = 0.0
    expected = {i: oracle.apply_geometry2d(imgs[i].astype(np.float64), res.matrix(rows[i], X[i]), 3, False, False) for i in seams}
    for i in seams:
        err = max(err, np.abs(out[i] - expected[i]).max() / np.abs(expected[i]).max())
    print(f"seams: applied images max {err:.3e} of the largest value (bound 3e-7)")
    for i in seams:
        assert np.abs(out[i] - expected[i]).max() <= 3e-7 * np.abs(expected[i]).max(), i
        assert np.abs(out[i] - imgs[i]).max() > 0.1
    others = np.ones(n, bool)
    others[seams] = False
    same = (out == imgs).all(axis=(1, 2))
    assert same[others].all(), f"particles whose identity transform is no copy: {np.nonzero(~same & others)[0][:20]}"
    h.close()


# ------------------------------------------------------------------ check 7: the program end to end
def _run_program(tmp, name, batch, extra):
    r = subprocess.run([PROG, "-i", str(tmp / "in.xmd"), "-o", str(tmp / f"{name}.stk"), "--ref", str(tmp / "ref.vol"), "--oresiduals",
                        str(tmp / f"{name}_res.stk"), "--oprojections", str(tmp / f"{name}_proj.stk"), "--batch", str(batch)] + extra,
                       stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=600)
    assert r.returncode == 0, r.stderr
    labels, rows = xmipp_io.read_xmd(str(tmp / f"{name}.xmd"))
    return labels, rows


@pytest.mark.parametrize("l1", [False, True], ids=["corr", "l1"])
def test_program_end_to_end(gpu, oracle, tmp_path, l1):
    xa, ctx, torch = gpu
    D, n = 32, 9
    vol = synth.phantom(D, seed=11, nblobs=9).astype(np.float32)
    rng = np.random.default_rng(7)
    imgs, rows = _particles(oracle, vol, n, rng, 0.25, False)
    imgs[3] = -imgs[3]                       # contrast-inverted: Pearson's sign follows the contrast, its cost is positive everywhere in bounds
    xmipp_io.write_volume(str(tmp_path / "ref.vol"), vol)
    xmipp_io.write_stack(str(tmp_path / "in.stk"), imgs)
    # the L1 run applies the final transform to other images than those it searched with (--applyTo imageOriginal)
    other = (imgs * 0.5 + np.random.default_rng(70).standard_normal(imgs.shape).astype(np.float32)).astype(np.float32)
    xmipp_io.write_stack(str(tmp_path / "other.stk"), other)
    labels = ["imageOriginal", "image", "angleRot", "angleTilt", "anglePsi", "shiftX", "shiftY", "flip", "itemId", "continuousScaleX", "continuousScaleY",
              "continuousX", "continuousY", "continuousFlip"]
    table = []
    for i, r in enumerate(rows):
        r["scale_x"] = 0.05 if i == 6 else 0.0          # particle 6: input scale outside --max_scale
        # the continuous* columns take precedence over shiftX / shiftY / flip (:430-439)
        table.append([f"{i + 1}@{tmp_path / 'other.stk'}", f"{i + 1}@{tmp_path / 'in.stk'}", r["rot"], r["tilt"], r["psi"], 99.0, -99.0, 1, 100 + i, r["scale_x"], 0.0, r["shift_x"],
                      r["shift_y"], 0])
    xmipp_io.write_xmd(str(tmp_path / "in.xmd"), [("noname", labels, table)])
    flags = ["--optimizeShift", "--optimizeAngles", "--max_shift", "4"] + (["--optimizeGray", "--applyTo", "imageOriginal"] if l1 else [])
    lab, out = _run_program(tmp_path, "big", 4096, flags)
    lab5, out5 = _run_program(tmp_path, "small", 5, flags)
    assert lab5 == lab and out5 != [] and len(out5) == len(out)
    for a, b in zip(out, out5):
        assert [v.replace("small", "big") for v in b] == a
    for suffix in ("", "_res", "_proj"):
        assert np.array_equal(xmipp_io.read_stack(str(tmp_path / f"big{suffix}.stk")), xmipp_io.read_stack(str(tmp_path / f"small{suffix}.stk")))
    # the library on the same input
    h = xa.ContinuousAssign2(ctx, torch.from_numpy(vol).cuda(), capacity=16, optimize_shift=1, optimize_angles=1, optimize_gray=int(l1),
                             **dict(PRM, max_shift=4.0))
    h.load(imgs, rows)
    X, cost, it, ev, en = h.refine()
    expect_gone = {6} | (set() if l1 else {3})
    assert {i for i in range(n) if en[i] != 1} == expect_gone
    col = {l: k for k, l in enumerate(lab)}
    for l in labels + ["imageOriginal", "cost", "weightContinuous2", "continuousScaleAngle", "corrIdx", "corrMask", "corrWeight", "imedValue",
                       "imageResidual", "imageRef"] + (["continuousA", "continuousB"] if l1 else []):
        assert l in col, l
    ids = [int(r[col["itemId"]]) - 100 for r in out]
    assert ids == [i for i in range(n) if i not in expect_gone]          # disabled rows removed, input columns kept
    shown = np.array([-c if not l1 else c for c in cost])
    best = shown[ids].min() if l1 else shown[ids].max()
    stack, res, proj = (xmipp_io.read_stack(str(tmp_path / f"big{sfx}.stk")) for sfx in ("", "_res", "_proj"))
    applied = h.apply(other if l1 else imgs, X)
    for r, i in zip(out, ids):
        def val(l):
            return float(r[col[l]])
        assert r[col["image"]] == f"{i + 1}@{tmp_path / 'big.stk'}" and r[col["imageOriginal"]] == f"{i + 1}@{tmp_path / 'in.stk'}"
        assert abs(val("angleRot") - (rows[i]["rot"] + X[i][7])) <= 1e-6 and abs(val("angleTilt") - (rows[i]["tilt"] + X[i][8])) <= 1e-6
        assert abs(val("anglePsi") - (rows[i]["psi"] + X[i][9])) <= 1e-6
        assert val("shiftX") == 0 and val("shiftY") == 0 and val("flip") == 0 and val("continuousFlip") == 0
        assert abs(val("continuousX") - (rows[i]["shift_x"] + X[i][2])) <= 1e-6 and abs(val("continuousY") - (rows[i]["shift_y"] + X[i][3])) <= 1e-6
        assert abs(val("cost") - shown[i]) <= 1e-6
        assert abs(val("weightContinuous2") - (best / shown[i] if l1 else shown[i] / best)) <= 1e-6
        assert val("corrWeight") == 0
        if l1:
            assert abs(val("continuousA") - X[i][0]) <= 1e-6 and abs(val("continuousB") - X[i][1]) <= 1e-6
        h.cost([i], X[i][None])
        m = h.measures(0)
        assert abs(val("corrIdx") - m[0]) <= 1e-6 and abs(val("corrMask") - m[1]) <= 1e-6 and abs(val("imedValue") - m[2]) <= 1e-6
        P, E, _ = (t.cpu().numpy() for t in h.last_images(0))
        assert np.array_equal(proj[i], P.astype(np.float32)) and np.array_equal(res[i], E.astype(np.float32))
        assert np.array_equal(stack[i], applied[i])
    assert not stack[6].any() and not proj[6].any() and (l1 or not proj[3].any())
    h.close()


# ------------------------------------------------------------------ check 8: handle hygiene, loud errors
def _held():
    from xmipp3_amd import _lib
    v = C.c_int64()
    assert _lib.lib().xh_device_bytes_held(C.byref(v)) == 0
    return v.value


def test_destroy_returns_every_byte_and_failed_create_leaves_nothing(gpu, oracle):
    xa, ctx, torch = gpu
    D = 32
    vol = torch.from_numpy(synth.phantom(D, seed=2, nblobs=5).astype(np.float32)).cuda()
    gc.collect()
    ctx.sync()
    before = _held()
    h = xa.ContinuousAssign2(ctx, vol, capacity=8, optimize_shift=1, **PRM)
    h.load(np.random.default_rng(0).standard_normal((5, D, D)).astype(np.float32))
    h.refine()
    assert _held() > before
    h.close()
    assert _held() == before
    big = torch.zeros((520, 520, 520), device="cuda")          # padded to 1040, above the projector's 1024
    with pytest.raises(xa.XhError):
        xa.ContinuousAssign2(ctx, big, capacity=8, optimize_shift=1, **PRM)
    assert _held() == before


def test_errors_are_loud(gpu):
    xa, ctx, torch = gpu
    D = 16
    vol = torch.zeros((D, D, D), device="cuda")
    h = xa.ContinuousAssign2(ctx, vol, capacity=2, optimize_shift=1, **PRM)
    with pytest.raises(xa.XhError):
        h.load(np.zeros((1, D, D + 2), np.float32))            # not square
    with pytest.raises(xa.XhError):
        h.load(np.zeros((1, D + 4, D + 4), np.float32))        # not the volume's size
    with pytest.raises(xa.XhError):
        h.refine()                                             # nothing loaded
    h.load(np.zeros((1, D, D), np.float32))
    with pytest.raises(xa.XhError):
        h.cost([1], np.zeros((1, VARS)))                       # no such particle
    h.close()
    h = xa.ContinuousAssign2(ctx, vol, capacity=2, **PRM)
    h.load(np.zeros((1, D, D), np.float32))
    with pytest.raises(xa.XhError):
        h.refine()                                             # nothing to optimise
    h.close()
