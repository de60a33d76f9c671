"""GPU parity of xmipp_volume_halves_restoration (xh_halves_*) against a numpy fp64 restatement of the reference's GPU restorator
(VolumeHalvesRestorator<double>: cuda_volume_halves_restorator.cpp, cuda_volume_restoration_kernels.{cpp,cu}, cuda_cdf.{cpp,cu}),
kept in this file: np.fft.rfftn / irfftn with the same un-normalised convention, np.sort for the CDF. Plus the program end to end."""
import math
import os
import subprocess

import numpy as np
import pytest

from tests import xmipp_io

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PROG = os.path.join(ROOT, "xmipp3_amd", "bin", "xmipp_volume_halves_restoration")
SHAPES = [(32, 32, 32), (33, 40, 36), (64, 64, 64)]


@pytest.fixture(scope="module")
def gpu():
    import torch
    import xmipp3_amd as xa
    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    return xa, xa.Context(0), torch


# ---------------------------------------------------------------- the restatement
def r2_of(shape):
    Z, Y, X = shape

    def dig(n, size):
        i = np.arange(n)
        return np.zeros(n) if size <= 1 else np.where(i <= (size >> 1), i, i - size) / float(size)
    fz, fy, fx = dig(Z, Z), dig(Y, Y), dig(X // 2 + 1, X)
    return fx[None, None, :] * fx[None, None, :] + fy[None, :, None] * fy[None, :, None] + fz[:, None, None] * fz[:, None, None]


def fft(v):
    return np.fft.rfftn(v)


def ifft(F, shape, scale=1.0):
    return np.fft.irfftn(F, s=shape, axes=(0, 1, 2), norm="forward") * scale


def probs():
    p, out = 0.005 / 2, []
    while p < 1:
        out.append(p)
        p += 0.005
    return np.array(out)


PROBS = probs()


def cdf_table(keys):
    """Gpu::CDF: [min, the 200 order statistics at round(p N) (half away from zero; N - 1 at most), max]"""
    v = np.sort(np.asarray(keys, np.float64).ravel())
    N = v.size
    idx = []
    for p in PROBS:
        x = p * N
        r = math.floor(x)
        idx.append(min(r + (1 if x - r >= 0.5 else 0), N - 1))
    return np.concatenate([[v[0]], v[idx], [v[-1]]])


def cdf_prob(xi, t):
    """Gpu::getCDFProbability, its binary search run on all elements at once"""
    mn, mx, x, p, N = t[0], t[-1], t[1:-1], PROBS, 200
    xi = np.asarray(xi, np.float64)
    out = np.zeros_like(xi)

    def interp(x_, x0, y0, xF, yF):
        return y0 + ((x_ - x0) * (yF - y0)) / (xF - x0)
    with np.errstate(all="ignore"):
        done = np.zeros(xi.shape, bool)
        for cond, val in ((xi > mx, 1.0), (xi < mn, 0.0)):
            m = cond & ~done
            out[m] = val
            done |= m
        m = (xi < x[0]) & ~done
        out[m] = interp(xi[m], mn, 0.0, x[0], p[0])
        done |= m
        m = (xi > x[N - 1]) & ~done
        out[m] = interp(xi[m], x[N - 1], p[N - 1], mx, 1.0)
        done |= m
        L = np.zeros(xi.shape, np.int64)
        R = np.full(xi.shape, N - 1, np.int64)
        act = ~done
        while act.any():
            M = L + (R - L) // 2
            M1 = np.minimum(M + 1, N - 1)
            xm, xm1 = x[M], x[M1]
            hit = act & (xi >= xm) & (xi <= xm1)
            val = np.where(xm == xm1, 0.5 * (p[M] + p[M1]), interp(xi, xm, p[M], xm1, p[M1]))
            out[hit] = val[hit]
            act &= ~hit
            lt = act & (xi < xm)
            R = np.where(lt, M, R)
            L = np.where(act & ~lt, M, L)
    return out


def estimate_s(V1, V2, mask):
    val = 0.5 * (V1 + V2)
    S = np.where((val <= 0) | ((mask == 0) if mask is not None else False), 0.0, val)
    F = fft(S)
    F[r2_of(S.shape) > 0.25] = 0
    return ifft(F, S.shape, 1.0 / S.size)


def denoise(V1, V2, iters, mask=None):
    V1, V2 = V1.copy(), V2.copy()
    for _ in range(iters):
        S = estimate_s(V1, V2, mask)
        tS = cdf_table((S * S)[mask != 0] if mask is not None else S * S)
        for V in (V1, V2):
            d = V - S
            tN = cdf_table(1.0 * d * d)
            e = V * V
            pN = cdf_prob(e, tN)
            m = pN < 1
            V[m] = (pN * cdf_prob(e, tS))[m] * V[m]
    return V1, V2


def spectra(V1, V2):
    S = estimate_s(V1, V2, None)
    return S, fft(S), fft(V1), fft(V2)


def sigma_cost(fVol, fV1, fV2, s1, s2, shape):
    R2 = r2_of(shape)
    K1, K2 = -0.5 / (s1 * s1), -0.5 / (s2 * s2)
    inv = 1.0 / (2 * float(fVol.size))
    m = R2 <= 0.25
    H1, H2 = np.exp(K1 * R2[m]), np.exp(K2 * R2[m])
    f, a, b = fVol[m], fV1[m], fV2[m]
    d1 = (f * H1 - a) * inv
    d2 = (f * H2 - b) * inv
    return float(np.sum(np.sqrt(d1.real ** 2 + d1.imag ** 2) + np.sqrt(d2.real ** 2 + d2.imag ** 2)))


def deconvolve(V1, V2, sigmas, lam):
    shape, inv = V1.shape, 1.0 / V1.size
    R2 = r2_of(shape)
    m = R2 <= 0.25
    for s1, s2 in sigmas:
        S, fVol, fV1, fV2 = spectra(V1, V2)
        K1, K2 = -0.5 / (s1 * s1), -0.5 / (s2 * s2)
        H1, H2 = np.exp(K1 * R2[m]), np.exp(K2 * R2[m])
        den = H1 * H1 + H2 * H2 + lam * R2[m]
        a, b = fV1[m], fV2[m]
        fVol[m] = (H1 * a.real + H2 * b.real) / den + 1j * ((H1 * a.imag + H2 * b.imag) / den)
        fV1[m] = a * (1.0 / H1)
        fV2[m] = b * (1.0 / H2)
        V1, V2 = ifft(fV1, shape, inv), ifft(fV2, shape, inv)
    sc = (sigmas[-1][0] + sigmas[-1][1]) / 2
    fVol[m] *= np.exp(-0.5 / (sc * sc) * R2[m])
    return V1, V2, S, ifft(fVol, shape, inv)


def filter_bank(V1, V2, step, overlap, wfun, wpow):
    shape, inv = V1.shape, 1.0 / V1.size
    R2 = r2_of(shape)
    F1, F2 = fft(V1 * inv), fft(V2 * inv)
    fstep = step * (1 - overlap)
    V1r, V2r, S = np.zeros(shape), np.zeros(shape), np.zeros(shape)
    w = 0.0
    with np.errstate(all="ignore"):
        while w < 0.5:
            band = (R2 >= w * w) & (R2 < (w + step) * (w + step))
            f1, f2 = ifft(np.where(band, F1, 0), shape), ifft(np.where(band, F2, 0), shape)
            d = f1 - f2
            t = cdf_table(0.5 * d * d)
            e1, e2 = f1 * f1, f2 * f2
            w1, w2 = cdf_prob(e1, t), cdf_prob(e2, t)
            if wfun == 0:
                wt = 0.5 * (w1 + w2)
            elif wfun == 1:
                wt = np.minimum(w1, w2)
            elif wfun == 2:
                wt = np.where(w1 + w2 == 0, 0.0, 0.5 * (w1 + w2) * (1 - np.abs(w1 - w2) / (w1 + w2)))
            else:
                wt = np.zeros(shape)
            wt = np.power(wt, float(int(wpow)))
            V1r += f1 * wt
            V2r += f2 * wt
            S += np.where(e1 > e2, f1 * wt, f2 * wt)
            w += fstep
    c = 1 - overlap
    return S * c, V1r * c, V2r * c


def difference(V1, V2, iters, K, mask=None):
    for _ in range(iters):
        D, S = V1 - V2, (V1 + V2) * 0.5
        sel = D[mask != 0] if mask is not None else D.ravel()
        size = sel.size
        avg, std = sel.sum() / size, (sel * sel).sum()
        if size > 1:
            std = std / size - avg * avg
            std *= size / (size - 1)
            std = math.sqrt(abs(std))
        else:
            std = 0.0
        std *= K
        with np.errstate(all="ignore"):
            k = -0.5 / (std * std) if std != 0 else -np.inf
            w = np.exp(k * D * D)
        if np.isinf(k):
            w[D == 0] = 0.0
        V1, V2 = S + (V1 - S) * w, S + (V2 - S) * w
    return V1, V2, (V1 + V2) * 0.5


# ---------------------------------------------------------------- data
def halves(shape, seed=0):
    """a band-limited positive phantom (Gaussian blobs) plus independent noise per half"""
    rng = np.random.default_rng(seed)
    Z, Y, X = shape
    z, y, x = np.meshgrid(np.arange(Z) - Z // 2, np.arange(Y) - Y // 2, np.arange(X) - X // 2, indexing="ij")
    ph = np.zeros(shape)
    for _ in range(6):
        c = rng.uniform(-0.25, 0.25, 3) * np.array(shape)
        s = rng.uniform(1.5, 4.0)
        ph += rng.uniform(0.5, 1.5) * np.exp(-((z - c[0]) ** 2 + (y - c[1]) ** 2 + (x - c[2]) ** 2) / (2 * s * s))
    return ph + 0.15 * rng.standard_normal(shape), ph + 0.15 * rng.standard_normal(shape)


def _close(got, exp, rel=1e-9):
    got, exp = np.asarray(got), np.asarray(exp)
    assert got.shape == exp.shape
    assert not np.isnan(got).any()
    peak = np.abs(exp).max()
    err = np.abs(got - exp).max()
    assert err <= rel * peak, (err, peak)


def _handle(gpu, V1, V2):
    xa, ctx, torch = gpu
    h = xa.HalvesRestoration(ctx, V1.shape)
    h.load(torch.from_numpy(V1).cuda(), torch.from_numpy(V2).cuda())
    return h


def _np(t):
    return t.cpu().numpy()


# ---------------------------------------------------------------- transforms and CDF
@pytest.mark.parametrize("shape", SHAPES + [(1, 20, 18), (7, 1, 9)])
def test_fft_roundtrip(gpu, shape):
    xa, ctx, torch = gpu
    v = np.random.default_rng(1).standard_normal(shape)
    h = xa.HalvesRestoration(ctx, shape)
    F = h.rfft(torch.from_numpy(v).cuda())
    exp = np.fft.rfftn(v)
    assert np.abs(_np(F) - exp).max() <= 1e-12 * np.abs(exp).max()
    back = h.irfft(F, 1.0 / v.size)
    assert np.abs(_np(back) - v).max() <= 1e-12 * np.abs(v).max()
    # the un-normalised inverse of an arbitrary half spectrum, against numpy's
    G = np.fft.rfftn(np.random.default_rng(2).standard_normal(shape))
    got = _np(h.irfft(torch.from_numpy(G).cuda()))
    ref = np.fft.irfftn(G, s=shape, axes=(0, 1, 2), norm="forward")
    assert np.abs(got - ref).max() <= 1e-12 * np.abs(ref).max()


def _cdf_inputs(shape):
    rng = np.random.default_rng(3)
    yield rng.standard_normal(shape)                                   # distinct values
    yield rng.integers(0, 4, shape) * 0.5                              # many ties, a quarter zeros
    yield np.where(rng.random(shape) < 0.9, 0.0, rng.standard_normal(shape))   # mostly zeros
    yield np.full(shape, 1.25)                                         # one value
    yield rng.standard_normal(shape) * np.exp(rng.uniform(-300, 300, shape))   # the whole exponent range


@pytest.mark.parametrize("shape", SHAPES)
def test_cdf_order_statistics_bit_exact(gpu, shape):
    xa, ctx, torch = gpu
    h = xa.HalvesRestoration(ctx, shape)
    rng = np.random.default_rng(4)
    b = rng.standard_normal(shape)
    mask = xa.halves_circular_mask(shape, -min(shape) / 3)
    small = np.zeros(shape, np.int32)
    small.ravel()[rng.choice(small.size, 150, replace=False)] = 1     # N < 200: ranks clamp to N - 1
    for a in _cdf_inputs(shape):
        ta, tb = torch.from_numpy(a).cuda(), torch.from_numpy(b).cuda()
        got = h.cdf(ta)
        assert np.array_equal(got.view(np.uint64), cdf_table(a * a).view(np.uint64))
        got = h.cdf(ta, mask=torch.from_numpy(mask).cuda())
        assert np.array_equal(got.view(np.uint64), cdf_table((a * a)[mask != 0]).view(np.uint64))
        got = h.cdf(ta, mask=torch.from_numpy(small).cuda())
        assert np.array_equal(got.view(np.uint64), cdf_table((a * a)[small != 0]).view(np.uint64))
        d = a - b
        got = h.cdf(ta, tb, mult=0.5)
        assert np.array_equal(got.view(np.uint64), cdf_table(0.5 * d * d).view(np.uint64))


def test_empty_mask_is_refused(gpu):
    xa, ctx, torch = gpu
    shape = (16, 16, 16)
    V1, V2 = halves(shape)
    h = _handle(gpu, V1, V2)
    with pytest.raises(xa.XhError, match="empty"):
        h.denoise(1, torch.zeros(shape, dtype=torch.int32, device="cuda"))


# ---------------------------------------------------------------- stages
@pytest.mark.parametrize("shape", SHAPES)
@pytest.mark.parametrize("masked", [False, True])
def test_denoise(gpu, shape, masked):
    xa, ctx, torch = gpu
    V1, V2 = halves(shape)
    mask = xa.halves_circular_mask(shape, -min(shape) / 3) if masked else None
    h = _handle(gpu, V1, V2)
    h.denoise(2, None if mask is None else torch.from_numpy(mask).cuda())
    e1, e2 = denoise(V1, V2, 2, mask)
    _close(_np(h.output("restored1")), e1)
    _close(_np(h.output("restored2")), e2)
    for name in ("filterBank", "deconvolved", "convolved", "avgDiff"):
        assert h.output(name) is None


@pytest.mark.parametrize("shape", SHAPES)
def test_sigma_cost_grid(gpu, shape):
    V1, V2 = halves(shape)
    h = _handle(gpu, V1, V2)
    h.deconv_spectra()
    _, fVol, fV1, fV2 = spectra(V1, V2)
    for s1 in (0.05, 0.2, 0.7, 1.9):
        for s2 in (0.1, 0.5, 1.3):
            exp = sigma_cost(fVol, fV1, fV2, s1, s2, shape)
            assert abs(h.sigma_cost(s1, s2) - exp) <= 1e-12 * abs(exp)


@pytest.mark.parametrize("shape", SHAPES)
def test_deconvolve(gpu, shape):
    V1, V2 = halves(shape)
    h = _handle(gpu, V1, V2)
    sig = h.deconvolve(2, 0.2, 0.001)
    assert sig.shape == (2, 2) and np.all((sig >= 0) & (sig <= 2))
    e1, e2, eS, eC = deconvolve(V1, V2, [tuple(s) for s in sig], 0.001)
    _close(_np(h.output("restored1")), e1)
    _close(_np(h.output("restored2")), e2)
    _close(_np(h.output("deconvolved")), eS)
    _close(_np(h.output("convolved")), eC)


@pytest.mark.parametrize("shape", SHAPES)
@pytest.mark.parametrize("wfun", [0, 1, 2, 3])
def test_filter_bank(gpu, shape, wfun):
    V1, V2 = halves(shape)
    h = _handle(gpu, V1, V2)
    step = 0.01 if shape == (32, 32, 32) else 0.04
    h.filter_bank(step, 0.5, wfun, 3.7)          # weightPower truncated to 3, as the reference's power(double, int)
    eS, e1, e2 = filter_bank(V1, V2, step, 0.5, wfun, 3.7)
    _close(_np(h.output("filterBank")), eS)
    _close(_np(h.output("restored1")), e1)
    _close(_np(h.output("restored2")), e2)


def test_filter_bank_zero_over_zero(gpu):
    """weightFun 2 where w1 + w2 = 0: in band 0 both halves' energies lie below every squared difference (V2 = V1 + 1 with mean(V1) =
    -1/2), so w1 = w2 = 0 at every voxel; the reference divides 0 by 0 there. The weight is 0."""
    shape = (16, 16, 16)
    rng = np.random.default_rng(5)
    V1 = rng.standard_normal(shape)
    V1 += -0.5 - V1.mean()
    V2 = V1 + 1.0
    h = _handle(gpu, V1, V2)
    h.filter_bank(0.05, 0.5, 2, 3)
    eS, e1, e2 = filter_bank(V1, V2, 0.05, 0.5, 2, 3)
    _close(_np(h.output("filterBank")), eS)
    _close(_np(h.output("restored1")), e1)


@pytest.mark.parametrize("shape", SHAPES)
@pytest.mark.parametrize("masked", [False, True])
def test_difference(gpu, shape, masked):
    xa, ctx, torch = gpu
    V1, V2 = halves(shape)
    mask = xa.halves_circular_mask(shape, min(shape) / 4) if masked else None
    h = _handle(gpu, V1, V2)
    h.difference(2, 1.5, None if mask is None else torch.from_numpy(mask).cuda())
    e1, e2, eA = difference(V1, V2, 2, 1.5, mask)
    _close(_np(h.output("restored1")), e1)
    _close(_np(h.output("restored2")), e2)
    _close(_np(h.output("avgDiff")), eA)


def test_difference_of_equal_halves(gpu):
    """V1 = V2: the standard deviation is 0 and the reference's weight is exp(-inf * 0) = NaN. The weight is 0: the average comes out."""
    V = halves((16, 16, 16))[0]
    h = _handle(gpu, V, V.copy())
    h.difference(1, 1.5)
    for name in ("restored1", "restored2", "avgDiff"):
        got = _np(h.output(name))
        assert not np.isnan(got).any()
        assert np.array_equal(got, (V + V) * 0.5)


# ---------------------------------------------------------------- the handle
def test_timed_filter_bank_changes_no_byte(gpu):
    """set_timing(True) puts four events and a wait into every band: the three outputs keep their bytes and band_timing reports the
    bands and three times. filter_bank resets them, set_timing does not"""
    xa, ctx, torch = gpu
    shape = (33, 40, 36)
    d1, d2 = (torch.from_numpy(v).cuda() for v in halves(shape))
    h = xa.HalvesRestoration(ctx, shape)

    def run():
        h.load(d1, d2)
        h.filter_bank(0.04, 0.5, 1, 3.0)
        return [_np(h.output(name)).tobytes() for name in ("filterBank", "restored1", "restored2")]

    out = run()
    bands, ms = h.band_timing()
    assert bands == 25 and not ms.any()                         # w = 0, 0.02 .. < 0.5; an untimed run reports no time
    h.set_timing(True)
    out_t = run()
    bands_t, ms_t = h.band_timing()
    print(f"{bands_t} bands, transforms / cdf / weights ms: {ms_t}")
    assert out_t == out and bands_t == bands
    assert ms_t.shape == (3,) and (ms_t >= 0).all() and ms_t.sum() > 0
    h.set_timing(False)
    assert np.array_equal(h.band_timing()[1], ms_t)             # the switch alone resets nothing
    assert run() == out
    bands_u, ms_u = h.band_timing()
    assert bands_u == bands and not ms_u.any()
    h.close()


def test_wrong_tensor_is_refused(gpu):
    """a tensor of another shape or type, or one that is not contiguous, is an XhError before its pointer reaches the library: for the
    volumes, and for the int32 masks, which a float64 tensor of the right shape is not"""
    xa, ctx, torch = gpu
    shape = (16, 18, 20)
    Z, Y, X = shape
    dv = torch.from_numpy(halves(shape)[0]).cuda()
    dm = torch.from_numpy(xa.halves_circular_mask(shape, -5)).cuda()
    h = xa.HalvesRestoration(ctx, shape)
    h.load(dv, dv)

    def wrong(good):
        other = torch.float32 if good.dtype == torch.float64 else torch.float64
        return [torch.zeros((Z, Y, X - 2), dtype=good.dtype, device="cuda"), good.to(other),
                torch.zeros((Z, Y, 2 * X), dtype=good.dtype, device="cuda")[:, :, ::2]]

    for bad in wrong(dv):
        for call in (lambda: h.load(bad, dv), lambda: h.load(dv, bad), lambda: h.rfft(bad), lambda: h.cdf(bad), lambda: h.cdf(dv, bad)):
            with pytest.raises(xa.XhError, match="HalvesRestoration: the volume"):
                call()
    for bad in wrong(dm) + [dv]:
        for call in (lambda: h.denoise(1, bad), lambda: h.difference(1, 1.5, bad), lambda: h.cdf(dv, mask=bad)):
            with pytest.raises(xa.XhError, match="HalvesRestoration: the mask"):
                call()
    with pytest.raises(xa.XhError, match="int32"):
        h.denoise(1, dv)
    h.denoise(1, dm)                                            # the handle still works
    h.close()


def test_close_with_work_in_flight(gpu):
    """close() right behind a launch: the handle waits for its stream before its buffers and events go"""
    xa, ctx, torch = gpu
    shape = (33, 40, 36)
    d1, d2 = (torch.from_numpy(v).cuda() for v in halves(shape))
    h = xa.HalvesRestoration(ctx, shape)
    h.load(d1, d2)
    h.denoise(1)
    h.close()
    assert h.h is None
    h2 = _handle(gpu, *halves(shape))                           # the context is in order: the next handle computes
    h2.denoise(1)
    e1, _ = denoise(*halves(shape), 1)
    _close(_np(h2.output("restored1")), e1)


# ---------------------------------------------------------------- stages past the grid cap
# Every per-voxel kernel and reduction runs on min(ceil(NF / 256), 4 CUs) workgroups of 256 and walks the rest in a grid-stride loop.
# (81, 80, 82): NF = 81 * 80 * 42 = 272 160 half-spectrum elements and N = 531 360 voxels, between one and two passes of 1024 threads
# per CU on 256 CUs, non-cubic with an odd dimension: the loops over the half spectrum take a second, partial pass (those over the
# voxels, on the same grid, a third; they already took a second in the shapes above).
# The restatements, the data and the tolerances are those of the per-stage tests above.
BIG = (81, 80, 82)


@pytest.fixture(scope="module")
def big(gpu):
    xa, ctx, torch = gpu
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    NF = BIG[0] * BIG[1] * (BIG[2] // 2 + 1)
    print(f"{BIG}: {NF} half-spectrum elements on {cus} CUs, grid cap {256 * 4 * cus} threads")
    assert NF > 256 * 4 * cus, f"{NF} half-spectrum elements do not exceed the grid cap of {256 * 4 * cus} threads on {cus} CUs"
    return halves(BIG)


def _report(what, got, exp):
    got, exp = np.asarray(got), np.asarray(exp)
    print(f"{BIG} {what}: max |device - numpy| = {np.abs(got - exp).max() / np.abs(exp).max():.3e} of the largest value")


def test_sigma_cost_grid_past_the_cap(gpu, big):
    """test_sigma_cost_grid's sigmas to its 1e-12 relative; and the same arguments twice give the same bits: 1024 partial sums on 256
    CUs, four per thread of the final workgroup, added in a fixed order. Measured on an MI355X: at most 5.6e-16 relative."""
    V1, V2 = big
    h = _handle(gpu, V1, V2)
    h.deconv_spectra()
    _, fVol, fV1, fV2 = spectra(V1, V2)
    worst = 0.0
    for s1 in (0.05, 0.2, 0.7, 1.9):
        for s2 in (0.1, 0.5, 1.3):
            exp = sigma_cost(fVol, fV1, fV2, s1, s2, BIG)
            got = h.sigma_cost(s1, s2)
            worst = max(worst, abs(got - exp) / abs(exp))
            print(f"{BIG} sigma_cost({s1}, {s2}): device {got!r} numpy {exp!r} relative {abs(got - exp) / abs(exp):.3e}")
            assert np.float64(h.sigma_cost(s1, s2)).tobytes() == np.float64(got).tobytes()
            assert abs(got - exp) <= 1e-12 * abs(exp)
    print(f"{BIG} sigma_cost: largest relative error {worst:.3e} (bound 1e-12)")


def test_deconvolve_past_the_cap(gpu, big):
    """test_deconvolve at its 1e-9 of the largest value. Measured on an MI355X: at most 1.6e-15."""
    V1, V2 = big
    h = _handle(gpu, V1, V2)
    sig = h.deconvolve(2, 0.2, 0.001)
    assert sig.shape == (2, 2) and np.all((sig >= 0) & (sig <= 2))
    e1, e2, eS, eC = deconvolve(V1, V2, [tuple(s) for s in sig], 0.001)
    pairs = [(name, _np(h.output(name)), e) for name, e in (("restored1", e1), ("restored2", e2), ("deconvolved", eS), ("convolved", eC))]
    for name, got, e in pairs:
        _report("deconvolve " + name, got, e)
    for name, got, e in pairs:
        _close(got, e)


@pytest.mark.parametrize("masked", [False, True])
def test_denoise_past_the_cap(gpu, big, masked):
    """test_denoise at its 1e-9 of the largest value. Measured on an MI355X: at most 1.5e-16."""
    xa, ctx, torch = gpu
    V1, V2 = big
    mask = xa.halves_circular_mask(BIG, -min(BIG) / 3) if masked else None
    h = _handle(gpu, V1, V2)
    h.denoise(2, None if mask is None else torch.from_numpy(mask).cuda())
    e1, e2 = denoise(V1, V2, 2, mask)
    g1, g2 = _np(h.output("restored1")), _np(h.output("restored2"))
    _report(f"denoise masked={masked} restored1", g1, e1)
    _report(f"denoise masked={masked} restored2", g2, e2)
    _close(g1, e1)
    _close(g2, e2)


@pytest.mark.parametrize("masked", [False, True])
def test_difference_past_the_cap(gpu, big, masked):
    """test_difference at its 1e-9 of the largest value. Measured on an MI355X: at most 1.5e-16."""
    xa, ctx, torch = gpu
    V1, V2 = big
    mask = xa.halves_circular_mask(BIG, min(BIG) / 4) if masked else None
    h = _handle(gpu, V1, V2)
    h.difference(2, 1.5, None if mask is None else torch.from_numpy(mask).cuda())
    exp = difference(V1, V2, 2, 1.5, mask)
    got = [_np(h.output(name)) for name in ("restored1", "restored2", "avgDiff")]
    for name, g, e in zip(("restored1", "restored2", "avgDiff"), got, exp):
        _report(f"difference masked={masked} {name}", g, e)
    for g, e in zip(got, exp):
        _close(g, e)


def test_filter_bank_past_the_cap(gpu, big):
    """test_filter_bank with weight function 1 and a step of 0.125 (8 bands at overlap 0.5) at its 1e-9 of the largest value.
    Measured on an MI355X: at most 9.1e-16."""
    V1, V2 = big
    h = _handle(gpu, V1, V2)
    h.filter_bank(0.125, 0.5, 1, 3.7)
    exp = filter_bank(V1, V2, 0.125, 0.5, 1, 3.7)
    got = [_np(h.output(name)) for name in ("filterBank", "restored1", "restored2")]
    for name, g, e in zip(("filterBank", "restored1", "restored2"), got, exp):
        _report("filter_bank " + name, g, e)
    for g, e in zip(got, exp):
        _close(g, e)


@pytest.mark.parametrize("shape", SHAPES)
def test_chain(gpu, shape):
    xa, ctx, torch = gpu
    V1, V2 = halves(shape, 7)
    mask = xa.halves_circular_mask(shape, -min(shape) / 3)
    tm = torch.from_numpy(mask).cuda()
    h = _handle(gpu, V1, V2)
    h.denoise(2, tm)
    sig = h.deconvolve(2, 0.2, 0.001)
    h.filter_bank(0.05, 0.5, 1, 3)
    h.difference(2, 1.5, tm)
    a, b = denoise(V1, V2, 2, mask)
    a, b, eS, eC = deconvolve(a, b, [tuple(s) for s in sig], 0.001)
    eF, a, b = filter_bank(a, b, 0.05, 0.5, 1, 3)
    a, b, eA = difference(a, b, 2, 1.5, mask)
    for name, e in (("restored1", a), ("restored2", b), ("filterBank", eF), ("deconvolved", eS), ("convolved", eC), ("avgDiff", eA)):
        _close(_np(h.output(name)), e)


# ---------------------------------------------------------------- the program
def _run(args, timeout=600):
    return subprocess.run([PROG] + args, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=timeout)


OUTS = ("restored1", "restored2", "filterBank", "deconvolved", "convolved", "avgDiff")


def _program_vs_handle(gpu, tmp, shape, stages, mask_args=(), mask=None, seed=0):
    """the program's outputs equal the handle's, run on the same float32 inputs with the same stages, bit for bit after the
    program's float32 write; absent outputs are not written"""
    xa, ctx, torch = gpu
    V1, V2 = (v.astype(np.float32) for v in halves(shape, seed))
    xmipp_io.write_volume(str(tmp / "h1.vol"), V1)
    xmipp_io.write_volume(str(tmp / "h2.vol"), V2)
    root = str(tmp / "out")
    args = ["--i1", str(tmp / "h1.vol"), "--i2", str(tmp / "h2.vol"), "--oroot", root]
    for k, v in stages.items():
        args += ["--" + k] + [str(x) for x in v]
    r = _run(args + list(mask_args))
    assert r.returncode == 0, r.stderr
    h = _handle(gpu, V1.astype(np.float64), V2.astype(np.float64))
    tm = None if mask is None else torch.from_numpy(mask).cuda()
    if "denoising" in stages:
        h.denoise(stages["denoising"][0], tm)
    if "deconvolution" in stages:
        h.deconvolve(*stages["deconvolution"])
    if "filterBank" in stages:
        h.filter_bank(*stages["filterBank"])
    if "difference" in stages:
        h.difference(*stages["difference"], mask=tm)
    for name in OUTS:
        exp = h.output(name)
        path = f"{root}_{name}.vol"
        if exp is None:
            assert not os.path.exists(path), path
        else:
            got = xmipp_io.read_volume(path)
            assert got.shape == shape
            assert np.array_equal(got, _np(exp).astype(np.float32)), name


def test_program_all_stages(gpu, tmp_path):
    _program_vs_handle(gpu, tmp_path, (32, 32, 32), {"denoising": [2], "deconvolution": [2, 0.2, 0.001], "filterBank": [0.05, 0.5, 1, 3],
                                                      "difference": [2, 1.5]})


def test_program_skipped_stages_write_nothing(gpu, tmp_path):
    _program_vs_handle(gpu, tmp_path, (32, 32, 32), {"difference": [1, 1.5]})
    assert sorted(os.listdir(tmp_path)) == ["h1.vol", "h2.vol", "out_avgDiff.vol", "out_restored1.vol", "out_restored2.vol"]


def test_program_circular_mask(gpu, tmp_path):
    xa = gpu[0]
    shape = (32, 32, 32)
    _program_vs_handle(gpu, tmp_path, shape, {"denoising": [1], "difference": [1, 1.5]}, ["--mask", "circular", "-10"],
                       xa.halves_circular_mask(shape, -10))


def test_program_binary_file_mask(gpu, tmp_path):
    xa = gpu[0]
    shape = (32, 32, 32)
    m = (np.random.default_rng(9).random(shape) < 0.4).astype(np.float32) * 2.5
    xmipp_io.write_volume(str(tmp_path / "mask.vol"), m)
    _program_vs_handle(gpu, tmp_path, shape, {"denoising": [1], "difference": [1, 1.5]}, ["--mask", "binary_file", str(tmp_path / "mask.vol")],
                       xa.halves_binary_mask(m))


def test_program_odd_box(gpu, tmp_path):
    _program_vs_handle(gpu, tmp_path, (33, 40, 36), {"denoising": [1], "deconvolution": [1, 0.2, 0.001], "filterBank": [0.1, 0.5, 2, 3],
                                                      "difference": [1, 1.5]}, seed=3)


def test_program_mask_of_another_size(gpu, tmp_path):
    V1, V2 = (v.astype(np.float32) for v in halves((16, 16, 16)))
    xmipp_io.write_volume(str(tmp_path / "h1.vol"), V1)
    xmipp_io.write_volume(str(tmp_path / "h2.vol"), V2)
    xmipp_io.write_volume(str(tmp_path / "m.vol"), np.ones((16, 16, 12), np.float32))
    r = _run(["--i1", str(tmp_path / "h1.vol"), "--i2", str(tmp_path / "h2.vol"), "--mask", "binary_file", str(tmp_path / "m.vol")])
    assert r.returncode != 0 and "Mask and input volumes have different dimensions" in r.stderr
