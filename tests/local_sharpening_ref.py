"""A numpy fp64 restatement of xmipp_volume_local_sharpening (LocalDeblur): reconstruction/volume_local_sharpening.cpp
(ProgLocSharpening), written from it line by line. Volumes are [Z, Y, X] float64. np.fft.rfftn / irfftn have FFTW's r2c / c2r semantics;
xmippCore's forward transform divides by N and its inverse does not, which is rfftn / N and irfftn * N.

The places where the reference divides by zero or reads what it never wrote are refused with ValueError, as the device code refuses
them (the list is at the head of xmipp3_amd/csrc/xh_ldb.hip).
"""
import math

import numpy as np

PI = math.pi
STEP = 0.2
AXES = (0, 1, 2)


def _rnd(x):
    return int(x + 0.5) if x > 0 else int(x - 0.5)


def digfreq2fft_idx(freq, size):
    """DIGFREQ2FFT_IDX as SURVEY.md Appendix B reads it"""
    idx = _rnd(size * freq)
    if idx < 0:
        idx += size
    return idx


def _axis_freq(nf, nreal):
    """FFT_IDX2DIGFREQ over the first nf indices of an axis of nreal points"""
    return np.array([(k if k <= (nreal >> 1) else k - nreal) / float(nreal) for k in range(nf)])


def un_map(shape):
    """iu of produceSideInfo (:78-102): sqrt((uz^2 + uy^2) + ux^2) over the half spectrum, 1e-38 at the origin"""
    Z, Y, X = shape
    uz, uy, ux = _axis_freq(Z, Z), _axis_freq(Y, Y), _axis_freq(X // 2 + 1, X)
    uz2 = (uz * uz)[:, None, None]
    uz2y2 = uz2 + (uy * uy)[None, :, None]
    u2 = uz2y2 + (ux * ux)[None, None, :]
    un = np.sqrt(u2)
    un[0, 0, 0] = 1e-38
    return un


def bands(zsize, sampling, max_res):
    """the loop of localfiltering (:231-244): (res, w, wL, idx) of every processed band; max_res is the loop's bound"""
    min_res = 2 * sampling
    if not (sampling > 0 and min_res - STEP > 0):
        raise ValueError("2 sampling - 0.2 <= 0: wL of the first band")
    if not math.isfinite(max_res):
        raise ValueError("the largest resolution is not finite")
    out = []
    lastidx = -1
    res = min_res
    while res < max_res:
        freq = sampling / res
        idx = digfreq2fft_idx(freq, zsize)
        if idx != lastidx:
            out.append((res, freq, sampling / (res - STEP), idx))
            lastidx = idx
        res += STEP
    return out


def side_info(vol, resmap, sampling):
    """produceSideInfo (:106-127): maxRes before the clamp, the clamped map, the outside set and desvOutside_Vorig"""
    value = resmap.ravel()
    max_res = 1e-38
    big = value[value > max_res]
    if big.size:
        max_res = float(big.max())
    res = resmap.copy()
    res[(res < 2 * sampling) & (res > 0)] = 2 * sampling
    outside = res < 2 * sampling
    N = int(outside.sum())
    if N > 1:
        aux = vol[outside]
        avg = aux.sum() / N
        desv = math.sqrt(abs((aux * aux).sum() / N - avg * avg) * N / (N - 1))
    else:
        desv = 0.0
    if N == vol.size:
        raise ValueError("no voxel of the resolution map is at or above 2 sampling")
    return {"maxRes": max_res, "res": res, "outside": outside, "desvOutside": desv}


def band_pass(F, un, w, wL, shape):
    """bandPassFilterFunction (:181-217): both branches use the same expression, so the band is w_inf <= un <= wL"""
    delta = wL - w
    w_inf = w - delta
    ideltal = PI / delta
    keep = ((un >= w) & (un <= wL)) | ((un <= w) & (un >= w_inf))
    Fb = np.where(keep, F * (0.5 * (1 + np.cos((un - w) * ideltal))), 0.0)
    return np.fft.irfftn(Fb, s=shape, axes=AXES) * float(np.prod(shape))


def localfilter(v, res, sampling, K, blist, un=None, perturb=None):
    """localfiltering (:219-283) of the volume v with the clamped map res. perturb = (rng, eps): every inverse transform is multiplied by
    1 + eps * normal noise (how much rounding the iteration amplifies)"""
    shape = v.shape
    un = un_map(shape) if un is None else un
    F = np.fft.rfftn(v, axes=AXES) / float(v.size)
    inside = ~(res < 2 * sampling)
    out = np.zeros(shape)
    lastweight = np.zeros(shape)
    weight = np.zeros(shape)
    for (r, w, wL, _) in blist:
        filtered = band_pass(F, un, w, wL, shape)
        if perturb is not None:
            filtered = filtered * (1 + perturb[1] * perturb[0].standard_normal(shape))
        weight[inside] = np.exp(-K * (r - res[inside]) * (r - res[inside]))
        filtered = np.where(inside, filtered * weight, 0.0)
        out += filtered
        lastweight += weight
    pos = lastweight > 0
    out[pos] /= lastweight[pos]
    return out


def run(vol, resmap, sampling=1.0, lam=1.0, K=0.025, niter=50, perturb=None):
    """ProgLocSharpening::run (:285-407). Returns a dict: sharpened, lambda, iterations (the last i), stopped, records (one dict per
    iteration: norm, porc, subst, lambda, stop), bands, and the side info"""
    if niter < 1:
        raise ValueError("Niter < 1: the sharpened map is never assigned")
    side = side_info(vol, resmap, sampling)
    res = side["res"]
    blist = bands(vol.shape[0], sampling, side["maxRes"] + 2)
    un = un_map(vol.shape)
    L = lambda v: localfilter(v, res, sampling, K, blist, un, perturb)      # noqa: E731
    lastnorm, lastporc = 0.0, 1.0
    bool1 = 1
    filtered = vol
    sharpened = None
    norm_orig = 0.0
    recs = []
    i = 0
    for i in range(1, niter + 1):
        op = L(filtered)
        filtered = vol - op
        if i == 1:
            norm_orig = math.sqrt(float((vol * vol).sum()))
        norm = math.sqrt(float((op * op).sum()))
        porc = lastnorm * 100 / norm
        subst = porc - lastporc
        if subst < 1 and bool1 == 1 and i > 2:
            bool1 = 2
        lastnorm, lastporc = norm, porc
        if i == 1 and lam == 1:
            lam = (norm_orig / norm) / 12
        filtered = L(filtered)
        Vk = vol if i == 1 else sharpened
        sharpened = Vk + lam * filtered
        floor = -4 * side["desvOutside"]
        sharpened[sharpened < floor] = floor
        filtered = sharpened
        recs.append({"norm": norm, "porc": porc, "subst": subst, "lambda": lam, "stop": bool1 == 2})
        if bool1 == 2:
            break
    out = {"sharpened": sharpened, "lambda": lam, "iterations": i, "stopped": bool1 == 2, "records": recs, "bands": blist}
    out.update(side)
    return out


def synth(shape, seed):
    """(volume, resolution map) at sampling 1: a smooth positive blob with a low-passed texture inside the sphere of radius
    R = min(shape) // 2 - 3, Gaussian noise of 0.02 everywhere; the map is 3 + 4 r / R inside the sphere and 0 outside"""
    rng = np.random.default_rng(seed)
    Z, Y, X = shape
    k, i, j = np.meshgrid(np.arange(Z) - Z // 2, np.arange(Y) - Y // 2, np.arange(X) - X // 2, indexing="ij")
    r = np.sqrt((k * k + i * i + j * j).astype(np.float64))
    R = min(shape) // 2 - 3
    blob = np.exp(-r * r / (2 * (0.6 * R) ** 2))
    un = un_map(shape)
    tex = np.fft.irfftn(np.fft.rfftn(rng.standard_normal(shape), axes=AXES) * np.exp(-0.5 * (un / 0.15) ** 2), s=shape, axes=AXES)
    tex /= tex.std()
    inside = r < R
    vol = np.where(inside, blob * (1 + 0.3 * tex), 0.0)
    vol = vol + 0.02 * rng.standard_normal(shape)
    resmap = np.where(inside, 3 + 4 * r / R, 0.0)
    return vol, resmap
