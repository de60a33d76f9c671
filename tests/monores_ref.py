"""A numpy fp64 restatement of xmipp_resolution_monogenic_signal: reconstruction/resolution_monogenic_signal.cpp (ProgMonogenicSignalRes)
and data/monogenic_signal.cpp (Monogenic), written from them line by line, with realGaussianFilter of data/fourier_filter.cpp. Volumes are
[Z, Y, X] float64. np.fft.rfftn / irfftn have FFTW's r2c / c2r semantics, the dropped imaginary parts of the x-Nyquist and DC columns
included; xmippCore's forward transform divides by N and its inverse does not, which is rfftn / N and irfftn * N, so a filter applied in
between is irfftn(filter * rfftn).

run() records, per evaluated frequency, the amplitude(s), the threshold, the statistics and the mask before and after the assignment,
which is what the device tests compare with. The places where the reference divides by zero or reads past an array are refused with
ValueError, as the device code refuses them (the list is at the head of xmipp3_amd/csrc/xh_mono.hip); the low-pass tail with
freqL == freq takes the value 1 at un == freq.
"""
import math

import numpy as np

PI = math.pi


def icdf_gauss(p):
    """Abramowitz-Stegun 26.2.23 (xmippCore's icdf_gauss is not in the tree)"""
    q = p if p < 0.5 else 1 - p
    t = math.sqrt(-2 * math.log(q))
    x = t - ((0.010328 * t + 0.802853) * t + 2.515517) / (((0.001308 * t + 0.189269) * t + 1.432788) * t + 1)
    return -x if p < 0.5 else x


def _rnd(x):
    return int(x + 0.5) if x > 0 else int(x - 0.5)


def digfreq2fft_idx(freq, size):
    idx = _rnd(size * freq)
    if idx < 0:
        idx += size
    return idx


def fft_idx2digfreq(idx, size):
    if size <= 1:
        return 0.0
    return (idx if idx <= (size >> 1) else idx - size) / float(size)


def _axis_freq(nf, nreal):
    """FFT_IDX2DIGFREQ over the first nf indices of an axis of nreal points"""
    return np.array([fft_idx2digfreq(k, nreal) for k in range(nf)])


def fourier_freq_vector(nf, nreal):
    v = _axis_freq(nf, nreal)
    v[0] = 1e-38
    return v


def fourier_freqs_3d(shape):
    """iu [Z, Y, X/2+1] and the three axis vectors (fourierFreqs_3D)"""
    Z, Y, X = shape
    xh = X // 2 + 1
    fz, fy, fx = fourier_freq_vector(Z, Z), fourier_freq_vector(Y, Y), fourier_freq_vector(xh, X)
    uz, uy, ux = _axis_freq(Z, Z), _axis_freq(Y, Y), _axis_freq(xh, X)
    uz2 = (uz * uz)[:, None, None]
    uz2y2 = uz2 + (uy * uy)[None, :, None]
    u2 = uz2y2 + (ux * ux)[None, None, :]
    iu = np.empty((Z, Y, xh))
    with np.errstate(divide="ignore"):
        iu[...] = 1 / np.sqrt(u2)
    iu[0, 0, 0] = 1e38
    return iu, fx, fy, fz


def xmipp_coords(shape):
    Z, Y, X = shape
    return np.meshgrid(np.arange(Z) - Z // 2, np.arange(Y) - Y // 2, np.arange(X) - X // 2, indexing="ij")


def r2_map(shape):
    k, i, j = xmipp_coords(shape)
    return k * k + i * i + j * j


def shell_sums(vol):
    """per shell r (r^2 <= R2 < (r + 1)^2): sum, sum2, N, what findCliffValue accumulates for one rad"""
    r2 = r2_map(vol.shape)
    sh = np.floor(np.sqrt(r2.astype(np.float64))).astype(np.int64)
    sh = np.where(sh * sh > r2, sh - 1, sh)
    sh = np.where((sh + 1) * (sh + 1) <= r2, sh + 1, sh)
    n = int(sh.max()) + 1
    s = np.bincount(sh.ravel(), weights=vol.ravel(), minlength=n)
    s2 = np.bincount(sh.ravel(), weights=(vol * vol).ravel(), minlength=n)
    cnt = np.bincount(sh.ravel(), minlength=n).astype(np.float64)
    return s, s2, cnt


def protein_radius(mask):
    sel = mask == 1
    vol = int(sel.sum())
    radius = int(math.sqrt(int(r2_map(mask.shape)[sel].max()))) if vol else 0
    return radius, vol


def cliff_radius(s, s2, cnt, radius, X):
    radiuslimit = X // 2
    last_std2 = 1e-38
    for rad in range(radius, radiuslimit):
        with np.errstate(all="ignore"):
            mean = s[rad] / cnt[rad]
            std2 = s2[rad] / cnt[rad] - mean * mean
            if std2 / last_std2 < 0.01:
                radiuslimit = rad - 1
                break
        last_std2 = std2
    return radiuslimit


def find_cliff_value(vol, radius, mask, rsmooth=0.0):
    s, s2, cnt = shell_sums(vol)
    radiuslimit = cliff_radius(s, s2, cnt, radius, vol.shape[2])
    raux = radiuslimit - rsmooth
    raux *= raux
    mask[r2_map(vol.shape).astype(np.float64) >= raux] = -1
    return radiuslimit


def resolution2eval(st, step, volsize, sampling, maxRes):
    """st: dict with count_res, resolution, last_resolution, freq, freqL, last_fourier_idx; returns (continueIter, breakIter)"""
    st["resolution"] = maxRes - st["count_res"] * step
    if not st["resolution"] > 0:
        st["count_res"] += 1
        return False, True
    st["freq"] = sampling / st["resolution"]
    st["count_res"] += 1
    Nyquist = 2 * sampling
    fourier_idx = digfreq2fft_idx(st["freq"], volsize)
    aux_frequency = fft_idx2digfreq(fourier_idx, volsize)
    st["freq"] = aux_frequency
    if fourier_idx == st["last_fourier_idx"]:
        return True, False
    st["last_fourier_idx"] = fourier_idx
    with np.errstate(divide="ignore"):
        st["resolution"] = float(np.float64(sampling) / np.float64(aux_frequency))
    if st["count_res"] == 0:
        st["last_resolution"] = st["resolution"]
    if st["resolution"] < Nyquist:
        return False, True
    st["freqL"] = sampling / (st["resolution"] + step)
    fourier_idx_2 = digfreq2fft_idx(st["freqL"], volsize)
    if fourier_idx_2 == fourier_idx:
        if fourier_idx > 0:
            st["freqL"] = fft_idx2digfreq(fourier_idx - 1, volsize)
        else:
            st["freqL"] = sampling / (st["resolution"] + step)
    return False, False


def resolution_sweep(volsize, sampling, maxRes, step, limit=100000):
    st = dict(count_res=0, resolution=0.0, last_resolution=maxRes, freq=0.0, freqL=0.0, last_fourier_idx=-1)
    out = []
    for _ in range(limit):
        cont, brk = resolution2eval(st, step, volsize, sampling, maxRes)
        if cont:
            out.append(("continue", st["resolution"], st["freq"]))
            continue
        if brk:
            out.append(("break", st["resolution"], st["freq"]))
            break
        out.append(("eval", st["resolution"], st["freq"]))
        st["last_resolution"] = st["resolution"]
    return out


def _irfftn(F, shape):
    return np.fft.irfftn(F, s=shape, axes=(0, 1, 2)) * float(np.prod(shape))


def _fft(v):
    return np.fft.rfftn(v) / float(v.size)


def amplitude_lpf(fftV, shape, freq, freqH, freqL, fr=None):
    """amplitudeMonoSig3D_LPF"""
    iu, fx, fy, fz = fr if fr is not None else fourier_freqs_3d(shape)
    un = 1.0 / iu
    with np.errstate(divide="ignore", invalid="ignore"):
        ideltal = np.float64(PI) / np.float64(freq - freqH)
        band = (freqH <= un) & (un <= freq)
        above = ~band & (un > freq)
        H = np.where(band, 0.5 * (1 + np.cos(np.where(band, (un - freq) * ideltal, 0.0))), 0.0)
    fftVRiesz = np.where(band, fftV * H, np.where(above, fftV, 0.0))
    aux = np.where(band | above, (-1j * fftVRiesz) * iu, 0.0)
    amplitude = _irfftn(fftVRiesz, shape) ** 2
    amplitude += _irfftn(fx[None, None, :] * aux, shape) ** 2
    amplitude += _irfftn(fz[:, None, None] * aux, shape) ** 2
    amplitude += _irfftn(fy[None, :, None] * aux, shape) ** 2
    amplitude = np.sqrt(amplitude)
    F = _fft(amplitude)
    if freqL != freq:
        raised_w = PI / (freqL - freq)
        tail = (freqL >= un) & (un >= freq)
        F = np.where(tail, F * (0.5 * (1 + np.cos(raised_w * (un - freq)))), np.where(un > freqL, 0.0, F))
    else:
        F = np.where(un > freqL, 0.0, F)
    return _irfftn(F, shape)


def monogenic_amplitude_3d_fourier(fftV, shape):
    iu, fx, fy, fz = fourier_freqs_3d(shape)
    aux = (-1j * fftV) * iu
    amplitude = _irfftn(fftV, shape) ** 2
    amplitude += _irfftn(fx[None, None, :] * aux, shape) ** 2
    amplitude += _irfftn(fy[None, :, None] * aux, shape) ** 2
    amplitude += _irfftn(fz[:, None, None] * aux, shape) ** 2
    return np.sqrt(amplitude)


def real_gaussian_filter(v, sigma):
    Z, Y, X = v.shape
    wz, wy, wx = _axis_freq(Z, Z), _axis_freq(Y, Y), _axis_freq(X // 2 + 1, X)
    s = (wx * wx)[None, None, :] + (wy * wy)[None, :, None]
    s = s + (wz * wz)[:, None, None]
    absw = np.sqrt(s)
    g = np.exp(-PI * PI * absw * absw * sigma * sigma)
    return np.fft.irfftn(np.fft.rfftn(v) * g, s=v.shape, axes=(0, 1, 2))


def statistics(volS, volN, mask, significance, halves):
    """statisticsInBinaryMask2 (halves) / statisticsInOutBinaryMask2"""
    sig = mask >= 1
    noi = (mask >= 0) if halves else (mask == 0)
    S, Nv = volS[sig], volN[noi]
    NS, NN = float(S.size), float(Nv.size)
    if NN == 0:
        raise ValueError("the noise set is empty")
    sumS, sumS2, sumN, sumN2 = S.sum(), (S * S).sum(), Nv.sum(), (Nv * Nv).sum()
    thr95 = np.sort(Nv)[int(Nv.size * significance)]
    with np.errstate(all="ignore"):
        meanS = np.float64(sumS) / NS
        meanN = sumN / NN
        sdS2 = np.float64(sumS2) / NS - meanS * meanS
        sdN2 = sumN2 / NN - meanN * meanN
    return dict(NS=NS, NN=NN, sumS=sumS, sumS2=sumS2, sumN=sumN, sumN2=sumN2, meanS=float(meanS), sdS2=float(sdS2), meanN=float(meanN), sdN2=float(sdN2),
                thr95=float(thr95))


def set_local_resolution(amp, mask, res, thr, resolution, resolution_2, halves):
    """setLocalResolutionHalfMaps / setLocalResolutionMap, in place"""
    act = mask >= 1
    hit = act & (amp > thr)
    miss = act & ~hit
    mask[hit] = 1
    res[hit] = resolution
    mask[miss] += 1
    drop = miss & (mask > 2)
    mask[drop] = 0 if halves else -1
    res[drop] = resolution_2


def refining_mask(fftV, shape, mask):
    amplitude = real_gaussian_filter(monogenic_amplitude_3d_fourier(fftV, shape), 4)
    noise = amplitude[mask == 0]
    if noise.size == 0:
        raise ValueError("refiningMask: the noise set is empty")
    thr = np.sort(noise)[int(noise.size * 0.95)]
    sig = mask >= 1
    mask[sig & (amplitude < thr)] = 0
    n = int((sig & ~(amplitude < thr)).sum())
    if n == 0:
        raise ValueError("refiningMask left no voxel")
    return n, float(thr), amplitude


def run(vol, mask, vol2=None, mask_excl=None, sampling=1.0, minRes=30.0, maxRes=1.0, freq_step=0.25, significance=0.95, gaussian=False,
        noiseOnlyInHalves=False):
    """ProgMonogenicSignalRes::run; returns a dict with the outputs and `steps`, one record per evaluated frequency"""
    shape = vol.shape
    halves = vol2 is not None
    out = {}
    if halves:
        V = 0.5 * (vol + vol2)
        out["mean"] = V
        fftN = _fft((vol - vol2) / 2)
    else:
        V = vol
    mask = mask.astype(np.int32).copy()
    radius, NVox = protein_radius(mask)
    if NVox == 0:
        raise ValueError("the mask has no voxel equal to 1")
    radiuslimit = find_cliff_value(V, radius, mask)
    if mask_excl is not None:
        if halves:
            if noiseOnlyInHalves:
                one = mask == 1
                mask[one & (mask_excl == 1)] = -1
                mask[~one] = -1
        else:
            mask[(mask == 1) & (mask_excl == 1)] = -1
    elif halves and noiseOnlyInHalves:
        mask[mask < 1] = -1
    fftV = _fft(V)
    fr = fourier_freqs_3d(shape)
    if freq_step < 0.25:
        freq_step = 0.25
    criticalZ = icdf_gauss(significance)
    max_meanS = -np.finfo(np.float64).tiny
    cut_value = 0.025
    minRes = 2 * sampling
    out.update(radius=radius, radiuslimit=radiuslimit)
    out["mask_side"] = mask.copy()
    if not noiseOnlyInHalves:
        NVox, thr0, amp0 = refining_mask(fftV, shape, mask)
        out.update(refine_threshold=thr0, refine_amplitude=amp0)
    out["nvoxels"] = NVox
    out["mask_refined_in"] = mask.copy()
    volsize = shape[2]
    res = np.zeros(shape)
    st = dict(count_res=0, resolution=0.0, last_resolution=maxRes, freq=0.0, freqL=0.0, last_fourier_idx=-1)
    lst, steps, it, stop = [], [], 0, None
    doNext = True
    while doNext:
        cont, brk = resolution2eval(st, freq_step, volsize, sampling, maxRes)
        if cont:
            continue
        if brk:
            stop = "range"
            break
        resolution, freq = st["resolution"], st["freq"]
        lst.append(resolution)
        resolution_2 = lst[0] if it < 2 else lst[it - 2]
        freqL, freqH = freq + 0.02, freq - 0.02
        if freqL >= 0.5:
            freqL = 0.5
        if freqH <= 0.0:
            freqH = 0.0
        ampS = amplitude_lpf(fftV, shape, freq, freqH, freqL, fr)
        ampN = amplitude_lpf(fftN, shape, freq, freqH, freqL, fr) if halves else ampS
        s = statistics(ampS, ampN, mask, significance, halves)
        rec = dict(s, resolution=resolution, freq=freq, freqH=freqH, freqL=freqL, ampS=ampS, mask_before=mask.copy(), threshold=0.0, z=0.0, assigned=0)
        steps.append(rec)
        leave = False
        if s["NS"] / NVox < cut_value:
            stop, doNext = "mask_done", False
        elif s["NS"] == 0:
            stop, leave = "no_points", True
        else:
            thr = s["meanN"] + criticalZ * math.sqrt(s["sdN2"]) if gaussian else s["thr95"]
            rec["threshold"] = thr
            if s["meanS"] > max_meanS:
                max_meanS = s["meanS"]
            if s["meanS"] < 0.001 * max_meanS:
                stop, leave = "low_signal", True
            else:
                set_local_resolution(ampS, mask, res, thr, resolution, resolution_2, halves)
                rec["assigned"] = 1
                rec["resolution_2"] = resolution_2
                z = (s["meanS"] - s["meanN"]) / math.sqrt(s["sdS2"] / s["NS"] + s["sdN2"] / s["NN"])
                rec["z"] = z
                if z < criticalZ:
                    stop, doNext = "ztest", False
                if doNext and resolution < minRes:
                    stop, doNext = "min_res", False
        rec["max_meanS"] = max_meanS
        rec["mask_after"] = mask.copy()
        if leave:
            break
        it += 1
        st["last_resolution"] = resolution
    mask = np.where(res == 0, 0, 1).astype(np.int32)
    if not lst:
        raise ValueError("no frequency was evaluated")
    # postProcessingLocalResolutions
    filt = res.copy()
    last_res = lst[-1] - 0.001
    Nyquist = 2 * sampling
    N = int((filt >= last_res).sum())
    if N == 0:
        raise ValueError("no voxel has a resolution")
    vals = np.sort(filt[filt > last_res])
    vals = np.concatenate([np.zeros(N - vals.size), vals])
    filling = vals[int(0.5 * N)]
    last_res = lst[-1]
    low = filt < last_res
    filt[low] = filling
    mask = np.where(low, 0, 1).astype(np.int32)
    smooth = real_gaussian_filter(filt, 3)
    chim = smooth.copy()
    inside = mask > 0
    chim[inside & (smooth > res)] = res[inside & (smooth > res)]
    chim[inside & (smooth < Nyquist)] = res[inside & (smooth < Nyquist)]
    final = np.where(mask == 0, 0.0, chim)
    out.update(refined_mask=mask, chimera=chim, resolution_map=final, steps=steps, stop=stop, resolutions=lst, criticalZ=criticalZ, res_raw=res,
               post_smooth=smooth, filling=float(filling), critical=dict(cut_value=cut_value))
    return out


# ---------------------------------------------------------------- synthetic maps
def synth_map(shape, seed, noise=0.3):
    """blobs low-passed to different local resolutions inside a sphere, plus Gaussian noise inside a larger sphere and exactly zero
    beyond it (what findCliffValue looks for). Returns (signal, noise sphere radius)."""
    rng = np.random.default_rng(seed)
    Z, Y, X = shape
    k, i, j = xmipp_coords(shape)
    r2 = k * k + i * i + j * j
    m = min(shape)
    sig = np.zeros(shape)
    for b in range(6):
        c = rng.uniform(-m * 0.18, m * 0.18, 3)
        w = rng.uniform(0.9, 2.6)                       # narrow blobs carry high frequencies, wide ones do not
        sig += rng.uniform(0.8, 1.5) * np.exp(-((k - c[0]) ** 2 + (i - c[1]) ** 2 + (j - c[2]) ** 2) / (2 * w * w))
    tex = rng.standard_normal(shape)
    half = k < 0
    tex = np.where(half, real_gaussian_filter(tex, 1.2), real_gaussian_filter(tex, 0.6))
    sig = sig * (1 + 1.5 * tex)
    return sig


def noise_in_sphere(shape, seed, sd, R):
    rng = np.random.default_rng(seed)
    n = rng.standard_normal(shape) * sd
    n[r2_map(shape) >= R * R] = 0.0
    return n


def protein_mask(shape, R):
    return (r2_map(shape) <= R * R).astype(np.int32)
