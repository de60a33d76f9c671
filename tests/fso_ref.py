"""A numpy restatement of the reference's reconstruction/resolution_fso.cpp (ProgFSO), the test oracle of xmipp_resolution_fso: the
compacted shell-sorted layout, the global FSC, the cone sums (in fp64 with the float weights, and in the as-written float32 sequential
form), the host decisions (directional FSC and resolution, FSO curve, Bingham statistic, resolution distribution), the 3DFSC with its float
accumulation, and a seeded synthetic pair of half maps. Line numbers are those of resolution_fso.cpp.

Float arithmetic is numpy float32 arithmetic (every operation rounds once, nothing is contracted). sinf, cosf and expf are taken as the
double function rounded to float, which is what a correctly rounded float function returns."""
import numpy as np

F32, F64 = np.float32, np.float64
DBL_MIN = np.finfo(np.float64).tiny


def sinf(x):
    return np.sin(np.asarray(x, F32).astype(F64)).astype(F32)


def cosf(x):
    return np.cos(np.asarray(x, F32).astype(F64)).astype(F32)


def expf(x):
    return np.exp(np.asarray(x, F32).astype(F64)).astype(F32)


def c_round(x):
    """C's round() of non-negative doubles: halves away from zero"""
    fl = np.floor(x)
    return np.where(x - fl >= 0.5, fl + 1, fl)


# ---------------------------------------------------------------- directions and the cone
def unit_vectors(rot_tilt_deg):
    """generateDirections :985 (the float matrix times the float of PI / 180) and fscDir_fast :408-410"""
    a = np.asarray(rot_tilt_deg, F32).reshape(-1, 2) * F32(np.pi / 180.0)
    rot, tilt = a[:, 0], a[:, 1]
    return np.stack([sinf(tilt) * cosf(rot), sinf(tilt) * sinf(rot), cosf(tilt)], 1).astype(F32)


def cone(anglecone_deg):
    """run :1344, fscDir_fast :419 and :425: (cosAngle, aux) as float32"""
    ang_con = anglecone_deg * np.pi / 180.0
    cosAngle = F32(np.cos(ang_con))
    t = F32(cosAngle - F32(1))
    aux = F32(4.0 / F64(F32(t * t)))
    return cosAngle, aux


def incomplete_gamma(x):
    """incompleteGammaFunction :510-569: the table is P(5, i / 2) to 5 significant digits, then to float"""
    idx = int(min(40, c_round(2 * x))) if 2 * x > 0 else 0
    t = 0.5 * idx
    P = 1 - np.exp(-t) * sum(t ** k / float(np.prod(np.arange(1, k + 1))) for k in range(5))
    return float(F32(float("%.4e" % P)))


# ---------------------------------------------------------------- layout and global FSC
def axis_freq(n, size):
    """defineFrequencies :124-140: FFT_IDX2DIGFREQ, DBL_MIN at index 0"""
    idx = np.arange(n)
    u = np.where(idx <= size // 2, idx, idx - size) / float(size)
    u[0] = DBL_MIN
    return u


def spectra(half1, half2, mask=None):
    """prepareData :1013-1024 and run :1324-1325 without CenterFFT (a common unit-modulus phase); the forward transform carries 1 / N"""
    m = 1.0 if mask is None else mask
    return np.fft.rfftn(half1 * m) / half1.size, np.fft.rfftn(half2 * m) / half2.size


def layout(shape, FT1, FT2):
    """defineFrequencies :111-205 and arrangeFSC_and_fscGlobal :209-321"""
    Z, Y, X = shape
    xh = X // 2 + 1
    uz, uy, ux = axis_freq(Z, Z)[:, None, None], axis_freq(Y, Y)[None, :, None], axis_freq(xh, X)[None, None, :]
    with np.errstate(divide="ignore", invalid="ignore"):
        f = np.sqrt((uz * uz + uy * uy) + ux * ux)
        iun = 1 / f
        f2 = 1 / iun
    j0 = (np.arange(xh) == 0)[None, None, :]
    i0 = (np.arange(Y) == 0)[None, :, None]
    kept = (f <= 0.5) & ~(j0 & (uy < 0)) & ~(i0 & j0 & (uz < 0)) & ~(f2 > 0.5)
    raster = np.flatnonzero(kept.ravel())
    shell_r = c_round(f2.ravel()[raster] * X).astype(np.int64)
    L = X // 2 + 1
    assert shell_r.max() < L
    order = np.argsort(shell_r, kind="stable")
    arr2indx = raster[order]
    freqidx = shell_r[order]
    k, rem = np.divmod(arr2indx, Y * xh)
    i, j = np.divmod(rem, xh)
    iu = iun.ravel()[arr2indx]
    with np.errstate(invalid="ignore"):
        fx = (ux.ravel()[j].astype(F32).astype(F64) * iu).astype(F32)
        fy = (uy.ravel()[i].astype(F32).astype(F64) * iu).astype(F32)
        fz = (uz.ravel()[k].astype(F32).astype(F64) * iu).astype(F32)
    z1, z2 = FT1.ravel()[arr2indx], FT2.ravel()[arr2indx]
    re = z1.real * z2.real + z1.imag * z2.imag
    absz1, absz2 = np.abs(z1), np.abs(z2)
    sums = np.stack([np.bincount(freqidx, w, L) for w in (re, absz1 * absz1, absz2 * absz2)], 1)
    return {"fx": fx, "fy": fy, "fz": fz, "freqidx": freqidx, "arr2indx": arr2indx, "real_z1z2": re.astype(F32),
            "absz1": (absz1.astype(F32).astype(F64) * absz1).astype(F32), "absz2": (absz2.astype(F32).astype(F64) * absz2).astype(F32),
            "sums": sums, "shell_count": np.bincount(freqidx, minlength=L), "L": L}


def global_fsc(sums):
    """:331"""
    with np.errstate(divide="ignore", invalid="ignore"):
        return sums[:, 0] / np.sqrt(sums[:, 1] * sums[:, 2])


def freq_axis(L, X, sampling):
    """:332"""
    return np.arange(L).astype(F32).astype(F64) / (X * sampling)


# ---------------------------------------------------------------- cones
def cone_weights(lay, d, cosAngle, aux):
    """fscDir_fast :431-443 for one direction: (in-cone mask, float32 weights of the in-cone coefficients)"""
    with np.errstate(invalid="ignore"):
        c = np.abs((d[0] * lay["fx"] + d[1] * lay["fy"]) + d[2] * lay["fz"])
        inside = c >= cosAngle
    t = c[inside] - F32(1)
    return inside, expf(-(t * t) * aux)


def cone_sums(lay, dirs, cosAngle, aux):
    """the sums of :453-455 in fp64 with the float weights: (sums [ndir, L, 3], in-cone counts [ndir])"""
    L = lay["L"]
    out, cnt = np.zeros((len(dirs), L, 3)), np.zeros(len(dirs), np.int64)
    cols = [lay[k].astype(F64) for k in ("real_z1z2", "absz1", "absz2")]
    for n, d in enumerate(np.asarray(dirs, F32)):
        inside, w = cone_weights(lay, d, cosAngle, aux)
        w64, idx = w.astype(F64), lay["freqidx"][inside]
        for c, col in enumerate(cols):
            out[n, :, c] = np.bincount(idx, w64 * col[inside], L)
        cnt[n] = int(inside.sum())
    return out, cnt


def cone_sums_as_written(lay, d, cosAngle, aux):
    """:453-455 as written for one direction: float products added to float accumulators in the order of the sorted coefficients"""
    L = lay["L"]
    inside, w = cone_weights(lay, np.asarray(d, F32), cosAngle, aux)
    idx = lay["freqidx"][inside]
    out = np.zeros((L, 3), F32)
    for c, k in enumerate(("real_z1z2", "absz1", "absz2")):
        terms = lay[k][inside] * w
        for s in np.unique(idx):
            out[s, c] = np.cumsum(terms[idx == s], dtype=F32)[-1]
    return out


def dir_fsc(sums):
    """:468-469: float32 [.., L] from sums [.., L, 3]"""
    with np.errstate(divide="ignore", invalid="ignore"):
        a = sums[..., 0] / (np.sqrt(sums[..., 1] * sums[..., 2]) + 1e-38)
    return np.maximum(0.0, a).astype(F32)


# ---------------------------------------------------------------- host decisions
def decide(dsums, dirs, xdim, sampling, thrs):
    """fscDir_fast :466-486 for every direction in ascending order, anistropyParameter :989-999, run :1426-1470.
    Returns fsc float32 [ndir, L], resolution [ndir], fso float32 [L], bingham [L]"""
    dirs = np.asarray(dirs, F32)
    fsc = dir_fsc(dsums)
    ndir, L = fsc.shape
    above = fsc.astype(F64) >= thrs
    aniParam = np.zeros(L, F32)
    freqMat = np.zeros((L, 3, 3))
    resol = np.full(ndir, -1.0)
    for k in range(ndir):
        T = np.outer(dirs[k], dirs[k]).astype(F64)          # float products (:415-417)
        freqMat[above[k]] += T
        aniParam[above[k]] += F32(1)
        below = np.flatnonzero((fsc[k].astype(F64) <= thrs) & (np.arange(L) > 2))
        if below.size:
            resol[k] = 1.0 / (F64(F32(below[0])) / (xdim * sampling))
    bingham = np.zeros(L)
    for i in range(L):
        if aniParam[i] > 0:
            T = freqMat[i] / F64(aniParam[i])
            trT2 = sum(sum(T[a, b] * T[b, a] for b in range(3)) for a in range(3))
            bingham[i] = 0.5 * 3.0 * (3.0 + 2) * F64(2 * aniParam[i]) * (trT2 - 1.0 / 3.0)
    fso = aniParam / F32(ndir)
    fso[:5] = 1
    return fsc, resol, fso, bingham


def resolution_distribution(dirs, resol, anglecone_deg):
    """resolutionDistribution :1194-1261: [360, 91]"""
    dirs = np.asarray(dirs, F32)
    ang_con = anglecone_deg * np.pi / 180.0
    cosAngle = cosf(F32(ang_con))
    t = F32(cosAngle - F32(1))
    aux = F32(4.0 / F64(F32(t * t)))
    rot = (np.arange(360) * np.pi / 180.0).astype(F32)
    tilt = (np.arange(91) * np.pi / 180.0).astype(F32)
    cr, sr, st, ct = cosf(rot), sinf(rot), sinf(tilt), cosf(tilt)
    xx, yy, zz = (st[None, :] * cr[:, None]).ravel(), (st[None, :] * sr[:, None]).ravel(), np.broadcast_to(ct[None, :], (360, 91)).ravel()
    w, wt = np.zeros(xx.size), np.zeros(xx.size)
    for k, d in enumerate(dirs):
        c = np.abs((d[0] * xx + d[1] * yy) + d[2] * zz)
        inside = c >= cosAngle
        tt = c[inside] - F32(1)
        wk = expf(-(tt * tt) * aux).astype(F64)
        w[inside] += wk * resol[k]
        wt[inside] += wk
    with np.errstate(divide="ignore", invalid="ignore"):
        return (w / wt).reshape(360, 91)


# ---------------------------------------------------------------- 3DFSC
def threedfsc(shape, lay, dirs, cosAngle, aux, fsc):
    """:496-506 over the directions in ascending order with the float accumulators, run :1501-1508, the line fixes :1521-1539,
    createFullFourier :1297-1306. Returns (half [Z, Y, X/2+1], full [Z, Y, X])"""
    Z, Y, X = shape
    assert Z == Y == X
    xh = X // 2 + 1
    n = lay["freqidx"].size
    threeD, norm = np.zeros(n, F32), np.zeros(n, F32)
    for k, d in enumerate(np.asarray(dirs, F32)):
        inside, w = cone_weights(lay, d, cosAngle, aux)
        w64 = w.astype(F64)
        threeD[inside] = (threeD[inside].astype(F64) + w64 * fsc[k][lay["freqidx"][inside]].astype(F64)).astype(F32)
        norm[inside] = (norm[inside].astype(F64) + w64).astype(F32)
    with np.errstate(divide="ignore", invalid="ignore"):
        value = (threeD / norm).astype(F64)
    value[np.isnan(value)] = 1.0
    half = np.zeros(Z * Y * xh)
    half[lay["arr2indx"]] = value
    half = half.reshape(Z, Y, xh)
    half[:, Y // 2 + 1:, 0] = half[:, Y // 2 + 1:, 1]
    half[:, 0, 0] = half[:, 0, 1]
    return half, complete_and_center(half, X)


def complete_and_center(half, X):
    """getCompleteFourier :1264-1294 and CenterFFT(.., true)"""
    Z, Y, xh = half.shape
    full = np.zeros((Z, Y, X))
    full[:, :, :xh] = half
    k, i = (Z - np.arange(Z)) % Z, (Y - np.arange(Y)) % Y
    j = np.arange(xh, X)
    full[:, :, xh:] = half[k[:, None, None], i[None, :, None], (X - j)[None, None, :]]
    return np.roll(full, (Z // 2, Y // 2, X // 2), axis=(0, 1, 2))


# ---------------------------------------------------------------- the synthetic pair
def synth(shape, seed, widths=(0.06, 0.14, 0.2), noise=1.0):
    """two half maps and a soft mask: blobs with texture, low-passed by exp(-q^4 / 2), q^2 = sum (u / width)^2 with the half-widths
    `widths` in cycles per pixel along z, y, x, scaled to unit deviation, plus independent white noise of deviation `noise`. Different
    widths make the resolution depend on the direction: at 64^3 the FSO slopes from 1 to the level of pure noise over a dozen shells,
    with equal widths it steps within two"""
    rng = np.random.default_rng(seed)
    Z, Y, X = shape
    z, y, x = np.meshgrid(np.arange(Z) - Z / 2, np.arange(Y) - Y / 2, np.arange(X) - X / 2, indexing="ij")
    vol = np.zeros(shape)
    R = 0.25 * min(shape)
    for _ in range(12):
        c = rng.uniform(-0.5, 0.5, 3) * R
        s = rng.uniform(0.1, 0.2) * min(shape)
        vol += rng.uniform(0.5, 1.0) * np.exp(-((z - c[0]) ** 2 + (y - c[1]) ** 2 + (x - c[2]) ** 2) / (2 * s * s))
    vol *= 1 + 2.0 * rng.standard_normal(shape)
    uz, uy, ux = np.fft.fftfreq(Z)[:, None, None], np.fft.fftfreq(Y)[None, :, None], np.fft.rfftfreq(X)[None, None, :]
    lp = np.exp(-0.5 * ((uz / widths[0]) ** 2 + (uy / widths[1]) ** 2 + (ux / widths[2]) ** 2) ** 2)
    sig = np.fft.irfftn(np.fft.rfftn(vol) * lp, s=shape, axes=(0, 1, 2))
    sig /= sig.std()
    halves = [sig + noise * rng.standard_normal(shape) for _ in range(2)]
    r = np.sqrt(z * z + y * y + x * x)
    edge = 0.42 * min(shape)
    mask = np.clip((edge - r) / 3.0 + 0.5, 0.0, 1.0)
    return halves[0], halves[1], mask
