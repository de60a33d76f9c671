"""numpy restatement of the PSD stage of xmipp_ctf_estimate_from_micrograph (reconstruction/ctf_estimate_from_micrograph.cpp, run()
:289-584, in doubles) and of xmipp_psd_estimate (reconstruction/psd_estimator.cpp, in floats), written from reading them: the piece lists
of the three modes, getPatchesLocation, constructPieceSmoother in both types, statisticsAdjust, the plane fit and normalize_ramp, both PSD
values, avg / std, half2whole, and the normalisation of psd_estimate. Sums run in the reference's order, element after element.

exact=True keeps the same per-term values and branches but takes every sum with math.fsum and every transform in extended precision:
tests/test_psd_ref.py derives the bounds of the GPU test from the difference.

Outside the reference tree, stated here (INTEGRATION.md marks them unpinned):
  statisticsAdjust(0, 1)   computeAvgStdev with sums in double and the N / (N - 1) deviation; a = 1 / stddev (0 where it is 0),
                           b = 0 - a avg; a value becomes (T)(a x + b)
  least_squares_plane_fit_All_Points   the normal equations of z = pA j + pB i + pC over the logical coordinates, solved through the
                           adjugate inverse of the 3 x 3 matrix
  reject_outliers          a 200-bin histogram, clamp to the percentiles 0.125 and 99.875, linear interpolation inside a bin
"""
import math

import numpy as np

PI_L = np.longdouble("3.14159265358979323846264338327950288")
STRIP = 4          # the column pass's strip of half-spectrum columns (xmipp3_amd.psd_strip(); tests/test_gpu_psd.py asserts it)
ADJUST, RAMP = 1, 2
MICROGRAPH, REGIONS, PARTICLES = 0, 1, 2


def _ceil(x):
    """xmippCore's CEIL"""
    return int(x) if x == int(x) else (int(x + 1) if x > 0 else int(x))


# ---------------------------------------------------------------- piece lists
def pieces(Y, X, pieceDim, overlap=0.5, skipBorders=2, mode=MICROGRAPH, pos=None):
    """:310-327, :371-414: (corners [(top, left)], slots [the 1-based N], div_Number). ValueError where the programs refuse"""
    if pieceDim > Y or pieceDim > X:
        raise ValueError("smaller than a piece")
    if mode == PARTICLES:
        divX, divY, div = 1, 1, len(pos)
    elif mode == MICROGRAPH:
        divX = _ceil(float(X) / (pieceDim * (1 - overlap))) - 1
        divY = _ceil(float(Y) / (pieceDim * (1 - overlap))) - 1
        div = divX * divY
    else:
        divX, divY = _ceil(float(X) / pieceDim), _ceil(float(Y) / pieceDim)
        if divX <= 2 * skipBorders or divY <= 2 * skipBorders:
            raise ValueError("not big enough to skip")
        div = divX * divY
    corners, slots = [], []
    for N in range(1, div + 1):
        skip = False
        if mode == PARTICLES:
            pj, pi = int(pos[N - 1][0]), int(pos[N - 1][1])
            if pj < pieceDim // 2 or pi < pieceDim // 2:
                raise ValueError("unsigned subtraction wraps")
            pj -= pieceDim // 2
            pi -= pieceDim // 2
        else:
            step = pieceDim
            if mode == MICROGRAPH:
                step = int((1 - overlap) * step)
            bi, bj = (N - 1) // divX, (N - 1) % divX
            if bi < skipBorders or bj < skipBorders or bi > divY - skipBorders - 1 or bj > divX - skipBorders - 1:
                skip = True
            pi, pj = bi * step, bj * step
        if pi + pieceDim > Y:
            pi = Y - pieceDim
        if pj + pieceDim > X:
            pj = X - pieceDim
        if not skip:
            corners.append((pi, pj))
            slots.append(N)
    if not corners:
        raise ValueError("no piece")
    return corners, slots, div


def patches(Y, X, py, px, borderX=0, borderY=0, overlap=0.5):
    """getPatchesLocation (psd_estimator.cpp:35-71): [(top, left)]; the steps in float arithmetic"""
    ov = np.float32(overlap)
    stepX = int(max((np.float32(1) - ov) * np.float32(px), np.float32(1)))
    stepY = int(max((np.float32(1) - ov) * np.float32(py), np.float32(1)))
    maxX, maxY = X - borderX - px, Y - borderY - py
    out = []
    y = borderY
    while y < maxY + stepY:
        ys = min(y, maxY)
        x = borderX
        while x < maxX + stepX:
            out.append((ys, min(x, maxX)))
            x += stepX
        y += stepY
    return out


# ---------------------------------------------------------------- taper
def taper_vectors(py, px, dtype):
    """the per-row and per-column factors of constructPieceSmoother (:143-189). Both axes take their fraction against YSIZE; in float the
    arithmetic is float up to the argument of the cosine, the cosine a double, the factor a float again"""
    T = np.dtype(dtype).type
    iHalfsize = T(2) / T(py)
    alpha = T(0.025)
    alpha1 = T(1) - alpha
    ialpha = T(1.0 / float(alpha))

    def vec(n):
        m = np.ones(n, dtype=T)
        for k in range(n):
            fraction = abs(T(k - n // 2) * iHalfsize)
            if fraction > alpha1:
                arg = (fraction - T(1)) * ialpha + T(1)
                m[k] = T(0.5 * (1 + math.cos(math.pi * float(arg))))
        return m
    return vec(py), vec(px)


def smoother(py, px, dtype):
    mY, mX = taper_vectors(py, px, dtype)
    return mY[:, None] * mX[None, :]          # (1 * maskY[i]) * maskX[j]: one rounding


# ---------------------------------------------------------------- sums
def _seq(v):
    """element after element, as the reference's loops add"""
    v = np.asarray(v, dtype=np.float64).ravel()
    return float(np.add.accumulate(v)[-1])


def _sum(v, exact):
    return math.fsum(np.asarray(v, dtype=np.float64).ravel()) if exact else _seq(v)


def statistics_adjust_ab(x, exact=False):
    """(a, b, stddev0) of statisticsAdjust(0, 1) for the values x (doubles)"""
    N = x.size
    avg0 = _sum(x, exact) / N
    stddev0 = 0.0
    if N > 1:
        stddev0 = _sum(x * x, exact) / N - avg0 * avg0
        stddev0 *= float(N) / float(N - 1)
        stddev0 = math.sqrt(abs(stddev0))
    a = 1.0 / stddev0 if stddev0 != 0.0 else 0.0
    return a, 0.0 - a * avg0, stddev0


def plane_inverse(py, px):
    """the inverse of the normal matrix of the plane fit, through the adjugate"""
    i = np.arange(py, dtype=np.float64) - py // 2
    j = np.arange(px, dtype=np.float64) - px // 2
    sxx, syy = float((j * j).sum()) * py, float((i * i).sum()) * px
    sxy, sx, sy = float(i.sum() * j.sum()), float(j.sum()) * py, float(i.sum()) * px
    A = [sxx, sxy, sx, sxy, syy, sy, sx, sy, float(py * px)]
    I = [A[8] * A[4] - A[7] * A[5], -(A[8] * A[1] - A[7] * A[2]), A[5] * A[1] - A[4] * A[2],
         -(A[8] * A[3] - A[6] * A[5]), A[8] * A[0] - A[6] * A[2], -(A[5] * A[0] - A[3] * A[2]),
         A[7] * A[3] - A[6] * A[4], -(A[7] * A[0] - A[6] * A[1]), A[4] * A[0] - A[3] * A[1]]
    det = A[0] * I[0] + A[3] * I[1] + A[6] * I[2]
    return [c / det for c in I]


def plane_fit(z, exact=False):
    """least_squares_plane_fit_All_Points: (pA, pB, pC) of z = pA j + pB i + pC over the logical coordinates of setXmippOrigin"""
    py, px = z.shape
    li = (np.arange(py, dtype=np.float64) - py // 2)[:, None]
    lj = (np.arange(px, dtype=np.float64) - px // 2)[None, :]
    b0, b1, b2 = _sum(lj * z, exact), _sum(li * z, exact), _sum(z, exact)
    I = plane_inverse(py, px)
    return (I[0] * b0 + I[1] * b1 + I[2] * b2, I[3] * b0 + I[4] * b1 + I[5] * b2, I[6] * b0 + I[7] * b1 + I[8] * b2)


def normalize_ramp(z, exact=False):
    """data/normalize.cpp:333-425 without a mask: (the image, stddevbg)"""
    py, px = z.shape
    N = py * px
    pA, pB, pC = plane_fit(z, exact)
    li = (np.arange(py, dtype=np.float64) - py // 2)[:, None]
    lj = (np.arange(px, dtype=np.float64) - px // 2)[None, :]
    aux = pB * li + pC
    r = z - (pA * lj + aux)
    avgbg = _sum(r, exact) / N
    stddevbg = math.sqrt(abs(_sum(r * r, exact) / N - avgbg * avgbg) * N / (N - 1))
    if stddevbg > 1e-6:
        r = r * (1.0 / stddevbg)
    return r, stddevbg


def prepare(window, dtype, flags, exact=False, info=None):
    """the piece as the transform reads it: adjust, subtract the plane, scale, times the taper. window: float32 [py, px]"""
    T = np.dtype(dtype).type
    py, px = window.shape
    x = window.astype(np.float64)                 # exact
    a, b, sd0 = statistics_adjust_ab(x, exact) if flags & ADJUST else (1.0, 0.0, None)
    v = (a * x + b).astype(T)
    sdbg = None
    if flags & RAMP:
        v, sdbg = normalize_ramp(v.astype(np.float64), exact)
    if info is not None:
        info.append((sd0, sdbg))
    return v.astype(T) * smoother(py, px, T)


# ---------------------------------------------------------------- transforms and PSD values
_DFT = {}


def _dft_l(n):
    if n not in _DFT:
        k = np.arange(n)
        a = (2 * PI_L) * ((np.outer(k, k) % n).astype(np.longdouble) / np.longdouble(n))
        _DFT[n] = np.cos(a) - 1j * np.sin(a)
    return _DFT[n]


def transform(piece, exact=False):
    """the un-normalised complete 2-D transform; in the piece's own precision, or in extended precision"""
    if exact:
        py, px = piece.shape
        return _dft_l(py) @ piece.astype(np.clongdouble) @ _dft_l(px)
    return np.fft.fft2(piece)


def psd_double(piece, exact=False):
    """:435-438: the modulus of the transform over py px, squared, times pieceDim^2 -- in that order"""
    py, px = piece.shape
    F = transform(piece, exact)
    if exact:
        m = np.hypot(F.real, F.imag) / np.longdouble(py * px)
        return (m * (m * np.longdouble(py * px))).astype(np.float64)
    m = np.hypot(F.real, F.imag) / float(py * px)
    return m * (m * float(py * px))


def psd_float(piece, exact=False):
    """psd_estimator.cpp:112-116: the modulus of the un-normalised transform, in floats"""
    F = transform(piece, exact)
    if exact:
        return np.hypot(F.real, F.imag).astype(np.float64)
    assert F.dtype == np.complex64
    re, im = F.real, F.imag
    return np.sqrt(re * re + im * im)


def half2whole(half, py, px):
    """psd_estimator.h:52-73: half [py, px // 2 + 1] -> [py, px]"""
    hx = px // 2 + 1
    out = np.zeros((py, px), dtype=half.dtype)
    for y in range(py):
        for x in range(px):
            mirror = x >= hx
            xS = px - x if mirror else x
            yS = (0 if y == 0 else py - y) if mirror else y
            out[y, x] = half[yS, xS]
    return out


def avg_std(psds, exact=False):
    """:443-463, :572-583: (avg, std, the variance before its root) of the pieces' PSDs, added in list order"""
    n = len(psds)
    if exact:
        flat = np.asarray(psds, dtype=np.float64).reshape(n, -1)
        s = np.array([math.fsum(flat[:, k]) for k in range(flat.shape[1])]).reshape(psds[0].shape)
        s2 = np.array([math.fsum(flat[:, k] * flat[:, k]) for k in range(flat.shape[1])]).reshape(psds[0].shape)
    else:
        s, s2 = psds[0].copy(), psds[0] * psds[0]
        for p in psds[1:]:
            s += p
            s2 += p * p
    idiv = 1.0 / n
    avg = s * idiv
    var = s2 * idiv
    var -= avg * avg
    var = np.where(var < 0, 0.0, var)
    return avg, np.sqrt(var), var


def sum_float(psds, exact=False):
    """psd_estimator.cpp:115: magnitudes[n] += mag in floats"""
    if exact:
        flat = np.asarray(psds, dtype=np.float64).reshape(len(psds), -1)
        return np.array([math.fsum(flat[:, k]) for k in range(flat.shape[1])]).reshape(psds[0].shape)
    s = np.zeros(psds[0].shape, dtype=np.float32)
    for p in psds:
        s += p
    return s


# ---------------------------------------------------------------- psd_estimate's normalisation
def reject_outliers(v, percentil_out=0.25, steps=200):
    """xmippCore's reject_outliers as stated above, on float32 values"""
    v = np.asarray(v, dtype=np.float32)
    hmin, hmax = float(v.min()), float(v.max())
    if hmax == hmin:
        return v.copy()
    step = (hmax - hmin) / steps
    istep = 1.0 / step
    idx = np.minimum(((v.astype(np.float64).ravel() - hmin) * istep).astype(np.int64), steps - 1)
    hist = np.bincount(idx, minlength=steps).astype(np.float64)

    def percentil(mass):
        required = hist.sum() * mass / 100.0
        acc, i = 0.0, 0
        while acc < required:
            acc += hist[i]
            i += 1
        i -= 1
        if i < 0:
            return hmin
        return hmin + (i + (required - (acc - hist[i])) / hist[i]) * step
    lo, hi = percentil(percentil_out / 2), percentil(100 - percentil_out / 2)
    out = v.copy()
    out[v < lo] = np.float32(lo)
    out[v > hi] = np.float32(hi)
    return out


def normalize_psd(psd):
    """psd_estimator.cpp:123-141 on the float32 result"""
    psd = np.asarray(psd, dtype=np.float32)
    pos = psd > 0
    min_val = psd[pos].min() if pos.any() else np.finfo(np.float32).max
    min_val = np.float32(10 * math.log10(float(min_val)))
    out = np.full(psd.shape, min_val, dtype=np.float32)
    out[pos] = (10 * np.log10(psd[pos].astype(np.float64))).astype(np.float32)
    return reject_outliers(out)


# ---------------------------------------------------------------- whole runs
def compute(case, exact=False):
    """everything a case yields: the prepared pieces [n, py, px], and avg / std / var (micrograph mode and the float path) or the stack of
    the pieces' own PSDs, and the deviations every piece took its branches on"""
    T = case["dtype"]
    py, px, flags = case["py"], case["px"], case["flags"]
    prepared, psds, info = [], [], []
    for img, corners in zip(case["mic"], case["corners"]):
        for (cy, cx) in corners:
            p = prepare(img[cy:cy + py, cx:cx + px], T, flags, exact, info)
            prepared.append(p)
            psds.append(psd_double(p, exact) if T == np.float64 else psd_float(p, exact))
    out = {"pieces": np.array(prepared), "info": info}
    if case["stack"]:
        out["stack"] = np.array(psds)
    elif T == np.float64:
        out["avg"], out["std"], out["var"] = avg_std(psds, exact)
    else:
        s = sum_float(psds, exact)
        out["avg"] = half2whole(s[:, :px // 2 + 1], py, px)          # the program mirrors the half it kept
    return out


def distance(a, b):
    return float(np.abs(np.asarray(a, dtype=np.float64) - np.asarray(b, dtype=np.float64)).max() / np.abs(np.asarray(b, dtype=np.float64)).max())


def micrograph(Y, X, seed, nimg=1, constant=None):
    """noise of deviation 1 on a mean of 1000 with a gradient of several deviations per piece; float32 values that are no short sums.
    constant: (top, left, side) of a region of exactly 1000"""
    rng = np.random.default_rng(seed)
    i, j = np.meshgrid(np.arange(Y), np.arange(X), indexing="ij")
    m = 1000.0 + rng.standard_normal((nimg, Y, X)) + 0.31 * j + 0.17 * i
    m = m.astype(np.float32)
    if constant:
        t, l, s = constant
        m[:, t:t + s, l:l + s] = np.float32(1000.0)
    return m


def make_case(name, dtype, Y, X, py, px=None, overlap=0.5, skipBorders=0, mode=MICROGRAPH, pos=None, nimg=1, constant=None, seed=0):
    px = py if px is None else px
    mic = micrograph(Y, X, 100 * py + px + seed, nimg, constant)
    if dtype == np.float64:
        corners, slots, div = pieces(Y, X, py, overlap, skipBorders, mode, pos)
        flags = ADJUST | RAMP
    else:
        corners, slots, div = patches(Y, X, py, px, 0, 0, overlap), None, None
        flags = ADJUST
    return {"name": name, "dtype": dtype, "mic": mic, "py": py, "px": px, "overlap": overlap, "skipBorders": skipBorders, "mode": mode,
            "pos": pos, "corners": [corners] * nimg, "slots": slots, "div": div, "flags": flags, "stack": mode != MICROGRAPH}


def cases():
    D, F = np.float64, np.float32
    return [
        make_case("d16_skip0_70_constant", D, 83, 61, 16, constant=(0, 0, 16)),       # more than one batch of 64; a piece with a = 0
        make_case("d16_skip2_18", D, 83, 61, 16, skipBorders=2),
        make_case("d16_overlap03_step11", D, 83, 61, 16, overlap=0.3),
        make_case("d17_odd_skip1", D, 83, 61, 17, skipBorders=1),
        make_case("d20_bluestein_skip2", D, 83, 61, 20, skipBorders=2),
        make_case("d33_15", D, 83, 61, 33),
        make_case("d96_fractional_taper_4", D, 130, 110, 96),                         # capacity pieces at capacity 4
        make_case("d16_regions_skip1", D, 83, 61, 16, skipBorders=1, mode=REGIONS),
        make_case("d16_particles_5", D, 83, 61, 16, mode=PARTICLES,                   # capacity + 1; the near-edge limit, past the far edge
                  pos=[(8, 8), (60, 82), (30, 40), (8, 82), (53, 75)]),
        make_case("d16_stack_of_two", D, 83, 61, 16, skipBorders=2, nimg=2),
        make_case("d16_one_piece", D, 24, 30, 16, overlap=0.0),
        make_case("d16_three_pieces", D, 16, 32, 16),                                 # capacity - 1
        make_case("f16x24_patches", F, 83, 61, 16, 24),
        make_case("f24x16_patches", F, 83, 61, 24, 16),
        make_case("f17_odd_constant", F, 83, 61, 17, constant=(0, 0, 17)),
    ]


_RESULTS = {}


def result(case):
    """the restatement's compute(case), once, shared and read-only"""
    if case["name"] not in _RESULTS:
        out = compute(case)
        for a in out.values():
            if isinstance(a, np.ndarray):
                a.setflags(write=False)
        _RESULTS[case["name"]] = out
    return _RESULTS[case["name"]]
