"""numpy restatement of what xmipp_reconstruct_significant computes per (image, gallery projection) pair and per weighting stage:
alignImages / alignImagesConsideringMirrors (data/filters.cpp:2047-2178) with bestNonwrappingShift (:1903-1985), imedDistance
(:1269-1318) and the two weightings of reconstruct_significant.cpp (:222-226, :288-369 per image, :439-492 per direction).

Composed from the oracle's pinned primitives (oracle/pyoracle.py: best_shift, correlation_matrix, translate2d, apply_geometry2d,
correlation_index, polar_layout, polar_avg_std, polar_fft_rings); the order-1 polar sampling, the 2 N - 1 angle rotational correlation,
fastCorrelation, imed and the cumulative density functions are written here. Every decision comes back with the MARGIN by which it was
taken (relative gap to the runner-up for arg-max picks and comparisons, distance to the threshold for threshold tests), so that a
comparison against another implementation can leave out the genuine near-ties, and with the same trace bits as the device.

TEST INFRASTRUCTURE ONLY."""
import numpy as np

from oracle import pyoracle as po
from tests import synth

SHIFT_THRESHOLD = 0.95
ROTATE_THRESHOLD = 1.0
TR_SHIFT, TR_ROT, TR_NONWRAP = 1, 2, 4

_coords = {}


def rings_of(D):
    return D // 5, D // 2


def polar_coords(D):
    """The float angle cache's sample coordinates (polar.cpp:57-83) of rings D / 5 .. D / 2 as the oracle's layout holds them. The
    oracle samples B-spline coefficients only, and a cubic B-spline reproduces a linear ramp, so sampling the ramps x and y far from
    any border returns every coordinate to about 1e-15; rounding to float32 recovers the cached floats exactly."""
    if D not in _coords:
        Ri, Ro = rings_of(D)
        big = 4 * D
        ramp = np.arange(-(big // 2), big - big // 2, dtype=np.float64)
        cx = po.polar_from_cartesian(np.tile(ramp, (big, 1)), Ri, Ro, -(big // 2), -(big // 2))
        cy = po.polar_from_cartesian(np.tile(ramp[:, None], (1, big)), Ri, Ro, -(big // 2), -(big // 2))
        _coords[D] = (cx.astype(np.float32).astype(np.float64), cy.astype(np.float32).astype(np.float64))
    return _coords[D]


def _realwrap(x, x0, xF):
    if x0 <= x <= xF:
        return x
    if x < x0:
        return x - int((x - x0) / (xF - x0) - 1) * (xF - x0)
    return x - int((x - xF) / (xF - x0) + 1) * (xF - x0)


def polar_sample_linear(img):
    """getPolarFromCartesianBSpline(.., BsplineOrder 1): interpolatedElement2DOutsideZero at the wrapped coordinates (polar.h:680-699)"""
    D = img.shape[0]
    first, last = -(D // 2), -(D // 2) + D - 1
    cx, cy = polar_coords(D)
    pad = np.zeros((D + 2, D + 2))
    pad[1:-1, 1:-1] = img
    xp, yp = cx.copy(), cy.copy()
    for a in (xp, yp):
        for k in np.nonzero((a < first - 1e-6) | (a > last + 1e-6))[0]:
            a[k] = _realwrap(a[k], first - 0.5, last + 0.5)
    x0, y0 = np.floor(xp).astype(int), np.floor(yp).astype(int)
    fx, fy = xp - x0, yp - y0

    def at(i, j):
        return pad[np.clip(i - first + 1, 0, D + 1), np.clip(j - first + 1, 0, D + 1)]
    d00, d01, d10, d11 = at(y0, x0), at(y0, x0 + 1), at(y0 + 1, x0), at(y0 + 1, x0 + 1)
    d0 = d00 + (d01 - d00) * fx
    d1 = d10 + (d11 - d10) * fx
    return d0 + (d1 - d0) * fy


def polar_fourier(img, conjugated):
    """polarFourierTransform<true>(img, conjugated, D / 5, D / 2, BsplineOrder 1) (polar.cpp:152-176)"""
    Ri, Ro = rings_of(img.shape[0])
    rings = polar_sample_linear(img)
    avg, std = po.polar_avg_std(rings, Ri, Ro)
    with np.errstate(all="ignore"):
        rings = (rings - avg) * (np.float64(1.0) / np.float64(std))      # a blank image: 1 / 0, and NaN from there on, as in the reference
    return po.polar_fft_rings(rings, Ri, Ro, conjugated)


def rotational_correlation(F1, F2, D):
    """rotationalCorrelation with the local transformer set to 2 N - 1 angles (filters.cpp:2058-2059, polar.cpp:99-148): the ring sum
    into N coefficients, the un-normalised inverse real transform of length 2 N - 1"""
    Ri, Ro = rings_of(D)
    nsam, _, _ = po.polar_layout(Ri, Ro)
    N = int(nsam[-1])
    Fsum = np.zeros(N, complex)
    off = 0
    for r, n in enumerate(nsam):
        w = 2. * np.pi * float(np.float32(r + Ri))
        k = n // 2 + 1
        a, b, c, d = F1[off:off + k].real, F1[off:off + k].imag, F2[off:off + k].real, F2[off:off + k].imag
        Fsum[:k] += w * (a * c - b * d) + 1j * (w * (b * c + a * d))
        off += k
    ln = 2 * N - 1
    j = np.arange(ln)[:, None]
    k = np.arange(1, N)[None, :]
    ph = 2.0 * np.pi * ((j * k) % ln) / ln
    return Fsum[0].real + 2.0 * (Fsum[1:].real[None, :] * np.cos(ph) - Fsum[1:].imag[None, :] * np.sin(ph)).sum(1)


def _gap(best, other):
    """relative gap of a comparison; NaN operands compare false whatever their last bits, so nothing is at stake: infinity"""
    g = abs(best - other) / max(abs(best), 1e-300)
    return np.inf if np.isnan(g) else g


def best_rotation(Fref, F, D):
    """best_rotation (polar.cpp:212-231): the first maximum; (angle, margin to the runner-up)"""
    corr = rotational_correlation(Fref, F, D)
    imax = 0 if np.isnan(corr[0]) else int(np.argmax(corr))             # nothing is greater than a NaN first element
    rest = np.delete(corr, imax)
    return imax * (360. / len(corr)), _gap(corr[imax], rest.max())


def fast_correlation(x, y):
    return float((x * y).sum() / x.size)


def best_nonwrapping_shift(Iref, I):
    """bestNonwrappingShift(Iref, FFT(Iref), I) (filters.cpp:1903-1985) -> (shiftX, shiftY, replaced, margins)"""
    D = Iref.shape[0]
    margins = []
    R = po.correlation_matrix(Iref, I)
    sd = np.sqrt(abs((R * R).mean() - R.mean() ** 2))
    if sd != 0:
        adj = (R - R.mean()) / sd
        flat = np.sort(adj.ravel())
        margins.append(_gap(flat[-1], flat[-2]))                       # the arg-max of the shift map
        margins.append(np.abs(adj - flat[-1] / 1.414).min() / max(abs(flat[-1]), 1e-300))      # the growth of the neighbourhood
    sx, sy, _ = po.best_shift(Iref, I)
    tX = sx - D if sx > 0 else sx + D
    tY = sy - D if sy > 0 else sy + D
    c = [fast_correlation(I, po.translate2d(Iref, -x, -y, degree=1, wrap=False)) for x, y in ((sx, sy), (tX, sy), (sx, tY), (tX, tY))]
    fx, fy = sx, sy
    if c[1] > c[0]:
        fx = tX
    if c[2] > c[0]:
        fy = tY
    if c[3] > c[0]:
        fx, fy = tX, tY
    # two copies shifted out of the frame correlate to exactly 0 on any implementation: 0 > 0 is no near-tie
    margins += [np.inf if c[0] == 0 and c[q] == 0 else _gap(c[0], c[q]) for q in (1, 2, 3)]
    return fx, fy, (fx != sx or fy != sy), margins


def _matmul3(r, m):
    o = np.empty((3, 3))
    for i in range(3):
        for q in range(3):
            o[i, q] = r[i, 0] * m[0, q] + r[i, 1] * m[1, q] + r[i, 2] * m[2, q]
    return o


def align_chain(Iref, Fref, I, rs):
    """One order of alignImages (filters.cpp:2061-2111): rs False = shift then rotate, True = rotate then shift.
    Returns dict(M, image, corr, trace, margins)."""
    D = Iref.shape[0]
    M = np.eye(3)
    cur = I.copy()
    sX = sY = SHIFT_THRESHOLD + 1.0
    rot = ROTATE_THRESHOLD + 1.0
    trace, margins = 0, []

    def shift_step(rnd):
        nonlocal M, cur, sX, sY, trace
        margins.append(min(abs(abs(sX) - SHIFT_THRESHOLD), abs(abs(sY) - SHIFT_THRESHOLD)))
        if (sX > SHIFT_THRESHOLD or sX < -SHIFT_THRESHOLD) or (sY > SHIFT_THRESHOLD or sY < -SHIFT_THRESHOLD):
            sX, sY, replaced, mg = best_nonwrapping_shift(Iref, cur)
            margins.extend(mg)
            M[0, 2] += sX
            M[1, 2] += sY
            cur = po.apply_geometry2d(I, M, 1, False, False)
            trace |= (TR_SHIFT | (TR_NONWRAP if replaced else 0)) << (3 * rnd)

    def rot_step(rnd):
        nonlocal M, cur, rot, trace
        margins.append(abs(rot - ROTATE_THRESHOLD))
        if rot > ROTATE_THRESHOLD:
            rot, mg = best_rotation(Fref, polar_fourier(cur, True), D)
            margins.append(mg)
            a = rot * np.pi / 180.0
            c, s = np.cos(a), np.sin(a)
            M = _matmul3(np.array([[c, s, 0.], [-s, c, 0.], [0., 0., 1.]]), M)
            cur = po.apply_geometry2d(I, M, 1, False, False)
            trace |= TR_ROT << (3 * rnd)

    for rnd in range(3):
        if rs:
            rot_step(rnd)
            shift_step(rnd)
        else:
            shift_step(rnd)
            rot_step(rnd)
    return {"M": M, "image": cur, "corr": po.correlation_index(cur, Iref), "trace": trace, "margins": margins}


_w49 = np.array([[np.exp(-0.5 * (a * a + b * b)) / np.sqrt(2.0 * np.pi) for b in range(-3, 4)] for a in range(-3, 4)])


def imed_distance(I1, I2):
    """imedDistance (filters.cpp:1269-1318); the 7 x 7 weights from their formula"""
    D = I1.shape[0]
    diff = I1 - I2
    mid = D // 2
    conv = np.zeros((D, D))
    for a in range(-3, 4):
        for b in range(-3, 4):
            conv[3:D - 3, 3:D - 3] += _w49[a + 3, b + 3] * diff[3 + a:D - 3 + a, 3 + b:D - 3 + b]
    i, j = np.mgrid[0:D, 0:D]
    inside = ((i - mid) ** 2 + (j - mid) ** 2 <= mid * mid) & (i >= 3) & (i < D - 3) & (j >= 3) & (j < D - 3)
    return float(np.sqrt((conv * diff)[inside].sum()))


def align_pair(Iref, Fref, I, check_mirrors=True):
    """alignImagesConsideringMirrors (check_mirrors) or alignImages of one pair. Returns dict(M, corr, imed, trace, chains, margin):
    chains [mirror][order] as align_chain returns them plus their imed; margin = the smallest margin of any decision of the pair."""
    chains = []
    for mirror in range(2 if check_mirrors else 1):
        src = I[:, ::-1].copy() if mirror else I
        pair = [align_chain(Iref, Fref, src, False), align_chain(Iref, Fref, src, True)]
        for c in pair:
            c["imed"] = imed_distance(Iref, c["image"])
            c["margin"] = min(c["margins"])
        chains.append(pair)
    rs = [int(p[1]["corr"] > p[0]["corr"]) for p in chains]
    pick = [_gap(p[1]["corr"], p[0]["corr"]) for p in chains]
    mir = int(check_mirrors and chains[1][rs[1]]["corr"] > chains[0][rs[0]]["corr"])
    if check_mirrors:
        pick.append(_gap(chains[1][rs[1]]["corr"], chains[0][rs[0]]["corr"]))
    win = chains[mir][rs[mir]]
    M = win["M"].copy()
    if mir:
        M[0, 0] *= -1
        M[1, 0] *= -1
    trace = mir | (rs[mir] << 1) | (chains[mir][0]["trace"] << 2) | (chains[mir][1]["trace"] << 11)
    margin = min([c["margin"] for p in chains for c in p] + pick)
    return {"M": M, "corr": win["corr"], "imed": win["imed"], "trace": trace, "chains": chains, "margin": margin, "rs": rs, "mirror": mir}


def gallery_transforms(gallery):
    return [polar_fourier(g, False) for g in gallery]


def align_all(gallery, images, check_mirrors=True):
    """Every (image, projection) pair: list over images of lists over projections of align_pair's dicts"""
    F = gallery_transforms(gallery)
    return [[align_pair(gallery[g], F[g], img, check_mirrors) for g in range(len(gallery))] for img in images]


# ---------------------------------------------------------------- weights
def cdf(values):
    """cumlativeDensityFunction as the project pins it: (1-based ascending rank) / n, equal values ranked by position"""
    v = np.asarray(values, np.float64)
    order = np.argsort(v, kind="stable")
    out = np.empty(len(v))
    out[order] = (np.arange(len(v)) + 1) / len(v)
    return out


def shifts_of(M):
    """transformationMatrix2Parameters2D(M.inv()) (reconstruct_significant.cpp:216-219) -> (flip, shiftX, shiftY, psi)"""
    m = M.ravel()
    o = np.empty(9)
    o[0] = m[8] * m[4] - m[7] * m[5]; o[1] = -(m[8] * m[1] - m[7] * m[2]); o[2] = m[5] * m[1] - m[4] * m[2]
    o[3] = -(m[8] * m[3] - m[6] * m[5]); o[4] = m[8] * m[0] - m[6] * m[2]; o[5] = -(m[5] * m[0] - m[3] * m[2])
    o[6] = m[7] * m[3] - m[6] * m[4]; o[7] = -(m[7] * m[0] - m[6] * m[1]); o[8] = m[4] * m[0] - m[3] * m[1]
    A = o * (1.0 / (m[0] * o[0] + m[3] * o[1] + m[6] * o[2]))
    flip = (A[0] * A[4] - A[1] * A[3]) < 0
    sgn = -1 if flip else 1
    cosine, sine = sgn * A[0], sgn * A[1]
    inv = 1 / np.sqrt(cosine * cosine + sine * sine)
    return bool(flip), A[2] * inv, A[5] * inv, float(np.degrees(np.arctan2(sine, cosine)))


def penalise(M, cc, imed, max_shift):
    """:222-226 -> penalised copies of cc and imed [N][G]"""
    cc, imed = cc.copy(), imed.copy()
    if max_shift > 0:
        for n in range(cc.shape[0]):
            for g in range(cc.shape[1]):
                _, sx, sy, _ = shifts_of(M[n, g])
                if abs(sx) > max_shift or abs(sy) > max_shift:
                    cc[n, g] /= 3
                    imed[n, g] *= 3
    return cc, imed


def image_weights(M, cc, imed, D, one_alpha, apply_fisher, use_imed, max_shift):
    """:288-369 on penalised cc, imed [N][G] -> weight [N][G] (0 where the pair is not selected)"""
    N, G = cc.shape
    w = np.zeros((N, G))
    with np.errstate(all="ignore"):
        for n in range(N):
            bestCorr, bestImed = cc[n].max(), imed[n].min()
            rl = bestCorr * one_alpha
            z = 0.5 * np.log((1 + rl) / (1 - rl))
            ccl = np.tanh(z - 2.96 * np.sqrt(1.0 / (D * D)))
            cdfcc, cdfimed = cdf(cc[n]), cdf(imed[n])
            for g in range(G):
                condition = (apply_fisher and cc[n, g] >= ccl) or not apply_fisher
                condition = condition and cdfcc[g] >= one_alpha
                if not condition:
                    continue
                if max_shift > 0:
                    _, sx, sy, _ = shifts_of(M[n, g])
                    if abs(sx) > max_shift or abs(sy) > max_shift:
                        continue
                t = cdfcc[g] * (cc[n, g] / bestCorr)
                if use_imed:
                    t *= (1 - cdfimed[g]) * (bestImed / imed[n, g])
                w[n, g] = t
    return w


def neighbour_counts(rot, tilt, n_vols, ang_distance):
    """k [g]: the directions of the same volume with Euler_distanceBetweenAngleSets(.., only_projdir) < ang_distance (:456-462)"""
    G = len(rot)
    nd = G // n_vols
    a, b = np.radians(rot), np.radians(tilt)
    d = np.stack([np.sin(b) * np.cos(a), np.sin(b) * np.sin(a), np.cos(b)], 1)
    k = np.zeros(G, int)
    for v in range(n_vols):
        for d1 in range(nd):
            for d2 in range(nd):
                if d1 != d2:
                    ang = np.degrees(np.arccos(np.clip(d[v * nd + d1] @ d[v * nd + d2], -1.0, 1.0)))
                    k[v * nd + d1] += ang < ang_distance
    return k


def repeated_list_cdf(values, copies):
    """the cdf of the first N entries of `values` repeated `copies` times, by the closed form: rank = copies . less + equalBefore + 1"""
    v = np.asarray(values, np.float64)
    N = len(v)
    less = (v[None, :] < v[:, None]).sum(1)
    eqb = np.array([(v[:i] == v[i]).sum() for i in range(N)])
    return (copies * less + eqb + 1) / (copies * N)


def direction_weights(w, cc, k, one_alpha, strict):
    """:439-492 as written: the direction's own N correlations repeated 1 + k times"""
    w = w.copy()
    N, G = cc.shape
    for g in range(G):
        c = repeated_list_cdf(cc[:, g], 1 + int(k[g]))
        iBest = 1.0 / cc[:, g].max()
        for n in range(N):
            if (c[n] >= one_alpha or not strict) and w[n, g] > 0:
                w[n, g] *= cc[n, g] * iBest * c[n]
            else:
                w[n, g] = 0
    return w


def weights(M, cc, imed, D, n_vols, rot, tilt, ang_distance, one_alpha, apply_fisher=False, use_imed=False, strict=False, max_shift=-1.0):
    """both stages -> (weight, penalised cc, penalised imed)"""
    cc, imed = penalise(M, cc, imed, max_shift)
    w = image_weights(M, cc, imed, D, one_alpha, apply_fisher, use_imed, max_shift)
    return direction_weights(w, cc, neighbour_counts(rot, tilt, n_vols, ang_distance), one_alpha, strict), cc, imed


# ---------------------------------------------------------------- the population of the parity tests
SEED = 2000
CASES = {20: (1, 7, 5), 32: (2, 6, 5), 48: (1, 7, 3)}          # D: (volumes, directions, images)
_population = {}


def _asymmetric_phantom(D, seed):
    """synth's blobs plus one off-centre blob: no projection has a symmetry that would make a correlation map tie"""
    vol = synth.phantom(D, seed=seed, nblobs=12)
    z, y, x = np.mgrid[-(D // 2):D - D // 2, -(D // 2):D - D // 2, -(D // 2):D - D // 2].astype(np.float64)
    s = D / 16.0
    return vol + 1.5 * np.exp(-((x - 0.2 * D) ** 2 + (y + 0.12 * D) ** 2 + (z - 0.07 * D) ** 2) / (2 * s * s))


def population(D):
    """The gallery [G][D][D], its direction angles and the images [N][D][D] of one parity case: gallery projections of asymmetric
    phantoms, every image a projection rotated, shifted by up to 5 px and possibly mirrored, with noise at SNR 1; image 0 carries a
    shift just beyond D / 2 (the circular correlation aliases it, and a non-wrapping alternative wins), image 1 is a projection as it stands (steps are skipped)."""
    if D in _population:
        return _population[D]
    from scipy import ndimage
    nv, nd, N = CASES[D]
    rng = np.random.default_rng(SEED + D)
    dirs = synth.fibonacci_directions(nd)
    gallery = np.stack([synth.project(_asymmetric_phantom(D, 7 + v), r, t, 0.0) for v in range(nv) for r, t in dirs])
    rot, tilt = np.tile(dirs[:, 0], nv), np.tile(dirs[:, 1], nv)
    images = np.empty((N, D, D))
    for i in range(N):
        g = 0 if i == 0 else int(rng.integers(len(gallery)))
        img = gallery[g]
        if i == 0:
            img = ndimage.shift(ndimage.rotate(img, 3.0, reshape=False, order=3, mode="constant"), (0.0, D / 2 + 1.5), order=1, mode="constant")
        elif i > 1:
            img = ndimage.rotate(img, float(rng.uniform(0, 360)), reshape=False, order=3, mode="constant")
            if rng.integers(2):
                img = img[:, ::-1]
            img = ndimage.shift(img, rng.uniform(-5, 5, 2), order=1, mode="constant")
        images[i] = img + rng.standard_normal(img.shape) * img.std()
    _population[D] = (np.ascontiguousarray(gallery), rot, tilt, images)
    return _population[D]


_reference = {}


def reference(D):
    """align_all of the case's population, computed once and shared"""
    if D not in _reference:
        gallery, _, _, images = population(D)
        _reference[D] = align_all(gallery, images, True)
    return _reference[D]


# ---------------------------------------------------------------- weights past one tile of 256 and one block
WEIGHT_D, WEIGHT_MAX_SHIFT, WEIGHT_ONE_ALPHA = 20, 3.0, 0.5
WEIGHT_SEED = 42             # (41 drew a direction of (5, 300) whose five correlations are equal: nothing for one_alpha to split under 40 degrees)
# (N, G): (volumes, directions per volume). The device ranks an image's G values through tiles of 256 (k_rs_image_weights) and a
# direction's N values through tiles of 256 in blocks of 256 images (k_rs_direction_weights)
WEIGHT_SHAPES = {(261, 12): (2, 6),          # N: two blocks, tiles 256 + 5
                 (5, 300): (2, 150),         # G: tiles 256 + 44
                 (257, 256): (1, 256)}       # N: a tile of one; G: one exact tile
# (apply_fisher, use_imed, strict, max_shift)
WEIGHT_OPTIONS = [(False, False, False, -1.0), (True, True, True, 3.0), (False, True, False, 3.0), (True, False, True, -1.0)]
WEIGHT_ANG = (10.0, 40.0)
_SIX = (np.array([0., 0., 0., 90., 180., 270.]), np.array([20., 28., 50., 90., 90., 120.]))   # 0 and 1 are 8 degrees apart, 2 is 30 from 0
_weight_population, _weight_stage = {}, {}


def weight_population(shape):
    """Hand-made inputs of both weighting stages, (M [N, G, 3, 3], cc [N, G], imed [N, G], n_vols, rot [G], tilt [G]). cc: multiples of
    1 / 64 in (0.05, 0.95), drawn towards the low end so that the Fisher limit of an image (a little below half its best correlation)
    lies among the values its percentile keeps, and up to a level of the image's own (1, 0.84, 0.68, 0.51, 0.35 of the range, in turn), so that what an image
    keeps lies on both sides of its directions' medians and --strictDirection has something to cut; imed: multiples of 1 / 8 in (1, 40): equal values are common. M: a rotation, for every
    fourth pair a mirror, and a shift of up to 2.9 px per axis, for roughly a tenth of the pairs 3.1 .. 6 px on one axis"""
    if shape not in _weight_population:
        N, G = shape
        nv, nd = WEIGHT_SHAPES[shape]
        rng = np.random.default_rng(WEIGHT_SEED + N + G)
        level = (1.0 - 0.65 * (np.arange(N) % 5) / 4.0)[:, None]
        cc = (4 + np.floor(57 * level * rng.uniform(0, 1, shape) ** 2)) / 64.0
        imed = rng.integers(9, 320, shape) / 8.0
        ang = rng.uniform(0, 2 * np.pi, shape)
        sh = rng.uniform(-2.9, 2.9, shape + (2,))
        far = rng.uniform(0, 1, shape) < 0.1
        axis = rng.integers(0, 2, shape)
        big = rng.uniform(3.1, 6.0, shape) * np.where(rng.integers(0, 2, shape) == 1, 1.0, -1.0)
        for a in range(2):
            sh[..., a] = np.where(far & (axis == a), big, sh[..., a])
        A = np.zeros(shape + (3, 3))
        c, s = np.cos(ang), np.sin(ang)
        flip = np.where(rng.integers(0, 4, shape) == 0, -1.0, 1.0)
        A[..., 0, 0], A[..., 0, 1], A[..., 0, 2] = flip * c, flip * s, sh[..., 0]
        A[..., 1, 0], A[..., 1, 1], A[..., 1, 2] = -s, c, sh[..., 1]
        A[..., 2, 2] = 1.0
        M = np.ascontiguousarray(np.linalg.inv(A))
        if nd == 6:
            rot, tilt = (np.tile(a, nv) for a in _SIX)
        else:
            dirs = synth.fibonacci_directions(nd)
            rot, tilt = np.tile(dirs[:, 0], nv), np.tile(dirs[:, 1], nv)
        _weight_population[shape] = (M, cc, imed, nv, rot, tilt)
    return _weight_population[shape]


def all_shifts(M):
    """shifts_of for every pair -> (shiftX [N, G], shiftY [N, G])"""
    N, G = M.shape[:2]
    out = np.array([shifts_of(M[n, g])[1:3] for n in range(N) for g in range(G)]).reshape(N, G, 2)
    return out[..., 0], out[..., 1]


def direction_angles(rot, tilt, n_vols):
    """the angles neighbour_counts compares with ang_distance: every ordered pair of different directions of one volume, in degrees"""
    nd = len(rot) // n_vols
    a, b = np.radians(rot), np.radians(tilt)
    d = np.stack([np.sin(b) * np.cos(a), np.sin(b) * np.sin(a), np.cos(b)], 1)
    return np.array([np.degrees(np.arccos(np.clip(d[v * nd + d1] @ d[v * nd + d2], -1.0, 1.0)))
                     for v in range(n_vols) for d1 in range(nd) for d2 in range(nd) if d1 != d2])


def weights_of(shape, ang_distance, options):
    """weights() of a weight_population, with what the options share (the penalty per max_shift, the neighbour counts per
    ang_distance, the per-image stage) computed once: the same calls in the same order as weights()"""
    M, cc0, imed0, nv, rot, tilt = weight_population(shape)
    apply_fisher, use_imed, strict, max_shift = options

    def once(key, f):
        if key not in _weight_stage:
            _weight_stage[key] = f()
        return _weight_stage[key]
    cc, imed = once((shape, "penalise", max_shift), lambda: penalise(M, cc0, imed0, max_shift))
    k = once((shape, "neighbours", ang_distance), lambda: neighbour_counts(rot, tilt, nv, ang_distance))
    w = once((shape, "image", apply_fisher, use_imed, max_shift), lambda: image_weights(M, cc, imed, WEIGHT_D, WEIGHT_ONE_ALPHA, apply_fisher, use_imed, max_shift))
    return once((shape, "direction", ang_distance, options), lambda: direction_weights(w, cc, k, WEIGHT_ONE_ALPHA, strict)), cc, imed
