"""numpy fp64 restatement of xmipp_volume_align (reconstruction/volume_align_prog.cpp, ProgAlignVolumes): applyTransformation's matrix and
its inverse, applyGeometry(LINEAR) with homogeneous 4 x 4 source coordinates (the direct form: x A00 + y A01 + z A02 + A03), the two-pass
correlationIndex and rms within a mask, the exhaustive search's ten loops, fitness, the search's first minimum and the Powell branch.

xmippCore is not in the reference tree. correlationIndex follows oracle/xo_bspline.cpp:330-346 (computeAvgStdev's integer N / (N - 1)) with
a mask added; the trilinear rule, realWRAP and the range tests are tests/symmetrize_ref.py's. `onepass` switches the fit between the
reference's two passes over Vaux (mean_y first, then sum (x - mean_x)(y - mean_y)) and the one-pass identity the device uses
(sum (x - mean_x) y - mean_y sum (x - mean_x)); the device tolerance is derived from the difference of the two
(tests/test_volume_align_ref.py). fitness_exact is the one-pass form with every sum taken exactly (math.fsum)."""
import math

import numpy as np

from tests.symmetrize_ref import ACC, interp_linear3d, inv3x3, phantom, realwrap, threshold_margin, wrap_edge_mask  # noqa: F401

COVARIANCE, LEAST_SQUARES = 1, 2


# ---------------------------------------------------------------- matrices
def euler_matrix(rot, tilt, psi):
    """Euler_angles2matrix, closed form (function_tests/test_geometry_main.cpp:46-65)"""
    a, b, g = rot * math.pi / 180.0, tilt * math.pi / 180.0, psi * math.pi / 180.0
    ca, cb, cg, sa, sb, sg = math.cos(a), math.cos(b), math.cos(g), math.sin(a), math.sin(b), math.sin(g)
    cc, cs, sc, ss = cb * ca, cb * sa, sb * ca, sb * sa
    return [[cg * cc - sg * sa, cg * cs + sg * ca, -cg * sb],
            [-sg * cc - cg * sa, -sg * cs + cg * ca, sg * sb],
            [sc, ss, cb]]


def _mul4(A, B):
    return [[sum((A[i][k] * B[k][j] for k in range(4)), 0.0) for j in range(4)] for i in range(4)]


def is_identity4(A):
    return bool(np.all(np.abs(np.asarray(A) - np.eye(4)) <= ACC))


def matrix(p):
    """applyTransformation's A (:61-91), its inverse (cofactor inverse of the 3 x 3 block, -Rinv t) and isIdentity; python floats"""
    flip, _, _, rot, tilt, psi, scale, z, y, x = (float(v) for v in p)
    if flip < 0:
        z = -z + 1
    E = euler_matrix(rot, tilt, psi)
    M = [E[0] + [0.0], E[1] + [0.0], E[2] + [0.0], [0.0, 0.0, 0.0, 1.0]]
    for i in range(4):
        M[i][2] *= flip
    T = [[1.0, 0.0, 0.0, x], [0.0, 1.0, 0.0, y], [0.0, 0.0, 1.0, z], [0.0, 0.0, 0.0, 1.0]]
    S = [[scale, 0.0, 0.0, 0.0], [0.0, scale, 0.0, 0.0], [0.0, 0.0, scale, 0.0], [0.0, 0.0, 0.0, 1.0]]
    A = np.array(_mul4(_mul4(M, T), S))
    Ri = inv3x3(A[:3, :3])
    Ainv = np.zeros((4, 4))
    Ainv[:3, :3] = Ri
    for r in range(3):
        Ainv[r, 3] = -(float(Ri[r, 0]) * float(A[0, 3]) + float(Ri[r, 1]) * float(A[1, 3]) + float(Ri[r, 2]) * float(A[2, 3]))
    Ainv[3, 3] = 1.0
    return A, Ainv, is_identity4(A)


# ---------------------------------------------------------------- applyTransformation
def source_coords4(shape, Ainv, wrap):
    """per axis (x first): the coordinate the range test saw, the coordinate after it, and whether the voxel takes the outside value"""
    Z, Y, X = shape
    z, y, x = np.meshgrid(*[np.arange(d, dtype=np.float64) - d // 2 for d in shape], indexing="ij")
    dims = (X, Y, Z)
    tested, final = [], []
    outside = np.zeros(shape, dtype=bool)
    for a in range(3):
        c = x * Ainv[a, 0] + y * Ainv[a, 1] + z * Ainv[a, 2] + Ainv[a, 3]
        cen = dims[a] // 2
        lo, hi = float(-cen), float(dims[a] - cen - 1)
        bad = (c < lo - ACC) | (c > hi + ACC)
        tested.append(c)
        if wrap:
            w = c.copy()
            if bad.any():
                w[bad] = realwrap(c[bad], lo - 0.5, hi + 0.5)
            final.append(w)
        else:
            final.append(c)
            outside |= bad
    return tested, final, outside


def apply_transformation(V2, p, wrap, coords=None):
    """applyTransformation (:56-97): applyGeometry(LINEAR, Vaux, V2, A, IS_NOT_INV, wrap), outside value 0, then the grey values.
    coords: a list that receives the coordinates the range tests saw"""
    V2 = np.asarray(V2, dtype=np.float64)
    _, Ainv, ident = matrix(p)
    if ident:
        out = V2.copy()
    else:
        tested, final, outside = source_coords4(V2.shape, Ainv, wrap)
        if coords is not None:
            coords.append(tested)
        inside = ~outside
        out = np.zeros(V2.shape)
        out[inside] = interp_linear3d(V2, *[f[inside] for f in final], wrap)
    gs, gsh = float(p[1]), float(p[2])
    if gs != 1 or gsh != 0:
        out = out * gs + gsh
    return out


# ---------------------------------------------------------------- the fits
def _inside(x, mask):
    return np.ones(x.shape, dtype=bool) if mask is None else np.asarray(mask) != 0


def avg_stdev(v):
    """computeAvgStdev: the deviation is sqrt(|sum v^2 / N - avg^2| (N / (N - 1))) with the quotient in integers"""
    n = v.size
    if n == 0:
        return 0.0, 0.0
    avg = float(v.sum()) / n
    if n <= 1:
        return avg, 0.0
    sd = float((v * v).sum()) / n - avg * avg
    sd *= float(n // (n - 1))
    return avg, math.sqrt(abs(sd))


def correlation_index(x, y, mask=None, onepass=False):
    m = _inside(x, mask)
    xs, ys = x[m], y[m]
    n = xs.size
    mean_x, sd_x = avg_stdev(xs)
    mean_y, sd_y = avg_stdev(ys)
    if n == 0 or abs(sd_x) < ACC or abs(sd_y) < ACC:
        return 0.0
    if onepass:
        r = float(((xs - mean_x) * ys).sum()) - mean_y * float((xs - mean_x).sum())
    else:
        r = float(((xs - mean_x) * (ys - mean_y)).sum())
    return r / ((sd_x * sd_y) * n)


def rms(x, y, mask=None):
    m = _inside(x, mask)
    n = int(m.sum())
    if n == 0:
        return 0.0
    d = x[m] - y[m]
    return math.sqrt(float((d * d).sum()) / n)


def fitness(V1, V2, p, method, wrap, mask=None, onepass=False, coords=None):
    vaux = apply_transformation(V2, p, wrap, coords)
    if method == COVARIANCE:
        return -correlation_index(V1, vaux, mask, onepass)
    return rms(V1, vaux, mask)


def fitness_exact(V1, V2, p, method, wrap, mask=None):
    """the fit from exact sums: the per-voxel fp64 terms of the one-pass form (y, y^2, (x - mean_x) y, (x - y)^2, and x, x^2, x - mean_x
    for what depends on V1 alone), every sum taken with math.fsum (the correctly rounded sum of its terms, whatever their order), then the
    finish in double as the device writes it. It decides whose rounding a difference between the device and the restatement is"""
    vaux = apply_transformation(V2, p, wrap)
    m = _inside(V1, mask)
    xs, ys = V1[m], vaux[m]
    n = xs.size
    if method == LEAST_SQUARES:
        if n == 0:
            return 0.0
        d = xs - ys
        return math.sqrt(math.fsum(d * d) / n)
    if n <= 1:
        return -0.0
    mean_x = math.fsum(xs) / n
    sd_x = math.sqrt(abs((math.fsum(xs * xs) / n - mean_x * mean_x) * float(n // (n - 1))))
    mean_y = math.fsum(ys) / n
    sd_y = math.sqrt(abs((math.fsum(ys * ys) / n - mean_y * mean_y) * float(n // (n - 1))))
    if abs(sd_x) < ACC or abs(sd_y) < ACC:
        return -0.0
    dx = xs - mean_x
    return -((math.fsum(dx * ys) - mean_y * math.fsum(dx)) / ((sd_x * sd_y) * n))


def stats(V1, mask=None):
    """what the device forms once: n, mean_x, stddev_x, sum (x - mean_x)"""
    xs = V1[_inside(V1, mask)]
    mean_x, sd_x = avg_stdev(xs)
    return float(xs.size), mean_x, sd_x, float((xs - mean_x).sum())


# ---------------------------------------------------------------- the searches
RANGE_NAMES = ("grey_scale", "grey_shift", "rot", "tilt", "psi", "scale", "z", "y", "x")


def trials(ranges, consider_mirror=False, tell=False):
    """the ten loops of :363-384 with double loop variables, and the progress bar's count `times` (:330-352). ranges: (first, last, step)
    of RANGE_NAMES in that order; a zero step is 1 (readParams)"""
    r = [(float(a), float(b), 1.0 if float(s) == 0 else float(s)) for a, b, s in ranges]
    times = 1
    if not tell:
        if consider_mirror:
            times *= 2
        for a, b, s in r:
            if a != b:
                times *= int(math.floor(1 + (b - a) / s))
    out = []

    def loop(level, cur):
        if level == 9:
            out.append(cur[:])
            return
        a, b, s = r[level]
        v = a
        while v <= b:
            cur.append(v)
            loop(level + 1, cur)
            cur.pop()
            v += s

    for mirror in range(2 if consider_mirror else 1):
        loop(0, [-1.0 if mirror else 1.0])
    return np.array(out, dtype=np.float64).reshape(-1, 10), times


def search(V1, V2, tr, method, wrap, mask=None, onepass=False):
    """(index of the first minimum, its fit, every fit), fit < best_fit || first (:388)"""
    fits = np.array([fitness(V1, V2, p, method, wrap, mask, onepass) for p in tr])
    best, idx = None, -1
    for t, f in enumerate(fits):
        if idx < 0 or f < best:
            best, idx = f, t
    return idx, float(best), fits


def local_steps(method, only_shift=False, dont_scale=False):
    """the steps of :412-418"""
    s = np.ones(9)
    if only_shift:
        s[:6] = 0
    if method == COVARIANCE:
        s[0] = s[1] = 0
    if dont_scale:
        s[5] = 0
    return s


def local(minimize, V1, V2, x0, method, wrap, mask=None, consider_mirror=False, only_shift=False, dont_scale=False):
    """--local (:406-446). minimize(f, x0, steps, ftol) -> (x, fmin, iterations): the library's Powell (xmipp3_amd.powell_minimize).
    Returns (best 10-vector, best fit, [(x, fit) per mirror])"""
    steps = local_steps(method, only_shift, dont_scale)
    best, best_fit, runs = None, 1e38, []
    first = True
    for mirror in range(2 if consider_mirror else 1):
        flip = -1.0 if mirror else 1.0
        x, f, _ = minimize(lambda v: fitness(V1, V2, [flip] + list(v), method, wrap, mask), np.array(x0, dtype=np.float64), steps, 0.01)
        runs.append((np.array(x), f))
        if f < best_fit or first:
            best, best_fit = np.concatenate([[flip], x]), f
        first = False
    return best, best_fit, runs


def ftol_halfwidths(V1, V2, best, method, wrap, mask=None, ftol=0.01, only_shift=False, dont_scale=False):
    """What Powell's stopping rule leaves open around a minimum `best` (10-vector): for every searched variable the largest step of the grid
    1e-3 2^k for which the fit at best +- step stays within ftol |fmin| of the minimum, the decrease below which a sweep ends the search.
    A fixed variable gets 0"""
    best = np.array(best, dtype=np.float64)
    fmin = fitness(V1, V2, best, method, wrap, mask)
    steps = local_steps(method, only_shift, dont_scale)
    out = np.zeros(9)
    for i in range(9):
        if steps[i] == 0:
            continue
        d = 1e-3
        while d < 64:
            worst = max(fitness(V1, V2, best + s * d * np.eye(10)[i + 1], method, wrap, mask) for s in (1.0, -1.0))
            if worst - fmin > ftol * abs(fmin):
                break
            out[i] = d
            d *= 2
    return out


# ---------------------------------------------------------------- the device tests' cases and bound
# bricks are 8 x 8 x 4 (X, Y, Z). (29, 41, 43): 6 x 6 x 8 = 288 bricks, past one step of the finish's stride of 256; (37, 49, 57):
# 8 x 7 x 10 = 560, so that threads 0 .. 47 of the finish add three bricks and the others two. Both leave a remainder on every axis
BIG_SHAPES = [(29, 41, 43), (37, 49, 57)]
SHAPES = [(16, 16, 16), (17, 17, 17), (9, 10, 12), (20, 18, 13)] + BIG_SHAPES


def bricks(shape):
    Z, Y, X = shape
    return ((X + 7) // 8) * ((Y + 7) // 8) * ((Z + 3) // 4)
# 16 times the largest relative difference (to max(1, |fit|)) between the two-pass fit and the one-pass identity over every trial of
# parity_cases(), rounded up to a power of ten (tests/test_volume_align_ref.py derives and asserts it)
BOUND = 1e-14
PLANTED = [1.0, 1.0, 0.0, 13.7, 41.3, -27.9, 0.93, 1.3, -2.6, 0.4]


def trial_list(shape, method, wrap):
    """generic poses, the identity, integer shifts, both flips, a shift larger than the box (wrap) or a pose that sends most of the box
    outside (dontWrap), grey values other than 1 / 0 under LEAST_SQUARES"""
    Z, Y, X = shape
    t = [PLANTED,
         [-1.0, 1.0, 0.0, -27.9, 13.7, 41.3, 1.08, 0.4, 1.3, -2.6],
         [1.0, 1.0, 0.0, 0.0, 0.0, 0.0, 1.0, 0.0, 0.0, 0.0],
         [1.0, 1.0, 0.0, 0.0, 0.0, 0.0, 1.0, 2.0, -1.0, 3.0],
         [-1.0, 1.0, 0.0, 0.0, 0.0, 0.0, 1.0, 0.0, 0.0, 0.0],
         [-1.0, 1.0, 0.0, 0.0, 0.0, 0.0, 1.0, -3.0, 2.0, 1.0],
         [1.0, 1.0, 0.0, 41.3, -27.9, 13.7, 1.0, -2.6, 0.4, 1.3],
         [1.0, 1.0, 0.0, 200.3, 100.7, -75.1, 1.08, 0.0, 0.0, 0.0]]
    if wrap:
        t.append([1.0, 1.0, 0.0, 0.0, 0.0, 0.0, 1.0, 0.4, -(Y + 3.3), X + 7.3])
        t.append([1.0, 1.0, 0.0, 13.7, 0.0, 0.0, 0.93, 2.0 * Z + 1.3, 0.4, -2.6])
    else:
        t.append([1.0, 1.0, 0.0, 13.7, 41.3, -27.9, 0.45, 1.3, -2.6, 0.4])
        t.append([1.0, 1.0, 0.0, 0.0, 0.0, 0.0, 1.0, 0.4, 0.7 * Y + 0.3, -(0.6 * X + 0.2)])
    if method == LEAST_SQUARES:
        t.append([1.0, 1.2, -0.05] + PLANTED[3:])
        t.append([-1.0, 0.8, 0.1, 0.0, 0.0, 0.0, 1.0, 0.0, 0.0, 0.0])
        t.append([1.0, 1.0, 0.07, 0.0, 0.0, 0.0, 1.0, 0.0, 0.0, 0.0])
    return np.array(t, dtype=np.float64)


def parity_cases():
    """(shape, method, wrap, masked) of every case the device's fits are compared on"""
    return [(s, m, w, k) for s in SHAPES for m in (COVARIANCE, LEAST_SQUARES) for w in (True, False) for k in (False, True)]


def circular_mask(shape, R1):
    """BinaryCircularMask about the Xmipp origin: R1 < 0 keeps r <= |R1|"""
    g = np.meshgrid(*[np.arange(d, dtype=np.float64) - d // 2 for d in shape], indexing="ij")
    r2 = g[0] * g[0] + g[1] * g[1] + g[2] * g[2]
    return (r2 <= R1 * R1 if R1 < 0 else r2 >= R1 * R1).astype(np.int32)


_VOLS = {}


def volumes(shape, wrap):
    """V2 a phantom, V1 the planted pose of it (float32 values, so that files carry them exactly) plus a little of another phantom"""
    key = (shape, wrap)
    if key not in _VOLS:
        V2 = phantom(shape, 7)
        V1 = apply_transformation(V2, PLANTED, wrap) + 0.02 * (phantom(shape, 8) - 0.25)
        _VOLS[key] = (V1.astype(np.float32).astype(np.float64), V2)
    return _VOLS[key]


def case_mask(shape, masked):
    return circular_mask(shape, -(min(shape) // 2 - 1.0)) if masked else None


def preconditions(shape, tr, wrap):
    """(the smallest distance of any tested coordinate of any trial to a threshold min - 1e-6 / max + 1e-6, the number of voxels with a
    coordinate within 1e-9 of a wrap edge)"""
    coords = []
    for p in tr:
        apply_transformation(np.zeros(shape), p, wrap, coords)
    margin = min((threshold_margin(shape, t) for t in coords), default=np.inf)
    edge = int(wrap_edge_mask(shape, coords).sum()) if wrap else 0
    return margin, edge


# ---------------------------------------------------------------- more than one tile of trials
TILE = 8                                            # VA_TILE: the trials of one workgroup
TILE_CAPACITIES = (8, 9, 13, 64)
# (method, wrap, masked) on 17^3: 13, 13 and 10 trials
TILE_CASES = [(LEAST_SQUARES, True, True), (LEAST_SQUARES, False, False), (COVARIANCE, True, False)]


def launches(m, capacity):
    """the trials of every launch of a list of m, and of every tile (blockIdx.y) of each"""
    out = []
    for t0 in range(0, m, capacity):
        mb = min(capacity, m - t0)
        out.append([min(TILE, mb - a) for a in range(0, mb, TILE)])
    return out


# ---------------------------------------------------------------- a search of more than 256 trials in one launch
LONG_SHAPE, LONG_METHOD, LONG_WRAP = (9, 10, 12), COVARIANCE, True
LONG_RANGES = [(1, 1, 1), (0, 0, 1), (1.7, 25.7, 4), (29.3, 53.3, 4), (-39.9, -15.9, 4), (0.93, 0.93, 1), (1.3, 1.3, 1), (-2.6, -2.6, 1), (0.4, 0.4, 1)]
LONG_CAPACITIES = (1024, 300, 256)
_LONG = {}


def long_search():
    """(pool of distinct trials [588, 10] with the restatement's fit of each, the index of the best in the pool, {name: indices into the
    pool}): the lists of the long search. The best trial is taken out of its place in the grid (a filler takes it) and planted
      "planted": at 4 and 5 (one chunk of k_va_select when per = 3), at 299 .. 302 and as the last of 595 entries.
                 per = 3: 299 | 300 are the last of chunk 99 and the first of chunk 100; 595 = 198 . 3 + 1, the last chunk holds one trial.
                 Launches of 300: 299 | 300 are the last of one launch and the first of the next, and 301 | 302 of the second launch
                 (295 trials, per = 2, local 1 | 2) lie in two chunks; the last chunk holds one trial.
      "late":    the same without the two at 4 and 5: the winner, 297, is the first of four; per = 3 keeps 297 .. 299 in chunk 99 and
                 300 in chunk 100; launches of 300 (per = 2) cut 297 | 298 into two chunks and 300 into the next launch.
      "last":    the last entry alone, index 588 of 589 = 196 . 3 + 1: a chunk of its own when per = 3 and when per = 2 (289 trials)."""
    if not _LONG:
        tr, _ = trials(LONG_RANGES, consider_mirror=True)
        V1, V2 = volumes(LONG_SHAPE, LONG_WRAP)
        idx, best, fits = search(V1, V2, tr, LONG_METHOD, LONG_WRAP)
        filler = 0 if idx != 0 else 1
        grid = [filler if t == idx else t for t in range(len(tr))]
        planted = grid[:4] + [idx, idx] + grid[4:297] + [idx] * 4 + grid[297:] + [idx]
        late = planted[:4] + planted[6:]
        last = grid + [idx]
        _LONG.update(tr=tr, fits=fits, best=idx, lists={"planted": np.array(planted), "late": np.array(late), "last": np.array(last)})
    return _LONG["tr"], _LONG["fits"], _LONG["best"], _LONG["lists"]


def select_chunks(m):
    """per of k_va_select for a launch of m fits"""
    return (m + 255) // 256


# ---------------------------------------------------------------- degenerate exits
DEGENERATE_SHAPE = (9, 10, 12)
SMALLEST_SHAPE = (2, 3, 5)


def degenerate_cases():
    """{name: (shape, V1, V2, mask, {wrap: extra trials})}: what leaves the fit by an early exit. Every case runs R.trial_list of its shape
    under both methods and both wraps, with the extra trials appended"""
    shape = DEGENERATE_SHAPE
    Z, Y, X = shape
    V1, V2 = volumes(shape, True)
    disc = case_mask(shape, True)
    one = np.zeros(shape, np.int32)
    one[Z // 2 + 1, Y // 2 - 2, X // 2 + 3] = 1
    odd = disc.copy()
    odd[disc != 0] = np.where(np.arange(int(disc.sum())) % 2 == 0, 2, -1)
    # twice the box away along every axis: under dontWrap every voxel is outside, COVARIANCE gives 0 and LEAST_SQUARES rms(V1)
    away = {False: [[1.0, 1.0, 0.0, 0.0, 0.0, 0.0, 1.0, 2.0 * Z, 2.0 * Y, 2.0 * X]], True: []}
    none = {False: [], True: []}
    s1, s2 = volumes(SMALLEST_SHAPE, True)
    edge = np.ones(SMALLEST_SHAPE, np.int32)
    edge[0, 0, 0] = edge[1, 2, 4] = 0
    return {"mask of zeros": (shape, V1, V2, np.zeros(shape, np.int32), none),
            "mask of one voxel": (shape, V1, V2, one, none),
            "mask values 2 and -1": (shape, V1, V2, odd, none),
            "constant V1": (shape, np.full(shape, 0.37), V2, None, none),
            "constant V2": (shape, V1, np.full(shape, 0.37), None, none),
            "all outside": (shape, V1, V2, None, away),
            "all outside, masked": (shape, V1, V2, disc, away),
            "2 x 3 x 5": (SMALLEST_SHAPE, s1, s2, None, none),
            "2 x 3 x 5, masked": (SMALLEST_SHAPE, s1, s2, edge, none)}


def degenerate_trials(name, method, wrap):
    shape, _, _, _, extra = degenerate_cases()[name]
    tr = trial_list(shape, method, wrap)
    return np.concatenate([tr, np.array(extra[wrap], dtype=np.float64).reshape(-1, 10)])
