"""numpy fp64 restatement of xmipp_reconstruct_wbp (reconstruction/reconstruct_wbp.cpp, ProgRecWbp): getAllMatrices, the image preparation of
apply2DFilterArbitraryGeometry, filterOneImage, simpleBackprojection and the symmetrisation and mask at the end. It follows the reference
literally, `xp += a00` along the row and the row-wise yp included. `direct=True` forms the source coordinates of selfApplyGeometry and of
symmetrizeVolume as the device does (x A00 + y A01 + A02); the back-projection's xp is carried along the row on the device as well.

Composed from what the tree already pins: Euler_angles2matrix (tests/volume_align_ref.py), the spline coefficients, the 2-D applyGeometry
and symmetrizeVolume (tests/symmetrize_ref.py, pinned to the oracle by tests/test_symmetrize_ref.py), numpy's transforms (the convention of
tests/test_oracle_pins.py: forward e^{-i}, here times 1 / D^2 on the way forward and nothing on the way back).

Readings that xmippCore, which is not in the tree, would settle (each pinned by tests/test_reconstruct_wbp_ref.py):
  - Tabsinc / TSINCVALUE: entry abs((int)(argum / 0.0001)) of sin(xx) / xx, xx = i * 0.0001 * PI, entry 0 = 1, (int)(D / 0.0001) entries;
  - FourierTransform gives the complete D x D transform times 1 / D^2; InverseFourierTransform reads columns 0 .. D / 2 of it
    (setFromCompleteFourier) and runs a complex-to-real transform; the filter loop's i, j are the centred logical indices;
  - getTransformationMatrix(A, true): the identity with the shifts in column 2, a flip negates A00 and A01 (the matrix readApplyGeo
    applies as IS_NOT_INV); reconstruct_wbp.cpp:554 applies it as IS_INV, so the image is sampled at (+-x + shiftX, y + shiftY);
  - Euler_apply_transf on a proper group: the copy's direction is row 2 of L E R itself."""
import math

import numpy as np

from tests import symmetrize_ref as S
from tests.volume_align_ref import euler_matrix

SAMPL = 0.0001
PI_L = np.longdouble("3.14159265358979323846264338327950288")
_TABLES = {}


def sinc_table(D):
    if D not in _TABLES:
        n = int(D / SAMPL)
        t = np.ones(n)
        for i in range(1, n):
            xx = i * SAMPL * math.pi
            t[i] = math.sin(xx) / xx
        _TABLES[D] = t
    return _TABLES[D]


# ---------------------------------------------------------------- matrices
def image_matrices(rot, tilt, psi):
    """(the filter's Euler_angles2matrix(-rot, tilt, -psi), :447; the back-projection's inverse of Euler_angles2matrix(rot, -tilt, psi), :373-374)"""
    return np.array(euler_matrix(-rot, tilt, -psi)), S.inv3x3(np.array(euler_matrix(rot, -tilt, psi)))


def _row2_times(E, R):
    return [sum((E[2][k] * float(R[k][j]) for k in range(3)), 0.0) for j in range(3)]


def all_matrices(angles, weights=None, R=()):
    """getAllMatrices (:308-359): mat_g [no_mats][4] and totimgs. angles [n][3]; weights: the --weight column or None; R: SL's matrices"""
    g, tot = [], 0.0
    for n, (rot, tilt, psi) in enumerate(angles):
        E = euler_matrix(rot, -tilt, psi)
        c = 1.0 if weights is None else float(weights[n])
        g.append([E[2][0], E[2][1], E[2][2], c])
        tot += c
        for Ri in R:
            g.append(_row2_times(E, Ri) + [c])
            tot += c
    return np.array(g), tot


# ---------------------------------------------------------------- sampled directions (reconstruction/directions.cpp, empty SymList)
def _realwrap(x, x0, xF):
    if x0 <= x <= xF:
        return x
    if x < x0:
        return x - int((x - x0) / (xF - x0) - 1) * (xF - x0)
    return x - int((x - xF) / (xF - x0) + 1) * (xF - x0)


def _close(rot, tilt, rot2, tilt2, rot_limit, tilt_limit):
    diff_rot, diff_tilt = abs(_realwrap(rot - rot2, -180, 180)), abs(_realwrap(tilt - tilt2, -180, 180))
    return (rot_limit - diff_rot) > 1e-3 and (tilt_limit - diff_tilt) > 1e-3


def even_distribution(sampling):
    """make_even_distribution(., ., sampling, SL, true) (:133-183); Euler_another_set(rot, tilt, psi) = (rot + 180, -tilt, psi - 180)"""
    x = 180. / sampling
    tilt_nstep = (int(x + 0.5) if x > 0 else int(x - 0.5)) + 1
    tilt_sam = 180. / tilt_nstep
    rots, tilts = [], []
    for tilt_step in range(tilt_nstep):
        tilt = (float(tilt_step) / (tilt_nstep - 1)) * 180.
        if tilt > 0:
            v = 360. * math.sin(tilt * math.pi / 180.) / sampling
            rot_nstep = int(v) if v == int(v) else (int(v + 1) if v > 0 else int(v))
        else:
            rot_nstep = 1
        rot_sam = 360. / float(rot_nstep)
        rot = 0.
        while rot < 360.:
            append = True
            for r2, t2 in zip(rots, tilts):
                if _close(rot, tilt, r2, t2, rot_sam, tilt_sam) or _close(rot, tilt, r2 + 180., -t2, rot_sam, tilt_sam):
                    append = False
                    break
            if append:
                rots.append(rot)
                tilts.append(tilt)
            rot += rot_sam
    return np.array(rots), np.array(tilts)


def _dist(rot1, tilt1, rot2, tilt2):
    a, b = abs(_realwrap(rot1 - rot2, -180, 180)), abs(_realwrap(tilt1 - tilt2, -180, 180))
    return math.sqrt((a * a) + (b * b))


def nearest_direction(rot, tilt, rots, tilts):
    """find_nearest_direction (:194-237) with distance_directions(., ., ., ., false) (:91-131): the first minimum"""
    opt, mindist = -1, 9999.
    for n, (r2, t2) in enumerate(zip(rots, tilts)):
        d = min(_dist(rot, tilt, r2, t2), _dist(rot, tilt, r2 + 180., -t2))
        if d < mindist:
            mindist, opt = d, n
    return opt


def sampled_matrices(angles, weights, sampling):
    """getSampledMatrices (:231-305) without symmetry: the counts are truncated to int (:276)"""
    rots, tilts = even_distribution(sampling)
    counts = [0.0] * len(rots)
    for n, (rot, tilt, _) in enumerate(angles):
        counts[nearest_direction(rot, tilt, rots, tilts)] += 1. if weights is None else float(weights[n])
    g, tot = [], 0.0
    for i, c in enumerate(counts):
        ci = int(c)
        if ci > 0:
            E = euler_matrix(rots[i], -tilts[i], 0.0)
            g.append([E[2][0], E[2][1], E[2][2], float(ci)])
            tot += ci
    return np.array(g), tot


def geometry_matrix(sx, sy, flip):
    A = np.array([[1.0, 0.0, float(sx)], [0.0, 1.0, float(sy)], [0.0, 0.0, 1.0]])
    if flip:
        A[0, 0] *= -1.0
        A[0, 1] *= -1.0
    return A


def rows_of(shifts, flips, weights, angles):
    """the [n][22] rows of ReconstructWbp.add"""
    r = np.zeros((len(angles), 22))
    for n, (rot, tilt, psi) in enumerate(angles):
        F, B = image_matrices(rot, tilt, psi)
        r[n, 0:2] = shifts[n]
        r[n, 2] = 1.0 if flips[n] else 0.0
        r[n, 3] = weights[n]
        r[n, 4:13] = F.reshape(9)
        r[n, 13:22] = B.reshape(9)
    return r


# ---------------------------------------------------------------- one image
def prepare(img, sx, sy, flip, weight, direct=False, coords=None):
    """:552-557. coords: a list that receives the coordinates the range tests saw"""
    img = np.asarray(img, dtype=np.float64)
    A = geometry_matrix(sx, sy, flip)
    if S.is_identity(A):
        out = img.copy()
    else:
        tested, final, _ = S.source_coords(img.shape, A, True, direct)          # IS_INV: A itself maps output to source
        if coords is not None:
            coords.append(tested)
        out = S.interp_bspline2d(S.prefilter(img), final[0], final[1])
    return out * float(weight)


def _dft_l(D, sign):
    k = np.arange(D)
    a = (2 * PI_L) * ((np.outer(k, k) % D).astype(np.longdouble) / np.longdouble(D))
    return np.cos(a) + (1j * sign) * np.sin(a)


def forward(P, exact=False):
    """FourierTransform times 1 / D^2, then CenterFFT(., true): logical (i, j) at [i + D // 2, j + D // 2]"""
    D = P.shape[0]
    if exact:
        W = _dft_l(D, -1)
        F = (W @ P.astype(np.clongdouble) @ W) / np.longdouble(D * D)
    else:
        F = np.fft.fft2(P) * (1.0 / (D * D))
    return np.roll(F, (D // 2, D // 2), axis=(0, 1))


def inverse(IMG, exact=False):
    """CenterFFT(., false), then InverseFourierTransform: the complex-to-real transform of columns 0 .. D / 2"""
    D = IMG.shape[0]
    F = np.roll(IMG, (-(D // 2), -(D // 2)), axis=(0, 1))
    H = F[:, :D // 2 + 1]
    if not exact:
        return np.fft.irfft2(H, s=(D, D), norm="forward")
    W = _dft_l(D, +1)
    G = np.zeros((D, D), dtype=np.clongdouble)
    G[:, :D // 2 + 1] = W @ H.astype(np.clongdouble)
    for j in range(D // 2 + 1, D):
        G[:, j] = np.conj(G[:, D - j])
    return (G @ W).real.astype(np.float64)


def logical(D):
    l = np.arange(D) - D // 2
    return np.meshgrid(l, l, indexing="ij")


def filter_terms(D, filt, g, diameter):
    """per cell and direction: (count_k * TSINC(argum), argum / 0.0001), [D][D][no_mats], centred"""
    table = sinc_table(D)
    K = float(diameter) / D
    i, j = logical(D)
    x, y = K * j, K * i
    a = np.asarray(filt, dtype=np.float64)
    fx = [a[0, 0] * gk[0] + a[1, 0] * gk[1] + a[2, 0] * gk[2] for gk in g]
    fy = [a[0, 1] * gk[0] + a[1, 1] * gk[1] + a[2, 1] * gk[2] for gk in g]
    terms = np.empty((D, D, len(g)))
    quot = np.empty((D, D, len(g)))
    for k in range(len(g)):
        argum = x * fx[k] + y * fy[k]
        q = argum / SAMPL
        quot[..., k] = q
        terms[..., k] = g[k][3] * table[np.abs(np.trunc(q).astype(np.int64))]
    return terms, quot


def weights_of(terms, exact=False):
    if exact:
        flat = terms.reshape(-1, terms.shape[-1])
        return np.array([math.fsum(r) for r in flat]).reshape(terms.shape[:2])
    w = np.zeros(terms.shape[:2])
    for k in range(terms.shape[-1]):
        w = w + terms[..., k]
    return w


def apply_filter(IMG, weight, threshold, diameter):
    """:478-486: the filtered transform and the number of cells under the threshold. `under` is decided on the weights given"""
    under = np.abs(weight) < threshold
    sgn = np.where(weight >= 0, 1.0, -1.0)
    div = np.where(under, sgn * (threshold * float(diameter)), weight * float(diameter))
    return IMG / div, int(under.sum())


def filter_image(P, filt, g, threshold, diameter, exact=False, under_from=None):
    """the filtered image simpleBackprojection reads, count_thr of the image, the weights. under_from: weights that decide the branch
    (the exact sums take the branch of the sequential ones: a condition, not a rounding)"""
    terms, _ = filter_terms(P.shape[0], filt, g, diameter)
    w = weights_of(terms, exact)
    IMG = forward(P, exact)
    if under_from is None:
        out, cnt = apply_filter(IMG, w, threshold, diameter)
    else:
        under = np.abs(under_from) < threshold
        sgn = np.where(under_from >= 0, 1.0, -1.0)
        div = np.where(under, sgn * (threshold * float(diameter)), w * float(diameter))
        out, cnt = IMG / div, int(under.sum())
    return inverse(out, exact), cnt, w


def backprojection_terms(img, B, diameter, direct=False, info=None):
    """simpleBackprojection's `value` at every voxel [D][D][D] and the voxels that pass every cut. info: receives xp, yp and the squared
    radii for the preconditions"""
    D = img.shape[0]
    B = np.asarray(B, dtype=np.float64)
    a00, a01, a10, a11, a20, a21 = B[0, 0], B[0, 1], B[1, 0], B[1, 1], B[2, 0], B[2, 1]
    radius2 = (diameter / 2.) * (diameter / 2.)
    dim2, dim1 = float(D // 2), float(D - 1)
    idx = np.arange(D, dtype=np.float64)
    z = (-idx + dim2)[:, None, None]
    y = (idx - dim2)[None, :, None]
    x = (idx - dim2)[None, None, :]
    z2 = z * z
    z2y2 = z2 + y * y
    r2 = x * x + z2y2
    keep = (z2 <= radius2) & (z2y2 <= radius2) & (r2 <= radius2)
    xpz, ypz = z * a20 + dim2, z * a21 + dim2
    x0 = 0 - dim2
    yp = np.broadcast_to(x0 * a01 + y * a11 + ypz, (D, D, 1))                    # tested and truncated once per row
    if direct:
        xp = x * a00 + y * a10 + xpz
    else:
        start = x0 * a00 + y * a10 + xpz
        steps = np.concatenate([start, np.full((D, D, D - 1), a00)], axis=2)
        xp = np.add.accumulate(steps, axis=2)                                    # xp += a00, one rounding per step
    keep = keep & ~((yp >= dim1) | (yp < 0.0)) & ~((xp >= dim1) | (xp < 0.0))
    l = np.clip(np.trunc(yp).astype(np.int64), 0, D - 2)
    m = np.clip(np.trunc(xp).astype(np.int64), 0, D - 2)
    scaley = yp - l
    scale1y = 1. - scaley
    scalex = xp - m
    scale1x = 1. - scalex
    value1 = scalex * img[l, m + 1] + scale1x * img[l, m]
    value2 = scalex * img[l + 1, m + 1] + scale1x * img[l + 1, m]
    value = scaley * value2 + scale1y * value1
    if info is not None:
        sphere = (z2 <= radius2) & (z2y2 <= radius2) & (r2 <= radius2)
        info.append({"xp": xp[sphere], "yp": np.broadcast_to(yp, (D, D, D))[sphere], "r2": [z2, z2y2, r2], "radius2": radius2})
    return np.where(keep, value, 0.0), keep


def finish(V, R, diameter, direct=False):
    """:566-579"""
    if len(R) == 0:
        return V
    out = S.symmetrize_volume(V, R, 3, True, direct=direct)
    D = V.shape[0]
    l = np.arange(D, dtype=np.float64) - D // 2
    k, i, j = np.meshgrid(l, l, l, indexing="ij")
    r2 = (k * k + i * i) + j * j
    R1 = diameter / 2.
    return np.where(r2 <= R1 * R1, out, 0.0)


# ---------------------------------------------------------------- the whole run
def reconstruct(case, exact=False, direct=False, collect=None):
    """(volume, filtered images, count_thr, kept voxels) of a case. exact: the weight sums by math.fsum, the transforms in extended
    precision, the voxel sums by math.fsum, on the same per-term values and the same branches. collect: a dict that receives what the
    preconditions look at"""
    D, n = case["D"], len(case["images"])
    g, thr, dia = case["g"], case["threshold"], case["diameter"]
    filtered = np.empty((n, D, D))
    terms = np.empty((n, D, D, D))
    kept = np.zeros((D, D, D), dtype=bool)
    count = 0
    for t in range(n):
        sx, sy = case["shifts"][t]
        coords = [] if collect is not None else None
        P = prepare(case["images"][t], sx, sy, case["flips"][t], case["weights"][t], direct, coords)
        F, B = image_matrices(*case["angles"][t])
        seq = filter_image(P, F, g, thr, dia)
        if exact:
            filtered[t], c, _ = filter_image(P, F, g, thr, dia, True, under_from=seq[2])
        else:
            filtered[t], c = seq[0], seq[1]
        count += c
        info = [] if collect is not None else None
        # the exact arm back-projects the sequential arm's filtered image: the same per-term values, only the voxel sum differs
        terms[t], k = backprojection_terms(seq[0], B, dia, False, info)
        kept |= k
        if collect is not None:
            collect.setdefault("weights", []).append(seq[2])
            collect.setdefault("quot", []).append(filter_terms(D, F, g, dia)[1])
            collect.setdefault("bp", []).append(info[0])
            collect.setdefault("coords", []).extend(coords)
    if exact:
        V = np.array([math.fsum(terms[:, a, b, c]) for a in range(D) for b in range(D) for c in range(D)]).reshape(D, D, D)
    else:
        V = np.zeros((D, D, D))
        for t in range(n):
            V = V + terms[t]
    return finish(V, case["R"], dia, direct), filtered, count, kept


def distance(a, b):
    return float(np.abs(np.asarray(a) - np.asarray(b)).max() / np.abs(np.asarray(b)).max())


def excluded(collect, threshold, D):
    """the cells and voxels a comparison would have to leave out: each must be 0 (the issue's four preconditions, and the image's range tests)"""
    out = {"threshold": 0, "index": 0, "taps": 0, "radius": 0, "wrap": 0}
    for w in collect["weights"]:
        out["threshold"] += int((np.abs(np.abs(w) - threshold) <= 1e-9 * threshold).sum())
    for q in collect["quot"]:
        r = np.rint(q)
        out["index"] += int(((np.abs(q - r) < 1e-9) & (q != r)).sum())
    for b in collect["bp"]:
        for c in (b["xp"], b["yp"]):
            out["taps"] += int(((np.abs(c) < 1e-9) | (np.abs(c - (D - 1)) < 1e-9)).sum())
        for r2 in b["r2"]:
            out["radius"] += int(((np.abs(r2 - b["radius2"]) < 1e-9) & (r2 != b["radius2"])).sum())
    for tested in collect.get("coords", []):
        if S.threshold_margin((D, D), tested) < 1e-9:
            out["wrap"] += 1
        out["wrap"] += int(S.wrap_edge_mask((D, D), [tested]).sum())
    return out


# ---------------------------------------------------------------- cases
TILE = 256        # the filter kernel's LDS tile (xmipp3_amd.wbp_tile(); tests/test_gpu_reconstruct_wbp.py asserts it)


def _unit_vectors(rng, n):
    v = rng.standard_normal((n, 3))
    v /= np.linalg.norm(v, axis=1)[:, None]
    v[0] = (0.0, 0.0, 1.0)                                  # an axis-aligned direction
    return v


def make_case(name, D, n, no_mats=None, radius=None, shifts="zero", flips=False, weights=None, sym=None, rel_threshold=0.005, seed=0, filsam=None):
    """no_mats None: --use_each_image, the directions of the images themselves (and their symmetry copies); a number: a direction list of
    that length, as sampled mode hands over, with integer counts"""
    rng = np.random.default_rng(1000 * D + n + 7 * seed)
    images = rng.standard_normal((n, D, D)).astype(np.float32)
    angles = np.stack([rng.uniform(0, 360, n), rng.uniform(5, 175, n), rng.uniform(0, 360, n)], axis=1)
    if shifts == "zero":
        sh = np.zeros((n, 2))
    elif shifts == "fractional":
        sh = rng.uniform(-3, 3, (n, 2))
    else:                                                   # "wrap": every third image moved by more than D
        sh = rng.uniform(-3, 3, (n, 2))
        sh[::3] += (D + 4.25, -(D + 2.5))
    fl = (rng.uniform(0, 1, n) < 0.5) if flips else np.zeros(n, dtype=bool)
    if flips:
        fl[0] = True
        sh[0] = 0.0                                         # a flip alone: integer source coordinates
    wt = np.ones(n) if weights is None else np.asarray(weights, dtype=np.float64)[np.arange(n) % len(weights)]
    R = S.group_matrices(sym) if sym else np.zeros((0, 3, 3))
    if filsam is not None:
        g, tot = sampled_matrices(angles, None if weights is None else wt, filsam)
    elif no_mats is None:
        g, tot = all_matrices(angles, None if weights is None else wt, R)
    else:
        g = np.concatenate([_unit_vectors(rng, no_mats), rng.integers(1, 4, (no_mats, 1)).astype(np.float64)], axis=1)
        tot = float(g[:, 3].sum())
    dia = D if radius is None else 2 * radius
    return {"name": name, "D": D, "images": images, "angles": angles, "shifts": sh, "flips": fl, "weights": wt, "g": g, "R": R,
            "threshold": rel_threshold * tot, "diameter": dia, "sym": sym, "filsam": filsam}


def cases():
    return [
        make_case("d16_tile_minus_1", 16, 5, no_mats=TILE - 1),
        make_case("d17_tile_flips", 17, 5, no_mats=TILE, shifts="fractional", flips=True),
        make_case("d20_each_wrap_r5", 20, 37, radius=5, shifts="wrap"),
        make_case("d33_tile_plus_1_weights", 33, 5, no_mats=TILE + 1, shifts="fractional", weights=(0.5, 3.0)),
        make_case("d33_two_tiles_threshold", 33, 1, no_mats=2 * TILE + 18, rel_threshold=0.2),
        make_case("d16_each_c3", 16, 37, sym="c3", shifts="fractional"),
        make_case("d20_each_d2_r5", 20, 5, sym="d2", radius=5),
        make_case("d17_each_weights_threshold", 17, 37, weights=(0.5, 3.0), rel_threshold=0.2, flips=True, shifts="fractional"),
        make_case("d20_sampled_15", 20, 37, filsam=15.0, shifts="fractional", weights=(0.5, 3.0)),
    ]


_RESULTS = {}


def result(case):
    """the restatement's (volume, filtered, count_thr, kept) of a case, computed once and shared"""
    if case["name"] not in _RESULTS:
        out = reconstruct(case)
        for a in out:
            if isinstance(a, np.ndarray):
                a.setflags(write=False)
        _RESULTS[case["name"]] = out
    return _RESULTS[case["name"]]
