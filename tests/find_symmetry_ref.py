"""numpy fp64 restatement of xmipp_volume_find_symmetry (reconstruction/volume_find_symmetry.cpp, ProgVolumeFindSymmetry): both cost
functions of evaluateSymmetry (:359-418), both exhaustive searches with the reference's loops and its first maximum above 0 (:164-203,
:221-241, :293-320), the gate (:396-399), the mask clipping of :280-288, the local branch, and the cylinder and tube masks of data/mask.cpp.

xmippCore is not in the reference tree. applyGeometry, the spline prefilter and interpolatedElement3DHelical (its recursion kept as
recursion) are tests/symmetrize_ref.py's, correlationIndex tests/volume_align_ref.py's. rotation3DMatrix(ang, axis) is restated as the
rotation by ang about the unit axis in the sense of rotation3DMatrix(ang, 'Z'); the sense cannot change a correlation beyond rounding,
because n and rot_sym - n are inverse rotations and the set of copies is the same either way.

The forms the device bound is derived from (tests/test_find_symmetry_ref.py):
  onepass      the reference's two passes over volume_sym (mean_y first) against the one-pass identity the device uses;
  nudge        every sin, cos and atan2 result of the helix moved by one ulp (np.nextafter), up or down: what a device libm may return;
  corr_exact   the one-pass form with every sum taken exactly (math.fsum)."""
import math

import numpy as np

from tests.symmetrize_ref import (ACC, _Helix, _helical_interp, apply_geometry, inv3x3, prefilter,  # noqa: F401
                                  threshold_margin)
from tests.volume_align_ref import BIG_SHAPES, SHAPES, bricks, circular_mask, correlation_index, euler_matrix, stats  # noqa: F401

GATED = -1e38


# ---------------------------------------------------------------- the axis cost
def rotation_about(ang, axis):
    """rotation3DMatrix(ang, axis); python floats in the order the library writes them"""
    x, y, z = (float(v) for v in axis)
    n = math.sqrt(x * x + y * y + z * z)
    x, y, z = x / n, y / n, z / n
    a = ang * math.pi / 180.0
    c, s = math.cos(a), math.sin(a)
    t = 1 - c
    return np.array([[t * x * x + c, t * x * y + s * z, t * x * z - s * y],
                     [t * x * y - s * z, t * y * y + c, t * y * z + s * x],
                     [t * x * z + s * y, t * y * z - s * x, t * z * z + c]])


def axis_of(rot, tilt):
    """row 2 of Euler_angles2matrix(rot, tilt, 0)"""
    return euler_matrix(rot, tilt, 0.0)[2]


def axis_matrices(rot, tilt, rot_sym):
    axis = axis_of(rot, tilt)
    return [rotation_about(360.0 / rot_sym * n, axis) for n in range(1, rot_sym)]


def axis_volume(V, rot, tilt, rot_sym, degree=1, coef=None, coords=None):
    """volume_sym of :378-389: V + sum_n applyGeometry(V, A_n), DONT_WRAP, outside 0, in the order n = 1 .. rot_sym - 1"""
    V = np.asarray(V, dtype=np.float64)
    if degree == 3 and coef is None:
        coef = prefilter(V)
    out = V.copy()
    for A in axis_matrices(rot, tilt, rot_sym):
        out = out + apply_geometry(V, A, degree, False, 0.0, True, coef, coords)
    return out


def axis_corr(V, rot, tilt, rot_sym, degree=1, mask=None, onepass=False, coef=None):
    return correlation_index(V, axis_volume(V, rot, tilt, rot_sym, degree, coef), mask, onepass)


# ---------------------------------------------------------------- the helical cost
def helix_range(Z, heightFraction):
    n = int(math.floor(heightFraction * Z + 0.5))              # round()
    zFirst = -(n // 2)
    return zFirst, zFirst + n - 1


def clip_mask(shape, mask, heightFraction):
    """:280-288: the mask (None: ones) zeroed outside [zFirst, zLast]"""
    Z = shape[0]
    m = np.ones(shape, np.int32) if mask is None else np.array(mask, dtype=np.int32)
    zFirst, zLast = helix_range(Z, heightFraction)
    k = np.arange(Z) - Z // 2
    m[(k < zFirst) | (k > zLast)] = 0
    return m


def gated(Z, zHelical, rotHelical, box=None):
    """:396-399; box = (z0, zF, rot0, rotF)"""
    if zHelical < 0 or zHelical > Z * 0.4:
        return True
    return box is not None and (zHelical < box[0] or zHelical > box[1] or rotHelical < box[2] or rotHelical > box[3])


def helical_depth(Z, zHelical, heightFraction, dihedral):
    """the recursion bound for the masked helix of this program: -1 no bound, else 0 or 1"""
    if not (zHelical > 0.0 and math.isfinite(zHelical)) or not (0.0 < heightFraction <= 1.0):
        return -1
    n = int(math.floor(heightFraction * Z + 0.5))
    if n < 1 or n > Z:
        return -1
    if dihedral and Z % 2 == 0 and n == Z:
        return 1 if 1.0 <= zHelical <= Z else -1
    return 0


def _nudged(v, nudge):
    if nudge == 0:
        return v
    return np.nextafter(v, np.inf if nudge > 0 else -np.inf)


def helical_volume(V, rot_deg, zHelical, mask, dihedral=False, heightFraction=1.0, Cn=1, nudge=0, stats=None):
    """symmetry_Helical (symmetries.cpp:1632-1705) with its mask (the clipped one) and rot0 = 0; rotHelical = DEG2RAD(rot_deg). Only the
    voxels of the mask are formed, the others stay 0. nudge: +1 / -1 moves every sin, cos and atan2 result by one ulp"""
    V = np.asarray(V, dtype=np.float64)
    Z, Y, X = V.shape
    rotHelical = rot_deg * math.pi / 180.0
    zFirst, zLast = helix_range(Z, heightFraction)
    iz = 1.0 / zHelical
    zH2 = int(math.floor(0.5 * zHelical))
    H = _Helix(V, zHelical, rotHelical)
    H.sin, H.cos = float(_nudged(np.float64(H.sin), nudge)), float(_nudged(np.float64(H.cos), nudge))
    Llength = int(math.ceil(Z * iz))
    sinCn = [float(_nudged(np.float64(math.sin(c * (2 * math.pi) / Cn)), nudge)) for c in range(Cn)]
    cosCn = [float(_nudged(np.float64(math.cos(c * (2 * math.pi) / Cn)), nudge)) for c in range(Cn)]
    inside = np.asarray(mask) != 0
    kk, ii, jj = np.nonzero(inside)
    kk, ii, jj = kk - Z // 2, ii - Y // 2, jj - X // 2
    k, i, j = kk.astype(np.float64), ii.astype(np.float64), jj.astype(np.float64)
    rot = _nudged(np.arctan2(i, j), nudge) + 0.0
    rho = np.sqrt(i * i + j * j)
    l0 = np.ceil((-(Z // 2) - kk) * iz)
    final, L = np.zeros(k.shape), np.zeros(k.shape)
    for t in range(Llength + 1):
        l = l0 + t
        kp_all = k + l * zHelical
        ok = (kp_all >= zFirst) & (kp_all <= zLast)
        if not ok.any():
            continue
        kp = kp_all[ok]
        rotp = rot[ok] + l[ok] * rotHelical
        ip, jp = rho[ok] * _nudged(np.sin(rotp), nudge), rho[ok] * _nudged(np.cos(rotp), nudge)
        w = np.ones(kp.shape)
        first = kp - zFirst <= zH2
        last = ~first & (zLast - kp <= zH2)
        w[first] = (kp[first] - zFirst + 1) / (zH2 + 1)
        w[last] = (zLast + 1 - kp[last]) / (zH2 + 1)
        f, Ls = final[ok], L[ok]
        pts = [(jp, ip, kp)] + [(cosCn[c] * jp - sinCn[c] * ip, sinCn[c] * jp + cosCn[c] * ip, kp) for c in range(1, Cn)]
        if dihedral:
            pts += [(jp, -ip, -kp)] + [(cosCn[c] * jp - sinCn[c] * (-ip), sinCn[c] * jp + cosCn[c] * (-ip), -kp) for c in range(1, Cn)]
        for x, y, z in pts:
            f = f + w * _helical_interp(H, x, y, z)
            Ls = Ls + w
        final[ok], L[ok] = f, Ls
    if stats is not None:
        stats["depth"] = H.depth
    out = np.zeros(V.shape)
    with np.errstate(invalid="ignore", divide="ignore"):
        out[inside] = final / L
    return out


def helical_corr(V, rot_deg, zHelical, mask=None, box=None, dihedral=False, heightFraction=1.0, Cn=1, onepass=False, nudge=0):
    """minus evaluateSymmetry of a helical trial: GATED where the gate returns 1e38. mask: the program's, before clipping"""
    Z = V.shape[0]
    if gated(Z, zHelical, rot_deg, box):
        return GATED
    m = clip_mask(V.shape, mask, heightFraction)
    return correlation_index(V, helical_volume(V, rot_deg, zHelical, m, dihedral, heightFraction, Cn, nudge), m, onepass)


def corr_exact(x, y, mask=None):
    """correlationIndex in the one-pass form with every sum taken exactly (math.fsum), then the finish in double as the device writes it"""
    m = np.ones(x.shape, dtype=bool) if mask is None else np.asarray(mask) != 0
    xs, ys = x[m], y[m]
    n = xs.size
    if n <= 1:
        return 0.0
    mean_x = math.fsum(xs) / n
    sd_x = math.sqrt(abs((math.fsum(xs * xs) / n - mean_x * mean_x) * float(n // (n - 1))))
    mean_y = math.fsum(ys) / n
    sd_y = math.sqrt(abs((math.fsum(ys * ys) / n - mean_y * mean_y) * float(n // (n - 1))))
    if abs(sd_x) < ACC or abs(sd_y) < ACC:
        return 0.0
    dx = xs - mean_x
    return (math.fsum(dx * ys) - mean_y * math.fsum(dx)) / ((sd_x * sd_y) * n)


# ---------------------------------------------------------------- the searches
def grid(range0, range1):
    """the two nested loops (:221-225, :293-303) with double loop variables, += and <=: (trials [count, 2], n_outer, n_inner)"""
    out, n_outer, n_inner = [], 0, 0
    u = float(range0[0])
    while u <= float(range0[1]):
        n_outer += 1
        v = float(range1[0])
        while v <= float(range1[1]):
            if n_outer == 1:
                n_inner += 1
            out.append((u, v))
            v += float(range1[2])
        u += float(range0[2])
    return np.array(out, dtype=np.float64).reshape(-1, 2), n_outer, n_inner


def choose(corrs):
    """threadEvaluateSymmetry with one thread (:167-196): the best starts at 0, corr > best. (-1, 0.0) where no correlation is above 0"""
    best, idx = 0.0, -1
    for t, c in enumerate(corrs):
        if c > best:
            best, idx = float(c), t
    return idx, best


def ftol_halfwidth(cost, best, ftol=0.01):
    """what Powell's stopping rule leaves open around a minimum `best` of cost: per variable the largest step of the grid 1e-3 2^k for
    which cost(best +- step) stays within ftol |fmin| of the minimum (tests/volume_align_ref.py measures --local's margin the same way)"""
    best = np.array(best, dtype=np.float64)
    fmin = cost(best)
    out = np.zeros(len(best))
    for i in range(len(best)):
        d = 1e-3
        while d < 64:
            worst = max(cost(best + s * d * np.eye(len(best))[i]) for s in (1.0, -1.0))
            if worst - fmin > ftol * abs(fmin):
                break
            out[i] = d
            d *= 2
    return out


# ---------------------------------------------------------------- masks
def _grids(shape):
    return np.meshgrid(*[np.arange(d, dtype=np.float64) - d // 2 for d in shape], indexing="ij")


def cylinder_mask(shape, R, H, center=(0.0, 0.0, 0.0)):
    """BinaryCylinderMask (data/mask.cpp:471-486) with the mode of :1396-1405: both negative keep the inside"""
    assert (R < 0 and H < 0) or (R > 0 and H > 0)
    k, i, j = _grids(shape)
    x0, y0, z0 = center
    r2 = (i - y0) * (i - y0) + (j - x0) * (j - x0)
    inside = (r2 <= R * R) & (np.abs(k - z0) <= abs(H) / 2)
    return (inside if R < 0 else ~inside).astype(np.int32)


def tube_mask(shape, R1, R2, H, center=(0.0, 0.0, 0.0)):
    """BinaryTubeMask (:261-276) with the mode of :1419-1429; as written: |k| < H, no z0 and no half"""
    assert (R1 < 0 and R2 < 0 and H < 0) or (R1 > 0 and R2 > 0 and H > 0)
    k, i, j = _grids(shape)
    x0, y0, _ = center
    r2 = (i - y0) * (i - y0) + (j - x0) * (j - x0)
    inside = (r2 >= R1 * R1) & (r2 <= R2 * R2) & (np.abs(k) < abs(H))
    return (inside if R1 < 0 else ~inside).astype(np.int32)


# ---------------------------------------------------------------- phantoms
TRUE_AXIS = (40.0, 55.0)                      # rot, tilt of the planted Cn axis: off the z axis
TRUE_HELIX = (-50.0, 4.3)                     # rot (degrees), rise (voxels) of the planted helix
_PH = {}


def _blobs(shape, centres, sigma, seed):
    k, i, j = _grids(shape)
    v = np.full(shape, 0.1)
    for (cz, cy, cx), a in centres:
        v = v + a * np.exp(-((k - cz) ** 2 + (i - cy) ** 2 + (j - cx) ** 2) / (2 * sigma * sigma))
    v = v + 0.02 * np.random.default_rng(seed).standard_normal(shape)
    return v.astype(np.float32).astype(np.float64)


def axis_phantom(shape, rot_sym):
    """Gaussian blobs placed by a true C(rot_sym) axis at TRUE_AXIS plus a little seeded noise; float32 values"""
    key = ("axis", shape, rot_sym)
    if key not in _PH:
        axis = np.array(axis_of(*TRUE_AXIS))
        r = 0.28 * min(shape)
        seeds = [np.array([0.9, 0.3, 0.5]), np.array([-0.2, 0.8, -0.6])]
        centres = []
        for q, (s, amp) in enumerate(zip(seeds, (1.0, 0.7))):
            p = s - axis * float(axis @ s)                      # perpendicular to the axis
            p = p / np.linalg.norm(p) * r * (1.0 - 0.35 * q) + axis * (0.12 * min(shape) * (1 - 2 * q))
            for n in range(rot_sym):
                x, y, z = rotation_about(360.0 / rot_sym * n, axis) @ p
                centres.append(((z, y, x), amp))
        _PH[key] = _blobs(shape, centres, 0.09 * min(shape) + 0.6, 11 + rot_sym)
    return _PH[key]


def helix_phantom(shape):
    """blobs along a true helix (TRUE_HELIX) about z, two strands of different weight and radius; float32 values"""
    key = ("helix", shape)
    if key not in _PH:
        Z, Y, X = shape
        rot, rise = TRUE_HELIX
        centres = []
        for phase, rad, amp in ((0.3, 0.26 * min(Y, X), 1.0), (2.1, 0.15 * min(Y, X), 0.6)):
            for l in range(-Z, Z + 1):
                z = 0.37 + l * rise
                if abs(z) > Z:
                    continue
                a = phase + l * rot * math.pi / 180.0
                centres.append(((z, rad * math.sin(a), rad * math.cos(a)), amp))
        _PH[key] = _blobs(shape, centres, 1.3, 23)
    return _PH[key]


# ---------------------------------------------------------------- the device tests' cases and bound
# (shape, rot_sym, degree, masked): every box with two of the (rot_sym, interpolation, mask) combinations so that each of rot_sym 2, 3, 7,
# LINEAR / BSPLINE3 and masked / unmasked meets every other value at least once, and rot_sym 4 for the z axis (coordinates that are
# integers up to the rounding of cos 90)
AXIS_CASES = [((16, 16, 16), 2, 1, False), ((16, 16, 16), 7, 3, True), ((16, 16, 16), 4, 1, False),
              ((17, 17, 17), 3, 3, False), ((17, 17, 17), 2, 1, True), ((17, 17, 17), 4, 3, True),
              ((9, 10, 12), 7, 1, False), ((9, 10, 12), 3, 3, True),
              ((20, 18, 13), 2, 3, True), ((20, 18, 13), 3, 1, False),
              ((29, 41, 43), 3, 1, True), ((29, 41, 43), 7, 3, False),
              ((37, 49, 57), 7, 1, True), ((37, 49, 57), 2, 3, False)]
# the true axis, the z axis, tilt 90, two generic ones
AXIS_TRIALS = np.array([TRUE_AXIS, (0.0, 0.0), (25.0, 90.0), (73.3, 31.7), (200.1, 64.9)])
# (shape, Cn, dihedral, heightFraction, mask kind). 16^3 and 20 x 18 x 13 have an even Z, the others an odd one; with heightFraction 1,
# the dihedral copies and an even Z the recursion reaches depth 1. Every fraction below 1 removes planes: round(0.95 Z) is 16 of 17,
# 19 of 20 and 28 of 29 (on Z = 9 it is 9, the same case as 1, so that box runs at 1)
HELICAL_CASES = [((16, 16, 16), 1, True, 1.0, None), ((17, 17, 17), 3, True, 1.0, "cylinder"), ((17, 17, 17), 1, False, 0.95, None),
                 ((9, 10, 12), 3, False, 1.0, None), ((20, 18, 13), 1, True, 0.95, "cylinder"), ((20, 18, 13), 3, True, 1.0, None),
                 ((29, 41, 43), 1, False, 1.0, "cylinder"), ((29, 41, 43), 1, True, 0.95, "cylinder"), ((37, 49, 57), 3, True, 1.0, "cylinder")]
HELICAL_BOX = (0.5, 12.0, -200.0, 200.0)      # z0, zF, rot0, rotF


def helical_trials(shape):
    """(rot, z): the planted helix (rise 4.3), rises of 5 and 1.0, a generic one; and trials the gate refuses: a negative rise, one above
    0.4 Z, one below z0 of the box, a rotation outside it. Z = 9 gates every rise above 3.6, so that box takes 2.3 and 3.5 for 4.3 and 5.
    37 x 49 x 57 leaves out the rise of 1 voxel (38 terms for each of 10^5 voxels and 6 copies in numpy); 29 x 41 x 43, whose finish also
    takes more than one step over the bricks, keeps it"""
    Z = shape[0]
    za, zb = (TRUE_HELIX[1], 5.0) if 0.4 * Z >= 5.0 else (2.3, 3.5)
    t = [(TRUE_HELIX[0], za), (10.0, -1.0), (TRUE_HELIX[0], zb), (33.3, 0.4 * Z + 0.5), (-120.5, za), (400.0, za), (20.0, 0.25)]
    if shape != BIG_SHAPES[1]:
        t.append((33.3, 1.0))
    return np.array(t, dtype=np.float64)


def case_mask(shape, kind):
    if kind is None:
        return None
    if kind == "circular":
        return circular_mask(shape, -(min(shape) // 2 - 1.0))
    if kind == "cylinder":
        return cylinder_mask(shape, -(min(shape[1:]) // 2 - 1.0), -(shape[0] - 3.0))
    raise ValueError(kind)


_AX, _HE = {}, {}


def axis_case(case):
    """the restatement of one axis case, computed once: dict of V, mask, coef, the volume_sym of every trial, the correlations in the
    three forms, the index and the tested coordinates' margin"""
    if case not in _AX:
        shape, rot_sym, degree, masked = case
        V = axis_phantom(shape, rot_sym)
        mask = case_mask(shape, "circular" if masked else None)
        coef = prefilter(V) if degree == 3 else None
        vols, coords = [], []
        for rot, tilt in AXIS_TRIALS:
            vols.append(axis_volume(V, rot, tilt, rot_sym, degree, coef, coords))
        two = np.array([correlation_index(V, y, mask, False) for y in vols])
        one = np.array([correlation_index(V, y, mask, True) for y in vols])
        ex = np.array([corr_exact(V, y, mask) for y in vols])
        margin = min(threshold_margin(shape, t) for t in coords)
        _AX[case] = dict(V=V, mask=mask, vols=vols, two=two, one=one, exact=ex, choice=choose(two), margin=margin)
    return _AX[case]


def helical_case(case, nudged=False):
    """the restatement of one helical case, computed once; nudged: also the correlations with the transcendentals moved by +-1 ulp"""
    key = (case, nudged)
    if key not in _HE:
        shape, Cn, dihedral, hf, kind = case
        V = helix_phantom(shape)
        mask = case_mask(shape, kind)
        m = clip_mask(shape, mask, hf)
        tr = helical_trials(shape)
        vols, depth = [], 0
        two, one, ex, up, down = (np.full(len(tr), GATED) for _ in range(5))
        for t, (rot, z) in enumerate(tr):
            if gated(shape[0], z, rot, HELICAL_BOX):
                vols.append(None)
                continue
            st = {}
            y = helical_volume(V, rot, z, m, dihedral, hf, Cn, 0, st)
            depth = max(depth, st["depth"])
            vols.append(y)
            two[t], one[t], ex[t] = correlation_index(V, y, m, False), correlation_index(V, y, m, True), corr_exact(V, y, m)
            if nudged:
                up[t] = correlation_index(V, helical_volume(V, rot, z, m, dihedral, hf, Cn, +1), m, True)
                down[t] = correlation_index(V, helical_volume(V, rot, z, m, dihedral, hf, Cn, -1), m, True)
        _HE[key] = dict(V=V, mask=mask, clipped=m, trials=tr, vols=vols, two=two, one=one, exact=ex, up=up, down=down, choice=choose(two), depth=depth)
    return _HE[key]


# 16 times the largest relative difference (to max(1, |corr|)) over every trial of AXIS_CASES and HELICAL_CASES between the restatement's
# forms, rounded up to a power of ten; tests/test_find_symmetry_ref.py derives and asserts it. Measured there: two-pass against one-pass
# 3.3e-16, nudged transcendentals against plain 1.8e-15, either against the exact sums 6.1e-15 (cubic splines on 9 x 10 x 12 under the
# circular mask, 257 voxels)
BOUND = 1e-13
