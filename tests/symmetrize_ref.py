"""numpy fp64 restatement of xmipp_transform_symmetrize (reconstruction/symmetrize.cpp, data/symmetries.cpp:1574-1705) and of the
xmippCore pieces under it: produceSplineCoefficients(BSPLINE3) on a volume, applyGeometry in 2-D and 3-D (LINEAR and BSPLINE3, WRAP and
DONT_WRAP), BinaryCircularMask's outside mean, symmetrizeVolume, symmetrizeImage, symmetry_Helical with interpolatedElement3DHelical's
recursion kept as recursion (vectorised over the points, one call per level), and the matrices of a point group, closed or --no_group.

xmippCore is not in the reference tree. applyGeometry follows the 2-D branch that oracle/xo_bspline.cpp:89-217 restates, with a z axis
added; tests/test_symmetrize_ref.py pins the 2-D form and the prefilter to the oracle. `direct` switches the source coordinates between
the reference's incremental form (A00 added along the row, the wrapped value carried on) and the direct form the device uses
(x A00 + y A01 + z A02); the device tolerance is derived from the difference of the two (tests/test_gpu_symmetrize.py)."""
import math

import numpy as np

ACC = 1e-6            # XMIPP_EQUAL_ACCURACY
Z_POLE = math.sqrt(3.0) - 2.0


# ---------------------------------------------------------------- matrices
def inv3x3(A):
    """by cofactors, in the order of the oracle's inv3x3; python floats, so no contraction"""
    a, b, c, d, e, f, g, h, i = (float(v) for v in np.asarray(A, dtype=np.float64).reshape(9))
    det = a * (e * i - f * h) - b * (d * i - f * g) + c * (d * h - e * g)
    k = 1.0 / det
    return np.array([[(e * i - f * h) * k, (c * h - b * i) * k, (b * f - c * e) * k],
                     [(f * g - d * i) * k, (a * i - c * g) * k, (c * d - a * f) * k],
                     [(d * h - e * g) * k, (b * g - a * h) * k, (a * e - b * d) * k]])


def is_identity(A):
    return bool(np.all(np.abs(np.asarray(A) - np.eye(3)) <= ACC))


def rotation2d_matrix(ang_deg):
    a = ang_deg * math.pi / 180.0
    c, s = math.cos(a), math.sin(a)
    return np.array([[c, s, 0.0], [-s, c, 0.0], [0.0, 0.0, 1.0]])


def rotation3d_x(ang_deg):
    """rotation3DMatrix(ang, 'X'); the program uses it at 180 degrees only, where the sign convention of the sine moves nothing"""
    a = ang_deg * math.pi / 180.0
    c, s = math.cos(a), math.sin(a)
    return np.array([[1.0, 0.0, 0.0], [0.0, c, -s], [0.0, s, c]])


def _mul(A, B):
    C = [[0.0] * 3 for _ in range(3)]
    for i in range(3):
        for j in range(3):
            for k in range(3):
                C[i][j] += float(A[i][k]) * float(B[k][j])
    return np.array(C)


def _rot_axis(ang, x, y, z):
    n = math.sqrt(x * x + y * y + z * z)
    x, y, z = x / n, y / n, z / n
    c, s = math.cos(ang), math.sin(ang)
    t = 1 - c
    return np.array([[t * x * x + c, t * x * y - s * z, t * x * z + s * y],
                     [t * x * y + s * z, t * y * y + c, t * y * z - s * x],
                     [t * x * z - s * y, t * y * z + s * x, t * z * z + c]])


def _same(A, B):
    return bool(np.all(np.abs(A - B) <= 1e-6))


def _generators(sym):
    s = sym.lower()
    phi = (1 + math.sqrt(5.0)) / 2
    if s[0] in "cd" and s[1:].isdigit():
        n = int(s[1:])
        gens = [_rot_axis(2 * math.pi / n, 0, 0, 1)] if n > 1 else []
        if s[0] == "d":
            gens.append(_rot_axis(math.pi, 1, 0, 0))
        return gens, 0.0
    if s == "t":
        return [_rot_axis(2 * math.pi / 3, 0, 0, 1), _rot_axis(math.pi, 0, math.sqrt(2.0 / 3.0), math.sqrt(1.0 / 3.0))], 0.0
    if s == "o":
        return [_rot_axis(2 * math.pi / 3, 1, 1, 1), _rot_axis(math.pi / 2, 0, 0, 1)], 0.0
    if s in ("i", "i1", "i2", "i3", "i4"):
        tilt = {"i1": 90.0, "i3": 31.7174745559, "i4": -31.7174745559}.get(s, 0.0)
        return [_rot_axis(math.pi, 0, 0, 1), _rot_axis(2 * math.pi / 5, -phi, -1, 0), _rot_axis(2 * math.pi / 3, -1, -phi * phi, 0)], tilt
    raise ValueError(sym)


def group_matrices(sym, no_group=False):
    """the R of SymList::getMatrices for a point-group name, identity excluded, in the order the host's SymList lists them. no_group
    (accuracy = -1): the powers of every generator line, without the closure"""
    gens, tilt = _generators(sym)
    I = np.eye(3)
    if no_group:
        R = []
        for g in gens:
            P = g
            while not _same(P, I):
                R.append(P)
                P = _mul(P, g)
                assert len(R) <= 240
    else:
        G = [I]
        grew = True
        while grew:
            grew = False
            for a in range(len(G)):
                for g in gens:
                    P = _mul(G[a], g)
                    if not any(_same(h, P) for h in G):
                        G.append(P)
                        grew = True
                    assert len(G) <= 240
        R = G[1:]
    if tilt != 0.0:
        b = tilt * math.pi / 180.0
        cb, sb = math.cos(b), math.sin(b)
        A = np.array([[cb, 0, -sb], [0, 1, 0], [sb, 0, cb]])
        R = [_mul(_mul(A, g), A.T) for g in R]
    return np.array(R).reshape(-1, 3, 3)


# ---------------------------------------------------------------- spline coefficients
def prefilter_axis(c, axis, dtype=np.float64):
    """the recursive filter of the oracle's prefilter1d along one axis, in place semantics on a copy"""
    c = np.moveaxis(np.array(c, dtype=dtype), axis, 0).copy()
    n = c.shape[0]
    if n == 1:
        return np.moveaxis(c, 0, axis)
    z = Z_POLE
    lam = (1.0 - z) * (1.0 - 1.0 / z)
    c *= lam
    s = c[0].copy()
    zk = z
    broke = False
    for k in range(1, n + 1):
        s = s + zk * c[k - 1]
        zk *= z
        if abs(zk) < 1e-300:
            broke = True
            break
    if not broke:
        for k in range(n + 1, 2 * n):
            s = s + zk * c[2 * n - k]
            zk *= z
        s = s / (1.0 - zk)
    c[0] = s
    for i in range(1, n):
        c[i] = c[i] + z * c[i - 1]
    c[n - 1] = (z / (z - 1.0)) * c[n - 1]
    for i in range(n - 2, -1, -1):
        c[i] = z * (c[i + 1] - c[i])
    return np.moveaxis(c, 0, axis)


def prefilter(v, dtype=np.float64):
    """produceSplineCoefficients(BSPLINE3): x, then y (, then z) lines. dtype: the type the filter is carried in"""
    v = np.asarray(v, dtype=dtype)
    for axis in range(v.ndim - 1, -1, -1):
        v = prefilter_axis(v, axis, dtype)
    return np.ascontiguousarray(v)


def bspline03(x):
    """in the type of x: 2 / 3 and 1 / 6 are rounded to it"""
    t = x.dtype.type
    a = np.abs(x)
    inner = a * a * (a - 2.0) * 0.5 + t(2) / t(3)
    b = a - 2.0
    outer = b * b * b * (-(t(1) / t(6)))
    return np.where(a < 1.0, inner, np.where(a < 2.0, outer, 0.0))


# ---------------------------------------------------------------- applyGeometry
def realwrap(x, x0, xF):
    L = xF - x0
    out = x.copy()
    lo, hi = x < x0, x > xF
    out[lo] = x[lo] - np.trunc((x[lo] - x0) / L - 1) * L
    out[hi] = x[hi] - np.trunc((x[hi] - xF) / L + 1) * L
    return out


def source_coords(shape, Ainv, wrap, direct):
    """for every output element and every axis (x first): the coordinate the range test saw, the coordinate after it (wrapped under wrap)
    and whether the element takes the outside value. shape (Y, X) with a homogeneous 3 x 3 Ainv, or (Z, Y, X) with a 3 x 3 Ainv"""
    nd = len(shape)
    dims = shape[::-1]                                        # x, y (, z)
    cen = [d // 2 for d in dims]
    lo = [float(-c) for c in cen]
    hi = [float(d - c - 1) for d, c in zip(dims, cen)]
    grids = np.meshgrid(*[np.arange(d, dtype=np.float64) - c for d, c in zip(shape, cen[::-1])], indexing="ij")
    if nd == 2:
        y, x = grids
        rows = [(Ainv[0, 0], Ainv[0, 1], Ainv[0, 2]), (Ainv[1, 0], Ainv[1, 1], Ainv[1, 2])]
        start = [x * r[0] + y * r[1] + r[2] for r in rows]
        step = [Ainv[0, 0], Ainv[1, 0]]
    else:
        z, y, x = grids
        start = [x * Ainv[r, 0] + y * Ainv[r, 1] + z * Ainv[r, 2] for r in range(3)]
        step = [Ainv[0, 0], Ainv[1, 0], Ainv[2, 0]]
    tested = [np.empty(shape) for _ in range(nd)]
    final = [np.empty(shape) for _ in range(nd)]
    outside = np.zeros(shape, dtype=bool)

    def test(c, a):
        bad = (c < lo[a] - ACC) | (c > hi[a] + ACC)
        if wrap:
            w = c.copy()
            if bad.any():
                w[bad] = realwrap(c[bad], lo[a] - 0.5, hi[a] + 0.5)
            return w, np.zeros_like(bad)
        return c, bad

    if direct:
        for a in range(nd):
            tested[a][...] = start[a]
            final[a], bad = test(start[a], a)
            outside |= bad
        return tested, final, outside
    X = shape[-1]
    cur = [s[..., 0].copy() for s in start]                   # the row's first element
    for j in range(X):
        for a in range(nd):
            tested[a][..., j] = cur[a]
            w, bad = test(cur[a], a)
            final[a][..., j] = w
            outside[..., j] |= bad
            cur[a] = w + step[a]                              # the wrapped value is carried on
    return tested, final, outside


def _mirror(l, n):
    return np.where(l < 0, -l - 1, np.where(l >= n, 2 * n - l - 1, l))


def interp_linear2d(V, xp, yp, wrap):
    Y, X = V.shape
    wx = xp + X // 2
    m1 = np.trunc(wx).astype(np.int64)
    wx = wx - m1
    m2 = m1 + 1
    wy = yp + Y // 2
    n1 = np.trunc(wy).astype(np.int64)
    wy = wy - n1
    n2 = n1 + 1
    if wrap:
        m2 = np.where(m2 >= X, 0, m2)
        n2 = np.where(n2 >= Y, 0, n2)
    mx, my = (wx != 0) & (m2 < X), (wy != 0) & (n2 < Y)
    m2c, n2c = np.minimum(m2, X - 1), np.minimum(n2, Y - 1)
    wx_1, wy_1 = 1 - wx, 1 - wy
    aux2 = wy_1 * wx_1
    tmp = aux2 * V[n1, m1]
    tmp = tmp + np.where(mx, (wy_1 - aux2) * V[n1, m2c], 0.0)
    aux2 = wy * wx_1
    tmp = tmp + np.where(my, aux2 * V[n2c, m1], 0.0)
    tmp = tmp + np.where(my & mx, (wy - aux2) * V[n2c, m2c], 0.0)
    return tmp


def interp_linear3d(V, xp, yp, zp, wrap):
    Z, Y, X = V.shape
    wx = xp + X // 2
    m1 = np.trunc(wx).astype(np.int64)
    wx = wx - m1
    m2 = m1 + 1
    wy = yp + Y // 2
    n1 = np.trunc(wy).astype(np.int64)
    wy = wy - n1
    n2 = n1 + 1
    wz = zp + Z // 2
    o1 = np.trunc(wz).astype(np.int64)
    wz = wz - o1
    o2 = o1 + 1
    if wrap:
        m2 = np.where(m2 >= X, 0, m2)
        n2 = np.where(n2 >= Y, 0, n2)
        o2 = np.where(o2 >= Z, 0, o2)
    mx, my, mz = (wx != 0) & (m2 < X), (wy != 0) & (n2 < Y), (wz != 0) & (o2 < Z)
    m2c, n2c, o2c = np.minimum(m2, X - 1), np.minimum(n2, Y - 1), np.minimum(o2, Z - 1)
    wx_1, wy_1, wz_1 = 1 - wx, 1 - wy, 1 - wz
    tmp = wz_1 * wy_1 * wx_1 * V[o1, n1, m1]
    tmp = tmp + np.where(mx, wz_1 * wy_1 * wx * V[o1, n1, m2c], 0.0)
    tmp = tmp + np.where(my, wz_1 * wy * wx_1 * V[o1, n2c, m1], 0.0)
    tmp = tmp + np.where(my & mx, wz_1 * wy * wx * V[o1, n2c, m2c], 0.0)
    tmp = tmp + np.where(mz, wz * wy_1 * wx_1 * V[o2c, n1, m1], 0.0)
    tmp = tmp + np.where(mz & mx, wz * wy_1 * wx * V[o2c, n1, m2c], 0.0)
    tmp = tmp + np.where(mz & my, wz * wy * wx_1 * V[o2c, n2c, m1], 0.0)
    tmp = tmp + np.where(mz & my & mx, wz * wy * wx * V[o2c, n2c, m2c], 0.0)
    return tmp


def interp_bspline2d(C, xp, yp):
    Y, X = C.shape
    x, y = xp + X // 2, yp + Y // 2
    l1 = np.ceil(x - 2).astype(np.int64)
    m1 = np.ceil(y - 2).astype(np.int64)
    columns = np.zeros_like(x)
    for t in range(4):
        m = m1 + t
        em = _mirror(m, Y)
        rows = np.zeros_like(x)
        for u in range(4):
            l = l1 + u
            rows = rows + C[em, _mirror(l, X)] * bspline03(x - l)
        columns = columns + rows * bspline03(y - m)
    return columns


def interp_bspline3d(C, xp, yp, zp):
    Z, Y, X = C.shape
    x, y, z = xp + X // 2, yp + Y // 2, zp + Z // 2
    l1 = np.ceil(x - 2).astype(np.int64)
    m1 = np.ceil(y - 2).astype(np.int64)
    n1 = np.ceil(z - 2).astype(np.int64)
    wx = [bspline03(x - (l1 + u)) for u in range(4)]
    el = [_mirror(l1 + u, X) for u in range(4)]
    slices = np.zeros_like(x)
    for tz in range(4):
        n = n1 + tz
        en = _mirror(n, Z)
        columns = np.zeros_like(x)
        for ty in range(4):
            m = m1 + ty
            em = _mirror(m, Y)
            rows = np.zeros_like(x)
            for u in range(4):
                rows = rows + C[en, em, el[u]] * wx[u]
            columns = columns + rows * bspline03(y - m)
        slices = slices + columns * bspline03(z - n)
    return slices


def apply_geometry(V, A, degree, wrap, outside=0.0, direct=True, coef=None, coords=None):
    """xmippCore applyGeometry(degree, V2, V1, A, IS_NOT_INV, wrap, outside) of an image (A homogeneous 3 x 3) or a volume (A 3 x 3, no shifts).
    coords: a list that receives the coordinates the range tests saw, for the callers' precondition"""
    V = np.asarray(V, dtype=np.float64)
    if is_identity(A):
        return V.copy()
    tested, final, out = source_coords(V.shape, inv3x3(A), wrap, direct)
    if coords is not None:
        coords.append(tested)
    inside = ~out
    res = np.full(V.shape, float(outside))
    pts = [f[inside] for f in final]
    if degree == 1:
        res[inside] = interp_linear2d(V, *pts, wrap) if V.ndim == 2 else interp_linear3d(V, *pts, wrap)
    else:
        C = prefilter(V) if coef is None else coef
        res[inside] = interp_bspline2d(C, *pts) if V.ndim == 2 else interp_bspline3d(C, *pts)
    return res


def rotate2d(V, ang, degree, wrap, outside=0.0, direct=False):
    return apply_geometry(V, rotation2d_matrix(ang), degree, wrap, outside, direct)


def threshold_margin(shape, tested):
    """the smallest distance of any tested coordinate to a threshold min - 1e-6 or max + 1e-6 of its axis"""
    dims = shape[::-1]
    best = np.inf
    for a, c in enumerate(tested):
        cen = dims[a] // 2
        for thr in (-cen - ACC, dims[a] - cen - 1 + ACC):
            best = min(best, float(np.abs(c - thr).min()))
    return best


def threshold_margin_both_forms(shape, As, wrap):
    """the precondition of a device comparison: the smallest distance to a threshold over the matrices As (as applyGeometry takes them,
    IS_NOT_INV) in the incremental and in the direct coordinate form"""
    best = np.inf
    for A in As:
        if is_identity(A):
            continue
        Ainv = inv3x3(A)
        for direct in (False, True):
            best = min(best, threshold_margin(shape, source_coords(shape, Ainv, wrap, direct)[0]))
    return best


def wrap_edge_mask(shape, coords, eps=1e-9):
    """The elements a WRAP run may not be compared on. realWRAP(c, min - 0.5, max + 0.5) sends max + 0.5 to itself and anything above it to
    just over min - 0.5; the interpolation at those two ends differs (at min - 0.5 the (int) truncation extrapolates from taps 0 and 1, at
    max + 0.5 it averages taps dim - 1 and 0), so the reference itself jumps where a coordinate sits on such an edge, and which side it
    falls on is decided by its last bit. Groups with entries of exactly 1/2 (the icosahedral ones) put coordinates exactly there on even
    boxes. coords: the tested coordinates of every matrix (and of both coordinate forms, when both are compared); an element is masked when
    any of them lies within eps of min - 0.5 + k dim for an integer k"""
    dims = shape[::-1]
    mask = np.zeros(shape, dtype=bool)
    for tested in coords:
        for a, c in enumerate(tested):
            L = float(dims[a])
            r = np.mod(c - (-(dims[a] // 2) - 0.5), L)
            mask |= np.minimum(r, L - r) < eps
    return mask


# ---------------------------------------------------------------- symmetrize
def outside_mean(V):
    """computeStats_within_binary_mask's average over BinaryCircularMask(min(dims) / 2, OUTSIDE_MASK)"""
    V = np.asarray(V, dtype=np.float64)
    return float(V[outside_mask(V.shape)].mean())


def outside_mask(shape):
    rad = min(shape) // 2
    grids = np.meshgrid(*[np.arange(d, dtype=np.float64) - d // 2 for d in shape], indexing="ij")
    r2 = np.zeros(shape)
    for g in grids:
        r2 = r2 + g * g
    return r2 >= float(rad * rad)


def symmetrize_volume(V, R, degree, wrap, sum_=False, direct=True, coords=None):
    """symmetrizeVolume (symmetrize.cpp:117-169) without helix and mask; R the matrices of SL.getMatrices"""
    V = np.asarray(V, dtype=np.float64)
    avg = 0.0 if wrap else outside_mean(V)
    C = prefilter(V) if degree == 3 else None
    out = V.copy()
    for Ri in R:
        out = out + apply_geometry(V, np.asarray(Ri).T, degree, wrap, avg, direct, C, coords)
    if not sum_:
        out = out * (1.0 / float(np.float32(len(R)) + np.float32(1.0)))
    return out


def symmetrize_image(I, order, degree, wrap, sum_=False, direct=True, coords=None):
    """symmetrizeImage (symmetrize.cpp:187-214)"""
    I = np.asarray(I, dtype=np.float64)
    avg = 0.0 if wrap else outside_mean(I)
    C = prefilter(I) if degree == 3 else None
    out = I.copy()
    for i in range(1, order):
        out = out + apply_geometry(I, rotation2d_matrix(360.0 / order * i), degree, wrap, avg, direct, C, coords)
    if not sum_:
        out = out * (1.0 / order)
    return out


def symmetrize_image_exact(I, order, degree, wrap):
    """symmetrize_image's direct form, averaged, evaluated in higher precision, to calibrate a bound where the incremental form drifts
    (it adds A00 along a row, so its distance to the direct form grows with the row). The source coordinates, and with them every
    truncation, ceil, comparison and tap index, are the float64 ones of source_coords; the fractions, the weights, the spline coefficients,
    the outside mean and every sum are carried in np.longdouble (64 bits of mantissa on x86). Not a restatement of the reference's
    operation order: the bilinear weights are the plain products"""
    LD = np.longdouble
    I = np.asarray(I, dtype=np.float64)
    Y, X = I.shape
    V = I.astype(LD)
    out_mask = outside_mask(I.shape)
    avg = LD(0) if wrap else V[out_mask].sum() / LD(int(out_mask.sum()))
    C = prefilter(I, LD) if degree == 3 else None
    out = V.copy()
    for i in range(1, order):
        _, final, outm = source_coords(I.shape, inv3x3(rotation2d_matrix(360.0 / order * i)), wrap, True)
        inside = ~outm
        x, y = final[0][inside] + X // 2, final[1][inside] + Y // 2          # float64: they decide the taps
        if degree == 1:
            m1, n1 = np.trunc(x).astype(np.int64), np.trunc(y).astype(np.int64)
            wx, wy = x.astype(LD) - m1, y.astype(LD) - n1
            m2, n2 = m1 + 1, n1 + 1
            if wrap:
                m2, n2 = np.where(m2 >= X, 0, m2), np.where(n2 >= Y, 0, n2)
            mx, my = (wx != 0) & (m2 < X), (wy != 0) & (n2 < Y)
            m2, n2 = np.minimum(m2, X - 1), np.minimum(n2, Y - 1)
            val = (1 - wy) * (1 - wx) * V[n1, m1] + np.where(mx, (1 - wy) * wx * V[n1, m2], 0) + np.where(my, wy * (1 - wx) * V[n2, m1], 0)
            val = val + np.where(my & mx, wy * wx * V[n2, m2], 0)
        else:
            l1, q1 = np.ceil(x - 2).astype(np.int64), np.ceil(y - 2).astype(np.int64)
            xl, yl = x.astype(LD), y.astype(LD)
            val = np.zeros(x.shape, dtype=LD)
            for t in range(4):
                row = np.zeros(x.shape, dtype=LD)
                for u in range(4):
                    row = row + C[_mirror(q1 + t, Y), _mirror(l1 + u, X)] * bspline03(xl - (l1 + u))
                val = val + row * bspline03(yl - (q1 + t))
        res = np.full(I.shape, avg, dtype=LD)
        res[inside] = val
        out = out + res
    return out * LD(1.0 / order)


# ---------------------------------------------------------------- helix
MAX_DEPTH = 6


class _Helix:
    def __init__(self, V, zHelical, rotHelical):
        self.V = V
        self.zHelical = zHelical
        self.sin, self.cos = math.sin(rotHelical), math.cos(rotHelical)
        self.depth = 0


def _helical_int(H, x, y, z, need, depth):
    """interpolatedElement3DHelicalInt for arrays of integer points; need: the corner's weight is not exactly 0"""
    V = H.V
    Z, Y, X = V.shape
    sz, sy, sx = -(Z // 2), -(Y // 2), -(X // 2)
    out = np.zeros(x.shape)
    inxy = (x >= sx) & (x <= sx + X - 1) & (y >= sy) & (y <= sy + Y - 1) & need
    inz = (z >= sz) & (z <= sz + Z - 1)
    a = inxy & inz
    out[a] = V[z[a] - sz, y[a] - sy, x[a] - sx]
    for b, sign in ((inxy & (z < sz), 1.0), (inxy & (z > sz + Z - 1), -1.0)):
        if not b.any():
            continue
        if depth + 1 > MAX_DEPTH:
            raise RecursionError("interpolatedElement3DHelical does not terminate")
        H.depth = max(H.depth, depth + 1)
        xb, yb, zb = x[b].astype(np.float64), y[b].astype(np.float64), z[b].astype(np.float64)
        if sign > 0:
            newx, newy = H.cos * xb - H.sin * yb, H.sin * xb + H.cos * yb
            out[b] = _helical_interp(H, newx, newy, zb + H.zHelical, depth + 1)
        else:
            newx, newy = H.cos * xb + H.sin * yb, -H.sin * xb + H.cos * yb
            out[b] = _helical_interp(H, newx, newy, zb - H.zHelical, depth + 1)
    return out


def _helical_interp(H, x, y, z, depth=0):
    """interpolatedElement3DHelical; a corner of weight exactly 0 is not evaluated (l + (h - l) 0 is l)"""
    x0, y0, z0 = np.floor(x).astype(np.int64), np.floor(y).astype(np.int64), np.floor(z).astype(np.int64)
    fx, fy, fz = x - x0, y - y0, z - z0
    x1, y1, z1 = x0 + 1, y0 + 1, z0 + 1
    hx, hy, hz = fx != 0, fy != 0, fz != 0
    t = np.ones(x.shape, dtype=bool)
    d000 = _helical_int(H, x0, y0, z0, t, depth)
    d001 = _helical_int(H, x1, y0, z0, hx, depth)
    d010 = _helical_int(H, x0, y1, z0, hy, depth)
    d011 = _helical_int(H, x1, y1, z0, hx & hy, depth)
    d100 = _helical_int(H, x0, y0, z1, hz, depth)
    d101 = _helical_int(H, x1, y0, z1, hz & hx, depth)
    d110 = _helical_int(H, x0, y1, z1, hz & hy, depth)
    d111 = _helical_int(H, x1, y1, z1, hz & hx & hy, depth)
    lin = lambda a, l, h: l + (h - l) * a
    dx00 = np.where(hx, lin(fx, d000, d001), d000)
    dx01 = np.where(hx, lin(fx, d100, d101), d100)
    dx10 = np.where(hx, lin(fx, d010, d011), d010)
    dx11 = np.where(hx, lin(fx, d110, d111), d110)
    dxy0 = np.where(hy, lin(fy, dx00, dx10), dx00)
    dxy1 = np.where(hy, lin(fy, dx01, dx11), dx01)
    return np.where(hz, lin(fz, dxy0, dxy1), dxy0)


def helical_depth(Z, zHelical, heightFraction, dihedral):
    """the recursion bound the device relies on: -1 no bound, else 0 or 1"""
    if not (1.0 < zHelical <= Z) or not (0.0 < heightFraction <= 1.0):
        return -1
    n = int(math.floor(heightFraction * Z + 0.5))
    if n < 1 or n > Z:
        return -1
    return 1 if (dihedral and Z % 2 == 0 and n == Z) else 0


def symmetry_helical(V, zHelical, rotHelical, rot0=0.0, dihedral=False, heightFraction=0.95, Cn=1, stats=None):
    """symmetry_Helical (symmetries.cpp:1632-1705), mask == nullptr. stats: a dict that receives the recursion depth reached"""
    V = np.asarray(V, dtype=np.float64)
    Z, Y, X = V.shape
    n = int(math.floor(heightFraction * Z + 0.5))              # round()
    zFirst = -(n // 2)
    zLast = zFirst + n - 1
    iz = 1.0 / zHelical
    zH2 = int(math.floor(0.5 * zHelical))
    H = _Helix(V, zHelical, rotHelical)
    Llength = int(math.ceil(Z * iz))
    sinCn = [math.sin(c * (2 * math.pi) / Cn) for c in range(Cn)]
    cosCn = [math.cos(c * (2 * math.pi) / Cn) for c in range(Cn)]
    kk, ii, jj = np.meshgrid(np.arange(Z) - Z // 2, np.arange(Y) - Y // 2, np.arange(X) - X // 2, indexing="ij")
    k, i, j = kk.ravel().astype(np.float64), ii.ravel().astype(np.float64), jj.ravel().astype(np.float64)
    rot = np.arctan2(i, j) + rot0
    rho = np.sqrt(i * i + j * j)
    l0 = np.ceil((-(Z // 2) - kk.ravel()) * iz)
    final, L = np.zeros(k.shape), np.zeros(k.shape)
    for t in range(Llength + 1):
        l = l0 + t
        kp_all = k + l * zHelical
        ok = (kp_all >= zFirst) & (kp_all <= zLast)
        if not ok.any():
            continue
        kp = kp_all[ok]
        rotp = rot[ok] + l[ok] * rotHelical
        ip, jp = rho[ok] * np.sin(rotp), rho[ok] * np.cos(rotp)
        w = np.ones(kp.shape)
        first = kp - zFirst <= zH2
        last = ~first & (zLast - kp <= zH2)
        w[first] = (kp[first] - zFirst + 1) / (zH2 + 1)
        w[last] = (zLast + 1 - kp[last]) / (zH2 + 1)
        f, Ls = final[ok], L[ok]

        def add(x, y, z):
            nonlocal f, Ls
            f = f + w * _helical_interp(H, x, y, z)
            Ls = Ls + w

        add(jp, ip, kp)
        for c in range(1, Cn):
            add(cosCn[c] * jp - sinCn[c] * ip, sinCn[c] * jp + cosCn[c] * ip, kp)
        if dihedral:
            add(jp, -ip, -kp)
            for c in range(1, Cn):
                add(cosCn[c] * jp - sinCn[c] * (-ip), sinCn[c] * jp + cosCn[c] * (-ip), -kp)
        final[ok], L[ok] = f, Ls
    if stats is not None:
        stats["depth"] = H.depth
    with np.errstate(invalid="ignore", divide="ignore"):
        return (final / L).reshape(V.shape)


def symmetrize_helical(V, zHelical, rotHelical, rot0=0.0, dihedral=False, heightFraction=0.95, Cn=1, degree=3, direct=True, stats=None):
    """symmetrizeVolume's helical / helicalDihedral branches (symmetrize.cpp:170-179)"""
    out = symmetry_helical(V, zHelical, rotHelical, rot0, dihedral, heightFraction, Cn, stats)
    if dihedral:
        out = (out + apply_geometry(out, rotation3d_x(180.0), degree, True, 0.0, direct)) * 0.5
    return out


# ---------------------------------------------------------------- the device tests' cases and bound
SMALL = [(20, 20, 20), (21, 21, 21), (18, 20, 23)]
BIG = (66, 70, 68)
GROUPS = ["c5", "d3", "o", "i1"]
# 16 times the largest relative difference between the incremental and the direct coordinate form over parity_cases(), rounded up to a
# power of ten (tests/test_symmetrize_ref.py derives and asserts it); relative to max|V_in|
BOUND = 1e-13


def parity_cases():
    """(shape, group, degree, wrap) of every point-group case the device is compared on"""
    out = [(s, g, d, w) for s in SMALL for g in GROUPS for d in (1, 3) for w in (True, False)]
    return out + [(BIG, "c5", d, w) for d in (1, 3) for w in (True, False)] + mid_cases()


# ---------------------------------------------------------------- the cases past the first lap (tests/test_gpu_symmetrize_laps.py)
MID = (36, 44, 41)            # every side different, one odd, Y and X leave partial bricks: 9 x 6 x 6 = 324 bricks of 4 x 8 x 8
MID_GROUPS = ["t", "i1"]
SY_BOX = 18 * 18 * 18         # the doubles of LDS the spline pass stages a brick's source box in
# a rotation with no special entries: the product of two turns about oblique axes
A0 = _mul(_rot_axis(0.7, 0.2, -0.5, 1.0), _rot_axis(-1.9, 1.0, 0.3, 0.1))
# 16 times the largest relative difference between the two coordinate forms over general_cases(), the list of matrix_list() and A0 at
# TILE_APPLY, rounded up to a power of ten (tests/test_symmetrize_ref.py derives and asserts it); relative to max|V_in|
BOUND_GENERAL = 1e-12


def mid_cases():
    """(shape, group, degree, wrap) of the point groups at MID: oblique axes, most bricks interior"""
    return [(MID, g, d, w) for g in MID_GROUPS for d in (1, 3) for w in (True, False)]


def general_matrices():
    """name -> A (as applyGeometry takes it, IS_NOT_INV) of the matrices that are no rotation. The inverse of s A0 stretches by 1 / s:
    below about 0.65 a brick's source box passes SY_BOX, at 1.7 nearly every box is staged. The shear's entries are not round, so that no
    coordinate falls on a wrap edge (tests/test_symmetrize_ref.py asserts it)"""
    return {
        "0.5 A0": 0.5 * A0,
        "0.62 A0": 0.62 * A0,
        "0.8 A0": 0.8 * A0,
        "1.7 A0": 1.7 * A0,
        "diag(0.45, 1, 2) A0": _mul(np.diag([0.45, 1.0, 2.0]), A0),
        "diag(-1, 1, 1) A0": _mul(np.diag([-1.0, 1.0, 1.0]), A0),
        "shear": np.array([[1.0, 0.8731, 0.0], [0.0, 1.0, 0.7919], [0.6843, 0.0, 1.0]]),
    }


def general_cases():
    """(name, degree, wrap) of every single-matrix case at MID"""
    return [(n, d, w) for n in general_matrices() for d in (1, 3) for w in (True, False)]


def matrix_list():
    """the R of the list that goes through set_matrices at MID: two rotations of t around an identity entry (applyGeometry's copy
    shortcut, in the middle of a list) and a matrix that is no rotation"""
    g = group_matrices("t")
    return np.array([g[0], np.eye(3) + 5e-7, (0.8 * A0).T, g[1]])


def staging_census(shape, Ainvs):
    """The decision of the spline pass (k_sy_pass_staged) for every (brick, matrix) pair, transcribed operation by operation: a brick of
    4 x 8 x 8 output voxels bounds its source points by the per-term minima and maxima of Ainv times its corners, adds the spline support
    and stages that box in LDS when it lies inside the volume and holds SY_BOX doubles at the most. Ainvs: the inverses the device forms
    (inv3x3 of what applyGeometry takes), identity entries left out. A precondition tool: it says which branch a case reaches, and is
    never used to predict or excuse a device result.
    Returns staged, border (the box leaves the volume), over (inside, above SY_BOX), largest (staged box, 0 if none) and partial (staged
    pairs on a brick that the volume cuts)"""
    Z, Y, X = shape
    dim = (X, Y, Z)
    nb_ = ((X + 7) // 8, (Y + 7) // 8, (Z + 3) // 4)
    side = (8, 8, 4)
    b = np.meshgrid(*[np.arange(n) for n in nb_], indexing="ij")                     # bx, by, bz
    p0 = [(b[c] * side[c] - dim[c] // 2).astype(np.float64) for c in range(3)]
    p1 = [(np.minimum(b[c] * side[c] + side[c] - 1, dim[c] - 1) - dim[c] // 2).astype(np.float64) for c in range(3)]
    cut = np.zeros(b[0].shape, dtype=bool)
    for c in range(3):
        cut |= b[c] * side[c] + side[c] - 1 > dim[c] - 1
    out = {"staged": 0, "border": 0, "over": 0, "largest": 0, "partial": 0}
    for Ainv in Ainvs:
        Ainv = np.asarray(Ainv, dtype=np.float64).reshape(3, 3)
        inside = np.ones(b[0].shape, dtype=bool)
        size = np.ones(b[0].shape, dtype=np.int64)
        for r in range(3):
            cmin, cmax = np.zeros(b[0].shape), np.zeros(b[0].shape)
            for c in range(3):
                u, v = Ainv[r, c] * p0[c], Ainv[r, c] * p1[c]
                cmin = cmin + np.minimum(u, v)
                cmax = cmax + np.maximum(u, v)
            ilo = np.floor(cmin + dim[r] // 2 - 2.0 - 1e-3).astype(np.int64)
            ihi = np.floor(cmax + dim[r] // 2 + 2.0 + 1e-3).astype(np.int64)
            inside &= (ilo >= 0) & (ihi <= dim[r] - 1)
            size = size * (ihi - ilo + 1)
        staged = inside & (size <= SY_BOX)
        out["staged"] += int(staged.sum())
        out["border"] += int((~inside).sum())
        out["over"] += int((inside & ~staged).sum())
        out["partial"] += int((staged & cut).sum())
        if staged.any():
            out["largest"] = max(out["largest"], int(size[staged].max()))
    return out


def prefilter_tile(X):
    """the rows of one workgroup of the x prefilter: what 48 KB of LDS hold of rows padded to an odd length, 64 at the most"""
    return max(1, min(64, 48 * 1024 // (8 * (X | 1))))


# shape -> the tile: the last X with the full tile, the first with a smaller one, two tiles with the second partial (78 rows), the size cap
TILE_SHAPES = {(5, 7, 95): 64, (5, 7, 96): 63, (3, 26, 131): 46, (2, 3, 1024): 5}
TILE_APPLY = (3, 26, 131)     # one spline applyGeometry (A0, wrap) reads the coefficients of its two tiles

# stacks: 17 images of 250 x 262 pass 256 . 16 pixels per CU on 256 CUs (1 113 500); 65 600 images of 4 x 6 pass the 65 535 workgroups of
# the outside mean, image i a copy of base image i % 7
STACK_BIG, STACK_ORDER = (17, 250, 262), 5
STACK_MANY, STACK_BASE = (65600, 4, 6), 7
# 16 times the largest relative distance of the direct form to symmetrize_image_exact over the stack cases, rounded up to a power of ten,
# or BOUND where that is smaller (tests/test_symmetrize_ref.py derives and asserts it); relative to max|I|
BOUND_IMAGES = BOUND


def big_stack():
    return np.stack([phantom(STACK_BIG[1:], 50 + i) for i in range(STACK_BIG[0])])


def base_images():
    return np.stack([phantom(STACK_MANY[1:], 70 + i) for i in range(STACK_BASE)])


# the helix past 256 . 16 voxels per CU on 256 CUs (1 050 600 voxels; Z flat, so that the restatement stays cheap):
# the box, then zHelical in voxels, rotHelical in degrees, the phase, Cn, heightFraction; not dihedral
HELIX_LAP = ((25, 206, 204), 4.3, -41.5, 0.2, 2, 0.95)


# ---------------------------------------------------------------- test data
def phantom(shape, seed=0):
    """positive blobs off the centre on a base level, no symmetry; float32 values so that files carry them exactly"""
    rng = np.random.default_rng(seed)
    grids = np.meshgrid(*[np.arange(d, dtype=np.float64) - d // 2 for d in shape], indexing="ij")
    v = np.full(shape, 0.25)
    for _ in range(5):
        c = [rng.uniform(-0.3, 0.3) * d for d in shape]
        s = rng.uniform(1.5, 3.5)
        r2 = sum((g - ci) ** 2 for g, ci in zip(grids, c))
        v = v + rng.uniform(0.5, 1.5) * np.exp(-r2 / (2 * s * s))
    v = v + 0.05 * rng.standard_normal(shape)
    return v.astype(np.float32).astype(np.float64)
