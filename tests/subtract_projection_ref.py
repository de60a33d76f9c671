"""numpy fp64 restatements: projectVolume in real space (reference libraries/data/projection.cpp:337-589), the comparator of xh_rsp,
and below it preProcess + processImage of libraries/reconstruction/subtract_projection.cpp, the comparator of xh_sub. The four rays of a pixel are walked one after the other into one running ray_sum, as the reference does; all pixels of a
ray walk together. Next to the plane it returns what the support checks need: the support (some step with diff_alpha > 0 on a voxel
with v > 0) and the marginal pixels, those whose answer hangs on a comparison that rounding could turn."""
import numpy as np

EQ = 1e-6          # XMIPP_EQUAL_ACCURACY
GAP = 1e-9         # a decision closer than this is marginal


def _round(v):
    # ROUND: (x > 0) ? (int)(x + 0.5) : (int)(x - 0.5); the cast truncates
    return np.where(v > 0, np.trunc(v + 0.5), np.trunc(v - 0.5)).astype(np.int64)


def project_volume(vol, E, offset=None):
    """vol [D][D][D] about the Xmipp origin, E the Euler matrix, offset the roffset (x, y) or None.
    Returns plane [D][D], support [D][D] bool, marginal [D][D] bool."""
    D = vol.shape[0]
    x0 = -(D // 2)
    xF = x0 + D - 1
    flat = np.ascontiguousarray(vol, np.float64).ravel()
    setv = np.zeros((D + 2,) * 3, bool)                    # v > 0 with a border, for "next to a set voxel"
    setv[1:-1, 1:-1, 1:-1] = vol > 0
    near = np.zeros((D + 1,) * 3, bool)                    # near[a, b, c]: any set voxel in setv[a:a+2, b:b+2, c:c+2]
    for a in (0, 1):
        for b in (0, 1):
            for c in (0, 1):
                near |= setv[a:a + D + 1, b:b + D + 1, c:c + D + 1]
    any_set = bool(setv.any())
    d = np.array(E[2], np.float64)
    d[d == 0] = EQ
    sgn = np.where(d >= 0, 1, -1)
    half = 0.5 * sgn
    inv = 1.0 / d
    step = 1.0 / 3.0
    ii, jj = np.mgrid[x0:xF + 1, x0:xF + 1]
    ii = ii.ravel().astype(np.float64)
    jj = jj.ravel().astype(np.float64)
    n = ii.size
    ray_sum = np.zeros(n)
    support = np.zeros(n, bool)
    marginal = np.zeros(n, bool)
    Et = np.asarray(E, np.float64).T
    for ray in range(4):
        rx = jj + step if ray & 2 else jj - step
        ry = ii + step if ray & 1 else ii - step
        rz = np.zeros(n)
        if offset is not None:
            rx = rx - offset[0]
            ry = ry - offset[1]
        p1 = [Et[c, 0] * rx + Et[c, 1] * ry + Et[c, 2] * rz for c in range(3)]
        ps = [p1[c] - half[c] for c in range(3)]
        amin = np.full(n, -np.inf)
        amax = np.full(n, np.inf)
        for c in range(3):
            lo = (x0 - 0.5 - p1[c]) * inv[c]
            hi = (xF + 0.5 - p1[c]) * inv[c]
            sw = lo < hi
            a, b = np.where(sw, lo, hi), np.where(sw, hi, lo)
            amin = a if c == 0 else np.fmax(a, amin)
            amax = b if c == 0 else np.fmin(b, amax)
        span = amax - amin
        act = ~(span < EQ)
        if any_set:
            marginal |= np.abs(span - EQ) < GAP
        v = [p1[c] + d[c] * amin for c in range(3)]
        idx = [np.clip(_round(v[c]), x0, xF) for c in range(3)]
        # an entry coordinate within GAP of a rounding boundary, where CLIP does not settle it
        amb = np.zeros(n, bool)
        for c in range(3):
            amb |= np.clip(_round(v[c] - GAP), x0, xF) != np.clip(_round(v[c] + GAP), x0, xF)
        alpha = amin.copy()
        hit = np.zeros(n, bool)
        first = True
        for _ in range(3 * D + 8):
            if not act.any():
                break
            k = np.nonzero(act)[0]
            xi, yi, zi = idx[0][k], idx[1][k], idx[2][k]
            ax = (xi.astype(np.float64) - ps[0][k]) * inv[0]
            ay = (yi.astype(np.float64) - ps[1][k]) * inv[1]
            az = (zi.astype(np.float64) - ps[2][k]) * inv[2]
            al = alpha[k]
            dx, dy, dz = np.abs(al - ax), np.abs(al - ay), np.abs(al - az)
            src = np.zeros(k.size, np.int64)
            da = dx.copy()
            m = dy < da
            src[m] = 1
            da[m] = dy[m]
            m = dz < da
            src[m] = 2
            da[m] = dz[m]
            # the choice of the axis hangs on the two smallest of the three
            three = np.sort(np.stack([dx, dy, dz]), axis=0)
            g = three[1] - three[0]
            ux, uy, uz = xi - x0, yi - x0, zi - x0
            inb = (ux >= 0) & (ux < D) & (uy >= 0) & (uy < D) & (uz >= 0) & (uz < D)
            val = np.zeros(k.size)
            val[inb] = flat[(uz[inb] * D + uy[inb]) * D + ux[inb]]
            ray_sum[k] += da * val
            hit[k] |= (da > 0) & (val > 0)
            new_alpha = np.where(src == 0, ax, np.where(src == 1, ay, az))
            g = np.minimum(g, np.abs((amax[k] - new_alpha) - EQ))
            g = np.where((da > 0) & (da < GAP) & (val > 0), 0.0, g)
            # near: the voxel, and the seven it can step into, hold a set voxel
            nx = np.clip(np.minimum(ux, ux + sgn[0]) + 1, 0, D)
            ny = np.clip(np.minimum(uy, uy + sgn[1]) + 1, 0, D)
            nz = np.clip(np.minimum(uz, uz + sgn[2]) + 1, 0, D)
            nr = near[nz, ny, nx]
            marginal[k] |= (g < GAP) & nr
            if first:
                marginal[k] |= amb[k] & nr
                first = False
            idx[0][k] = xi + np.where(src == 0, sgn[0], 0)
            idx[1][k] = yi + np.where(src == 1, sgn[1], 0)
            idx[2][k] = zi + np.where(src == 2, sgn[2], 0)
            alpha[k] = new_alpha
            act[k] = (amax[k] - new_alpha) > EQ
        assert not act.any(), "a ray outlived 3 D + 8 steps"
        support |= hit
    plane = (ray_sum * 0.25).reshape(D, D)
    top = np.abs(plane).max()
    marginal |= (plane.ravel() > 0) & (plane.ravel() < GAP * top)
    return plane, support.reshape(D, D), marginal.reshape(D, D)


def blob_mask(D, centre=(1.5, -2.0, 0.5), radii=(0.22, 0.3, 0.18)):
    """A binary ellipsoid off the centre, [z][y][x] about the Xmipp origin; radii as fractions of D."""
    z, y, x = np.mgrid[0:D, 0:D, 0:D] - D // 2
    r = ((x - centre[0]) / (radii[0] * D)) ** 2 + ((y - centre[1]) / (radii[1] * D)) ** 2 + ((z - centre[2]) / (radii[2] * D)) ** 2
    return (r <= 1.0).astype(np.float64)


# orientations whose Euler matrix has 0 and +-1 entries up to the rounding of sin / cos, and seeded generic ones
EXACT_ANGLES = [(0.0, 0.0, 0.0), (90.0, 0.0, 0.0), (0.0, 90.0, 0.0), (90.0, 90.0, 90.0), (0.0, 180.0, 270.0)]


def generic_angles(n, seed=20240607):
    rng = np.random.default_rng(seed)
    return [(float(rng.uniform(0, 360)), float(rng.uniform(5, 175)), float(rng.uniform(0, 360))) for _ in range(n)]


OFFSET = (1.3, -2.7)


# ------------------------------------------------------------------ the subtraction pipeline
def freq_map(D, sampling=1.0, max_resolution=-1.0):
    """wi [D][D/2+1] (subtract_projection.cpp L554-563: YSIZE on both axes) and maxwiIdx (L572-580). C's round: half away from zero."""
    fy = np.array([(i if i <= D // 2 else i - D) / D for i in range(D)])[:, None]
    fx = (np.arange(D // 2 + 1) / D)[None, :]
    wi = np.floor(np.sqrt(fy * fy + fx * fx) * D + 0.5).astype(np.int64)
    if max_resolution == -1.0:
        max_resolution = sampling
    cut = (sampling / max_resolution) / np.sqrt(2.0)
    return wi, int(np.floor(D * cut + 0.5))


PRM = dict(sampling=1.0, max_resolution=-1.0, padding=2.0, cirmaskrad=-1.0, subtract=0, real_space=0, ignore_ctf=0, boost=0, non_negative=0)


class Subtract:
    """preProcess + processImage of subtract_projection.cpp for one set of program parameters. `fit` and `choose` are the library's host
    functions (xa.sub_fit, xa.sub_choose): the restatement feeds them its own sums. `ctf_image(kw, Np)` gives getValueAt() with K = 1 on
    the half spectrum [Np][Np/2+1] at the sampling rate."""

    def __init__(self, oracle, vol, roi, maskvol, prm, fit, choose, ctf_image):
        self.o, self.prm, self.fit, self.choose, self.ctf_image = oracle, prm, fit, choose, ctf_image
        D = self.D = vol.shape[0]
        self.roi, self.maskvol = roi, maskvol
        ivM = np.ones_like(vol) if roi is None else (roi if prm["subtract"] else roi * (-1) + 1)
        self.V = vol * ivM
        maxres = prm["sampling"] if prm["max_resolution"] == -1.0 else prm["max_resolution"]
        if not prm["real_space"]:
            # the stated deviation: the device's projector takes floats
            self.fp = oracle.FP(self.V.astype(np.float32).astype(np.float64), prm["padding"], 0.5 * (prm["sampling"] / maxres), 3)
        R = D / 2 if prm["cirmaskrad"] == -1.0 else prm["cirmaskrad"]
        y, x = np.mgrid[0:D, 0:D] - D // 2
        self.circle = ((y * y + x * x) <= R * R).astype(np.float64)          # RaisedCosineMask(R, R)
        self.wi, self.maxwi = freq_map(D, prm["sampling"], prm["max_resolution"])
        self.fit_cells = (self.wi > 0) & (self.wi < self.maxwi)
        self.a11 = float((2 * self.wi[self.fit_cells]).sum())

    def process(self, img, row):
        o, prm, D = self.o, self.prm, self.D
        N = D * D
        E = o.euler_matrix(row["rot"], row["tilt"], row["psi"])
        roff = (-row.get("shift_x", 0.0), -row.get("shift_y", 0.0))
        s = {"marginal": np.zeros((D, D), bool)}
        if prm["real_space"]:
            P = project_volume(self.V, E, roff)[0]
        else:
            A = np.eye(3)
            A[0, 2], A[1, 2] = roff
            P = o.apply_geometry2d(self.fp.project(row["rot"], row["tilt"], row["psi"]), A, 1, False, True)
        s["P"] = P
        Pctf = P
        if row.get("ctf") and not prm["ignore_ctf"]:
            pad = int(prm["padding"])
            Np, off = pad * (D - 1) + 1, (pad - 1) * (D // 2)
            big = np.zeros((Np, Np))
            big[off:off + D, off:off + D] = P
            ctf = self.ctf_image(row["ctf"], Np) * row["ctf"].get("K", 1.0)
            Pctf = np.fft.irfft2(np.fft.rfft2(big) * ctf, s=(Np, Np))[off:off + D, off:off + D]
        s["Pctf"] = Pctf
        if self.maskvol is not None:
            plane, _, marg = project_volume(self.maskvol, E, roff)
            Pmask = (plane > 0).astype(np.float64)
            s["marginal"] |= marg
        else:
            Pmask = self.circle
        if self.roi is not None:
            plane, _, marg = project_volume(self.roi, E, roff)
            M = (plane > 0).astype(np.float64)
            s["marginal"] |= marg
            iM = M if prm["subtract"] else M * (-1) + 1
        else:
            M = np.zeros((D, D))
            iM = M + 1
        s["PmaskImg"], s["M"], s["iM"] = Pmask, M, iM
        inside = Pmask > 0
        Pm = np.where(inside, Pctf, 0.0)
        Im = np.where(inside, np.asarray(img, np.float64), 0.0)
        PF, IF = np.fft.rfft2(Pm) / N, np.fft.rfft2(Im) / N
        sel = (iM > 0) & inside
        b = (Im[sel].sum() - Pctf[sel].sum()) / sel.sum()       # applyCTF wrote its result into P (L237)
        I2 = Im - b
        IiMF, PiMF = np.fft.rfft2(I2 * iM) / N, np.fft.rfft2(Pm * iM) / N
        w = self.wi[self.fit_cells]
        ir, ii, pr, pi = (a[self.fit_cells] for a in (IiMF.real, IiMF.imag, PiMF.real, PiMF.imag))
        terms = [ir * pr + ii * pi, pr * pr + pi * pi, pr + pi, ir + ii]
        sums = np.stack([np.bincount(w, t, self.maxwi + 1) for t in terms], axis=1)
        mags = np.stack([np.bincount(w, a, self.maxwi + 1) for a in (np.abs(ir * pr) + np.abs(ii * pi), terms[1], np.abs(pr) + np.abs(pi),
                                                                       np.abs(ir) + np.abs(ii))], axis=1)
        s["sums"], s["sum_magnitudes"] = sums, mags
        beta00, beta01, beta1 = self.fit(sums, self.maxwi, self.a11)
        ws = np.arange(self.maxwi + 1.0)
        a01 = float((ws * sums[:, 2]).sum())
        s["cond"] = float(np.linalg.cond(np.array([[sums[:, 1].sum(), a01], [a01, self.a11]])))
        T1 = beta01 + beta1 * self.wi
        PF0 = np.where(self.wi < self.maxwi, PF * beta00, PF)
        PF1 = PF * T1
        PF1[0, 0] = IiMF[0, 0]
        e0, e1 = IF - PF0, IF - PF1
        R2adj, model, R20adj = self.choose((IF.real + IF.imag).sum(), (IF.real ** 2 + IF.imag ** 2).sum(), (e0.real ** 2 + e0.imag ** 2).sum(),
                                           (e1.real ** 2 + e1.imag ** 2).sum(), IF.size)
        cells = 2.0 * IF.size
        varY = (IF.real ** 2 + IF.imag ** 2).sum() / cells - ((IF.real + IF.imag).sum() / cells) ** 2
        R21adj = 1.0 - (((e1.real ** 2 + e1.imag ** 2).sum() / cells) / varY) * (cells - 1.0) / (cells - 2.0)
        s["R2_gap"] = abs(R21adj - R20adj)
        if prm["boost"]:
            T = beta00 if model == 0 else T1
            Idiff = np.fft.irfft2(IF / T * N, s=(D, D))
        else:
            Idiff = I2 - np.fft.irfft2((PF0 if model == 0 else PF1) * N, s=(D, D))
        disable = bool(prm["non_negative"] and beta00 < 0)
        s.update(Idiff=Idiff, b=b, beta00=beta00, betas=(beta00, beta01, beta1), R2adj=R2adj, R20adj=R20adj, model=model,
                 beta0=beta00 if model == 0 else beta01, beta1=0.0 if model == 0 else beta1, disable=disable,
                 enabled=-1 if prm["non_negative"] and (disable or R2adj < 0) else 1)
        return s
