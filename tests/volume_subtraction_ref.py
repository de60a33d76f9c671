"""A numpy fp64 restatement of xmipp_volume_subtraction: reconstruction/volume_subtraction.cpp (ProgVolumeSubtraction), written from its
text. Volumes are [Z, Y, X] float64, spectra [Z, Y, X // 2 + 1]. np.fft.rfftn / irfftn have FFTW's r2c / c2r semantics; xmippCore's
forward transform divides by N and its inverse does not, which is rfftn / N and irfftn * N (parity unpinned).

The places where the reference writes past an array or divides by zero are refused with ValueError, as the device code refuses them
(the list is at the head of xmipp3_amd/csrc/xh_vsub.hip).
"""
import math

import numpy as np

PI = math.pi
AXES = (0, 1, 2)
RAISED_W = 0.02
ENERGIES = ("amplitude", "minmax", "mask", "phase", "nonneg", "scale", "filter")


def ft(v):
    """FourierTransformer::FourierTransform: the forward transform carries the 1 / N"""
    return np.fft.rfftn(v, axes=AXES) / v.size


def ift(F, shape):
    """inverseFourierTransform: un-normalised"""
    return np.fft.irfftn(F, s=shape, axes=AXES) * (shape[0] * shape[1] * shape[2])


def _fast_freq(n, size):
    """FFT_IDX2DIGFREQ_FAST over the first n indices: the index (minus the size above size / 2) times 1 / size"""
    isize = 1.0 / size
    idx = np.arange(n)
    return np.where(idx <= size // 2, idx, idx - size) * isize


def _w_fast(shape, nz, ny, nx):
    """sqrt(wx wx + (wy wy + wz wz)) of :163-171 and :241-249 over the first (nz, ny, nx) indices"""
    Z, Y, X = shape
    wz, wy, wx = _fast_freq(nz, Z), _fast_freq(ny, Y), _fast_freq(nx, X)
    wz2 = (wz * wz)[:, None, None]
    wy2_wz2 = (wy * wy)[None, :, None] + wz2
    return np.sqrt((wx * wx)[None, None, :] + wy2_wz2)


def _digfreq(n, size):
    """FFT_IDX2DIGFREQ: a division"""
    idx = np.arange(n)
    return np.where(idx <= size // 2, idx, idx - size) / float(size)


def _absw(shape):
    """the frequency of FourierFilter::maskValue over the half spectrum"""
    Z, Y, X = shape
    wz, wy, wx = _digfreq(Z, Z), _digfreq(Y, Y), _digfreq(X // 2 + 1, X)
    return np.sqrt((wx * wx)[None, None, :] + (wy * wy)[None, :, None] + (wz * wz)[:, None, None])


def num_bins(shape):
    """:235"""
    Z, Y, X = shape
    return int(math.floor(math.sqrt((X // 2) ** 2 + (Y // 2) ** 2 + (Z // 2) ** 2)))


def octant_bins(shape):
    """round(w X) of :250 over the octant k < Z/2, i < Y/2, j < X/2 (C's round: halves away from zero; w >= 0)"""
    Z, Y, X = shape
    return np.floor(_w_fast(shape, Z // 2, Y // 2, X // 2) * X + 0.5).astype(np.int64)


def max_bin(shape):
    return int(octant_bins(shape).max())


def radial_overflows(shape):
    """whether radialAverage writes past radial_mean on this box"""
    return max_bin(shape) >= num_bins(shape)


def radial_average(mag, shape):
    """radialAverage :223-257: the octant only; an empty bin gives 0 / 0 = NaN"""
    if radial_overflows(shape):
        raise ValueError("the radial average's largest bin reaches the number of bins")
    Z, Y, X = shape
    nb = num_bins(shape)
    b = octant_bins(shape).ravel()
    v = mag[:Z // 2, :Y // 2, :X // 2].ravel()
    s = np.bincount(b, weights=v, minlength=nb)
    c = np.bincount(b, minlength=nb).astype(np.float64)
    with np.errstate(invalid="ignore", divide="ignore"):
        return s / c


def full_shell_average(mag, shape):
    """not the reference: the same bins over every coefficient of the half spectrum, to show what the octant leaves out"""
    Z, Y, X = shape
    nb = num_bins(shape)
    b = np.minimum(np.floor(_w_fast(shape, Z, Y, X // 2 + 1) * X + 0.5).astype(np.int64), nb - 1).ravel()
    s = np.bincount(b, weights=mag.ravel(), minlength=nb)
    c = np.bincount(b, minlength=nb).astype(np.float64)
    with np.errstate(invalid="ignore", divide="ignore"):
        return s / c


def rad_quotient(v1mag, vmag, shape):
    """computeRadQuotient :259-275: min(q, 1), then NaN -> 0"""
    with np.errstate(invalid="ignore", divide="ignore"):
        q = radial_average(v1mag, shape) / radial_average(vmag, shape)
    q = np.where(q > 1.0, 1.0, q)          # std::min(q, 1.0) keeps a NaN
    q[np.isnan(q)] = 0.0
    return q


def extract_phase(F):
    """:197-203"""
    phi = np.arctan2(F.imag, F.real)
    return np.cos(phi) + 1j * np.sin(phi)


def stddev(v):
    """computeStddev, the estimator the device uses for both volumes; std1 / std2 does not depend on N against N - 1"""
    N = v.size
    avg = v.sum() / N
    return math.sqrt(abs((v * v).sum() / N - avg * avg) * N / (N - 1)) if N > 1 else 0.0


def lowpass_raised_cosine(v, cut):
    """FourierFilter LOWPASS RAISED_COSINE, w1 = cut, raised_w = 0.02 (:277-282, fourier_filter.cpp:426-432)"""
    w = _absw(v.shape)
    m = np.where(w < cut, 1.0, np.where(w < cut + RAISED_W, (1 + np.cos(PI / RAISED_W * (w - cut))) / 2, 0.0))
    return ift(ft(v) * m, v.shape)


def smooth_mask(mask, sigma):
    """filterMask :332-338: REALGAUSSIAN, exp(-PI^2 w^2 sigma^2) (fourier_filter.cpp:437-438)"""
    w = _absw(mask.shape)
    return ift(ft(mask) * np.exp(-PI * PI * w * w * sigma * sigma), mask.shape)


def create_mask(shape, mask1, mask2):
    """createMask :317-330: the product when both are given, else ones"""
    if mask1 is not None and mask2 is not None:
        return mask1 * mask2
    return np.ones(shape)


class Reference:
    """what run derives from V1 (:424-427, :432, :435)"""

    def __init__(self, v1, mask):
        self.shape = v1.shape
        self.mask = mask
        self.v1 = np.maximum(0.0, v1 * mask)
        self.v1min, self.v1max = float(self.v1.min()), float(self.v1.max())
        self.std1 = stddev(self.v1)
        if not self.std1 > 0:
            raise ValueError("the masked, clipped reference is constant")
        self.v1mag = np.abs(ft(self.v1))


def _energy(vdiff, v):
    """computeEnergy :205-211"""
    d = vdiff - v
    return math.sqrt((d * d).sum() / d.size)


def run_iteration(ref, v, phase, lam, radavg, cut, quotient=None, rec=None, vdiff=None, near=None):
    """runIteration :362-418. rec: a dict that receives the energies, vdiff the volume of the step before (returned updated). near: a
    list that receives the number of coefficients whose modulus lies in [0.5e-10, 2e-10] at the amplitude step"""
    shape = ref.shape
    F = ft(v)
    if radavg:
        Z, Y, X = shape
        iw = np.minimum(np.floor(_w_fast(shape, Z, Y, X // 2 + 1) * X).astype(np.int64), quotient.size - 1)
        F = F * ((1 - lam) + lam * quotient[iw])
    else:
        mod = np.abs(F)
        if near is not None:
            near.append(int(((mod >= 0.5e-10) & (mod <= 2e-10)).sum()))
        big = mod > 1e-10
        with np.errstate(invalid="ignore", divide="ignore"):
            F = np.where(big, F * (((1 - lam) + lam * ref.v1mag) / mod), F)
    steps = []
    v = ift(F, shape)
    steps.append(v)
    v = np.where(v < ref.v1min, ref.v1min, np.where(v > ref.v1max, ref.v1max, v))
    steps.append(v)
    v = v * ref.mask
    steps.append(v)
    v = ift(np.abs(ft(v)) * phase, shape)
    steps.append(v)
    v = np.maximum(0.0, v)
    steps.append(v)
    std2 = stddev(v)
    if not std2 > 0:
        raise ValueError("stddev(V) == 0 after the phase step")
    v = v * (ref.std1 / std2)
    steps.append(v)
    if cut != 0:
        v = lowpass_raised_cosine(v, cut)
        steps.append(v)
    if rec is not None:
        for name, s in zip(ENERGIES, steps):
            rec[name] = _energy(vdiff, s)
            vdiff = s
        if cut == 0:
            rec["filter"] = 0.0
    return v, vdiff


def adjust(ref, v, niter=5, lam=1.0, radavg=False, cut=0.0, perturb=None):
    """run :428-442. Returns a dict: adjusted, energies (one dict per iteration), near (see run_iteration), quotient, prepared (the
    masked, clipped input). perturb: an array added to the prepared input, for the amplification measurement"""
    if not 0 <= lam <= 1:
        raise ValueError("lambda outside [0, 1]")
    if not 0 <= cut <= 0.5:
        raise ValueError("cutFreq outside [0, 0.5]")
    if niter < 0:
        raise ValueError("a negative number of iterations")
    v = np.maximum(0.0, v * ref.mask)
    if perturb is not None:
        v = v + perturb
    out = {"prepared": v, "energies": [], "near": [], "quotient": None, "states": [v]}
    Fv = ft(v)
    phase = extract_phase(Fv)
    if radavg:
        out["quotient"] = rad_quotient(ref.v1mag, np.abs(Fv), ref.shape)
    vdiff = v
    for _ in range(niter):
        rec = {}
        v, vdiff = run_iteration(ref, v, phase, lam, radavg, cut, out["quotient"], rec, vdiff, out["near"])
        out["energies"].append(rec)
        out["states"].append(v)
    out["adjusted"] = v
    return out


def subtraction(v1_raw, vadj, masksub, cut):
    """subtraction :284-306: (the difference, V1 filtered)"""
    v1f = lowpass_raised_cosine(v1_raw, cut) if cut != 0 else v1_raw
    out = v1_raw * (1 - masksub) + (v1f - np.minimum(vadj, v1f)) * masksub
    return out, v1f


def synth(shape, seed):
    """(V1, V, mask) as a float file stores them: two overlapping Gaussian blobs of different weight plus noise for V1, a scaled single
    blob plus noise for V, an ellipsoidal binary mask"""
    Z, Y, X = shape
    rng = np.random.default_rng(seed)
    z, y, x = np.meshgrid(np.arange(Z) - Z / 2.0, np.arange(Y) - Y / 2.0, np.arange(X) - X / 2.0, indexing="ij")

    def blob(cz, cy, cx, s):
        return np.exp(-(((z - cz * Z) / (s * Z)) ** 2 + ((y - cy * Y) / (s * Y)) ** 2 + ((x - cx * X) / (s * X)) ** 2))

    v1 = 1.0 * blob(0.02, -0.03, 0.05, 0.16) + 0.6 * blob(-0.12, 0.1, -0.08, 0.10) + 0.05 * rng.standard_normal(shape)
    v = 2.5 * blob(0.02, -0.03, 0.05, 0.16) + 0.12 * rng.standard_normal(shape) + 0.05
    mask = ((z / (0.42 * Z)) ** 2 + (y / (0.40 * Y)) ** 2 + (x / (0.38 * X)) ** 2 <= 1.0).astype(np.float64)
    return tuple(a.astype(np.float32).astype(np.float64) for a in (v1, v, mask))
