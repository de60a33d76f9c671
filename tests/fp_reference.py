"""Two references for the FourierProjector that share no code with it: plain numpy, float64 throughout, neither the oracle nor
the library. `vol` is [z][y][x] with the Xmipp origin at D // 2; an image is [y][x] with the same origin.

A (exact_view): at a view whose Euler matrix has only 0 / +-1 entries every frequency of the slice is a node of the padded grid
   (integer padding), where cubic B-spline interpolation of spline coefficients returns the sample. The projection is then the
   band-limited sum of the volume along one axis, whatever the padding. Exact below the Nyquist row (max_freq < 0.5).
B (direct_sum): the continuous Fourier transform of the voxels evaluated at the slice's frequencies, at any angle. The projector
   approximates it by padding and interpolating; the two differ by that method's own error."""
import numpy as np

from tests import synth

# (rot, tilt, psi) whose Euler matrices are signed permutations; between them they sum over each of the three axes and take
# every combination of transposing and flipping
EXACT_VIEWS = [(0, 0, 0), (0, 0, 90), (0, 180, 0), (180, 0, 0), (0, 90, 0), (0, -90, 0), (90, 90, 0), (90, 90, 90)]


def band_mask(D, max_freq):
    """The frequencies of the D x (D // 2 + 1) half spectrum that a projection keeps."""
    fy = np.fft.fftfreq(D)[:, None]
    fx = np.fft.rfftfreq(D)[None, :]
    return (fy * fy + fx * fx) <= max_freq * max_freq


def flip_about_origin(a, axis):
    """index i -> 2 (D // 2) - i, periodically: the sample at -r about the Xmipp origin."""
    a = np.flip(a, axis)
    return np.roll(a, 1, axis) if a.shape[axis] % 2 == 0 else a


def axis_sums(vol):
    """The three sums exact_view picks from: over z [y][x], over y [z][x], over x [z][y]."""
    v = np.asarray(vol, np.float64)
    return {"z": v.sum(0), "y": v.sum(1), "x": v.sum(2)}


def view_from_sums(sums, rot, tilt, psi):
    """The unfiltered projection [y'][x'] at an axis-aligned view from axis_sums(vol). The image axis x' runs along row 0 of the
    Euler matrix and y' along row 1 (signed volume axes X, Y or Z), the sum runs over the axis that is left."""
    E = synth.euler_matrix(rot, tilt, psi)
    R = np.rint(E)
    assert np.abs(E - R).max() < 1e-12 and (np.abs(R).sum(1) == 1).all(), "not an axis-aligned view"
    ax, ay = int(np.argmax(np.abs(R[0]))), int(np.argmax(np.abs(R[1])))        # 0 = X, 1 = Y, 2 = Z
    S = sums["xyz"[3 - ax - ay]]               # the array's axes: what is left of (Z, Y, X), in that order
    if ay < ax:                                # y' has to be axis 0: it is when its volume axis comes first in (Z, Y, X)
        S = S.T
    if R[1, ay] < 0:
        S = flip_about_origin(S, 0)
    if R[0, ax] < 0:
        S = flip_about_origin(S, 1)
    return S


def band_limit(S, max_freq, ctf=None):
    D = S.shape[0]
    F = np.fft.rfft2(S) * band_mask(D, max_freq)
    if ctf is not None:
        F = F * np.asarray(ctf, np.float64)
    return np.fft.irfft2(F, s=(D, D))


def exact_view(sums, rot, tilt, psi, max_freq, ctf=None):
    """Reference A from axis_sums(vol); ctf: optional [D][D // 2 + 1] multiplier."""
    return band_limit(view_from_sums(sums, rot, tilt, psi), max_freq, ctf)


def direct_sum(vol, rot, tilt, psi, max_freq):
    """Reference B: V(f) = sum vol[z, y, x] exp(-2 pi i (fX (x - c) + fY (y - c) + fZ (z - c))), c = D // 2, at
    f = freqx E[0] + freqy E[1] (freqy[D / 2] = +0.5 for even D), moved to the image's origin and inverted."""
    v = np.asarray(vol, np.float64)
    D = v.shape[0]
    c = D // 2
    xh = D // 2 + 1
    E = synth.euler_matrix(rot, tilt, psi)
    fy = np.fft.fftfreq(D)
    if D % 2 == 0:
        fy[D // 2] = 0.5
    fx = np.arange(xh) / D
    keep = (fy[:, None] ** 2 + fx[None, :] ** 2) <= max_freq * max_freq
    ii, jj = np.nonzero(keep)
    f = fx[jj, None] * E[0][None, :] + fy[ii, None] * E[1][None, :]            # [npix, (X, Y, Z)]
    r = np.arange(D) - c
    ex, ey, ez = (np.exp(-2j * np.pi * f[:, a, None] * r[None, :]) for a in range(3))
    V = np.empty(len(ii), np.complex128)
    for p0 in range(0, len(ii), 256):                                          # [256, D, D] complex at a time
        s = slice(p0, p0 + 256)
        t = np.tensordot(ex[s], v, axes=(1, 2))                                # [p, z, y]
        t = np.einsum("pzy,py->pz", t, ey[s])
        V[s] = np.einsum("pz,pz->p", t, ez[s])
    F = np.zeros((D, xh), np.complex128)
    F[ii, jj] = V * np.exp(-2j * np.pi * (ii + jj) * c / D)
    return np.fft.irfft2(F, s=(D, D))
