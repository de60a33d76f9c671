"""The FourierProjector oracle (oracle/xo_fourproj.cpp) against two references that share none of its code (tests/fp_reference.py).
The oracle restates the reference program line by line, and the device is tested for parity with it: a shared misreading (a
transposed Euler matrix, the sign of a centring phase, an off-by-one in the crop's start, the sense of rot) would pass every
parity test. These run without a device and pin the conventions themselves; tests/test_gpu_fp.py uses the same helpers on the
device at the sizes the oracle is too slow for."""
import numpy as np
import pytest

from tests import fp_reference as ref
from tests import synth

NOISE_CASES = [(40, 2, 0.45), (45, 3, 0.49), (64, 2, 0.49), (50, 1, 0.45)]
DIRECT_ANGLES = [(10, 170, 33), (123, 57, -40), (271.5, 91, 12)]
# (D, padding, max_freq, bound): twice the deviation measured when the references were written
DIRECT_CASES = [(32, 2, 0.45, 2e-4), (45, 2, 0.4, 2e-4), (32, 3, 0.45, 4e-5), (32, 1, 0.45, 4e-3)]


def ctf_image(D):
    """A multiplier of both signs on the half spectrum."""
    fy = np.fft.fftfreq(D)[:, None]
    fx = np.fft.rfftfreq(D)[None, :]
    return np.cos(30.0 * (fx * fx + fy * fy)) * np.exp(-4.0 * (fx * fx + fy * fy))


@pytest.fixture(scope="module")
def noise_case(oracle):
    made = {}

    def get(D, padding, maxf):
        if (D, padding, maxf) not in made:
            vol = np.random.default_rng(D).standard_normal((D, D, D))
            made[(D, padding, maxf)] = (oracle.FP(vol, padding, maxf, 3), ref.axis_sums(vol))
        return made[(D, padding, maxf)]
    return get


@pytest.mark.parametrize("with_ctf", [False, True])
@pytest.mark.parametrize("D,padding,maxf", NOISE_CASES)
def test_oracle_is_exact_at_axis_aligned_views(noise_case, D, padding, maxf, with_ctf):
    """White noise, integer padding, max_freq < 0.5: the oracle equals the band-limited axis sum to fp64 rounding at all eight
    views (measured 2e-14 .. 6e-14 of the image maximum, with and without a CTF image; the bound is the project's fp64 parity
    bound). White noise has no symmetry that could hide a transposed or mirrored image."""
    o, sums = noise_case(D, padding, maxf)
    ctf = ctf_image(D) if with_ctf else None
    for view in ref.EXACT_VIEWS:
        exp = ref.exact_view(sums, *view, maxf, ctf)
        got = o.project(*view, ctf=ctf)
        dev = np.abs(got - exp).max() / np.abs(exp).max()
        print(f"D={D} pad={padding} maxf={maxf} ctf={with_ctf} view={view}: {dev:.2e}")
        assert dev <= 1e-12, (view, dev)


def test_oracle_at_production_parameters_on_a_phantom(oracle):
    """max_freq = 0.5 keeps the Nyquist row, where the slice's frequency is the last node of the padded grid and the oracle's
    taps mirror at the crop boundary: a smooth volume moves by 1e-8 of the image maximum there (measured at D = 64, padding 2)."""
    D = 64
    vol = synth.phantom(D, seed=11, nblobs=9)
    o = oracle.FP(vol, 2.0, 0.5, 3)
    sums = ref.axis_sums(vol)
    for view in ref.EXACT_VIEWS:
        exp = ref.exact_view(sums, *view, 0.5)
        dev = np.abs(o.project(*view) - exp).max() / np.abs(exp).max()
        print(f"view={view}: {dev:.2e}")
        assert dev <= 1e-7, (view, dev)


def test_view_table():
    """view_from_sums derives transposes and flips from the Euler matrix; these are the conventions found by hand."""
    D = 6
    vol = np.random.default_rng(0).standard_normal((D, D, D))
    s = ref.axis_sums(vol)
    fl = ref.flip_about_origin
    table = {(0, 0, 0): s["z"], (0, 0, 90): fl(s["z"].T, 0), (0, 180, 0): fl(s["z"], 1), (180, 0, 0): fl(fl(s["z"], 0), 1),
             (0, 90, 0): fl(s["x"].T, 1), (0, -90, 0): s["x"].T, (90, 90, 0): fl(fl(s["y"].T, 0), 1), (90, 90, 90): fl(s["y"], 1)}
    assert sorted(table) == sorted(ref.EXACT_VIEWS)
    for view, exp in table.items():
        assert np.array_equal(ref.view_from_sums(s, *view), exp), view
    with pytest.raises(AssertionError):
        ref.view_from_sums(s, 10, 0, 0)


@pytest.mark.parametrize("D,padding,maxf,bound", DIRECT_CASES)
def test_oracle_follows_the_direct_fourier_sum(oracle, D, padding, maxf, bound):
    """General angles against the continuous transform of the voxels. The deviation is the interpolation error of the padded
    B-spline scheme; measured, max over the three angles, relative to the image maximum: (32, 2, 0.45) 8.2e-5, (45, 2, 0.4) 8.0e-5,
    (32, 3, 0.45) 1.6e-5, (32, 1, 0.45) 1.7e-3. The bounds are twice that; a convention error is of order 1."""
    vol = synth.phantom(D, seed=5, nblobs=9)
    o = oracle.FP(vol, padding, maxf, 3)
    for a in DIRECT_ANGLES:
        exp = ref.direct_sum(vol, *a, maxf)
        dev = np.abs(o.project(*a) - exp).max() / np.abs(exp).max()
        print(f"D={D} pad={padding} maxf={maxf} angles={a}: {dev:.2e}")
        assert dev <= bound, (a, dev)
