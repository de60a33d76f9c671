"""CPU checks of xmipp_volume_halves_restoration: the reference program's refusals and messages come before any device is touched;
the host Powell minimiser (xh_powell_minimize) against scipy's; the program's two mask types against numpy."""
import math
import os
import subprocess

import numpy as np
import pytest

from tests import xmipp_io

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PROG = os.path.join(ROOT, "xmipp3_amd", "bin", "xmipp_volume_halves_restoration")


@pytest.fixture(scope="module")
def xa():
    import __graft_entry__ as g
    g.build()
    assert os.path.exists(PROG)
    import xmipp3_amd
    return xmipp3_amd


def _run(args):
    return subprocess.run([PROG] + args, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=120)


def test_help_lists_the_reference_flags(xa):
    r = _run(["--help"])
    assert r.returncode == 0 and "USAGE" in r.stderr
    for flag in ("--i1", "--i2", "--oroot", "--denoising", "--deconvolution", "--filterBank", "--difference", "--mask", "--center"):
        assert flag in r.stderr
    for defaults in ("--oroot <=volumeRestored>", "--denoising <=0>", "--deconvolution <=0> <=0.2> <=0.001>", "--filterBank <=0> <=0.5> <=1> <=3>",
                     "--difference <=0> <=1.5>"):
        assert defaults in r.stderr
    assert "--dev" not in r.stderr and "--device" not in r.stderr


@pytest.mark.parametrize("args,code,msg", [
    ([], 3, "Parameter --i1 is mandatory"),
    (["--denoising", "-1"], 1, "`denoising N` has to be non-negative integer"),
    (["--deconvolution", "-2"], 1, "`deconvolution N` has to be non-negative integer"),
    (["--filterBank", "0.6"], 1, "`filterBank step` parameter has to be in interval [0, 0.5]."),
    (["--filterBank", "-0.1"], 1, "`filterBank step` parameter has to be in interval [0, 0.5]."),
    (["--filterBank", "0.01", "1.5"], 1, "`filterBank overlap` parameter has to be in interval [0, 1]"),
    (["--filterBank", "0.01", "0.5", "4"], 1, "`filterBank weightFun` parameter has to be 0, 1 or 2"),
    (["--filterBank", "0.01", "0.5", "-1"], 1, "`filterBank weightFun` parameter has to be 0, 1 or 2"),
    (["--difference", "-1"], 1, "`difference N` has to be non-negative integer"),
    (["--mask", "cylinder", "3"], 61, "--mask cylinder: only the binary_file and circular mask types are supported"),
    (["--mask", "real_file", "m.vol"], 61, "--mask real_file: only the binary_file and circular mask types are supported"),
    (["--mask", "circular", "0"], 2, "MaskProgram: circular mask with radius 0"),
])
def test_refusals(xa, args, code, msg):
    base = [] if args == [] else ["--i1", "a.vol", "--i2", "b.vol"]
    r = _run(base + args)
    assert r.returncode == code, r.stderr
    assert msg in r.stderr


def test_weight_fun_3_is_accepted(xa, tmp_path):
    """the reference's check admits 3 although its message names 0, 1 or 2: the arguments pass, the missing file is what stops it"""
    r = _run(["--i1", str(tmp_path / "none.vol"), "--i2", "b.vol", "--filterBank", "0.01", "0.5", "3", "3"])
    assert r.returncode == 20 and "cannot open" in r.stderr


def test_size_refusals(xa, tmp_path):
    xmipp_io.write_volume(str(tmp_path / "a.vol"), np.zeros((8, 8, 8), np.float32))
    xmipp_io.write_volume(str(tmp_path / "b.vol"), np.zeros((8, 8, 6), np.float32))
    xmipp_io.write_volume(str(tmp_path / "m.vol"), np.ones((8, 6, 8), np.float32))
    r = _run(["--i1", str(tmp_path / "a.vol"), "--i2", str(tmp_path / "b.vol")])
    assert r.returncode == 41 and "Input volumes have different dimensions" in r.stderr
    r = _run(["--i1", str(tmp_path / "a.vol"), "--i2", str(tmp_path / "a.vol"), "--mask", "binary_file", str(tmp_path / "m.vol")])
    assert r.returncode == 41 and "Mask and input volumes have different dimensions" in r.stderr


# ---------------------------------------------------------------- Powell
def _rosenbrock(x):
    return (1 - x[0]) ** 2 + 100 * (x[1] - x[0] ** 2) ** 2


def _quadratic(x):
    return 1.0 + (x[0] - 0.3) ** 2 + 2 * (x[1] + 1.1) ** 2 + 0.5 * (x[0] - 0.3) * (x[1] + 1.1) + 0.7 * (x[2] - 2.0) ** 2


def _barrier(x):
    """the shape of restorationSigmaCost: 1e38 outside [0, 2]^2"""
    if x[0] < 0 or x[1] < 0 or x[0] > 2 or x[1] > 2:
        return 1e38
    return 0.5 + (x[0] - 0.7) ** 2 + 2 * (x[1] - 1.3) ** 2 + 0.3 * (x[0] - 0.7) * (x[1] - 1.3)


def _barrier_edge(x):
    """a barrier whose minimum lies on the edge of the box"""
    if x[0] < 0 or x[1] < 0 or x[0] > 2 or x[1] > 2:
        return 1e38
    return 2.0 + (x[0] - 2.5) ** 2 + (x[1] - 0.4) ** 2


@pytest.mark.parametrize("f,p0,ftol", [(_rosenbrock, [-1.2, 1.0], 1e-10), (_quadratic, [0.0, 0.0, 0.0], 0.01), (_quadratic, [5.0, -4.0, 1.0], 0.01),
                                        (_barrier, [0.2, 0.2], 0.01), (_barrier, [1.9, 0.1], 0.01), (_barrier_edge, [0.2, 0.2], 0.01)])
def test_powell_against_scipy(xa, f, p0, ftol):
    from scipy.optimize import minimize
    n = len(p0)
    p, fmin, it = xa.powell_minimize(f, p0, np.ones(n), ftol)
    r = minimize(f, np.array(p0, float), method="Powell", options={"ftol": ftol, "xtol": 1e-12, "direc": np.eye(n)})
    assert it >= 1 and math.isclose(fmin, f(p), rel_tol=1e-15)
    if f is _rosenbrock:
        assert np.allclose(p, [1.0, 1.0], atol=1e-3) and np.allclose(r.x, [1.0, 1.0], atol=1e-3)
        assert fmin <= 1e-8 and r.fun <= 1e-8
    else:
        assert abs(fmin - r.fun) <= ftol * (abs(fmin) + abs(r.fun)), (p, fmin, r.x, r.fun)
    if f in (_barrier, _barrier_edge):
        assert np.all((p >= 0) & (p <= 2))


def test_powell_reads_variables_one_based(xa):
    """the cost sees x[1] .. x[n], as xmippCore passes them (restorationSigmaCost reads x[1], x[2])"""
    import ctypes as C
    from xmipp3_amd._lib import COST_FN, lib
    seen = []

    def cb(x, _user):
        seen.append((x[1], x[2]))
        return (x[1] - 0.25) ** 2 + (x[2] - 0.75) ** 2
    p = np.array([1.0, 1.0])
    fret, it = C.c_double(), C.c_int32()
    steps = np.ones(2)
    assert lib().xh_powell_minimize(2, p.ctypes.data_as(C.c_void_p), steps.ctypes.data_as(C.c_void_p), 0.01, COST_FN(cb), None,
                                    C.byref(fret), C.byref(it)) == 0
    assert seen[0] == (1.0, 1.0)
    assert np.allclose(p, [0.25, 0.75], atol=1e-3)


# ---------------------------------------------------------------- masks
@pytest.mark.parametrize("shape", [(16, 16, 16), (15, 20, 17)])
@pytest.mark.parametrize("R,center", [(-5.0, (0, 0, 0)), (4.5, (0, 0, 0)), (-3.0, (1.5, -2.0, 0.5))])
def test_circular_mask(xa, shape, R, center):
    Z, Y, X = shape
    k, i, j = np.meshgrid(np.arange(Z) - Z // 2, np.arange(Y) - Y // 2, np.arange(X) - X // 2, indexing="ij")
    r2 = (k - center[2]) ** 2.0 + (i - center[1]) ** 2.0 + (j - center[0]) ** 2.0
    exp = (r2 <= R * R) if R < 0 else (r2 >= R * R)
    got = xa.halves_circular_mask(shape, R, center)
    assert got.dtype == np.int32 and np.array_equal(got, exp.astype(np.int32))


def test_binary_mask(xa):
    v = np.array([0.0, 0.4, 0.99, 1.0, 2.5, -0.7, -1.0, 3.0], np.float32)
    assert np.array_equal(xa.halves_binary_mask(v), (v.astype(np.int32) != 0).astype(np.int32))
    assert np.array_equal(xa.halves_binary_mask(v), [0, 0, 0, 1, 1, 0, 1, 1])
