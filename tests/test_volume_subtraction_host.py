"""CPU checks of xmipp_volume_subtraction: properties of the numpy restatement (tests/volume_subtraction_ref.py), the bound on the
radial bins against the library's host function, and the program's option parsing and refusals, which come before any device is
touched."""
import os
import subprocess

import numpy as np
import pytest

from tests import volume_subtraction_ref as R
from tests import xmipp_io

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PROG = os.path.join(ROOT, "xmipp3_amd", "bin", "xmipp_volume_subtraction")
SHAPE = (30, 28, 24)
# Z x Y x X: where X is the largest side by enough, round(w X) over the octant reaches the number of bins
OVERFLOW = [(24, 28, 30), (25, 30, 36), (81, 80, 82)]
FIT = [(30, 28, 24), (36, 30, 25), (82, 80, 81), (32, 32, 32), (27, 27, 27), (48, 48, 48)]


@pytest.fixture(scope="module")
def xa():
    import __graft_entry__ as g
    g.build()
    assert os.path.exists(PROG)
    import xmipp3_amd
    return xmipp3_amd


@pytest.fixture(scope="module")
def case():
    v1, v, mask = R.synth(SHAPE, 5)
    return R.Reference(v1, mask), v


def _run(args):
    return subprocess.run([PROG] + args, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=120)


# ---------------------------------------------------------------- the restatement
def test_quotient_lies_in_0_1_with_nan_bins_zeroed():
    shape = (36, 30, 25)                                   # a box with empty bins: 0 / 0 in both means
    v1, v, mask = R.synth(shape, 5)
    ref = R.Reference(v1, mask)
    vmag = np.abs(R.ft(np.maximum(0.0, v * mask)))
    m1, m2 = R.radial_average(ref.v1mag, shape), R.radial_average(vmag, shape)
    empty = np.isnan(m1)
    assert empty.sum() > 0 and np.array_equal(empty, np.isnan(m2))
    q = R.rad_quotient(ref.v1mag, vmag, shape)
    assert q.shape == (R.num_bins(shape),) and not np.isnan(q).any()
    assert (q >= 0).all() and (q <= 1).all() and (q[empty] == 0).all() and (q[~empty] > 0).all()
    assert (q == 1).any() or (m1[~empty] / m2[~empty] <= 1).all()


@pytest.mark.parametrize("radavg", [False, True])
def test_output_is_non_negative_with_the_reference_deviation(case, radavg):
    ref, v = case
    out = R.adjust(ref, v, 5, 1.0, radavg, 0.0)["adjusted"]
    assert (out >= 0).all() and (out == 0).any()
    assert abs(R.stddev(out) - ref.std1) <= 1e-12 * ref.std1
    # the low pass comes last and rings: it undoes both
    filtered = R.adjust(ref, v, 5, 1.0, radavg, 0.3)["adjusted"]
    assert (filtered < 0).any()


def test_lambda_0_leaves_the_amplitudes_alone(case):
    """with --radavg the amplitude step multiplies by (1 - l) + l q, which is 1 at lambda 0: the first real-space state is the input
    again, to the rounding of a transform pair"""
    ref, v = case
    prepared = np.maximum(0.0, v * ref.mask)
    F = R.ft(prepared)
    q = R.rad_quotient(ref.v1mag, np.abs(F), SHAPE)
    rec = {}
    R.run_iteration(ref, prepared, R.extract_phase(F), 0.0, True, 0.0, q, rec, prepared)
    assert rec["amplitude"] <= 1e-14 * prepared.max()
    rec1 = {}
    R.run_iteration(ref, prepared, R.extract_phase(F), 1.0, True, 0.0, q, rec1, prepared)
    assert rec1["amplitude"] > 1e-3 * prepared.max()


def test_lambda_0_without_radavg_sets_every_amplitude_to_one(case):
    """the plain step multiplies by ((1 - l) + l V1mag) / mod (:145), which is 1 / mod at lambda 0, not 1: every coefficient above the
    threshold gets modulus 1. Kept as the reference has it"""
    ref, v = case
    prepared = np.maximum(0.0, v * ref.mask)
    F = R.ft(prepared)
    mod = np.abs(F)
    assert (mod > 1e-10).all()
    rec = {}
    R.run_iteration(ref, prepared, R.extract_phase(F), 0.0, False, 0.0, None, rec, prepared)
    unit = R.ift(F / mod, SHAPE)
    d = unit - prepared
    assert abs(rec["amplitude"] - np.sqrt((d * d).sum() / d.size)) <= 1e-12 * rec["amplitude"] and rec["amplitude"] > prepared.max()


def test_the_average_takes_the_octant_only(case):
    """the quirk: k < Z/2, i < Y/2, j < X/2 leaves out the negative frequencies of y and z, which a full shell average includes"""
    ref, _ = case
    octant = R.radial_average(ref.v1mag, SHAPE)
    full = R.full_shell_average(ref.v1mag, SHAPE)
    both = ~np.isnan(octant) & ~np.isnan(full)
    assert both.sum() >= 10
    assert np.abs(octant[both] - full[both]).max() > 1e-3 * np.abs(full[both]).max()


def test_a_single_mask_is_no_mask():
    m = np.zeros(SHAPE)
    assert R.create_mask(SHAPE, m, None).all() and R.create_mask(SHAPE, None, m).all() and not R.create_mask(SHAPE, m, m).any()


def test_refusals_of_the_restatement(case):
    ref, v = case
    for kw in ({"lam": -0.1}, {"lam": 1.5}, {"cut": 0.6}, {"cut": -0.1}, {"niter": -1}):
        with pytest.raises(ValueError):
            R.adjust(ref, v, **kw)
    with pytest.raises(ValueError, match="constant"):
        R.Reference(np.zeros(SHAPE), np.ones(SHAPE))
    with pytest.raises(ValueError, match="stddev"):
        R.adjust(ref, np.zeros(SHAPE), 1)


# ---------------------------------------------------------------- the bound on the radial bins
@pytest.mark.parametrize("shape", OVERFLOW + FIT)
def test_radial_overflow_bound(xa, shape):
    nb, mb = xa.vsub_radial_bins(shape)
    assert nb == R.num_bins(shape) and mb == R.max_bin(shape)
    assert (mb >= nb) == R.radial_overflows(shape) == (shape in OVERFLOW)
    if shape in OVERFLOW:
        with pytest.raises(ValueError):
            R.radial_average(np.zeros((shape[0], shape[1], shape[2] // 2 + 1)), shape)


# ---------------------------------------------------------------- the program
def test_help_lists_the_reference_options_and_defaults(xa):
    r = _run(["--help"])
    assert r.returncode == 0
    for t in ("--i1 <arg>", "--i2 <arg>", "[-o <=>]", "[--sub]", "[--sigma <=3>]", "[--iter <=5>]", "[--mask1 <=>]", "[--mask2 <=>]", "[--maskSub <=>]",
              "[--cutFreq <=0>]", "[--lambda <=1>]", "[--radavg]", "[--computeEnergy]", "[--saveV1 <=>]", "[--saveV2 <=>]", "[--dev <=0>]"):
        assert t in r.stderr, t


FILES = ["--i1", "/nonexistent/a.mrc", "--i2", "/nonexistent/b.mrc"]


def _shown(r):
    return dict(l.split(": ", 1) for l in r.stdout.splitlines() if ": " in l)


def test_defaults_are_the_reference_ones_and_a_missing_file_stops_before_any_device(xa):
    r = _run(FILES)
    assert r.returncode == 20 and "cannot open" in r.stderr
    s = _shown(r)
    assert s["Sigma"] == "3" and s["Iterations"] == "5" and s["Cutoff frequency"] == "0" and s["Relaxation factor"] == "1"
    assert s["Match radial averages"] == "0" and s["Subtraction"] == "0" and s["Output"] == "output_volume.mrc"
    assert s["Save volume 1 filtered"] == "volume1_filtered.mrc" and s["Save volume 2 adjusted"] == "volume2_adjusted.mrc"
    r = _run(FILES + ["--sub", "--radavg", "--iter", "2", "--sigma", "4", "--cutFreq", "0.25", "--lambda", "0.5", "-o", "x.mrc", "--saveV1", "a.mrc", "--saveV2", "b.mrc"])
    s = _shown(r)
    assert s["Sigma"] == "4" and s["Iterations"] == "2" and s["Cutoff frequency"] == "0.25" and s["Relaxation factor"] == "0.5"
    assert s["Match radial averages"] == "1" and s["Subtraction"] == "1" and s["Output"] == "x.mrc"
    assert s["Save volume 1 filtered"] == "a.mrc" and s["Save volume 2 adjusted"] == "b.mrc"


def test_the_input_volumes_are_mandatory(xa):
    assert _run(["--i1", "/nonexistent/a.mrc"]).returncode != 0
    assert _run(["--i2", "/nonexistent/b.mrc"]).returncode != 0


def test_bad_device_is_refused(xa):
    r = _run(FILES + ["--dev", "x"])
    assert r.returncode != 0 and "Invalid GPU device" in r.stderr


@pytest.mark.parametrize("extra,text", [(["--lambda", "1.5"], "outside [0, 1]"), (["--lambda", "-0.1"], "outside [0, 1]"), (["--cutFreq", "0.6"], "outside [0, 0.5]"),
                                        (["--cutFreq", "-0.1"], "outside [0, 0.5]"), (["--iter", "-1"], "negative number of iterations"),
                                        (["--sigma", "-2"], "negative sigma")])
def test_refused_options(xa, extra, text):
    r = _run(FILES + extra)
    assert r.returncode != 0 and text in r.stderr and "cannot open" not in r.stderr


def _write(tmp_path, name, shape):
    fn = str(tmp_path / name)
    xmipp_io.write_volume(fn, np.zeros(shape, np.float32))
    return fn


@pytest.mark.parametrize("which", ["--i2", "--mask1", "--mask2", "--maskSub"])
def test_different_shapes_are_refused_before_any_device(xa, tmp_path, which):
    a, b = _write(tmp_path, "a.vol", (8, 8, 8)), _write(tmp_path, "b.vol", (8, 8, 8))
    odd = _write(tmp_path, "odd.vol", (8, 8, 6))
    args = {"--i1": a, "--i2": b, "--mask1": a, "--mask2": a, "--maskSub": a}
    args[which] = odd
    cmd = [x for kv in args.items() for x in kv] + ["--sub", "-o", str(tmp_path / "o.mrc")]
    r = _run(cmd)
    assert r.returncode != 0 and "different dimensions" in r.stderr
    assert not (tmp_path / "o.mrc").exists()


@pytest.mark.parametrize("shape", OVERFLOW[:2])
def test_radavg_on_an_overflowing_box_is_refused_before_any_device(xa, tmp_path, shape):
    a = _write(tmp_path, "a.vol", shape)
    r = _run(["--i1", a, "--i2", a, "--radavg", "-o", str(tmp_path / "o.mrc")])
    assert r.returncode != 0 and "largest bin" in r.stderr
    assert not (tmp_path / "o.mrc").exists()
