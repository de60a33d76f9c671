"""CPU checks of the xmipp_volume_find_symmetry program: its usage lines, every refusal arriving before a device is opened with a message
that names the option, the trial grids (xh_fsym_grid) against the reference's loops, and the cylinder and tube masks against the
restatement. None needs a device: a refusal that came after opening one would fail here with the library's error instead."""
import os
import subprocess

import numpy as np
import pytest

import xmipp3_amd as xa
from tests import find_symmetry_ref as R
from tests import xmipp_io

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PROG = os.path.join(ROOT, "xmipp3_amd", "bin", "xmipp_volume_find_symmetry")
ERR_ARG_INCORRECT, ERR_ARG_MISSING, ERR_MATRIX_DIM, ERR_VALUE_INCORRECT, ERR_GPU, ERR_NOT_IMPLEMENTED = 2, 3, 41, 50, 60, 61


def run(*args):
    return subprocess.run([PROG] + [str(a) for a in args], capture_output=True, text=True)


@pytest.fixture(scope="module")
def files(tmp_path_factory):
    d = tmp_path_factory.mktemp("fsym")
    xmipp_io.write_volume(d / "volume.vol", R.helix_phantom((12, 12, 12)))
    xmipp_io.write_volume(d / "other.vol", R.helix_phantom((12, 10, 12)))
    xmipp_io.write_volume(d / "empty.vol", np.zeros((12, 12, 12)))
    xmipp_io.write_volume(d / "flat.vol", np.zeros((1, 12, 12)))
    top = np.zeros((12, 12, 12))
    top[11] = 1                                            # the plane k = 5 alone: outside [zFirst, zLast] of --heightFraction 0.5
    xmipp_io.write_volume(d / "top.vol", top)
    return d


def test_usage_lines():
    r = run("--help")
    assert r.returncode == 0
    for line in ("Find a symmetry rotational axis.",
                 "Symmetry axis (rot,tilt)= 10 20 -->    0.33682   0.059391    0.93969",
                 "It is important that the volume is correctly centered.",
                 "-i <arg> : Volume to process",
                 "[-o <=>] : Metadata with the orientation of the symmetry axis In helical mode, there is a file called output.xmp",
                 "[--thr <=1>] : Number of threads",
                 "--sym <arg> <=0> : Symmetry mode",
                 "rot <n> (Order of the rotational axis), helical (Helical symmetry.), helicalDihedral (Helical-Dihedral symmetry.)",
                 "[--sym2 <=C1>] : Additional Cn symmetry. Only for helical and helicalDihedral",
                 "[--rot <=0> <=355> <=5>] : Limits for rotational angle search",
                 "[--tilt <=0> <=90> <=5>] : Limits for tilt angle search",
                 "[--localRot <arg> <arg>] : Perform a local search around this angle",
                 "[--useSplines] : Use cubic B-Splines for the interpolations",
                 "[-z <=1> <=10> <=0.5>] : Search space for the shift in Z (in Angstroms)",
                 "[--sampling <=1>] : Sampling rate in A/pix",
                 "[--rotHelical <=-357> <=357> <=3>] : Search space for rotation around Z",
                 "[--localHelical <arg> <arg>] : Perform a local search around this angle and shift",
                 "[--heightFraction <=1>] : Use this fraction of the volume",
                 "Restrict the comparison to the mask area.",
                 "[--device <=0>] : HIP device (one device only)",
                 "xmipp_volume_find_symmetry -i volume.vol --sym rot 3",
                 "xmipp_volume_find_symmetry -i volume --sym helical -z 0 6 1 --mask circular -32 --thr 2 -o parameters.xmd"):
        assert line in r.stderr, line


@pytest.mark.parametrize("inp,args,code,words", [
    ("volume.vol", ("--sym", "rot", 3, "--mask", "gaussian", 3), ERR_NOT_IMPLEMENTED, "--mask gaussian: only the binary_file, circular, cylinder and tube mask types"),
    ("volume.vol", ("--sym", "rot", 3, "--mask", "binary_file", "{d}/other.vol"), ERR_MATRIX_DIM, "other.vol is 12 x 10 x 12, the volume 12 x 12 x 12"),
    ("volume.vol", ("--sym", "rot", 3, "--mask", "binary_file", "{d}/empty.vol"), ERR_VALUE_INCORRECT, "--mask selects no voxel"),
    ("volume.vol", ("--sym", "rot", 3, "--mask", "circular", 30), ERR_VALUE_INCORRECT, "--mask selects no voxel"),
    ("volume.vol", ("--sym", "helical", "--heightFraction", 0.5, "--mask", "binary_file", "{d}/top.vol"), ERR_VALUE_INCORRECT,
     "--mask selects no voxel within --heightFraction"),
    ("volume.vol", ("--sym", "rot", 3, "--mask", "cylinder", -3, 4), ERR_ARG_INCORRECT, "cannot determine mode for cylinder (--mask cylinder <R> <H>)"),
    ("volume.vol", ("--sym", "rot", 3, "--mask", "tube", -3, -4), ERR_ARG_INCORRECT, "cannot determine mode for tube (--mask tube <R1> <R2> <H>)"),
    ("flat.vol", ("--sym", "rot", 3), ERR_MATRIX_DIM, "is an image (12 x 12 x 1): this program needs a volume"),
    ("volume.vol", ("--sym", "rot", 1), ERR_ARG_INCORRECT, "--sym rot 1: the order of the axis must be 2 .. 99"),
    ("volume.vol", ("--sym", "rot"), ERR_ARG_INCORRECT, "--sym rot 0: the order of the axis must be 2 .. 99"),
    ("volume.vol", ("--sym", "screw"), ERR_ARG_INCORRECT, "--sym screw: the modes are rot <n>, helical and helicalDihedral"),
    ("volume.vol", ("--sym", "rot", 3, "--rot", 0, "nan", 5), ERR_ARG_INCORRECT, "--rot: a value is not finite"),
    ("volume.vol", ("--sym", "rot", 3, "--tilt", 0, "inf", 5), ERR_ARG_INCORRECT, "--tilt: a value is not finite"),
    ("volume.vol", ("--sym", "helical", "-z", 1, "inf", 1), ERR_ARG_INCORRECT, "-z: a value is not finite"),
    ("volume.vol", ("--sym", "rot", 3, "--rot", 0, 355, 0.01, "--tilt", 0, 90, 0.01), ERR_ARG_INCORRECT, "at most 2097152 trials"),
    ("volume.vol", ("--sym", "rot", 3, "--rot", 0, 355, 0), ERR_ARG_INCORRECT, "never ends"),
    ("volume.vol", ("--sym", "helical", "--rotHelical", -357, 357, -3), ERR_ARG_INCORRECT, "never ends"),
    ("volume.vol", ("--sym", "rot", 3, "--rot", 10, 5, 1), ERR_ARG_INCORRECT, "(--rot and --tilt) hold no trial"),
    ("volume.vol", ("--sym", "rot", 3, "--device", "0,1"), ERR_ARG_INCORRECT, "--device 0,1: this program runs on one device"),
    ("volume.vol", ("--sym", "helical", "-z", 0, 6, 1), ERR_ARG_INCORRECT, "-z: a rise of 0 (0 voxels) is not supported: the rise must be above 0"),
    ("volume.vol", ("--sym", "helicalDihedral", "-z", 1, 6, 1, "--sampling", 2), ERR_ARG_INCORRECT, "at least 1 voxel for helicalDihedral"),
    ("volume.vol", ("--sym", "helical", "--sym2", "D3"), ERR_ARG_INCORRECT, "--sym2 D3: C<n> with n in 1 .. 99"),
    ("volume.vol", ("--sym", "helical", "--sym2", "C0"), ERR_ARG_INCORRECT, "--sym2 C0: C<n> with n in 1 .. 99"),
    ("volume.vol", ("--sym", "helical", "--heightFraction", 1.2), ERR_ARG_INCORRECT, "--heightFraction 1.2: the fraction must be in (0, 1]"),
    ("volume.vol", ("--sym", "helical", "--sampling", 0), ERR_ARG_INCORRECT, "--sampling 0: the sampling rate must be above 0"),
])
def test_refusals_come_before_any_device(files, inp, args, code, words):
    r = run("-i", files / inp, *[str(a).format(d=files) for a in args])
    assert r.returncode == code and words in r.stderr and r.stderr.startswith(f"XMIPP_ERROR {code}:"), r.stderr
    assert r.stdout == ""


def test_sides_above_1024_are_refused_from_the_header(tmp_path):
    hdr = xmipp_io._spider_header(1025, 2, 2, 3, 0, 0, 0)
    with open(tmp_path / "wide.vol", "wb") as f:
        f.write(hdr.tobytes())
        f.write(np.zeros(1025 * 2 * 2, np.float32).tobytes())
    r = run("-i", tmp_path / "wide.vol", "--sym", "rot", 3)
    assert r.returncode == ERR_MATRIX_DIM and "1025 x 2 x 2 is not supported" in r.stderr, r.stderr


@pytest.mark.parametrize("r0,r1,count", [
    ((0, 355, 5), (0, 90, 5), 72 * 19),                      # the default axis search
    ((-357, 357, 3), (1, 10, 0.5), 239 * 19),                # the default helical search
    ((0, 10, 3), (-1, 1, 0.4), None),                        # steps that do not divide their ranges
    ((0, 0, 1), (0, 1, 0.1), None),                          # 0.1 summed ten times against 1 in doubles
    ((7.5, 7.5, 2), (3.25, 3.25, 1), 1),                     # equal bounds
    ((0, 10, 5), (3, 1, 1), 0),                              # first > last in the inner loop: no trial
])
def test_grids_equal_the_reference_loops(r0, r1, count):
    got, n_outer, n_inner = xa.fsym_grid(r0, r1)
    want, w_outer, w_inner = R.grid(r0, r1)
    assert got.shape == want.shape and np.array_equal(got, want) and (n_outer, n_inner) == (w_outer, w_inner)
    if count is not None:
        assert len(got) == count
    if len(got):
        assert len(got) == n_outer * n_inner


def test_a_tenth_summed_ten_times_stops_short_of_one():
    """v += 0.1 from 0 reaches 0.9999999999999999 after ten steps, which is <= 1: eleven trials, and the last is not 1.0. From 0 to 0.3 the
    third sum is 0.30000000000000004, which is above 0.3: three trials, not the four of the exact grid. The loop is what is kept"""
    got, _, n_inner = xa.fsym_grid((0, 0, 1), (0, 1, 0.1))
    assert n_inner == 11 and got[10, 1] == 0.9999999999999999 and got[10, 1] != 1.0
    got, _, n_inner = xa.fsym_grid((0, 0, 1), (0, 0.3, 0.1))
    assert n_inner == 3 and got[:, 1].tolist() == [0.0, 0.1, 0.2]


def test_grid_refusals():
    with pytest.raises(xa.XhError, match="more than 100 trials"):
        xa.fsym_grid((0, 355, 5), (0, 90, 5), limit=100)
    for bad in ((0, 10, 0), (0, 10, -1), (1e17, 2e17, 1)):
        with pytest.raises(xa.XhError, match="never ends"):
            xa.fsym_grid(bad, (0, 1, 1))
        with pytest.raises(xa.XhError, match="never ends"):
            xa.fsym_grid((0, 1, 1), bad)
    with pytest.raises(xa.XhError, match="not finite"):
        xa.fsym_grid((0, float("nan"), 1), (0, 1, 1))


def test_masks_against_the_restatement():
    for shape in ((9, 10, 12), (16, 16, 16)):
        for R_, H_ in ((-4.0, -7.0), (4.5, 6.0)):
            assert np.array_equal(xa.halves_cylinder_mask(shape, R_, H_, (0.5, -1.0, 1.0)), R.cylinder_mask(shape, R_, H_, (0.5, -1.0, 1.0)))
        for a, b, c in ((-2.0, -5.0, -3.0), (2.0, 4.5, 3.0)):
            assert np.array_equal(xa.halves_tube_mask(shape, a, b, c, (0.5, -1.0, 1.0)), R.tube_mask(shape, a, b, c, (0.5, -1.0, 1.0)))
    # as written: the cylinder takes |k - z0| <= H / 2, the tube |k| < H
    c = xa.halves_cylinder_mask((9, 8, 8), -3.0, -4.0)
    assert c[:, 4, 4].tolist() == [0, 0, 1, 1, 1, 1, 1, 0, 0]
    t = xa.halves_tube_mask((9, 8, 8), -1.0, -3.0, -2.0)
    assert t[:, 4, 6].tolist() == [0, 0, 0, 1, 1, 1, 0, 0, 0] and t[4, 4, 4] == 0
    with pytest.raises(xa.XhError, match="cannot determine mode for cylinder"):
        xa.halves_cylinder_mask((8, 8, 8), -3.0, 4.0)
    with pytest.raises(xa.XhError, match="cannot determine mode for tube"):
        xa.halves_tube_mask((8, 8, 8), 1.0, 3.0, 0.0)


@pytest.mark.parametrize("line", [
    "--sym rot 3",
    "--sym helical -z 1 4 1 --mask circular -5 --thr 2 -o {d}/parameters.xmd",
    "--sym rot 2 --localRot 20 10 --useSplines",
])
def test_the_reference_example_lines_parse(files, line):
    """The example lines are read and pass every check; where there is no device the run ends at opening one (the library's error) with
    nothing written, where there is one it ends well with the report"""
    r = run("-i", files / "volume.vol", *line.format(d=files).split())
    assert r.returncode in (0, ERR_GPU), r.stderr
    if r.returncode == 0:
        assert "Symmetry" in r.stdout
    else:
        assert r.stdout == "" and not os.path.exists(files / "parameters.xmd") and not os.path.exists(files / "parameters.xmp")
