"""CPU checks of the xmipp_volume_align program: its usage lines, every refusal arriving before a device is opened with a message that
names the option, and the reference's two example command lines. None needs a device: a refusal that came after opening one would fail
here with the library's error instead."""
import os
import subprocess

import numpy as np
import pytest

from tests import volume_align_ref as R
from tests import xmipp_io

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PROG = os.path.join(ROOT, "xmipp3_amd", "bin", "xmipp_volume_align")
ERR_ARG_INCORRECT, ERR_ARG_MISSING, ERR_MATRIX_DIM, ERR_VALUE_INCORRECT, ERR_GPU, ERR_NOT_IMPLEMENTED = 2, 3, 41, 50, 60, 61


def run(*args):
    return subprocess.run([PROG] + [str(a) for a in args], capture_output=True, text=True)


@pytest.fixture(scope="module")
def files(tmp_path_factory):
    d = tmp_path_factory.mktemp("valign")
    xmipp_io.write_volume(d / "volume1.vol", R.phantom((12, 12, 12), 1))
    xmipp_io.write_volume(d / "volume2.vol", R.phantom((12, 12, 12), 2))
    xmipp_io.write_volume(d / "other.vol", R.phantom((12, 10, 12), 3))
    xmipp_io.write_volume(d / "empty.vol", np.zeros((12, 12, 12)))
    xmipp_io.write_volume(d / "flat.vol", np.zeros((1, 12, 12)))
    return d


def test_usage_lines():
    r = run("--help")
    assert r.returncode == 0
    for line in ("Align two volumes varying orientation, position and scale",
                 "--i1 <arg> : the first volume to align",
                 "--i2 <arg> : the second one",
                 "[--rot <=0> <=0> <=1>] : in degrees",
                 "[--scale <=1> <=1> <=1>] : size scale margin",
                 "[--grey_scale <=1> <=1> <=1>] : grey scale margin",
                 "[--grey_shift <=0> <=0> <=1>] : grey shift margin",
                 "[-z <=0> <=0> <=1>] : Z position in pixels",
                 "[-x <=0> <=0> <=1>] : X position in pixels",
                 "[--consider_mirror] : Consider the mirror volume",
                 "[--show_fit] : Show fitness values",
                 "[--apply <=>] : Apply best movement to --i2 and store results in this file",
                 "[--covariance] : Covariance fitness criterion",
                 "[--least_squares] : LS fitness criterion",
                 "[--local] : Use local optimizer instead of exhaustive search",
                 "[--frm <=0.25> <=10> <=-90> <=90>] : Use Fast Rotational Matching, if tilt0 and tiltF are left as -90 and 90 they do not effect the results",
                 "[--onlyShift] : Only shift",
                 "[--dontScale] : Do not look for scale changes",
                 "[--copyGeo <=>] : copy transformation matrix in a txt file. ('A' matrix elements)",
                 "[--copyGray <=>] : copy gray scale and shift txt file.)",
                 "[--store <=>] : copy angles and shifts to a txt file.",
                 "[--dontWrap] : Do not wrap input2 when aligning to input1",
                 "[--device <=0>] : HIP device (one device only)",
                 "xmipp_volume_align --i1 volume1.vol --i2 volume2.vol --rot 0 360 15 --tilt 0 180 15 --psi 0 360 15",
                 "xmipp_volume_align --i1 volume1.vol --i2 volume2.vol --rot 45 --tilt 60 --psi 90 --local --apply volume2aligned.vol"):
        assert line in r.stderr, line


@pytest.mark.parametrize("i2,args,code,words", [
    ("volume2.vol", ("--frm",), ERR_NOT_IMPLEMENTED, "--frm: Fast Rotational Matching calls the external Python package sh_alignment"),
    ("volume2.vol", ("--mask", "gaussian", 3), ERR_NOT_IMPLEMENTED, "--mask gaussian: only the binary_file and circular mask types"),
    ("other.vol", (), ERR_MATRIX_DIM, "--i1 and --i2 have different dimensions (12 x 12 x 12 and 12 x 10 x 12)"),
    ("volume2.vol", ("--mask", "binary_file", "{d}/other.vol"), ERR_MATRIX_DIM, "other.vol is 12 x 10 x 12, the volumes 12 x 12 x 12"),
    ("volume2.vol", ("--mask", "binary_file", "{d}/empty.vol"), ERR_VALUE_INCORRECT, "--mask selects no voxel"),
    ("volume2.vol", ("--mask", "circular", 30), ERR_VALUE_INCORRECT, "--mask selects no voxel"),
    ("volume2.vol", ("--device", "0,1"), ERR_ARG_INCORRECT, "--device 0,1: this program runs on one device"),
    ("volume2.vol", ("--rot", 0, 360, 0.5, "--tilt", 0, 180, 0.5, "--psi", 0, 360, 0.5), ERR_ARG_INCORRECT, "at most 2097152 trials"),
    ("volume2.vol", ("--rot", 0, 360, -15), ERR_ARG_INCORRECT, "never ends"),
    ("volume2.vol", ("--grey_scale", 0.8, 1.2, 0.1), ERR_ARG_MISSING, "--grey_scale requires --least_squares"),
    ("volume2.vol", ("--grey_shift", -0.1, 0.1, 0.1, "--covariance"), ERR_ARG_MISSING, "--grey_shift requires --least_squares"),
])
def test_refusals_come_before_any_device(files, i2, args, code, words):
    r = run("--i1", files / "volume1.vol", "--i2", files / i2, *[str(a).format(d=files) for a in args])
    assert r.returncode == code and words in r.stderr and r.stderr.startswith(f"XMIPP_ERROR {code}:"), r.stderr
    assert r.stdout == ""


def test_sides_outside_2_to_1024_are_refused(files, tmp_path):
    r = run("--i1", files / "flat.vol", "--i2", files / "flat.vol")
    assert r.returncode == ERR_MATRIX_DIM and "a box of 12 x 12 x 1 is not supported (2 .. 1024 a side)" in r.stderr
    # a header alone says 1025 a side: the refusal comes from the header, before the values are read
    hdr = xmipp_io._spider_header(1025, 2, 2, 3, 0, 0, 0)
    with open(tmp_path / "wide.vol", "wb") as f:
        f.write(hdr.tobytes())
        f.write(np.zeros(1025 * 2 * 2, np.float32).tobytes())
    r = run("--i1", tmp_path / "wide.vol", "--i2", tmp_path / "wide.vol")
    assert r.returncode == ERR_MATRIX_DIM and "1025 x 2 x 2 is not supported" in r.stderr, r.stderr


@pytest.mark.parametrize("line", [
    "--rot 0 360 15 --tilt 0 180 15 --psi 0 360 15",
    "--rot 45 --tilt 60 --psi 90 --local --apply {d}/volume2aligned.vol",
])
def test_the_reference_example_lines_parse(files, line):
    """Both example lines are read and pass every check; where there is no device the run ends at opening one (the library's error) with
    nothing written, where there is one it ends well with the report"""
    r = run("--i1", files / "volume1.vol", "--i2", files / "volume2.vol", *line.format(d=files).split())
    assert r.returncode in (0, ERR_GPU), r.stderr
    if r.returncode == 0:
        assert "The best correlation is for" in r.stdout
    else:
        assert r.stdout == "" and not os.path.exists(files / "volume2aligned.vol")
