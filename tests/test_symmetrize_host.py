"""CPU checks of the xmipp_transform_symmetrize program: its usage lines and show() text, every refusal arriving before a device is
opened with its wording, the image / volume --sym errors, and that a run without -o writes nowhere but the input. None of them needs a device: a refusal that came after opening one would fail here with the library's error instead."""
import os
import subprocess

import numpy as np
import pytest

from tests import symmetrize_ref as R
from tests import xmipp_io

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PROG = os.path.join(ROOT, "xmipp3_amd", "bin", "xmipp_transform_symmetrize")
ERR_ARG_INCORRECT, ERR_ARG_MISSING, ERR_GPU, ERR_NOT_IMPLEMENTED = 2, 3, 60, 61


def run(*args):
    return subprocess.run([PROG] + [str(a) for a in args], capture_output=True, text=True)


@pytest.fixture(scope="module")
def files(tmp_path_factory):
    d = tmp_path_factory.mktemp("sym")
    xmipp_io.write_volume(d / "v.vol", R.phantom((12, 12, 12), 1))
    xmipp_io.write_stack(d / "s.stk", np.stack([R.phantom((12, 12), 2), R.phantom((12, 12), 3)]))
    xmipp_io.write_xmd(d / "geo.xmd", [("noname", ["image", "shiftX"], [[str(d / "v.vol"), 1.5]])])
    xmipp_io.write_xmd(d / "two.xmd", [("noname", ["image"], [[str(d / "v.vol")], [str(d / "v.vol")]])])
    return d


def test_usage_lines():
    r = run("--help")
    assert r.returncode == 0
    for line in ("Symmetrize volumes and images",
                 "--sym <arg> : For 2D images: a number For 3D volumes: a symmetry file or point-group description",
                 "I, I1, I2, I3, I4, I5, Ih, helical, dihedral, helicalDihedral",
                 "[--sym2 <=C1>] : Only for helical, or helicalDihedral You may use any other Cn symmetry",
                 "[--helixParams <arg> <arg> <=0>] : Helical parameters z(Angstroms), rot(degrees), rotPhase(degrees)",
                 "[--heightFraction <=0.95>] : Height fraction used for symmetrizing a helix",
                 "[--sampling <=1>] : Sampling rate (A/pixel). Used only for helical parameters",
                 "[--no_group] : For 3D volumes: do not generate symmetry subgroup",
                 "[--dont_wrap] : by default, the image/volume is wrapped",
                 "[--sum] : compute the sum of the images/volumes instead of the average. This is useful for symmetrizing pieces",
                 "[--mask_in <arg>] : symmetrize only in the masked area",
                 "[--spline <=3>] : Spline order for the interpolation (valid values are 1 and 3)",
                 "[--device <=0>] : HIP device (one device only)",
                 "xmipp_transform_symmetrize -i input.sel --sym 6",
                 "xmipp_transform_symmetrize -i input.vol --sym i3 --dont_wrap"):
        assert line in r.stderr, line


def test_show_text(files):
    # the run stops at the image / volume check, after show()
    r = run("-i", files / "v.vol", "--sym", "6", "--dont_wrap", "--spline", 1)
    assert r.stdout.splitlines() == [f"Input File: {files / 'v.vol'}", "Symmetry: 6", "No group: 0", "Wrap:     0", "Sum:      0", "Spline:   1"]
    r = run("-i", files / "s.stk", "-o", files / "out.stk", "--sym", "helical", "--sym2", "C2", "--helixParams", 7.5, 30, 5, "--sampling", 1.5, "--sum", "--no_group")
    assert r.stdout.splitlines() == [f"Input File: {files / 's.stk'}", f"Output File: {files / 'out.stk'}", "Symmetry: helical", "No group: 1", "Wrap:     1",
                                     "Sum:      1", "Spline:   3", "RotHelical: 30", "RotPhaseHelical: 5", "ZHelical:   7.5Height fraction: 0.95", "Symmetry2: C2"]
    assert r.returncode == ERR_ARG_INCORRECT and "Helical symmetrization is not meant for images" in r.stderr
    assert run("-i", files / "v.vol", "--sym", "6", "-v", 0).stdout == ""


@pytest.mark.parametrize("args,code,words", [
    (("--sym", "c3", "--mask_in", "m.vol"), ERR_NOT_IMPLEMENTED, "selfArrayByArrayMask"),
    (("--sym", "dihedral"), ERR_NOT_IMPLEMENTED, "symmetry_Dihedral"),
    (("--sym", "c3", "--spline", 2), ERR_ARG_INCORRECT, "--spline 2: valid values are 1 and 3"),
    (("--sym", "c3", "--device", "0,1"), ERR_ARG_INCORRECT, "this program runs on one device"),
    (("--sym", "helical", "--helixParams", 1.0, 30), ERR_ARG_INCORRECT, "never terminates"),
    (("--sym", "helical", "--helixParams", 3.0, 30, "--sampling", 4.0), ERR_ARG_INCORRECT, "a rise of 0.75 voxels"),
    (("--sym", "helicalDihedral", "--helixParams", 13.0, 30), ERR_ARG_INCORRECT, "bounded only for 1 < rise <= Z"),
    (("--sym", "helical", "--helixParams", 4.0, 30, "--heightFraction", 1.2), ERR_ARG_INCORRECT, "0 < heightFraction <= 1"),
    (("--sym", "helical", "--helixParams", 4.0, 30, "--sym2", "d2"), ERR_ARG_INCORRECT, "a Cn symmetry is expected"),
])
def test_refusals_come_before_any_device(files, args, code, words):
    r = run("-i", files / "v.vol", *args)
    assert r.returncode == code and words in r.stderr and r.stderr.startswith(f"XMIPP_ERROR {code}:"), r.stderr


def test_geometry_columns_are_refused(files):
    r = run("-i", files / "geo.xmd", "--sym", "c3")
    assert r.returncode == ERR_NOT_IMPLEMENTED and "geometry column shiftX" in r.stderr and "readApplyGeo" in r.stderr


def test_several_volumes_with_an_output_are_refused(files):
    r = run("-i", files / "two.xmd", "-o", files / "out.stk", "--sym", "c3")
    assert r.returncode == ERR_NOT_IMPLEMENTED and "stack of volumes" in r.stderr


def test_a_stack_of_volumes_is_refused_and_left_alone(tmp_path):
    """a Spider stack whose images have Z > 1, with and without -o: refused before anything is written"""
    vols = np.stack([R.phantom((6, 8, 8), 5), R.phantom((6, 8, 8), 6)]).astype(np.float32)
    with open(tmp_path / "vs.stk", "wb") as f:
        f.write(xmipp_io._spider_header(8, 8, 6, 3, 2, 2, 0).tobytes())
        for i in range(2):
            f.write(xmipp_io._spider_header(8, 8, 6, 3, 0, 0, i + 1).tobytes())
            f.write(vols[i].tobytes())
    before = open(tmp_path / "vs.stk", "rb").read()
    for extra in ((), ("-o", tmp_path / "out.stk")):
        r = run("-i", tmp_path / "vs.stk", "--sym", "c3", *extra)
        assert r.returncode == ERR_NOT_IMPLEMENTED and "stack of volumes" in r.stderr, r.stderr
    assert open(tmp_path / "vs.stk", "rb").read() == before and sorted(os.listdir(tmp_path)) == ["vs.stk"]


def test_image_and_volume_symmetry_errors(files):
    r = run("-i", files / "s.stk", "--sym", "c6")
    assert r.returncode == ERR_ARG_MISSING and "The symmetry order is not valid for images" in r.stderr
    r = run("-i", files / "v.vol", "--sym", "6")
    assert r.returncode == ERR_ARG_MISSING and "The symmetry description is not valid for volumes" in r.stderr
    r = run("-i", files / "v.vol", "--sym", "c1")
    assert r.returncode == ERR_ARG_MISSING and "The symmetry description is not valid for volumes" in r.stderr


def test_without_an_output_only_the_input_is_written(tmp_path):
    """With -o absent the output name is the input's. Where there is no device the run ends at opening one (the library's error) with the
    input untouched; where there is one the input changes. Either way nothing else appears next to it."""
    v = R.phantom((12, 12, 12), 4)
    xmipp_io.write_volume(tmp_path / "v.vol", v)
    r = run("-i", tmp_path / "v.vol", "--sym", "c3", "-v", 0)
    assert r.returncode in (0, ERR_GPU), r.stderr
    assert sorted(os.listdir(tmp_path)) == ["v.vol"]
    same = np.array_equal(xmipp_io.read_volume(tmp_path / "v.vol"), v.astype(np.float32))
    assert same == (r.returncode == ERR_GPU)
