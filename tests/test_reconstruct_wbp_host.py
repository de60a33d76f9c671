"""CPU checks of the xmipp_reconstruct_wbp program: its usage lines, every refusal arriving before a device is opened with its own
message, make_even_distribution and find_nearest_direction (xh_wbp_even_distribution, xh_wbp_nearest_direction) against the restatement,
the matrices the program hands to the device, and the shift-direction reading. None needs a device: a refusal that came after opening one
would fail here with the library's error instead."""
import os
import subprocess

import numpy as np
import pytest

import xmipp3_amd as xa
from tests import reconstruct_wbp_ref as R
from tests import xmipp_io

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PROG = os.path.join(ROOT, "xmipp3_amd", "bin", "xmipp_reconstruct_wbp")
ERR_ARG_INCORRECT, ERR_MD_NOOBJ, ERR_MATRIX_DIM, ERR_NOT_IMPLEMENTED = 2, 30, 41, 61
LABELS = ["image", "angleRot", "angleTilt", "anglePsi", "shiftX", "shiftY", "flip", "weight"]


def run(*args):
    return subprocess.run([PROG] + [str(a) for a in args], capture_output=True, text=True)


def _xmd(path, names, weights=None):
    rows = [[n, 10.0 * k, 20.0 + k, 5.0, 0.5, -0.25, 0, 1.0 if weights is None else weights[k]] for k, n in enumerate(names)]
    xmipp_io.write_xmd(str(path), [("particles", LABELS, rows)])
    return path


@pytest.fixture(scope="module")
def files(tmp_path_factory):
    d = tmp_path_factory.mktemp("wbp")
    rng = np.random.default_rng(0)
    xmipp_io.write_stack(str(d / "a.stk"), rng.standard_normal((3, 12, 12)))
    xmipp_io.write_stack(str(d / "b.stk"), rng.standard_normal((1, 10, 10)))
    xmipp_io.write_stack(str(d / "c.stk"), rng.standard_normal((1, 10, 12)))
    a = [f"{k + 1:06d}@{d / 'a.stk'}" for k in range(3)]
    _xmd(d / "good.xmd", a)
    _xmd(d / "mixed.xmd", a + [f"000001@{d / 'b.stk'}"])
    _xmd(d / "oblong.xmd", [f"000001@{d / 'c.stk'}"])
    _xmd(d / "noweight.xmd", a, weights=[0.0, 0.0, 0.0])
    hdr = xmipp_io._spider_header(1025, 1025, 1, 1, 0, 0, 0)
    with open(d / "wide.spi", "wb") as f:
        f.write(hdr.tobytes())
        f.write(np.zeros(1025 * 1025, np.float32).tobytes())
    _xmd(d / "wide.xmd", [str(d / "wide.spi")])
    return d


def test_usage_lines():
    r = run("--help")
    assert r.returncode == 0
    for line in ("Generate 3D reconstruction from projections using the Weighted BackProjection algorithm.",
                 "-i <arg> : selection file with input images and Euler angles",
                 "[-o <=wbp.vol>] : filename for output volume",
                 "[--doc <=>] : Ignore headers and get angles from this docfile",
                 "[--radius <=-1>] : Reconstruction radius. int=-1 means radius=dim/2",
                 "[--sym <=>] : Enforce symmetry",
                 "[--threshold <=0.005>] : Lower (relative) threshold for filter values",
                 "[--filsam <=5>] : Angular sampling rate for geometry filter",
                 "[--use_each_image] : Use each image instead of sampled representatives for filter",
                 "[--weight] : Use weights stored in image headers or the input metadata",
                 "[--device <=0>] : HIP device (one device only)",
                 "xmipp_reconstruct_wbp -i images.sel -o reconstruction.vol"):
        assert line in r.stdout + r.stderr, line


@pytest.mark.parametrize("inp,args,code,words", [
    ("good.xmd", ("--sym", "c3"), ERR_NOT_IMPLEMENTED, "--sym without --use_each_image"),
    ("good.xmd", ("--sym", "ci", "--use_each_image"), ERR_NOT_IMPLEMENTED, "--sym ci: a group with mirrors or an inversion"),
    ("good.xmd", ("--sym", "c3v", "--use_each_image"), ERR_NOT_IMPLEMENTED, "--sym c3v: a group with mirrors or an inversion"),
    ("mixed.xmd", ("--use_each_image",), ERR_MATRIX_DIM, "b.stk is 10 x 10, the first image 12 x 12"),
    ("oblong.xmd", ("--use_each_image",), ERR_MATRIX_DIM, "images of 12 x 10 x 1: square images are expected"),
    ("wide.xmd", ("--use_each_image",), ERR_MATRIX_DIM, "images of 1025 pixels a side are not supported (2 .. 1024)"),
    ("good.xmd", ("--use_each_image", "--device", "0,1"), ERR_ARG_INCORRECT, "--device 0,1: this program runs on one device"),
    ("good.xmd", ("--use_each_image", "--radius", 7), ERR_ARG_INCORRECT, "--radius 7: beyond half the image (12 pixels)"),
    ("good.xmd", ("--filsam", 0.1), ERR_ARG_INCORRECT, "--filsam 0.1: a sampling between 0.5 and 180 degrees"),
    ("noweight.xmd", ("--use_each_image", "--weight"), ERR_MD_NOOBJ, "there is no input file with weight!=0"),
])
def test_refusals_come_before_any_device(files, inp, args, code, words):
    r = run("-i", files / inp, "-o", files / "never.vol", "-v", 0, *args)
    assert r.returncode == code and words in r.stderr and r.stderr.startswith(f"XMIPP_ERROR {code}:"), r.stderr
    assert not os.path.exists(files / "never.vol")


def test_show_text(files):
    r = run("-i", files / "good.xmd", "--sym", "c3", "--radius", 4, "--weight")
    assert r.returncode == ERR_NOT_IMPLEMENTED                       # refused while the options are read: nothing is shown
    assert "Weighted-back projection" not in r.stderr


@pytest.mark.parametrize("sampling,count", [(5.0, 1666), (15.0, 188), (30.0, 48), (7.5, 746)])
def test_even_distribution(sampling, count):
    rot, tilt = xa.wbp_even_distribution(sampling)
    want_rot, want_tilt = R.even_distribution(sampling)
    assert len(rot) == count
    assert np.array_equal(rot, want_rot) and np.array_equal(tilt, want_tilt)
    assert tilt[0] == 0.0 and rot[0] == 0.0 and tilt.max() <= 180.0
    with pytest.raises(xa.XhError, match="sampling"):
        xa.wbp_even_distribution(0.1)


def test_nearest_direction_binning():
    rot, tilt = xa.wbp_even_distribution(15.0)
    rng = np.random.default_rng(11)
    for r, t in zip(rng.uniform(-360, 720, 200), rng.uniform(-180, 360, 200)):
        assert xa.wbp_nearest_direction(r, t, rot, tilt) == R.nearest_direction(r, t, rot, tilt)
    k = 57
    assert xa.wbp_nearest_direction(rot[k], tilt[k], rot, tilt) == k
    assert xa.wbp_nearest_direction(rot[k] + 180.0, -tilt[k], rot, tilt) == k                # Euler_another_set of it
    assert xa.wbp_nearest_direction(10.0, 20.0, [], []) == -1
    # the counts are truncated: weights of 0.5 alone leave no direction
    g, tot = R.sampled_matrices([(10.0, 20.0, 0.0), (200.0, 100.0, 0.0)], [0.5, 3.7], 15.0)
    assert len(g) == 1 and g[0, 3] == 3.0 and tot == 3.0


def test_image_matrices():
    """what the program hands to the device is what the restatement forms: the three -tilt conventions"""
    for rot, tilt, psi in ((10.5, 33.25, -70.0), (0.0, 0.0, 0.0), (359.0, 179.5, 12.0)):
        g, F, B = xa.wbp_image_matrices(rot, tilt, psi)
        Fr, Br = R.image_matrices(rot, tilt, psi)
        E = np.array(R.euler_matrix(rot, -tilt, psi))
        assert np.array_equal(F, Fr) and np.array_equal(B, Br) and np.array_equal(g, E[2])
        assert np.allclose(B, E.T, atol=1e-15)


def test_shift_direction_reading():
    """the reading this program takes of reconstruct_wbp.cpp:552-554 (unpinned): IS_INV with readApplyGeo's matrix, so a
    positive shiftX moves the content towards negative x"""
    img = np.zeros((16, 16))
    img[8, 11] = 1.0
    out = R.prepare(img, 2.0, 0.0, False, 1.0)
    assert np.unravel_index(np.argmax(out), out.shape) == (8, 9)
