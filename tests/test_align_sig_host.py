"""CPU checks of xmipp_align_significant: its flags parse, and the refusals of AProgAlignSignificant::check / validate
(aalign_significant.cpp:192-218) and of a second --dev come with their exit status and message before any device is touched."""
import os
import subprocess

import numpy as np
import pytest

from tests import xmipp_io

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PROG = os.path.join(ROOT, "xmipp3_amd", "bin", "xmipp_align_significant")


@pytest.fixture(scope="module")
def prog():
    import __graft_entry__ as g
    g.build()
    assert os.path.exists(PROG)
    return PROG


def _run(args):
    return subprocess.run([PROG] + args, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=120)


def _inputs(tmp, nref, nimg, ref_size=16, img_size=16, ref_label=True):
    rng = np.random.default_rng(0)
    xmipp_io.write_stack(str(tmp / "refs.stk"), rng.standard_normal((nref, ref_size, ref_size)).astype(np.float32))
    xmipp_io.write_stack(str(tmp / "imgs.stk"), rng.standard_normal((nimg, img_size, img_size)).astype(np.float32))
    labels = ["image", "ref"] if ref_label else ["image"]
    xmipp_io.write_xmd(str(tmp / "refs.xmd"), [("noname", labels, [[f"{i + 1}@{tmp}/refs.stk", i + 1][:len(labels)] for i in range(nref)])])
    xmipp_io.write_xmd(str(tmp / "imgs.xmd"), [("noname", ["image"], [[f"{i + 1}@{tmp}/imgs.stk"] for i in range(nimg)])])
    return ["-i", str(tmp / "imgs.xmd"), "-r", str(tmp / "refs.xmd"), "-o", "out.xmd", "--odir", str(tmp)]


def test_help_lists_the_reference_flags(prog):
    r = _run(["--help"])
    assert r.returncode == 0 and "USAGE" in r.stderr
    for flag in ("-i", "-r", "-o", "--odir", "--thr", "--angDistance", "--keepBestN", "--allowInputSwap", "--useWeightInsteadOfCC", "--oUpdatedRefs", "--dev"):
        assert f" {flag}" in r.stderr or f"[{flag}" in r.stderr, flag


def test_missing_mandatory_and_unknown_flags(prog, tmp_path):
    r = _run(["-i", "a.xmd", "-o", "b.xmd"])
    assert r.returncode == 3 and "XMIPP_ERROR 3" in r.stderr and "-r" in r.stderr
    r = _run(["-i", "a.xmd", "-r", "b.xmd", "-o", "c.xmd", "--bogus"])
    assert r.returncode != 0 and "Unknown parameter '--bogus'" in r.stderr


def test_keep_best_n_above_the_number_of_references(prog, tmp_path):
    r = _run(_inputs(tmp_path, 3, 4) + ["--keepBestN", "4"])
    assert r.returncode == 62 and "--keepBestN is higher than number of references" in r.stderr


def test_one_reference(prog, tmp_path):
    r = _run(_inputs(tmp_path, 1, 4))
    assert r.returncode == 62 and "We need at least two references" in r.stderr


def test_size_mismatch(prog, tmp_path):
    r = _run(_inputs(tmp_path, 3, 4, ref_size=16, img_size=20))
    assert r.returncode == 62 and "Dimensions of the images to align and reference images do not match" in r.stderr


def test_missing_ref_label(prog, tmp_path):
    r = _run(_inputs(tmp_path, 3, 4, ref_label=False))
    assert r.returncode == 31 and "missing MDL_REF label" in r.stderr


def test_swap_is_checked_in_the_swapped_roles(prog, tmp_path):
    # with --allowInputSwap and more references than images the images become the references: a single image is then refused
    r = _run(_inputs(tmp_path, 3, 1) + ["--allowInputSwap"])
    assert r.returncode == 62 and "We are swapping reference images" in r.stderr and "We need at least two references" in r.stderr


def test_several_devices_are_refused(prog, tmp_path):
    r = _run(_inputs(tmp_path, 3, 4) + ["--dev", "0", "1"])
    assert r.returncode != 0 and "several devices are not supported" in r.stderr
    r = _run(_inputs(tmp_path, 3, 4) + ["--dev", "-1"])
    assert r.returncode != 0 and "XMIPP_ERROR" in r.stderr
