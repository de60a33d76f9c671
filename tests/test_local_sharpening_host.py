"""CPU checks of xmipp_volume_local_sharpening (LocalDeblur): the band list against the numpy restatement
(tests/local_sharpening_ref.py), and the program's option parsing and refusals, which come before any device is touched."""
import os
import subprocess

import numpy as np
import pytest

from tests import local_sharpening_ref as R
from tests import xmipp_io

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PROG = os.path.join(ROOT, "xmipp3_amd", "bin", "xmipp_volume_local_sharpening")


@pytest.fixture(scope="module")
def xa():
    import __graft_entry__ as g
    g.build()
    assert os.path.exists(PROG)
    import xmipp3_amd
    return xmipp3_amd


def _run(args):
    return subprocess.run([PROG] + args, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=120)


# (1, 9): plain; (1.34, 12.5): a sampling rate that is no multiple of the step; (0.8, 30): res advances far enough for the repeated
# additions to differ from a product, and many resolutions share an index
@pytest.mark.parametrize("size", [20, 21, 32])
@pytest.mark.parametrize("sampling,max_res", [(1.0, 9.0), (1.34, 12.5), (0.8, 30.0)])
def test_band_list_is_the_restatement_bit_for_bit(xa, size, sampling, max_res):
    got = xa.ldb_bands(size, sampling, max_res)
    exp = R.bands(size, sampling, max_res)
    assert len(got) == len(exp) >= 5
    for g, e in zip(got, exp):
        assert g[0] == e[0] and g[1] == e[1] and g[2] == e[2] and g[3] == e[3]
    # consecutive bands never share an index, and some resolution of the loop was skipped for sharing one
    idx = [g[3] for g in got]
    assert all(a != b for a, b in zip(idx, idx[1:]))
    nres = 0
    res = 2 * sampling
    while res < max_res:
        nres += 1
        res += 0.2
    assert len(got) < nres
    assert got[0][0] == 2 * sampling and all(a[0] < b[0] for a, b in zip(got, got[1:])) and got[-1][0] < max_res


def test_res_advances_by_repeated_addition(xa):
    got = xa.ldb_bands(1000, 1.0, 30.0)                  # a size at which every resolution has an index of its own for a while
    res, k = 2.0, 0
    seen = {g[0] for g in got}
    prod_differs = False
    while res < 30.0:
        if res in seen and res != 2.0 + k * 0.2:
            prod_differs = True
        res += 0.2
        k += 1
    assert prod_differs


def test_band_list_refuses_a_sampling_without_a_first_band(xa):
    for s in (0.1, 0.05, 0.0, -1.0):
        with pytest.raises(xa.XhError, match="sampling"):
            xa.ldb_bands(32, s, 9.0)
        with pytest.raises(ValueError):
            R.bands(32, s, 9.0)
    with pytest.raises(xa.XhError, match="finite"):
        xa.ldb_bands(32, 1.0, float("inf"))


def test_help_lists_the_reference_options_and_defaults(xa):
    r = _run(["--help"])
    assert r.returncode == 0
    for t in ("--vol <=>", "--resolution_map <=>", "--sampling <=1>", "-o <=Sharpening.vol>", "[--md <=params.xmd>]", "[-l <=1>]", "[-k <=0.025>]",
              "[-i <=50>]", "[-n <=1>]", "[--dev <=0>]"):
        assert t in r.stderr, t


# as in the reference, the options without brackets are mandatory, their defaults notwithstanding
FILES = ["--vol", "/nonexistent/a.vol", "--resolution_map", "/nonexistent/r.vol", "-o", "/nonexistent/o.vol"]
BASE = FILES + ["--sampling", "1"]


def _shown(r):
    return dict(l.split(": ", 1) for l in r.stdout.splitlines() if ": " in l)


def test_defaults_are_the_reference_ones_and_a_missing_file_stops_before_any_device(xa):
    r = _run(BASE)
    assert r.returncode == 20 and "cannot open" in r.stderr
    s = _shown(r)
    assert s["sampling"] == "1" and s["output"] == "/nonexistent/o.vol" and s["md"] == "params.xmd" and s["lambda"] == "1" and s["K"] == "0.025"
    assert s["Niter"] == "50" and s["Nthread"] == "1"
    r = _run(FILES + ["-n", "7", "-l", "0.5", "-k", "0.1", "-i", "3", "--sampling", "1.5"])
    s = _shown(r)
    assert s["Nthread"] == "7" and s["lambda"] == "0.5" and s["K"] == "0.1" and s["Niter"] == "3" and s["sampling"] == "1.5"


def test_bad_device_is_refused(xa):
    r = _run(BASE + ["--dev", "x"])
    assert r.returncode != 0 and "Invalid GPU device" in r.stderr


@pytest.mark.parametrize("extra,text", [(["--sampling", "0.1"], "2 sampling - 0.2"), (["--sampling", "0.05"], "2 sampling - 0.2"),
                                        (["--sampling", "1", "-i", "0"], "never assigned")])
def test_refused_options(xa, extra, text):
    r = _run(FILES + extra)
    assert r.returncode != 0 and text in r.stderr and "cannot open" not in r.stderr


def test_volumes_of_different_shapes_are_refused_before_any_device(xa, tmp_path):
    xmipp_io.write_volume(str(tmp_path / "a.vol"), np.zeros((8, 8, 8), np.float32))
    xmipp_io.write_volume(str(tmp_path / "r.vol"), np.zeros((8, 8, 6), np.float32))
    r = _run(["--vol", str(tmp_path / "a.vol"), "--resolution_map", str(tmp_path / "r.vol"), "--sampling", "1", "-o", str(tmp_path / "o.vol"), "--md",
              str(tmp_path / "p.xmd")])
    assert r.returncode != 0 and "different dimensions" in r.stderr
    assert not (tmp_path / "o.vol").exists()
