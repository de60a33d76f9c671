"""CPU checks of xmipp_angular_sph_alignment: the variables each stage of the search frees against a numpy restatement of the reference's
minimizepos (reconstruction/angular_sph_alignment.cpp:472-482) and of the steps processImage sets (:351-358), the program's defaults, the
refusal of degrees the basis is not written out for, and the program's command line, all before any device is touched."""
import ctypes as C
import itertools
import os
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PROG = os.path.join(ROOT, "xmipp3_amd", "bin", "xmipp_angular_sph_alignment")
XH_ERR_UNSUPPORTED = -5


@pytest.fixture(scope="module")
def xa():
    import __graft_entry__ as g
    g.build()
    assert os.path.exists(PROG)
    import xmipp3_amd
    return xmipp3_amd


def num_coefficients(l1, l2):
    """numCoefficients (:451-470), by its own counting of even and odd radial degrees"""
    nc = 0
    for h in range(l2 + 1):
        num_sph = 2 * h + 1
        count = l1 - h + 1
        num_even = (count >> 1) + (1 if (count & 1) and not (h & 1) else 0)
        nc += num_sph * num_even if h % 2 == 0 else num_sph * (count - num_even)
    return nc


def steps_ref(L1, L2, stage, deformation, alignment, defocus):
    """the steps vector of processImage for stage h (:342-358); the freed variables are where it is 1"""
    vec = num_coefficients(L1, L2)
    total = 3 * vec + 8
    steps = np.zeros(total)
    if alignment:
        steps[total - 8:total - 3] = 1
    if defocus:
        steps[total - 3:] = 1
    if deformation:
        size = num_coefficients(L1, stage)              # minimizepos
        for idx in range(size):
            steps[idx] = steps[idx + vec] = steps[idx + 2 * vec] = 1
    return steps


@pytest.mark.parametrize("L1,L2", [(3, 2), (5, 4), (2, 1), (1, 0)])
def test_stage_active(xa, L1, L2):
    assert num_coefficients(L1, L2) == xa.vds_num_terms(L1, L2)
    for stage in range(L2 + 1):
        for flags in itertools.product((False, True), repeat=3):
            got = xa.asa_stage_active(L1, L2, stage, *flags)
            want = np.flatnonzero(steps_ref(L1, L2, stage, *flags))
            assert got.dtype == np.int32 and np.array_equal(got, want), (L1, L2, stage, flags)
    out, n = np.zeros(200, np.int32), C.c_int32()
    assert xa.lib().xh_asa_stage_active(L1, L2, L2 + 1, 7, out.ctypes.data_as(C.c_void_p), C.byref(n)) == -1      # no such stage
    assert xa.lib().xh_asa_stage_active(L1, L2, 0, 8, out.ctypes.data_as(C.c_void_p), C.byref(n)) == -1           # no such flag


def test_defaults(xa):
    from xmipp3_amd._lib import AsaParams
    p = AsaParams()
    xa.lib().xh_asa_defaults(C.byref(p))
    assert (p.max_shift, p.max_angular_change, p.max_resolution, p.sampling) == (-1.0, 5.0, 4.0, 1.0)
    assert (p.Rmax, p.RDef, p.l1, p.l2, p.lambda_) == (-1.0, -1.0, 3, 2, 0.01)
    assert (p.optimize_alignment, p.optimize_deformation, p.optimize_defocus, p.phase_flipped) == (0, 0, 0, 0)


@pytest.mark.parametrize("L1,L2", [(6, 2), (3, 5)])
def test_unsupported_degrees(xa, L1, L2):
    out, n = np.zeros(400, np.int32), C.c_int32()
    assert xa.lib().xh_asa_stage_active(L1, L2, 1, 7, out.ctypes.data_as(C.c_void_p), C.byref(n)) == XH_ERR_UNSUPPORTED
    assert b"not supported" in xa.lib().xh_last_error()
    with pytest.raises(xa.XhError, match="not supported"):
        xa.asa_stage_active(L1, L2, 1)


def _run(args):
    return subprocess.run([PROG] + args, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=120)


OPTIONS = ["-i", "-o", "--ref", "--mask", "--odir", "--max_shift", "--max_angular_change", "--max_resolution", "--sampling", "--Rmax", "--RDef",
           "--l1", "--l2", "--regularization", "--optimizeAlignment", "--optimizeDeformation", "--optimizeDefocus", "--phaseFlipped", "--resume",
           "--device", "--useCPU"]


def test_program_help(xa):
    r = _run(["--help"])
    assert r.returncode == 0
    for flag in OPTIONS:
        assert flag in r.stderr, flag
    for defaults in ("--max_shift <=-1>", "--max_angular_change <=5>", "--max_resolution <=4>", "--sampling <=1>", "--Rmax <=-1>", "--RDef <=-1>",
                     "--l1 <=3>", "--l2 <=2>", "--regularization <=0.01>", "--odir <=.>"):
        assert defaults in r.stderr, defaults


def test_program_arguments(xa):
    r = _run(["-i", "a.xmd", "-o", "b.xmd", "--optimizeDeformation"])
    assert r.returncode != 0 and "Parameter --ref is mandatory" in r.stderr
    r = _run(["-i", "a.xmd", "-o", "b.xmd", "--ref", "v.vol", "--optimizeDeformation", "--l2", "5"])
    assert r.returncode != 0 and "l2 = 5" in r.stderr and "not supported" in r.stderr
    r = _run(["-i", "a.xmd", "-o", "b.xmd", "--ref", "v.vol", "--optimizeDeformation", "--l2", "0"])
    assert r.returncode != 0 and "--l2" in r.stderr and "no stage" in r.stderr
    r = _run(["-i", "a.xmd", "-o", "b.xmd", "--ref", "v.vol"])
    assert r.returncode != 0 and "nothing to search" in r.stderr
