"""CPU checks of xmipp_forward_art_zernike3d: the order of presentation against a numpy restatement of the reference's sortOrthogonal
(reconstruction_adapt_cuda11/forward_art_zernike3d_gpu.cpp:628-690), the schedule of --save_iter (:587-592), the program's defaults and
help, and the refusals that happen before any device is touched: degrees the basis is not written out for, a coefficient vector of the
wrong length, metadata without angles."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from tests import xmipp_io

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PROG = os.path.join(ROOT, "xmipp3_amd", "bin", "xmipp_forward_art_zernike3d")
XH_ERR_UNSUPPORTED = -5
ERR_ARG_INCORRECT, ERR_MD_MISSINGLABEL = 2, 32


@pytest.fixture(scope="module")
def xa():
    import __graft_entry__ as g
    g.build()
    assert os.path.exists(PROG)
    import xmipp3_amd
    return xmipp3_amd


def sort_orthogonal_ref(oracle, rot, tilt, sort_last):
    """sortOrthogonal (:628-690): `product` starts at zero and keeps accumulating over the rounds; ties go to the lowest index"""
    n = len(rot)
    v = np.array([oracle.euler_matrix(rot[i], tilt[i], 0.0)[2] for i in range(n)])
    chosen = np.zeros(n, bool)
    product = np.zeros(n)
    order = np.zeros(n, np.int32)
    chosen[0] = True
    min_prod_proj = 0
    for i in range(1, n):
        min_prod = float(np.finfo(np.float32).max)          # MAXFLOAT
        rowi_1 = v[order[i - 1]]
        drop = sort_last != -1 and i > sort_last
        if drop:
            rowi_N_1 = v[order[i - sort_last - 1]]
        for j in range(n):
            if chosen[j]:
                continue
            product[j] += abs(float(np.dot(rowi_1, v[j])))
            if drop:
                product[j] -= abs(float(np.dot(rowi_N_1, v[j])))
            if product[j] < min_prod:
                min_prod, min_prod_proj = product[j], j
        order[i] = min_prod_proj
        chosen[min_prod_proj] = True
    return order


@pytest.mark.parametrize("sort_last", [2, 5, -1])
def test_sort_orthogonal(xa, oracle, sort_last):
    rng = np.random.default_rng(7)
    rot, tilt = rng.uniform(-180, 180, 40), rng.uniform(0, 180, 40)
    got = xa.faz_sort_orthogonal(rot, tilt, sort_last)
    want = sort_orthogonal_ref(oracle, rot, tilt, sort_last)
    assert got.dtype == np.int32 and sorted(got) == list(range(40)) and got[0] == 0
    assert np.array_equal(got, want)
    # the case is what it says: the three settings give three orders
    assert not np.array_equal(got, xa.faz_sort_orthogonal(rot, tilt, {2: 5, 5: -1, -1: 2}[sort_last]))


def save_schedule_ref(n, s):
    """run() :554, :587-592: current_save_iter starts at 1, is compared after every image, reset to 1 on a save and incremented always"""
    flags, cur = [], 1
    for _ in range(n):
        hit = cur == s and s > 0
        if hit:
            cur = 1
        flags.append(int(hit))
        cur += 1
    return flags


@pytest.mark.parametrize("s,images", [(1, [1]), (2, [2, 3, 4, 5, 6, 7, 8, 9, 10]), (3, [3, 5, 7, 9])])
def test_save_schedule(xa, s, images):
    got = xa.faz_save_schedule(10, s)
    assert list(got) == save_schedule_ref(10, s)
    # the first after s images, then every s - 1
    assert [k + 1 for k in np.flatnonzero(got)] == images
    assert not xa.faz_save_schedule(10, 0).any()


def test_defaults(xa):
    from xmipp3_amd._lib import FazParams
    p = FazParams()
    xa.lib().xh_faz_defaults(C.byref(p))
    assert (p.RDef, p.sampling, p.lambda_, p.ltv, p.ltk, p.ll1, p.lst) == (-1.0, 1.0, 0.01, 1e-4, 1e-4, 1e-4, 1e-4)
    assert (p.l1, p.l2, p.step, p.use_zernike, p.use_ctf, p.phase_flipped) == (3, 2, 1, 0, 0, 0)


def test_unsupported_degrees_and_coefficient_count(xa):
    L = xa.lib()
    assert L.xh_faz_check(6, 2, -1) == XH_ERR_UNSUPPORTED and b"not supported" in L.xh_last_error()
    assert L.xh_faz_check(3, 5, -1) == XH_ERR_UNSUPPORTED
    vec = xa.vds_num_terms(3, 2)
    assert L.xh_faz_check(3, 2, 3 * vec) == 0 and L.xh_faz_check(3, 2, -1) == 0
    assert L.xh_faz_check(3, 2, 3 * vec + 8) != 0
    msg = L.xh_last_error().decode()
    assert str(3 * vec + 8) in msg and str(3 * vec) in msg


def _run(args, cwd=None):
    return subprocess.run([PROG] + args, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=120, cwd=cwd)


OPTIONS = ["-i", "-o", "--ref", "--maskf", "--maskb", "--odir", "--sampling", "--RDef", "--l1", "--l2", "--blobr", "--step", "--sigma", "--mr", "--dSize",
           "--ltv", "--ltk", "--ll1", "--lst", "--sym", "--useZernike", "--useCTF", "--phaseFlipped", "--regularization", "--niter", "--debug_iter",
           "--onlyPositive", "--save_iter", "--sort_last", "--sort_random", "--resume", "--dev"]


def test_program_help(xa):
    r = _run(["--help"])
    assert r.returncode == 0
    for flag in OPTIONS:
        assert flag in r.stderr, flag
    for defaults in ("--odir <=.>", "--sampling <=1>", "--RDef <=-1>", "--l1 <=3>", "--l2 <=2>", "--blobr <=4>", "--step <=1>", "--sigma <=2>", "--mr <=0>",
                     "--dSize <=0>", "--ltv <=1e-4>", "--ltk <=1e-4>", "--ll1 <=1e-4>", "--lst <=1e-4>", "--sym <=c1>", "--regularization <=0.01>",
                     "--niter <=1>", "--save_iter <=0>", "--sort_last <=2>", "--dev <=0>"):
        assert defaults in r.stderr, defaults


def _table(tmp_path, labels, rows):
    xmipp_io.write_stack(str(tmp_path / "in.stk"), np.zeros((len(rows), 16, 16), np.float32))
    xmipp_io.write_xmd(str(tmp_path / "in.xmd"), [("noname", ["image"] + labels, [[f"{q + 1}@{tmp_path / 'in.stk'}"] + r for q, r in enumerate(rows)])])
    return ["-i", str(tmp_path / "in.xmd"), "-o", "out.vol", "--odir", str(tmp_path)]


def test_program_refusals_before_a_device(xa, tmp_path):
    r = _run(["-i", "a.xmd", "-o", "b.vol", "--l1", "6", "--l2", "2"])
    assert r.returncode == ERR_ARG_INCORRECT and "l1 = 6" in r.stderr and "not supported" in r.stderr
    r = _run(["-i", "a.xmd", "-o", "b.vol", "--dev", "0", "1"])
    assert r.returncode != 0 and "several devices" in r.stderr
    # metadata without angles
    args = _table(tmp_path, ["shiftX", "shiftY"], [[0.0, 0.0], [1.0, 0.5]])
    r = _run(args)
    assert r.returncode == ERR_MD_MISSINGLABEL and "projection angles are missing" in r.stderr
    # a coefficient vector of the wrong length: the 3 vecSize + 8 variables of the alignment program's search, as that program writes them
    vec = xa.vds_num_terms(3, 2)
    good = "[ " + " ".join("0.010000" for _ in range(3 * vec)) + " ]"
    bad = "[ " + " ".join("0.010000" for _ in range(3 * vec + 8)) + " ]"

    def raw_table(vectors):
        with open(tmp_path / "in.xmd", "w") as f:
            f.write("# XMIPP_STAR_1 * \n# \ndata_noname\nloop_\n _image\n _angleRot\n _angleTilt\n _anglePsi\n _sphCoefficients\n _cost\n")
            for q, v in enumerate(vectors):
                f.write(f" {q + 1}@{tmp_path / 'in.stk'} 10.0 20.0 30.0 {v} 0.5 \n")
    raw_table([good, bad])
    r = _run(args + ["--useZernike"])
    assert r.returncode == ERR_ARG_INCORRECT and "row 2" in r.stderr and str(3 * vec + 8) in r.stderr and f"= {3 * vec}" in r.stderr
    assert not os.path.exists(tmp_path / "out.vol")
