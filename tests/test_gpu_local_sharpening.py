"""GPU parity of xmipp_volume_local_sharpening (xh_ldb_*, LocalDeblur in api.py) against the numpy fp64 restatement of the reference
(tests/local_sharpening_ref.py): the side info, one localfiltering call, the batch seams, the full iteration, and the program end to end.
The inputs are the restatement's seeded synthetic volume and resolution map (24 x 20 x 18 and 21^3: non-cubic, odd, no powers of two).
The restatement of a shape is computed once and shared.

The bound of 1e-10 of the restatement's maximum is the one test_gpu_monores.py and the halves tests hold the same fp64 transforms to. The
iteration does not amplify rounding: 1e-15 of relative noise on every inverse transform of the restatement moves the final map by
5e-16 of its maximum (R.run(..., perturb=...))."""
import os
import subprocess

import numpy as np
import pytest

from tests import local_sharpening_ref as R
from tests import xmipp_io

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PROG = os.path.join(ROOT, "xmipp3_amd", "bin", "xmipp_volume_local_sharpening")
SHAPES = [(24, 20, 18), (21, 21, 21)]
SAMPLING, K = 1.0, 0.025


@pytest.fixture(scope="module")
def gpu():
    import torch
    import xmipp3_amd as xa
    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    return xa, xa.Context(0), torch


_IN, _REF, _LF = {}, {}, {}


def inputs(shape):
    """the synthetic pair as a float file stores it, so that the program reads the same numbers"""
    if shape not in _IN:
        v, rm = R.synth(shape, 7)
        _IN[shape] = (v.astype(np.float32).astype(np.float64), rm.astype(np.float32).astype(np.float64))
    return _IN[shape]


def ref_run(shape, lam=1.0, niter=50):
    key = (shape, lam, niter)
    if key not in _REF:
        v, rm = inputs(shape)
        _REF[key] = R.run(v, rm, SAMPLING, lam, K, niter)
    return _REF[key]


def ref_localfilter(shape):
    if shape not in _LF:
        v, _ = inputs(shape)
        ref = ref_run(shape)
        _LF[shape] = R.localfilter(v, ref["res"], SAMPLING, K, ref["bands"])
    return _LF[shape]


def loaded(gpu, shape, batch=8):
    xa, ctx, torch = gpu
    v, rm = inputs(shape)
    m = xa.LocalDeblur(ctx, shape, batch=batch)
    m.load(torch.from_numpy(v).cuda(), torch.from_numpy(rm).cuda(), SAMPLING, K)
    return m


# ---------------------------------------------------------------- side info
@pytest.mark.parametrize("shape", SHAPES)
def test_side_info(gpu, shape):
    xa, ctx, torch = gpu
    v, rm = inputs(shape)
    # some voxels inside (0, 2 sampling) for the clamp, one above the synthetic maximum that the clamp must not hide from maxRes
    rm = rm.copy()
    rm[shape[0] // 2, shape[1] // 2, shape[2] // 2 - 2:shape[2] // 2 + 2] = [0.5, 1.999, 1e-30, 7.25]
    exp = R.side_info(v, rm, SAMPLING)
    assert int(((rm > 0) & (rm < 2)).sum()) == 3
    m = xa.LocalDeblur(ctx, shape)
    m.load(torch.from_numpy(v).cuda(), torch.from_numpy(rm).cuda(), SAMPLING, K)
    info = m.info()
    got = m.resmap().cpu().numpy()
    assert info["maxRes"] == exp["maxRes"] == 7.25
    assert np.array_equal(got, exp["res"])
    assert np.array_equal(got < 2 * SAMPLING, exp["outside"]) and info["noutside"] == int(exp["outside"].sum()) > 1
    assert abs(info["desvOutside"] - exp["desvOutside"]) <= 1e-12 * exp["desvOutside"]
    bl = R.bands(shape[0], SAMPLING, exp["maxRes"] + 2)
    assert [(b["res"], b["w"], b["wL"], b["idx"]) for b in info["bands"]] == bl


def test_one_outside_voxel_gives_a_deviation_of_zero(gpu):
    xa, ctx, torch = gpu
    shape = SHAPES[0]
    v, _ = inputs(shape)
    rm = np.full(shape, 5.0)
    rm[1, 2, 3] = 0.0
    assert R.side_info(v, rm, SAMPLING)["desvOutside"] == 0.0
    m = xa.LocalDeblur(ctx, shape)
    m.load(torch.from_numpy(v).cuda(), torch.from_numpy(rm).cuda(), SAMPLING, K)
    info = m.info()
    assert info["noutside"] == 1 and info["desvOutside"] == 0.0 and info["maxRes"] == 5.0


# ---------------------------------------------------------------- one localfiltering call
@pytest.mark.parametrize("shape", SHAPES)
def test_localfilter(gpu, shape):
    xa, ctx, torch = gpu
    v, _ = inputs(shape)
    ref = ref_run(shape)
    exp = ref_localfilter(shape)
    m = loaded(gpu, shape)
    bands = m.info()["bands"]
    # a band that skips nothing and one that skips most lines
    assert any(b["wL"] > 0.5 and b["kcount"] == shape[0] and b["jcount"] == shape[2] // 2 + 1 for b in bands)
    low = [b for b in bands if b["wL"] < 0.2]
    assert low and all(b["kcount"] * b["jcount"] < 0.5 * shape[0] * (shape[2] // 2 + 1) for b in low)
    got = m.localfilter(torch.from_numpy(v).cuda()).cpu().numpy()
    err = float(np.abs(got - exp).max() / np.abs(exp).max())
    print(f"localfilter {shape}: {len(bands)} bands, error {err:.3e} of the maximum")
    assert err <= 1e-10
    assert ref["outside"].sum() > 0 and not got[ref["outside"]].any()


def test_kept_line_table_never_drops_a_line_with_a_band_element(gpu):
    """the table against the band test itself, over every band of both shapes and of a finer sampling"""
    xa, ctx, torch = gpu
    for shape in SHAPES:
        un = R.un_map(shape)
        Z, Y, X = shape
        kk = np.minimum(np.arange(Z), Z - np.arange(Z))[:, None, None]
        jj = np.arange(X // 2 + 1)[None, None, :]
        for b in loaded(gpu, shape).info()["bands"]:
            delta = b["wL"] - b["w"]
            passing = (un >= b["w"] - delta) & (un <= b["wL"])
            kmax = (b["kcount"] - 1) // 2 if b["kcount"] < Z else Z
            assert not (passing & ((kk > kmax) | (jj >= b["jcount"]))).any(), (shape, b)


def test_batch_seams_give_the_same_bytes(gpu):
    xa, ctx, torch = gpu
    shape = SHAPES[0]
    v, _ = inputs(shape)
    dv = torch.from_numpy(v).cuda()
    nb = len(ref_run(shape)["bands"])
    assert 8 < nb < 16
    out = {b: loaded(gpu, shape, batch=b).localfilter(dv).cpu().numpy().tobytes() for b in (1, 3, 4, 8, 16)}
    for b in (3, 4, 8, 16):
        assert out[b] == out[1], b


# ---------------------------------------------------------------- the full run
@pytest.mark.parametrize("shape", SHAPES)
def test_full_run(gpu, shape):
    ref = ref_run(shape)
    # a condition on the input: no iteration of the restatement sits on the stop rule's threshold
    assert all(abs(r["subst"] - 1) >= 1e-3 for r in ref["records"])
    assert ref["stopped"] and 3 < ref["iterations"] < 50
    m = loaded(gpu, shape)
    got, lam, its = m.run(1.0, 50)
    assert len(its) == ref["iterations"] and [r["stop"] for r in its] == [r["stop"] for r in ref["records"]] and its[-1]["stop"]
    assert abs(lam - ref["lambda"]) <= 1e-12 * ref["lambda"] and lam != 1.0
    for g, e in zip(its, ref["records"]):
        assert abs(g["norm"] - e["norm"]) <= 1e-10 * e["norm"]
    err = float(np.abs(got.cpu().numpy() - ref["sharpened"]).max() / np.abs(ref["sharpened"]).max())
    print(f"run {shape}: {len(its)} iterations, lambda {lam:.6f}, error {err:.3e} of the maximum")
    assert err <= 1e-10
    assert (ref["sharpened"] == -4 * ref["desvOutside"]).any()           # the floor was reached


@pytest.mark.parametrize("niter", [3, 2])
def test_fixed_lambda_ends_by_count(gpu, niter):
    """no estimate of lambda, and the loop runs out of iterations: with 2 the stop rule cannot fire (i > 2), with 3 the restatement sets
    the flag in the last iteration, which changes nothing. The map is returned either way"""
    shape = SHAPES[0]
    ref = ref_run(shape, 0.5, niter)
    assert ref["iterations"] == niter and ref["lambda"] == 0.5 and ref["stopped"] == (niter == 3)
    assert all(abs(r["subst"] - 1) >= 1e-3 for r in ref["records"])
    got, lam, its = loaded(gpu, shape).run(0.5, niter)
    assert lam == 0.5 and len(its) == niter and [r["stop"] for r in its] == [r["stop"] for r in ref["records"]]
    err = float(np.abs(got.cpu().numpy() - ref["sharpened"]).max() / np.abs(ref["sharpened"]).max())
    print(f"fixed lambda {shape}, {niter} iterations: error {err:.3e} of the maximum")
    assert err <= 1e-10


def test_two_runs_give_the_same_bytes(gpu):
    shape = SHAPES[1]
    a, la, ia = loaded(gpu, shape).run(1.0, 50)
    b, lb, ib = loaded(gpu, shape).run(1.0, 50)
    assert a.cpu().numpy().tobytes() == b.cpu().numpy().tobytes() and la == lb and ia == ib


def test_refusals(gpu):
    xa, ctx, torch = gpu
    shape = SHAPES[0]
    v, rm = inputs(shape)
    dv, dr = torch.from_numpy(v).cuda(), torch.from_numpy(rm).cuda()
    m = xa.LocalDeblur(ctx, shape)
    with pytest.raises(xa.XhError, match="nothing is loaded"):
        m.run()
    with pytest.raises(xa.XhError, match="no voxel at or above"):
        m.load(dv, torch.from_numpy(np.minimum(rm, 0.0) - (rm == 0)).cuda(), SAMPLING, K)
    with pytest.raises(xa.XhError, match="sampling"):
        m.load(dv, dr, 0.1, K)
    with pytest.raises(xa.XhError, match="shape"):
        m.load(dv, torch.zeros((24, 20, 16), dtype=torch.float64, device="cuda"), SAMPLING, K)
    m.load(dv, dr, SAMPLING, K)
    with pytest.raises(xa.XhError, match="never be assigned"):
        m.run(1.0, 0)


# ---------------------------------------------------------------- the program
def test_program_writes_what_the_api_returns(gpu, tmp_path):
    shape = SHAPES[0]
    v, rm = inputs(shape)
    got, lam, its = loaded(gpu, shape).run(1.0, 50)
    xmipp_io.write_volume(str(tmp_path / "v.vol"), v)
    xmipp_io.write_volume(str(tmp_path / "res.vol"), rm)
    args = ["--vol", str(tmp_path / "v.vol"), "--resolution_map", str(tmp_path / "res.vol"), "--sampling", "1", "-o", str(tmp_path / "sharp.vol"), "--md",
            str(tmp_path / "params.xmd"), "-n", "3"]
    r = subprocess.run([PROG] + args, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=120)
    assert r.returncode == 0, r.stderr
    assert np.array_equal(xmipp_io.read_volume(str(tmp_path / "sharp.vol")), got.cpu().numpy().astype(np.float32))
    labels, rows = xmipp_io.read_xmd(str(tmp_path / "params.xmd"))
    assert labels == ["iterationNumber", "cost"] and len(rows) == 1
    assert int(rows[0][0]) == len(its) and rows[0][1] == "%.6f" % lam
