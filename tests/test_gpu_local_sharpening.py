"""GPU parity of xmipp_volume_local_sharpening (xh_ldb_*, LocalDeblur in api.py) against the numpy fp64 restatement of the reference
(tests/local_sharpening_ref.py): the side info, one localfiltering call, the batch seams, the full iteration, and the program end to end.
The inputs are the restatement's seeded synthetic volume and resolution map: at 24 x 20 x 18 and 21^3 (non-cubic, odd, no powers of
two), and at the shapes of tests/volume_tiles.py, where the kernels of xh_ldb.hip leave the tile of those two (power-of-two lines, two
to four outputs per thread in k_ldb_rows, fewer than 8 rows or lines per workgroup, one pair per LDS chunk, 64 KiB of LDS in the line
passes, a second lap of the grid-stride loops). The map is 0 outside a small sphere and such voxels are 0 on both sides, so the tests
count from the input the compared voxels per register slot and in the tail workgroup, and the shapes with a tail also run on the pair
rolled until its sphere lies on the last rows. The restatement of a case is computed once and shared.

The bound of 1e-10 of the restatement's maximum is the one test_gpu_monores.py and the halves tests hold the same fp64 transforms to. The
iteration does not amplify rounding: 1e-15 of relative noise on every inverse transform of the restatement moves the final map by
5e-16 of its maximum (R.run(..., perturb=...))."""
import os
import subprocess

import numpy as np
import pytest

from tests import local_sharpening_ref as R
from tests import volume_tiles as T
from tests import xmipp_io

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PROG = os.path.join(ROOT, "xmipp3_amd", "bin", "xmipp_volume_local_sharpening")
SHAPES = [(24, 20, 18), (21, 21, 21)]
ALL_SHAPES = SHAPES + T.TILE_SHAPES          # what each of T.TILE_SHAPES reaches: tests/volume_tiles.py, asserted by tests/test_volume_tiles.py
BIG = T.BIG
SAMPLING, K = 1.0, 0.025


@pytest.fixture(scope="module")
def gpu():
    import torch
    import xmipp3_amd as xa
    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    return xa, xa.Context(0), torch


_IN, _SIDE, _REF, _LF = {}, {}, {}, {}
NO_ROLL = (0, 0, 0)
# the shapes whose last workgroup of k_ldb_rows is a tail (nr < rpb), on the pair rolled so that the tail rows and every register slot
# hold voxels of the inside set (T.ROLLS): on the pair as synthesised those rows lie outside the map's sphere and compare 0 with 0
ROLLED = [(s, T.ROLLS[s]) for s in ((21, 21, 21), T.X160, T.X300)]


def inputs(shape, sampling=SAMPLING, roll=NO_ROLL):
    """the synthetic pair as a float file stores it, so that the program reads the same numbers. The map is in the units of sampling 1:
    at another sampling rate it is multiplied by the rate. roll: circular steps along (z, y, x), the same for both volumes"""
    key = (shape, sampling, roll)
    if key not in _IN:
        v, rm = (np.roll(a, roll, axis=(0, 1, 2)) for a in R.synth(shape, 7))
        _IN[key] = (v.astype(np.float32).astype(np.float64), (rm * sampling).astype(np.float32).astype(np.float64))
    return _IN[key]


def ref_side(shape, sampling=SAMPLING, roll=NO_ROLL):
    """the side info and the band list of run (:297-298)"""
    key = (shape, sampling, roll)
    if key not in _SIDE:
        v, rm = inputs(shape, sampling, roll)
        side = R.side_info(v, rm, sampling)
        side["bands"] = R.bands(shape[0], sampling, side["maxRes"] + 2)
        _SIDE[key] = side
    return _SIDE[key]


def ref_run(shape, lam=1.0, niter=50, sampling=SAMPLING, k=K, roll=NO_ROLL):
    key = (shape, lam, niter, sampling, k, roll)
    if key not in _REF:
        v, rm = inputs(shape, sampling, roll)
        _REF[key] = R.run(v, rm, sampling, lam, k, niter)
    return _REF[key]


def ref_localfilter(shape, roll=NO_ROLL):
    key = (shape, roll)
    if key not in _LF:
        v, _ = inputs(shape, roll=roll)
        side = ref_side(shape, roll=roll)
        _LF[key] = R.localfilter(v, side["res"], SAMPLING, K, side["bands"])
    return _LF[key]


def loaded(gpu, shape, batch=8, sampling=SAMPLING, k=K, roll=NO_ROLL):
    xa, ctx, torch = gpu
    v, rm = inputs(shape, sampling, roll)
    m = xa.LocalDeblur(ctx, shape, batch=batch)
    m.load(torch.from_numpy(v).cuda(), torch.from_numpy(rm).cuda(), sampling, k)
    return m


def compared(shape, roll=NO_ROLL):
    """the voxels of the inside set per register slot of k_ldb_rows and in its tail workgroup (T.ldb_compared), from the input used"""
    return T.ldb_compared(shape, ~ref_side(shape, roll=roll)["outside"])


@pytest.fixture(scope="module")
def big(gpu):
    """BIG takes the loops over the half spectrum (k_ldb_split) into a second lap: more elements than the grid cap has threads"""
    xa, ctx, torch = gpu
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    NF = T.tiling(BIG).NF
    print(f"{BIG}: {NF} half-spectrum elements on {cus} CUs, grid cap {256 * 4 * cus} threads")
    assert NF > 256 * 4 * cus, f"{NF} half-spectrum elements do not exceed the grid cap of {256 * 4 * cus} threads on {cus} CUs"
    return BIG


# ---------------------------------------------------------------- side info
def _check_side_info(gpu, shape, sampling, planted):
    """planted: three values inside (0, 2 sampling) for the clamp, one above the synthetic maximum that the clamp must not hide from maxRes"""
    xa, ctx, torch = gpu
    v, rm = inputs(shape, sampling)
    rm = rm.copy()
    assert planted[3] > rm.max()
    rm[shape[0] // 2, shape[1] // 2, shape[2] // 2 - 2:shape[2] // 2 + 2] = planted
    exp = R.side_info(v, rm, sampling)
    assert int(((rm > 0) & (rm < 2 * sampling)).sum()) == 3
    m = xa.LocalDeblur(ctx, shape)
    m.load(torch.from_numpy(v).cuda(), torch.from_numpy(rm).cuda(), sampling, K)
    info = m.info()
    got = m.resmap().cpu().numpy()
    assert info["maxRes"] == exp["maxRes"] == planted[3]
    assert np.array_equal(got, exp["res"])
    assert int((got == 2 * sampling).sum()) >= 3
    assert np.array_equal(got < 2 * sampling, exp["outside"]) and info["noutside"] == int(exp["outside"].sum()) > 1
    assert abs(info["desvOutside"] - exp["desvOutside"]) <= 1e-12 * exp["desvOutside"]
    bl = R.bands(shape[0], sampling, exp["maxRes"] + 2)
    assert [(b["res"], b["w"], b["wL"], b["idx"]) for b in info["bands"]] == bl


@pytest.mark.parametrize("shape", SHAPES)
def test_side_info(gpu, shape):
    _check_side_info(gpu, shape, SAMPLING, [0.5, 1.999, 1e-30, 7.25])


def test_side_info_at_another_sampling(gpu):
    """2 sampling is the clamp, the outside set and the first band at once: here it is 3.0, not the 2.0 of every other test"""
    _check_side_info(gpu, SHAPES[1], 1.5, [0.5, 2.999, 1e-30, 11.25])


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
def _check_localfilter(gpu, shape, roll=NO_ROLL):
    xa, ctx, torch = gpu
    v, _ = inputs(shape, roll=roll)
    side = ref_side(shape, roll=roll)
    exp = ref_localfilter(shape, roll)
    m = loaded(gpu, shape, roll=roll)
    # what of k_ldb_rows this input compares: a voxel of the outside set is 0 on both sides whatever its workgroup did
    per_slot, tail = compared(shape, roll)
    print(f"localfilter {shape} roll {roll}: compared voxels per register slot {per_slot}, in the tail workgroup {tail}")
    if roll != NO_ROLL:
        assert tail > 0 and all(c > 0 for c in per_slot)
    elif shape != T.X300:
        # as synthesised, X300's slot 3 (row 2 of a workgroup, x >= 168) lies beside the sphere: its rolled case fills it
        assert all(c > 0 for c in per_slot)
    bands = m.info()["bands"]
    assert len(bands) == len(side["bands"])
    # a band that skips nothing and one that skips most lines. Both hold at every shape of this file: the first band's wL is
    # sampling / (2 sampling - 0.2) > 0.5 whatever the size, and below wL = 0.2 the table keeps at most 0.23 of the lines
    assert any(b["wL"] > 0.5 and b["kcount"] == shape[0] and b["jcount"] == shape[2] // 2 + 1 for b in bands)
    low = [b for b in bands if b["wL"] < 0.2]
    assert low and all(b["kcount"] * b["jcount"] < 0.5 * shape[0] * (shape[2] // 2 + 1) for b in low)
    got = m.localfilter(torch.from_numpy(v).cuda()).cpu().numpy()
    err = float(np.abs(got - exp).max() / np.abs(exp).max())
    print(f"localfilter {shape} roll {roll}: {len(bands)} bands, error {err:.3e} of the maximum")
    assert err <= 1e-10
    assert side["outside"].sum() > 0 and not got[side["outside"]].any()


@pytest.mark.parametrize("shape", ALL_SHAPES)
def test_localfilter(gpu, shape):
    _check_localfilter(gpu, shape)


@pytest.mark.parametrize("shape,roll", ROLLED)
def test_localfilter_compares_the_tail_rows(gpu, shape, roll):
    """the tail workgroup of k_ldb_rows (nr < rpb: 1 of 8 rows, 3 of 6, 2 of 3) and every register slot on voxels that are compared"""
    _check_localfilter(gpu, shape, roll)


def test_localfilter_past_the_grid_cap(gpu, big):
    """a second lap of k_ldb_split's grid-stride loop"""
    _check_localfilter(gpu, big)


def test_kept_line_table_never_drops_a_line_with_a_band_element(gpu):
    """the table against the band test itself, over every band of every shape and of a finer sampling"""
    xa, ctx, torch = gpu
    for shape in ALL_SHAPES:
        un = R.un_map(shape)
        Z, Y, X = shape
        kk = np.minimum(np.arange(Z), Z - np.arange(Z))[:, None, None]
        jj = np.arange(X // 2 + 1)[None, None, :]
        for sampling in (SAMPLING, 0.8):
            bands = loaded(gpu, shape, sampling=sampling).info()["bands"]
            assert len(bands) == len(ref_side(shape, sampling)["bands"]) >= 9
            for b in bands:
                delta = b["wL"] - b["w"]
                passing = (un >= b["w"] - delta) & (un <= b["wL"])
                kmax = (b["kcount"] - 1) // 2 if b["kcount"] < Z else Z
                assert not (passing & ((kk > kmax) | (jj >= b["jcount"]))).any(), (shape, sampling, b)


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


@pytest.mark.parametrize("shape,batches,roll", [(T.X160, (1, 2, 8, 16), NO_ROLL), (T.Z260, (1, 3, 8, 64), NO_ROLL),
                                                (T.X160, (1, 2, 8, 16), T.ROLLS[T.X160])])
def test_batch_seams_at_the_tile_edges(gpu, shape, batches, roll):
    """X160: ppc is 1 at every batch, so the pairs of a batch go through LDS one after the other (the p0 loop of k_ldb_rows, its second
    __syncthreads, the reuse of LDS between chunks) while the number of chunks per launch changes with the batch. Z260: 33 bands, so
    with nbuf 4 the ninth batch holds one band and the odd-nb path runs without a partner; with 64 one batch holds them all. The rolled
    X160 has compared voxels in the tail workgroup, whose chunks reuse LDS like any other's"""
    xa, ctx, torch = gpu
    v, _ = inputs(shape, roll=roll)
    dv = torch.from_numpy(v).cuda()
    nb = len(ref_side(shape, roll=roll)["bands"])
    assert roll == NO_ROLL or compared(shape, roll)[1] > 0
    if shape == T.X160:
        assert all(T.tiling(shape, b).ppc == 1 for b in batches) and nb > 8
    else:
        assert nb == 33 and nb % T.tiling(shape, 3).nbuf == 1 and nb % T.tiling(shape, 8).nbuf == 1 and nb < T.tiling(shape, 64).nbuf
    out = {b: loaded(gpu, shape, batch=b, roll=roll).localfilter(dv).cpu().numpy().tobytes() for b in batches}
    for b in batches[1:]:
        assert out[b] == out[1], b


# ---------------------------------------------------------------- the full run
def _check_full_run(gpu, shape, sampling=SAMPLING, k=K, roll=NO_ROLL):
    ref = ref_run(shape, sampling=sampling, k=k, roll=roll)
    # a condition on the input: no iteration of the restatement sits on the stop rule's threshold
    margin = min(abs(r["subst"] - 1) for r in ref["records"])
    assert margin >= 1e-3
    assert ref["stopped"] and 3 < ref["iterations"] < 50
    m = loaded(gpu, shape, sampling=sampling, k=k, roll=roll)
    got, lam, its = m.run(1.0, 50)
    assert len(its) == ref["iterations"] and [r["stop"] for r in its] == [r["stop"] for r in ref["records"]] and its[-1]["stop"]
    assert abs(lam - ref["lambda"]) <= 1e-12 * ref["lambda"] and lam != 1.0
    for g, e in zip(its, ref["records"]):
        assert abs(g["norm"] - e["norm"]) <= 1e-10 * e["norm"]
    err = float(np.abs(got.cpu().numpy() - ref["sharpened"]).max() / np.abs(ref["sharpened"]).max())
    print(f"run {shape} roll {roll} sampling {sampling} K {k}: {len(ref['bands'])} bands, {len(its)} iterations (margin {margin:.3f}), lambda {lam:.6f}, "
          f"error {err:.3e} of the maximum")
    assert err <= 1e-10
    assert (ref["sharpened"] == -4 * ref["desvOutside"]).any()           # the floor was reached


@pytest.mark.parametrize("shape", ALL_SHAPES)
def test_full_run(gpu, shape):
    _check_full_run(gpu, shape)


@pytest.mark.parametrize("shape,roll", ROLLED[1:])
def test_full_run_compares_the_tail_rows(gpu, shape, roll):
    """the iteration with the tail workgroup of k_ldb_rows at rpb = 6 and 3 on compared voxels"""
    per_slot, tail = compared(shape, roll)
    assert tail > 0 and all(c > 0 for c in per_slot)
    _check_full_run(gpu, shape, roll=roll)


@pytest.mark.parametrize("shape,sampling,k", [((21, 21, 21), 1.5, 0.05), ((24, 20, 18), 0.8, 0.01)])
def test_full_run_at_other_constants(gpu, shape, sampling, k):
    """every other device test runs at sampling 1 and K = 0.025; the map is in the units of the sampling rate"""
    _check_full_run(gpu, shape, sampling, k)


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


def test_timed_run_changes_no_byte(gpu):
    """set_timing(True) puts a wait after every stage: the map, lambda and the records keep their bytes, the five stages report times,
    and set_timing resets them"""
    xa = gpu[0]
    m = loaded(gpu, SHAPES[0])
    out, lam, its = m.run(0.5, 3)
    assert set(m.stage_ms().values()) == {0.0}                  # an untimed run reports nothing
    m.set_timing(True)
    out_t, lam_t, its_t = m.run(0.5, 3)
    ms = m.stage_ms()
    print(f"stage ms: {ms}")
    assert out_t.cpu().numpy().tobytes() == out.cpu().numpy().tobytes() and lam_t == lam and its_t == its
    assert list(ms) == list(xa.LocalDeblur.STAGES) and len(ms) == 5
    assert all(v >= 0.0 for v in ms.values()) and sum(ms.values()) > 0.0
    m.set_timing(False)
    assert set(m.stage_ms().values()) == {0.0}
    out_u, lam_u, its_u = m.run(0.5, 3)
    assert out_u.cpu().numpy().tobytes() == out.cpu().numpy().tobytes() and lam_u == lam and its_u == its
    assert set(m.stage_ms().values()) == {0.0}
    m.close()


def test_two_iterations_past_the_grid_cap(gpu, big):
    """four operators at BIG with a fixed lambda (a 50-iteration run at this size belongs to no test), and the same bytes twice"""
    ref = ref_run(big, 0.5, 2)
    assert ref["iterations"] == 2 and not ref["stopped"]
    got, lam, its = loaded(gpu, big).run(0.5, 2)
    assert lam == 0.5 and len(its) == 2 and not its[-1]["stop"]
    for g, e in zip(its, ref["records"]):
        assert abs(g["norm"] - e["norm"]) <= 1e-10 * e["norm"]
    err = float(np.abs(got.cpu().numpy() - ref["sharpened"]).max() / np.abs(ref["sharpened"]).max())
    print(f"fixed lambda {big}, 2 iterations: error {err:.3e} of the maximum")
    assert err <= 1e-10
    again, _, its2 = loaded(gpu, big).run(0.5, 2)
    assert again.cpu().numpy().tobytes() == got.cpu().numpy().tobytes() and its2 == its


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
