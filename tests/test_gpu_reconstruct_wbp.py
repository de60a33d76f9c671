"""GPU parity of xmipp_reconstruct_wbp (xh_wbp_*, ReconstructWbp in api.py) against the numpy fp64 restatement
(tests/reconstruct_wbp_ref.py): the filtered images, the volume, count_thr and the set of voxels outside every cut of every case, the
filter's weights and the sinc table, independence of the batch capacity, run-to-run identity, and the program end to end.

Cases (R.cases()): D = 16 (aligned), 17 (odd: dim2, the odd CenterFFT, no unpaired row), 20 (Bluestein lines) and 33 (a remainder on
every tile); 1, 5 and 37 images; direction lists of 255, 256, 257 and 530 entries around the filter kernel's LDS tile of 256 directions
(xmipp3_amd.wbp_tile(), asserted below), and --use_each_image lists of 37, 20 and, with c3, 111; the default radius and 5; zero shifts
(the identity copy), fractional shifts, shifts larger than D (wrap) and flips, one of them with zero shifts; weights 0.5 and 3 (a weight of
0 never reaches the device: the program removes those rows, tests/test_reconstruct_wbp_host.py); c3 and d2 under --use_each_image; the
default threshold and 0.2, under which 1074 and 9328 cells take the threshold branch; sampled mode at --filsam 15 with weights (18
directions, the counts truncated). Every case runs at capacities 1, 4 and 64 and a
second time at 64: the same bytes.

Bound: 1e-14 of the largest value, for the volume and for the filtered images. It is not taken from the device:
tests/test_reconstruct_wbp_ref.py derives it as 16 times the largest relative difference (5.9e-16, filtered images of the 33-pixel
case with 257 directions; volumes 4.2e-16) between the restatement and the same per-term values summed with math.fsum (the transforms in
extended precision), rounded up to a power of ten, and asserts the preconditions of every case on the restatement alone: 0 cells and 0
voxels are left out. count_thr and the voxels outside every cut: exact equality. The program's volume file holds 32-bit floats, so half
an ulp of the largest value is added there.
Measured on one MI355X, largest over the cases: filtered images 2.6e-15 (d20_each_wrap_r5), volumes 2.8e-15 (d16_each_c3, through the
symmetrisation; without symmetry 1.1e-15), the weights and the sinc table bit-equal, count_thr equal (0 to 9 328), the program's float32
volume 3.5e-8 of the largest value; the same bytes at every capacity and from the second run."""
import os
import subprocess

import numpy as np
import pytest

from tests import reconstruct_wbp_ref as R
from tests import xmipp_io

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PROG = os.path.join(ROOT, "xmipp3_amd", "bin", "xmipp_reconstruct_wbp")
BOUND = 1e-14
CASES = R.cases()
CAPACITIES = (1, 4, 64, 64)


@pytest.fixture(scope="module")
def gpu():
    import torch
    import xmipp3_amd as xa
    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    return xa, xa.Context(0), torch


def run(gpu, case, capacity):
    xa, ctx, _ = gpu
    w = xa.ReconstructWbp(ctx, case["D"], capacity)
    w.set_directions(case["g"], case["threshold"], case["diameter"])
    rows = R.rows_of(case["shifts"], case["flips"], case["weights"], case["angles"])
    filtered = w.add(case["images"], rows, filtered=True)
    raw = w.volume().cpu().numpy()
    w.finish(case["R"])
    out = w.volume().cpu().numpy(), filtered, w.count_thr(), raw
    w.close()
    return out


def test_tile_and_table(gpu):
    xa, ctx, _ = gpu
    assert xa.wbp_tile() == R.TILE
    for D in (16, 33):
        w = xa.ReconstructWbp(ctx, D, 1)
        assert np.array_equal(w.table(), R.sinc_table(D))
        w.close()


@pytest.mark.parametrize("case", CASES, ids=[c["name"] for c in CASES])
def test_parity_and_capacities(gpu, case):
    want_V, want_F, want_count, want_kept = R.result(case)
    first = None
    for capacity in CAPACITIES:
        V, F, count, raw = run(gpu, case, capacity)
        if first is None:
            first = (V, F, count, raw)
            dV, dF = R.distance(V, want_V), R.distance(F, want_F)
            print(f"{case['name']}: volume {dV:.2e}, filtered images {dF:.2e}, count_thr {count} (bound {BOUND:g})")
            assert count == want_count
            # the voxels no image reaches keep the exact zero they started from
            assert np.array_equal(raw[~want_kept], np.zeros((~want_kept).sum()))
            assert np.all(raw[want_kept] != 0)
            assert dF <= BOUND
            assert dV <= BOUND
        else:
            assert count == first[2]
            assert V.tobytes() == first[0].tobytes()
            assert F.tobytes() == first[1].tobytes()
            assert raw.tobytes() == first[3].tobytes()


@pytest.mark.parametrize("case", [CASES[1], CASES[4], CASES[5]], ids=lambda c: c["name"])
def test_weights(gpu, case):
    """the filter's weight at every cell: the pairs that are computed once, the unpaired row and column of an even D, the cells that count alone"""
    xa, ctx, _ = gpu
    w = xa.ReconstructWbp(ctx, case["D"], 2)
    w.set_directions(case["g"], case["threshold"], case["diameter"])
    rows = R.rows_of(case["shifts"], case["flips"], case["weights"], case["angles"])
    F, _ = R.image_matrices(*case["angles"][0])
    want = R.weights_of(R.filter_terms(case["D"], F, case["g"], case["diameter"])[0])
    got = w.weights(rows[0])
    assert w.count_thr() == 0
    w.close()
    print(f"{case['name']}: weights {R.distance(got, want):.2e}")
    assert np.array_equal(got, want)            # the same terms added in the same order


def test_reset_and_continue(gpu):
    """a second reconstruction on the same handle after reset, and images added in two calls: the same bytes as one call"""
    xa, ctx, _ = gpu
    case = CASES[2]
    rows = R.rows_of(case["shifts"], case["flips"], case["weights"], case["angles"])
    w = xa.ReconstructWbp(ctx, case["D"], 4)
    w.set_directions(case["g"], case["threshold"], case["diameter"])
    w.add(case["images"], rows)
    one, c1 = w.volume().cpu().numpy(), w.count_thr()
    w.reset()
    assert w.count_thr() == 0 and not w.volume().cpu().numpy().any()
    w.add(case["images"][:10], rows[:10])
    w.add(case["images"][10:], rows[10:])
    assert w.volume().cpu().numpy().tobytes() == one.tobytes() and w.count_thr() == c1
    w.close()


def test_refusals(gpu):
    xa, ctx, _ = gpu
    w = xa.ReconstructWbp(ctx, 16, 2)
    case = CASES[0]
    rows = R.rows_of(case["shifts"], case["flips"], case["weights"], case["angles"])
    with pytest.raises(xa.XhError, match="no directions"):
        w.add(case["images"], rows)
    with pytest.raises(xa.XhError, match="diameter"):
        w.set_directions(case["g"], 1.0, 18)
    bad = case["g"].copy()
    bad[3, 1] = 1.5
    with pytest.raises(xa.XhError, match="unit vector"):
        w.set_directions(bad, 1.0, 16)
    w.set_directions(case["g"], 1.0, 16)
    bad = rows.copy()
    bad[1, 14] = np.nan
    with pytest.raises(xa.XhError, match="not finite"):
        w.add(case["images"], bad)
    w.close()
    with pytest.raises(xa.XhError, match="1024"):
        xa.ReconstructWbp(ctx, 1025, 1)


def _write_inputs(tmp_path, case):
    stack = str(tmp_path / "images.stk")
    xmipp_io.write_stack(stack, case["images"])
    rows = []
    for n in range(len(case["images"])):
        rot, tilt, psi = case["angles"][n]
        rows.append([f"{n + 1:06d}@{stack}", repr(float(rot)), repr(float(tilt)), repr(float(psi)), repr(float(case["shifts"][n][0])),
                     repr(float(case["shifts"][n][1])), int(case["flips"][n]), repr(float(case["weights"][n]))])
    xmd = str(tmp_path / "images.xmd")
    xmipp_io.write_xmd(xmd, [("particles", ["image", "angleRot", "angleTilt", "anglePsi", "shiftX", "shiftY", "flip", "weight"], rows)])
    return xmd


EACH = "--use_each_image"


@pytest.mark.parametrize("case,args", [(CASES[2], [EACH, "--radius", "5"]), (CASES[5], [EACH, "--sym", "c3"]),
                                        (CASES[7], [EACH, "--weight", "--threshold", "0.2"]), (CASES[8], ["--filsam", "15", "--weight"])],
                         ids=lambda v: v["name"] if isinstance(v, dict) else None)
def test_program(gpu, tmp_path, case, args):
    """the binary end to end, every image's direction or the sampled ones: the volume it writes and the line it prints against the restatement"""
    assert os.path.exists(PROG), "xmipp_reconstruct_wbp is not built"
    want_V, _, want_count, _ = R.result(case)
    xmd = _write_inputs(tmp_path, case)
    out = str(tmp_path / "wbp.vol")
    r = subprocess.run([PROG, "-i", xmd, "-o", out] + args, capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr
    n, D = len(case["images"]), case["D"]
    pct = np.float32(want_count * 100.) / np.float32(n * D * D)
    assert f"Fourier pixels for which the threshold was not reached: {pct:g} %" in r.stderr
    got = xmipp_io.read_volume(out).astype(np.float64)
    top = np.abs(want_V).max()
    d = np.abs(got - want_V).max() / top
    print(f"{case['name']}: program volume {d:.2e}")
    assert d <= BOUND + 2.0 ** -24
