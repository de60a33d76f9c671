"""GPU parity of the PSD stage (xh_psd_*, PsdEstimator in api.py) against the numpy restatement (tests/psd_ref.py): the prepared pieces, avg,
the variance and the stacks of every case, the taper, independence of the batch capacity, run-to-run identity, and both programs end to end.

Cases (R.cases()): piece sides 16 (half width 9: a remainder on the column strip of xmipp3_amd.psd_strip() = 4 columns, asserted below),
17 (odd: the unpaired row, the mirror without a Nyquist column, the odd origin), 20 (Bluestein lines), 33, and 96, the one side whose taper
is fractional; float patches of 16 x 24 and 24 x 16 (both axes take their taper fraction against the rows) and 17 x 17. Micrographs of
83 rows x 61 columns at overlap 0.5: skipBorders 0 (70 pieces, more than a batch of 64, the far-edge clamp on both axes), 2 (18 pieces),
overlap 0.3 (step 11), regions mode, particles mode with coordinates at the near-edge limit and past the far edge, a stack of two images,
exactly one piece; 3, 4 and 5 pieces around a capacity of 4. Data: noise of deviation 1 on a mean of 1000 with a gradient of several
deviations per piece, a region of exactly 1000 that makes one piece constant (a = 0, no scaling, a zero PSD in the average), float32 values
that are no short sums. Every case runs at capacities 1, 4, 64 and a second time at 64: the same bytes.

Bounds, of the largest value: 1e-11 in double, 1e-5 in float. They are not taken from the device: tests/test_psd_ref.py derives each as
16 times the largest relative difference over the cases (double 3.4e-13, the variance of d16_skip0_70_constant; float 1.4e-7, the sum of
f24x16_patches) between the restatement, which adds element after element as the reference does, and the same per-term values summed with
math.fsum with the transforms in extended precision, rounded up to a power of ten; it also asserts on the restatement alone that every
deviation a branch tests is exactly 0 or above 1e-3. The variance is compared as std^2 against the largest avg^2 (the root of a cancelled
difference has no fixed relative bound); with one piece it is only checked to be below the bound. The double program's .psd file holds
32-bit floats, so half an ulp of the largest value is added there.
Measured on one MI355X, largest over the cases: prepared pieces 8.0e-14 (d16_one_piece) in double and 8.4e-8 (f16x24_patches) in float,
avg 6.7e-14 and 1.2e-7, the variance 3.4e-13 of the largest avg^2 (d16_skip0_70_constant; 0 with one piece), stacks 1.1e-13; the same bytes
at every capacity and from the second run; the programs' files 4.4e-8 (double, 32-bit files) and 1.2e-7 (float), the normalised float PSD
3.8e-6 dB.
"""
import os
import subprocess

import numpy as np
import pytest

from tests import psd_ref as R
from tests import xmipp_io

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIN = os.path.join(ROOT, "xmipp3_amd", "bin")
BOUND = {np.float64: 1e-11, np.float32: 1e-5}
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
    _, Y, X = case["mic"].shape
    e = xa.PsdEstimator(ctx, Y, X, case["py"], case["px"], capacity, case["dtype"])
    out = {"pieces": [], "stack": []}
    for img, corners in zip(case["mic"], case["corners"]):
        e.load(img)
        out["pieces"].append(e.piece(corners))
        if case["stack"]:
            out["stack"].append(e.add(corners, stack=True))
        else:
            e.add(corners)
    out["pieces"] = np.concatenate(out["pieces"])
    if case["stack"]:
        out["stack"] = np.concatenate(out["stack"])
    else:
        del out["stack"]
        out["avg"], out["std"], out["n"] = e.result()
    e.close()
    return out


def test_strip_and_smoother(gpu):
    xa, ctx, _ = gpu
    assert xa.psd_strip() == R.STRIP
    for py, px, T in ((16, 16, np.float64), (96, 96, np.float64), (17, 17, np.float32), (16, 24, np.float32), (96, 96, np.float32)):
        e = xa.PsdEstimator(ctx, 100, 100, py, px, 1, T)
        got, want = e.smoother(), R.smoother(py, px, T)
        e.close()
        assert got.dtype == want.dtype
        assert np.abs(got.astype(np.float64) - want.astype(np.float64)).max() <= 4 * np.finfo(T).eps
    assert (R.smoother(96, 96, np.float64) % 1 != 0).any() and not (R.smoother(33, 33, np.float64) % 1 != 0).any()


@pytest.mark.parametrize("case", CASES, ids=[c["name"] for c in CASES])
def test_parity_and_capacities(gpu, case):
    want, bound = R.result(case), BOUND[case["dtype"]]
    first = None
    for capacity in CAPACITIES:
        got = run(gpu, case, capacity)
        if first is None:
            first = got
            d = R.distance(got["pieces"], want["pieces"])
            print(f"{case['name']}: pieces {d:.2e} (bound {bound:g})")
            assert d <= bound
            if case["stack"]:
                d = R.distance(got["stack"], want["stack"])
                print(f"{case['name']}: stack {d:.2e}")
                assert d <= bound
                continue
            n = sum(len(c) for c in case["corners"])
            assert got["n"] == n
            d = R.distance(got["avg"], want["avg"])
            print(f"{case['name']}: avg {d:.2e}")
            assert d <= bound
            if case["dtype"] == np.float64:
                top = float((want["avg"] ** 2).max())
                dv = float(np.abs(got["std"] ** 2 - want["var"]).max() / top)
                print(f"{case['name']}: variance {dv:.2e} of the largest avg^2")
                assert dv <= bound
                if n == 1:
                    assert float((got["std"] ** 2).max() / top) <= bound
        else:
            for k, v in first.items():
                if isinstance(v, np.ndarray):
                    assert got[k].tobytes() == v.tobytes(), (k, capacity)


def test_reset_and_continue(gpu):
    """pieces added in two calls give the bytes of one call; after reset the handle starts again"""
    xa, ctx, _ = gpu
    case = CASES[1]
    corners = case["corners"][0]
    e = xa.PsdEstimator(ctx, 83, 61, 16, 16, 4)
    e.load(case["mic"][0])
    e.add(corners)
    one = e.result()
    e.reset()
    with pytest.raises(xa.XhError, match="no piece"):
        e.result()
    e.add(corners[:7])
    e.add(corners[7:])
    two = e.result()
    e.close()
    assert two[2] == one[2] and two[0].tobytes() == one[0].tobytes() and two[1].tobytes() == one[1].tobytes()


def test_refusals(gpu):
    xa, ctx, _ = gpu
    e = xa.PsdEstimator(ctx, 83, 61, 16, 16, 4)
    with pytest.raises(xa.XhError, match="no micrograph"):
        e.add([(0, 0)])
    e.load(CASES[1]["mic"][0])
    for bad in ((68, 0), (0, 46), (-1, 0)):
        with pytest.raises(xa.XhError, match="leaves the micrograph"):
            e.add([bad])
    e.close()
    with pytest.raises(xa.XhError, match="1024"):
        xa.PsdEstimator(ctx, 2000, 2000, 1025, 1025, 1)
    with pytest.raises(xa.XhError, match="square"):
        xa.PsdEstimator(ctx, 83, 61, 16, 24, 1, np.float64)
    f = xa.PsdEstimator(ctx, 83, 61, 16, 24, 1, np.float32)
    f.load(CASES[1]["mic"][0])
    with pytest.raises(xa.XhError, match="double path"):
        f.add([(0, 0)], flags=3)
    f.close()


def _run(prog, args):
    path = os.path.join(BIN, prog)
    assert os.path.exists(path), f"{prog} is not built"
    r = subprocess.run([path] + args, capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr
    return r


@pytest.mark.parametrize("case", [CASES[0], CASES[3], CASES[9]], ids=lambda c: c["name"])
def test_program_micrograph(gpu, tmp_path, case):
    """xmipp_ctf_estimate_from_micrograph --dont_estimate_ctf: <oroot>.psd against the restatement's avg"""
    mic = str(tmp_path / "mic.stk")
    xmipp_io.write_stack(mic, case["mic"])
    _run("xmipp_ctf_estimate_from_micrograph", ["--micrograph", mic, "--dont_estimate_ctf", "--pieceDim", str(case["py"]), "--overlap", repr(case["overlap"]),
                                                 "--skipBorders", str(case["skipBorders"])])
    got = xmipp_io.read_volume(os.path.splitext(mic)[0] + ".psd")[0].astype(np.float64)
    want = R.result(case)["avg"]
    d = R.distance(got, want)
    print(f"{case['name']}: program avg {d:.2e}")
    assert d <= BOUND[np.float64] + 2.0 ** -24


@pytest.mark.parametrize("case", [CASES[7], CASES[8]], ids=lambda c: c["name"])
def test_program_stack(gpu, tmp_path, case):
    """regions and particles: <oroot>.psdstk with piece N at 1-based slot N, skipped slots zero; particles: the psd column"""
    mic = str(tmp_path / "mic.stk")
    xmipp_io.write_stack(mic, case["mic"])
    pos = str(tmp_path / "mic.pos")
    rows = [[int(x), int(y)] for x, y in (case["pos"] or [(20, 20)])]
    xmipp_io.write_xmd(pos, [("particles", ["xcoor", "ycoor"], rows)])
    mode = "regions" if case["mode"] == R.REGIONS else "particles"
    root = str(tmp_path / "out")
    _run("xmipp_ctf_estimate_from_micrograph", ["--micrograph", mic, "--oroot", root, "--dont_estimate_ctf", "--pieceDim", str(case["py"]),
                                                 "--skipBorders", str(case["skipBorders"]), "--mode", mode, pos])
    got = xmipp_io.read_stack(root + ".psdstk").astype(np.float64)
    want = R.result(case)["stack"]
    assert len(got) == case["slots"][-1]
    full = np.zeros_like(got)
    for s, w in zip(case["slots"], want):
        full[s - 1] = w
    d = R.distance(got, full)
    print(f"{case['name']}: program stack {d:.2e}")
    assert d <= BOUND[np.float64] + 2.0 ** -24
    skipped = sorted(set(range(1, len(got) + 1)) - set(case["slots"]))
    assert all(not got[s - 1].any() for s in skipped)
    if mode == "particles":
        text = open(pos).read()
        assert "_psd" in text and f"{len(rows):06d}@{root}.psdstk" in text


@pytest.mark.parametrize("case,normalize", [(CASES[12], False), (CASES[13], True), (CASES[14], False)], ids=lambda v: v["name"] if isinstance(v, dict) else None)
def test_program_psd_estimate(gpu, tmp_path, case, normalize):
    mic = str(tmp_path / "mic.stk")
    xmipp_io.write_stack(mic, case["mic"])
    out = str(tmp_path / "psd.spi")
    _run("xmipp_psd_estimate", ["-i", mic, "-o", out, "--overlap", repr(case["overlap"]), "--patches", str(case["px"]), str(case["py"]), "--threads", "3"]
         + ([] if normalize else ["--skipNormalization"]))
    got = xmipp_io.read_volume(out)[0]
    want = R.result(case)["avg"]
    if normalize:
        # 10 log10 of a value p known to BOUND * max moves by 10 / ln(10) * BOUND * max / p decibels: largest at the smallest positive value
        tolerance = 10 / np.log(10) * BOUND[np.float32] * float(want.max() / want[want > 0].min())
        d = float(np.abs(got.astype(np.float64) - R.normalize_psd(want)).max())
        print(f"{case['name']}: program normalised psd, largest absolute difference {d:.2e} dB (tolerance {tolerance:.2e})")
        assert d <= tolerance
    else:
        d = R.distance(got, want)
        print(f"{case['name']}: program psd {d:.2e}")
        assert d <= BOUND[np.float32]
