"""CPU checks of the restatement of the PSD stage (tests/psd_ref.py): against the answers the reference's own tests pin, against closed
values, against exact sums, and the preconditions of every GPU case (tests/test_gpu_psd.py). The bounds of the GPU test are derived here,
from the restatement alone."""
import math

import numpy as np
import pytest

from tests import psd_ref as R

CASES = R.cases()
BOUND = {np.float64: 1e-11, np.float32: 1e-5}       # what test_bounds_are_derived_from_exact_sums derives; tests/test_gpu_psd.py holds the device to them


def test_plane_fit_and_normalize_ramp_answers():
    """test_geometry_main.cpp:140-166: the 4 x 4 image i + j over the logical coordinates gives the plane (1, 1, 0), and normalize_ramp
    leaves nothing of it"""
    l = np.arange(4, dtype=np.float64) - 2
    img = l[:, None] + l[None, :]
    a, b, c = R.plane_fit(img)
    assert abs(a - 1) < 1e-6 and abs(b - 1) < 1e-6 and abs(c) < 1e-6
    out, sd = R.normalize_ramp(img)
    assert np.abs(out).sum() < 1e-6 and not sd > 1e-6
    # a general plane on an odd, oblong grid, and the scaling branch
    rng = np.random.default_rng(0)
    li, lj = (np.arange(7.0) - 3)[:, None], (np.arange(10.0) - 5)[None, :]
    z = 0.25 * lj - 1.5 * li + 3.0
    assert np.allclose(R.plane_fit(z), (0.25, -1.5, 3.0), atol=1e-12)
    out, sd = R.normalize_ramp(z + rng.standard_normal(z.shape))
    assert sd > 0.5 and out.std(ddof=1) == pytest.approx(1.0, rel=1e-12)


@pytest.mark.parametrize("x,y", [(10, 10), (4, 10), (11, 10), (10, 11), (11, 11), (5, 11), (128, 96), (127, 97)])
def test_half2whole_properties(x, y):
    """the two properties test_psd_estimator.cpp:42-61 checks, at its small parameter sets (its 4096-pixel ones run the same index rule)"""
    hx = x // 2 + 1
    half = np.arange(y * hx, dtype=np.float64).reshape(y, hx)
    out = R.half2whole(half, y, x)
    assert np.array_equal(out[:, :hx], half)
    for yy in range(y):
        for xx in range(x - hx):
            assert out[yy, x - xx - 1] == half[(y - yy) % y, xx + 1]


def test_half2whole_is_the_complete_transform_of_a_real_input():
    rng = np.random.default_rng(1)
    for py, px in ((16, 16), (17, 17), (16, 24), (17, 20)):
        F = np.abs(np.fft.fft2(rng.standard_normal((py, px))))
        assert np.allclose(R.half2whole(F[:, :px // 2 + 1], py, px), F, rtol=1e-12, atol=1e-12)


def test_patch_list_properties():
    """test_psd_estimator.cpp:68-169 (windowCoords) at its parameter sets: the number of patches and the corners they may take"""
    overlaps = (0.0, 0.2, 0.9)
    counter = 0
    for inX in (32, 256, 512):
        for inY in (32, 256, 512, 513):
            for pX in (5, 64, 367, 512):
                if pX > inX:
                    continue
                for pY in (5, 64, 367, 512):
                    if pY > inY:
                        continue
                    for bX in (0, 5):
                        if pX + 2 * bX > inX:
                            continue
                        for bY in (0, 5):
                            if pY + 2 * bY > inY:
                                continue
                            counter = (counter + 1) % 3
                            ov = np.float32(overlaps[counter])
                            res = R.patches(inY, inX, pY, pX, bX, bY, float(ov))
                            stepX = int(max((np.float32(1) - ov) * np.float32(pX), np.float32(1)))
                            stepY = int(max((np.float32(1) - ov) * np.float32(pY), np.float32(1)))
                            divX, divY = math.ceil(np.float32(inX) / np.float32(stepX)), math.ceil(np.float32(inY) / np.float32(stepY))
                            xs = {min(bX + k * stepX, inX - pX - bX) for k in range(divX)}
                            ys = {min(bY + k * stepY, inY - pY - bY) for k in range(divY)}
                            assert len(res) == len(xs) * len(ys)
                            for (t, l) in res:
                                assert l in xs and t in ys and l + pX - 1 < inX and t + pY - 1 < inY


def test_piece_lists():
    """the counts the cases were chosen for, the far-edge clamp, the skip rule, the three refusals"""
    c, s, div = R.pieces(83, 61, 16, 0.5, 0)
    assert len(c) == 70 == div and s == list(range(1, 71)) and c[-1] == (67, 45) and c[0] == (0, 0) and c[1] == (0, 8)
    c, s, div = R.pieces(83, 61, 16, 0.5, 2)
    assert len(c) == 18 and div == 70 and s[0] == 2 * 7 + 3 and c[0] == (16, 16)
    assert R.pieces(83, 61, 16, 0.3, 0)[0][1] == (0, 11)
    c, s, div = R.pieces(83, 61, 16, 0.5, 1, R.REGIONS)
    assert div == 24 and len(c) == 8 and c[0] == (16, 16) and c[-1] == (64, 32)
    c, s, _ = R.pieces(83, 61, 16, 0.5, 2, R.PARTICLES, [(8, 8), (60, 82)])
    assert c == [(0, 0), (67, 45)] and s == [1, 2]
    for kw, words in ((dict(mode=R.REGIONS, skipBorders=2), "skip"), (dict(mode=R.PARTICLES, pos=[(7, 30)]), "wraps"), (dict(skipBorders=4), "no piece"),
                      (dict(pieceDim=62), "smaller")):
        with pytest.raises(ValueError, match=words):
            R.pieces(83, 61, **{"pieceDim": 16, **kw})
    assert len(R.pieces(24, 30, 16, 0.0, 0)[0]) == 1 and len(R.pieces(16, 32, 16, 0.5, 0)[0]) == 3


def test_taper_closed_values():
    """an even side up to 80 and an odd one up to 39 only take 0 and 1: the outermost row of an even side has fraction 1 and the value 0, and
    a second row beyond 0.975 needs (P - 2) / P > 0.975, P > 80; an odd side has (P - 1) / P > 0.975 from P = 41 on. At 96 the row next
    to the outermost one is 0.5 (1 + cos(pi (1 - 40 / 48)))"""
    assert len(np.unique(R.taper_vectors(41, 41, np.float64)[0])) == 2 and R.taper_vectors(41, 41, np.float64)[0][0] not in (0.0, 1.0)
    for P in (16, 17, 20, 33, 39, 80):
        for T in (np.float64, np.float32):
            m = R.taper_vectors(P, P, T)[0]
            assert set(np.unique(m)) <= {0.0, 1.0}
            assert m[0] == (0.0 if P % 2 == 0 else 1.0) and np.all(m[1:] == 1)
    for T, eps in ((np.float64, 1e-13), (np.float32, 1e-5)):
        m = R.taper_vectors(96, 96, T)[0]
        assert m.dtype == T and abs(float(m[0])) < eps and np.all(m[2:95] == 1)
        assert float(m[1]) == pytest.approx(0.5 * (1 + math.cos(math.pi * (1 - 40 / 48))), abs=20 * eps)
        assert float(m[95]) == pytest.approx(float(m[1]), abs=20 * eps)
    # both axes take their fraction against the number of rows (constructPieceSmoother reads YSIZE twice)
    mY, mX = R.taper_vectors(96, 128, np.float64)
    assert np.all(mY[2:95] == 1) and (mX[:18] != 1).sum() >= 15 and np.all(mX[18:111] == 1) and mX[17] != 1 and mX[111] != 1
    s = R.smoother(96, 96, np.float32)
    assert s.dtype == np.float32 and s[1, 1] == np.float32(R.taper_vectors(96, 96, np.float32)[0][1]) ** 2


def test_statistics_adjust():
    rng = np.random.default_rng(2)
    x = (1000 + 3 * rng.standard_normal((16, 24))).astype(np.float32).astype(np.float64)
    a, b, sd = R.statistics_adjust_ab(x)
    assert sd == pytest.approx(x.std(ddof=1), rel=1e-9)
    v = a * x + b
    assert abs(v.mean()) < 1e-9 and v.std(ddof=1) == pytest.approx(1.0, rel=1e-9)
    assert R.statistics_adjust_ab(np.full((16, 16), 1000.0)) == (0.0, 0.0, 0.0)


def test_parseval_for_the_psd_of_a_piece():
    """sum of the double PSD = sum of the squares of the piece (|F|^2 / (py px)^2 times pieceDim^2, summed over the plane); the float PSD is
    the modulus of the un-normalised transform"""
    rng = np.random.default_rng(3)
    for P in (16, 17, 20):
        p = rng.standard_normal((P, P))
        assert R.psd_double(p).sum() == pytest.approx((p * p).sum(), rel=1e-12)
        assert R.distance(R.psd_double(p), R.psd_double(p, exact=True)) < 1e-14
        q = p.astype(np.float32)
        assert (R.psd_float(q).astype(np.float64) ** 2).sum() == pytest.approx(float((q.astype(np.float64) ** 2).sum()) * P * P, rel=1e-5)


def test_avg_std():
    rng = np.random.default_rng(4)
    ps = [np.abs(rng.standard_normal((4, 4))) for _ in range(5)]
    avg, std, var = R.avg_std(ps)
    assert np.allclose(avg, np.mean(ps, axis=0), rtol=1e-14) and np.allclose(std, np.std(ps, axis=0), rtol=1e-12)
    assert not R.avg_std(ps[:1])[2].max() > 1e-15


def test_normalisation_reading():
    """10 log10 with the smallest positive value as the floor of the others, then the clamp to the percentiles 0.125 and 99.875"""
    rng = np.random.default_rng(5)
    v = (100 * np.abs(rng.standard_normal((40, 50)))).astype(np.float32)
    v[0, 0], v[1, 1], v[2, 2] = 0.0, 1e-3, 1e7
    out = R.normalize_psd(v)
    db = 10 * np.log10(np.where(v > 0, v, v[v > 0].min()).astype(np.float64))
    assert out.dtype == np.float32 and out.min() > db.min() and out.max() < db.max()
    inner = (out > out.min()) & (out < out.max())
    assert inner.sum() >= v.size - 6 and np.array_equal(out[inner], db.astype(np.float32)[inner])
    assert np.array_equal(R.reject_outliers(np.full(7, 2.0, np.float32)), np.full(7, 2.0, np.float32))


@pytest.mark.parametrize("case", CASES, ids=[c["name"] for c in CASES])
def test_preconditions(case):
    """conditions, not measurements: every deviation a branch tests (stddev0 != 0, stddevbg > 1e-6) is exactly 0 or above 1e-3, in the
    restatement and with exact sums, so no branch can flip with rounding; pieces of deviation 0 are prepared as exact zeros"""
    r = R.result(case)
    e = R.compute(case, exact=True)
    zeros = 0
    for (sd0, sdbg), (esd0, esdbg), piece in zip(r["info"], e["info"], r["pieces"]):
        for a, b in ((sd0, esd0), (sdbg, esdbg)):
            if a is None:
                continue
            assert (a == 0.0 and b == 0.0) or (a > 1e-3 and b > 1e-3)
        if sd0 == 0.0:
            zeros += 1
            assert not piece.any()
    assert zeros == (1 if "constant" in case["name"] else 0)
    for cs, img in zip(case["corners"], case["mic"]):
        for (cy, cx) in cs:
            assert 0 <= cy <= img.shape[0] - case["py"] and 0 <= cx <= img.shape[1] - case["px"]
    # the widening is exercised: the float32 values are no short sums
    assert (np.frexp(case["mic"].astype(np.float64))[0] * 2.0 ** 24 % 2 == 1).mean() > 0.3


def test_bounds_are_derived_from_exact_sums():
    """one bound per element type: 16 times the largest relative difference over the cases between the restatement and the same per-term
    values summed with math.fsum, the transforms in extended precision; up to a power of ten"""
    worst = {np.float64: 0.0, np.float32: 0.0}
    for case in CASES:
        r, e = R.result(case), R.compute(case, exact=True)
        d = {"pieces": R.distance(r["pieces"], e["pieces"])}
        if case["stack"]:
            d["stack"] = R.distance(r["stack"], e["stack"])
        else:
            d["avg"] = R.distance(r["avg"], e["avg"])
            if case["dtype"] == np.float64 and len(r["pieces"]) > 1:
                d["variance"] = float(np.abs(r["var"] - e["var"]).max() / (e["avg"] ** 2).max())
        print(case["name"], {k: f"{v:.2e}" for k, v in d.items()})
        worst[case["dtype"]] = max(worst[case["dtype"]], *d.values())
    for T, w in worst.items():
        derived = 10.0 ** math.ceil(math.log10(16 * w))
        print(f"{np.dtype(T).name}: largest {w:.2e}, bound {derived:g}")
        assert derived == BOUND[T]
