"""CPU checks of xmipp_resolution_fso: the direction generator, the incomplete gamma table, the host-only decisions of the library against
the numpy restatement (tests/fso_ref.py), properties of the restatement itself on the synthetic pair, and the program's refusals, which
come before any device is touched."""
import os
import subprocess

import numpy as np
import pytest

from tests import fso_ref as R
from tests import xmipp_io

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PROG = os.path.join(ROOT, "xmipp3_amd", "bin", "xmipp_resolution_fso")
EPS32 = 2.0 ** -24
THRS = 0.143


@pytest.fixture(scope="module")
def xa():
    import __graft_entry__ as g
    g.build()
    assert os.path.exists(PROG)
    import xmipp3_amd
    return xmipp3_amd


def _run(args):
    return subprocess.run([PROG] + args, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=120)


def _vec64(a):
    r, t = np.radians(a[:, 0].astype(np.float64)), np.radians(a[:, 1].astype(np.float64))
    return np.stack([np.sin(t) * np.cos(r), np.sin(t) * np.sin(r), np.cos(t)], 1)


_CASE = {}


def case(shape, widths):
    """the restatement on the synthetic pair (masked), with the 321 directions: computed once per (shape, widths)"""
    import xmipp3_amd as xa
    key = (shape, widths)
    if key not in _CASE:
        h1, h2, m = (a.astype(np.float32).astype(np.float64) for a in R.synth(shape, 3, widths))
        lay = R.layout(shape, *R.spectra(h1, h2, m))
        dirs = R.unit_vectors(xa.fso_directions(3))
        cosA, aux = R.cone(17.0)
        dsums, cnt = R.cone_sums(lay, dirs, cosA, aux)
        _CASE[key] = {"lay": lay, "dirs": dirs, "cone": (cosA, aux), "dsums": dsums, "cnt": cnt, "decide": R.decide(dsums, dirs, shape[2], 1.0, THRS)}
    return _CASE[key]


# ---------------------------------------------------------------- the direction generator
@pytest.mark.parametrize("level,n", [(0, 6), (1, 21), (2, 81), (3, 321)])
def test_direction_counts_unit_vectors_and_antipodal_uniqueness(xa, level, n):
    a = xa.fso_directions(level)
    assert a.shape == (n, 2) and a.dtype == np.float32
    assert (a[:, 0] >= 0).all() and (a[:, 0] < 360).all() and (a[:, 1] >= 0).all() and (a[:, 1] <= 90).all()
    assert np.array_equal(a.astype(np.float64), np.round(a.astype(np.float64), 4).astype(np.float32).astype(np.float64))     # 4 decimals of a degree
    v = _vec64(a)
    assert np.abs(np.linalg.norm(v, axis=1) - 1).max() < 1e-12
    u = xa.fso_unit_vectors(a)
    assert np.abs(np.linalg.norm(u.astype(np.float64), axis=1) - 1).max() < 4 * EPS32
    # no direction is another one or its antipode: the closest pair of the level is its edge, 63.4 degrees halved per round
    c = np.abs(v @ v.T) - np.eye(n)
    assert np.degrees(np.arccos(c.max())) > 0.9 * 63.4 / 2 ** level


def test_nearest_neighbour_separation_at_level_3(xa):
    v = _vec64(xa.fso_directions(3))
    c = np.abs(v @ v.T) - 2 * np.eye(321)
    nn = np.degrees(np.arccos(np.clip(c.max(1), -1, 1)))
    print(f"nearest-neighbour separation: {nn.min():.3f} .. {nn.max():.3f} degrees")
    assert 7.9 <= nn.min() and nn.max() <= 9.1


def test_level_order(xa):
    a3 = xa.fso_directions(3)
    for level, n in ((0, 6), (1, 21), (2, 81)):
        assert np.array_equal(a3[:n], xa.fso_directions(level))
    assert a3[0, 1] == 0 and np.allclose(a3[1:6, 1], np.degrees(np.arctan(2.0)), atol=1e-4)
    assert sorted(a3[1:6, 0].tolist()) == [36.0, 108.0, 180.0, 252.0, 324.0]


def test_unit_vectors_and_cone_against_the_restatement(xa):
    a = xa.fso_directions(3)
    # sinf and cosf may differ from the rounded double function in the last bit, and so may their product
    assert np.abs(xa.fso_unit_vectors(a).astype(np.float64) - R.unit_vectors(a).astype(np.float64)).max() <= 4 * EPS32
    for ang in (17.0, 5.0, 30.0, 89.0):
        c, aux = xa.fso_cone(ang)
        rc, raux = R.cone(ang)
        assert c == float(rc) and aux == float(raux), ang
    for ang in (0.0, 90.0, -5.0, 120.0):
        with pytest.raises(xa.XhError, match="cone angle"):
            xa.fso_cone(ang)


# ---------------------------------------------------------------- the gamma table
def test_gamma_table_equals_the_formula(xa):
    for i in range(41):
        x = i / 2
        P = 1 - np.exp(-x) * sum(x ** k / float(np.prod(np.arange(1, k + 1))) for k in range(5))
        got = xa.fso_incomplete_gamma(x)
        assert got == float(np.float32(float("%.5g" % P))) == R.incomplete_gamma(x), i
    assert xa.fso_incomplete_gamma(0.0) == 0.0 and xa.fso_incomplete_gamma(20.0) == float(np.float32(0.99998))
    # round(2 x), clamped
    assert xa.fso_incomplete_gamma(0.24) == xa.fso_incomplete_gamma(0.0) and xa.fso_incomplete_gamma(0.25) == xa.fso_incomplete_gamma(0.5)
    assert xa.fso_incomplete_gamma(1e9) == xa.fso_incomplete_gamma(20.0) and xa.fso_incomplete_gamma(-3.0) == 0.0
    assert xa.fso_incomplete_gamma(7.3) == xa.fso_incomplete_gamma(7.5) and xa.fso_incomplete_gamma(7.2) == xa.fso_incomplete_gamma(7.0)


# ---------------------------------------------------------------- the restatement on the synthetic pair
def _mid(fso):
    return int(((fso > 0.3) & (fso < 0.7)).sum())


def test_isotropic_pair_steps_and_anisotropic_pair_slopes():
    shape = (64, 64, 64)
    iso = case(shape, (0.12, 0.12, 0.12))["decide"][2]
    ani = case(shape, (0.06, 0.14, 0.2))["decide"][2]
    print("isotropic  ", np.round(iso[5:], 2))
    print("anisotropic", np.round(ani[5:], 2))
    for fso in (iso, ani):
        assert fso[:8].min() > 0.9 and fso[-8:].max() < 0.2        # from 1 to the level that pure noise reaches
    assert _mid(iso) <= 2 and _mid(ani) >= 4
    # the anisotropic pair resolves x better than z: the directions near the x axis reach further than those near z
    c = case(shape, (0.06, 0.14, 0.2))
    resol, dirs = c["decide"][1], c["dirs"]
    near_x, near_z = np.abs(dirs[:, 0]) > 0.95, np.abs(dirs[:, 2]) > 0.95
    assert near_x.sum() > 5 and near_z.sum() > 5 and np.median(resol[near_x]) < 0.7 * np.median(resol[near_z])


def test_a_coefficient_lies_in_fourteen_cones_on_average():
    for shape in ((32, 32, 32), (24, 28, 30)):
        c = case(shape, (0.06, 0.14, 0.2))
        mean = c["cnt"].sum() / c["lay"]["freqidx"].size
        print(shape, f"{mean:.2f} cones per coefficient")
        assert 13.5 < mean < 14.5


def test_fp64_and_as_written_float_cone_sums_agree_to_the_float_noise():
    """the as-written form adds n float products to a float: each add rounds by at most 2^-24 of a partial sum that sum |term| bounds, and
    |num| <= sqrt(den1 den2), so the FSC moves by at most 2 n 2^-24, plus the rounding of the stored float"""
    shape = (32, 32, 32)
    c = case(shape, (0.06, 0.14, 0.2))
    lay, (cosA, aux) = c["lay"], c["cone"]
    worst = 0.0
    for k in (0, 7, 100, 320):
        inside, _ = R.cone_weights(lay, c["dirs"][k], cosA, aux)
        n = np.bincount(lay["freqidx"][inside], minlength=lay["L"])
        aw = R.dir_fsc(R.cone_sums_as_written(lay, c["dirs"][k], cosA, aux).astype(np.float64)).astype(np.float64)
        err = np.abs(aw - R.dir_fsc(c["dsums"][k]).astype(np.float64))
        assert n.max() > 20 and (err <= (2 * n + 2) * EPS32).all(), k
        worst = max(worst, err.max())
    print(f"as-written float32 against fp64: at most {worst:.3e}")


# ---------------------------------------------------------------- the library's host decisions
@pytest.mark.parametrize("shape", [(32, 32, 32), (24, 28, 30)])
def test_decisions_equal_the_restatement(xa, shape):
    c = case(shape, (0.06, 0.14, 0.2))
    fsc, resol, fso, bingham = c["decide"]
    g_fsc, g_resol, g_fso, g_bingham = xa.fso_decide(c["dsums"], c["dirs"], shape[2], 1.0, THRS)
    assert np.array_equal(g_fsc, fsc) and np.array_equal(g_resol, resol) and np.array_equal(g_fso, fso)
    assert np.abs(g_bingham - bingham).max() <= 1e-9 * max(1.0, np.abs(bingham).max())
    assert (resol > 0).any() and 0 < fso[5:].min() < fso[5:].max() and bingham.max() > 1
    # another sampling rate and threshold
    g = xa.fso_decide(c["dsums"], c["dirs"], shape[2], 1.7, 0.5)
    e = R.decide(c["dsums"], c["dirs"], shape[2], 1.7, 0.5)
    assert np.array_equal(g[1], e[1]) and np.array_equal(g[2], e[2]) and not np.array_equal(e[2], fso)


def test_resolution_distribution_against_the_restatement(xa):
    """sinf and cosf of the grid may differ in the last bit between the two: a grid point within 1e-6 of a cone's edge is marginal and
    left out. The grid is in whole degrees and so are some directions: the pole (0, 0) alone has the 360 grid points of tilt 17, 1.1 % of the
    grid, on its edge, so up to 3 % may be marginal. Elsewhere the weights differ by a few 2^-24 relative, and the quotient of the weighted sums with them"""
    c = case((32, 32, 32), (0.06, 0.14, 0.2))
    dirs, resol = c["dirs"], c["decide"][1]
    exp = R.resolution_distribution(dirs, resol, 17.0)
    got = xa.fso_resolution_distribution(dirs, resol, 17.0)
    rot, tilt = np.radians(np.arange(360.0))[:, None], np.radians(np.arange(91.0))[None, :]
    p = np.stack([np.sin(tilt) * np.cos(rot), np.sin(tilt) * np.sin(rot), np.cos(tilt) * np.ones_like(rot)], -1)
    edge = np.abs(np.abs(p @ dirs.astype(np.float64).T) - float(R.cone(17.0)[0])).min(-1)
    ok = edge > 1e-6
    assert ok.mean() >= 0.97 and np.isfinite(exp).all()
    err = np.abs(got - exp)[ok] / np.abs(exp)[ok]
    print(f"resolution distribution: {int((~ok).sum())} marginal grid points, largest relative difference elsewhere {err.max():.3e}")
    assert err.max() <= 1e-5


# ---------------------------------------------------------------- the program
def test_help_lists_the_reference_options_and_defaults(xa):
    r = _run(["--help"])
    assert r.returncode == 0
    for t in ("--half1 <arg>", "--half2 <arg>", "[-o <=>]", "[--sampling <=1>]", "[--mask <=>]", "[--anglecone <=17>]", "[--threshold <=0.143>]",
              "[--threedfsc_filter]", "[--threads <=1>]", "[--dev <=0>]"):
        assert t in r.stderr, t


@pytest.fixture(scope="module")
def files(tmp_path_factory):
    d = tmp_path_factory.mktemp("fso")
    out = {}
    for name, shape in (("a", (8, 8, 8)), ("b", (8, 8, 8)), ("c", (8, 8, 10)), ("small", (6, 6, 6)), ("flat1", (8, 10, 12)), ("flat2", (8, 10, 12))):
        out[name] = str(d / (name + ".vol"))
        xmipp_io.write_volume(out[name], np.zeros(shape, np.float32))
    out["dir"] = str(d / "out")
    return out


def test_refusals_before_any_device(xa, files):
    a, b, o = files["a"], files["b"], files["dir"]
    cases = [
        (["--half1", a, "--half2", b], "-o is empty"),
        (["--half1", a, "--half2", files["c"], "-o", o], "half maps have different dimensions"),
        (["--half1", a, "--half2", b, "--mask", files["c"], "-o", o], "mask and the half maps have different dimensions"),
        (["--half1", files["small"], "--half2", files["small"], "-o", o], "sides below 8"),
        (["--half1", files["flat1"], "--half2", files["flat2"], "-o", o, "--threedfsc_filter"], "cubic"),
    ] + [(["--half1", a, "--half2", b, "-o", o, "--anglecone", v], "inside (0, 90)") for v in ("0", "90", "-5", "120")]
    for args, text in cases:
        r = _run(args)
        assert r.returncode != 0 and text in r.stderr, (args, r.stderr)
        assert "xmipp_hip" not in r.stderr and not os.path.exists(os.path.join(o, "GlobalFSC.xmd"))


def test_bad_device_is_refused(xa, files):
    r = _run(["--half1", files["a"], "--half2", files["b"], "-o", files["dir"], "--dev", "x"])
    assert r.returncode != 0 and "Invalid GPU device" in r.stderr
