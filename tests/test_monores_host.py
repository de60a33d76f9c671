"""CPU checks of xmipp_resolution_monogenic_signal (MonoRes): icdf_gauss, resolution2eval over whole sweeps and the shell walk of
findCliffValue against the numpy restatement (tests/monores_ref.py); the program's option parsing, which comes before any device is
touched."""
import math
import os
import statistics
import subprocess

import numpy as np
import pytest

from tests import monores_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PROG = os.path.join(ROOT, "xmipp3_amd", "bin", "xmipp_resolution_monogenic_signal")


@pytest.fixture(scope="module")
def xa():
    import __graft_entry__ as g
    g.build()
    assert os.path.exists(PROG)
    import xmipp3_amd
    return xmipp3_amd


def _run(args):
    return subprocess.run([PROG] + args, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=120)


def _as2623(p):
    q = min(p, 1 - p)
    t = math.sqrt(-2 * math.log(q))
    x = t - ((0.010328 * t + 0.802853) * t + 2.515517) / (((0.001308 * t + 0.189269) * t + 1.432788) * t + 1)
    return -x if p < 0.5 else x


@pytest.mark.parametrize("p", [0.9, 0.95, 0.99])
def test_icdf_gauss_is_the_stated_formula(xa, p):
    assert abs(xa.mono_icdf_gauss(p) - _as2623(p)) <= 1e-12
    assert abs(R.icdf_gauss(p) - _as2623(p)) <= 1e-12


@pytest.mark.parametrize("p", [0.9, 0.95, 0.99, 0.5001, 0.75, 0.999, 0.1, 0.05, 0.01])
def test_icdf_gauss_within_the_published_bound(xa, p):
    assert abs(xa.mono_icdf_gauss(p) - statistics.NormalDist().inv_cdf(p)) <= 4.5e-4


def test_icdf_gauss_refuses_the_ends(xa):
    for p in (0.0, 1.0, -0.1, 1.5):
        with pytest.raises(xa.XhError):
            xa.mono_icdf_gauss(p)


@pytest.mark.parametrize("size", [20, 21, 32])
@pytest.mark.parametrize("sampling,max_res,step", [(1.0, 12.0, 0.25), (1.34, 20.0, 0.5), (0.8, 7.3, 0.25)])
def test_resolution2eval_sweep(xa, size, sampling, max_res, step):
    got = xa.mono_resolution_sweep(size, sampling, max_res, step)
    exp = R.resolution_sweep(size, sampling, max_res, step)
    assert [g[0] for g in got] == [e[0] for e in exp]                       # the same continue / break decisions
    assert got[-1][0] == "break" and sum(g[0] == "eval" for g in got) >= 4
    for g, e in zip(got, exp):
        if g[0] == "eval":
            assert g[1] == e[1] and g[2] == e[2]                             # the same list of resolutions, bit for bit
    res = [g[1] for g in got if g[0] == "eval"]
    assert all(a > b for a, b in zip(res, res[1:])) and res[-1] >= 2 * sampling


def test_resolution2eval_ends_at_a_resolution_of_zero(xa):
    """maxRes a multiple of the step and a sampling rate so fine that Nyquist is never reached first: the reference divides by 0"""
    got = xa.mono_resolution_sweep(32, 1e-3, 1.0, 0.25)
    assert got[-1][0] == "break" and len(got) <= 5


@pytest.mark.parametrize("shape,Rzero", [((24, 24, 24), 9), ((21, 21, 21), 7), ((32, 32, 32), 13)])
def test_cliff_walk_finds_the_zeroed_radius(xa, shape, Rzero):
    rng = np.random.default_rng(3)
    v = rng.standard_normal(shape)
    v[R.r2_map(shape) >= Rzero * Rzero] = 0.0
    s, s2, n = R.shell_sums(v)
    assert s.size <= xa.mono_num_shells(shape)
    assert xa.mono_cliff_radius(s, s2, n, 3, shape[2]) == Rzero - 1
    assert R.cliff_radius(s, s2, n, 3, shape[2]) == Rzero - 1
    # no cliff: the walk ends at X / 2
    w = rng.standard_normal(shape)
    s, s2, n = R.shell_sums(w)
    assert xa.mono_cliff_radius(s, s2, n, 3, shape[2]) == shape[2] // 2


def test_help_lists_the_reference_options_and_defaults(xa):
    r = _run(["--help"])
    assert r.returncode == 0
    for t in ("--vol <=>", "--mask <=>", "--minRes <=30>", "--maxRes <=1>", "--sampling_rate <=1>", "-o <=>", "[--vol2 <=>]", "[--maskExcl <=>]",
              "[--step <=0.25>]", "[--significance <=0.95>]", "[--threads <=4>]", "[--noiseonlyinhalves]", "[--gaussian]", "[--dev <=0>]"):
        assert t in r.stderr, t


BASE = ["--vol", "/nonexistent/a.mrc", "--mask", "/nonexistent/m.mrc", "-o", "/nonexistent", "--minRes", "30", "--maxRes", "1", "--sampling_rate", "1"]


def _shown(r):
    return dict(l.split(": ", 1) for l in r.stdout.splitlines() if ": " in l)


def test_defaults_are_the_reference_ones(xa):
    r = _run(BASE)
    assert r.returncode == 20 and "cannot open" in r.stderr           # the options passed; the missing file stops it, no device yet
    s = _shown(r)
    assert s["step"] == "0.25" and s["significance"] == "0.95" and s["gaussian"] == "0" and s["noiseonlyinhalves"] == "0"
    assert s["minRes"] == "30" and s["maxRes"] == "1" and s["sampling_rate"] == "1"


@pytest.mark.parametrize("given,shown", [("0.1", "0.25"), ("0.25", "0.25"), ("0.7", "0.7")])
def test_step_is_floored(xa, given, shown):
    r = _run(BASE + ["--step", given, "--threads", "9", "--gaussian"])
    s = _shown(r)
    assert s["step"] == shown and s["gaussian"] == "1"


def test_missing_mask_is_an_error(xa):
    r = _run([a for a in BASE if a not in ("--mask", "/nonexistent/m.mrc")])
    assert r.returncode != 0 and "--mask" in r.stderr
    r = _run(BASE[:2] + ["--mask", ""] + BASE[4:])
    assert r.returncode != 0 and "a mask ought to be provided" in r.stderr


def test_bad_device_is_refused(xa):
    r = _run(BASE + ["--dev", "x"])
    assert r.returncode != 0 and "Invalid GPU device" in r.stderr
