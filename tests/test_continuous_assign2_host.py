"""CPU checks of the continuous assignment's host machinery: the lockstep Powell scheduler (xh_powell_minimize_batch, one coroutine per
search) must return, bit for bit, what the sequential minimiser returns problem by problem; the program's flags, refusals and its
XMIPP_ERROR where no device is present."""
import os
import subprocess

import numpy as np
import pytest

from tests import xmipp_io

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PROG = os.path.join(ROOT, "xmipp3_amd", "bin", "xmipp_angular_continuous_assign2")


@pytest.fixture(scope="module")
def xa():
    import __graft_entry__ as g
    g.build()
    import xmipp3_amd
    return xmipp3_amd


# analytic costs of mixed dimension (those of test_halves_restoration_host.py's Powell tests and the like)
def _rosenbrock(x):
    return (1 - x[0]) ** 2 + 100 * (x[1] - x[0] ** 2) ** 2


def _quadratic(x):
    return 1.0 + (x[0] - 0.3) ** 2 + 2 * (x[1] + 1.1) ** 2 + 0.5 * (x[0] - 0.3) * (x[1] + 1.1) + 0.7 * (x[2] - 2.0) ** 2


def _barrier(x):
    if x[0] < 0 or x[1] < 0 or x[0] > 2 or x[1] > 2:
        return 1e38
    return 0.5 + (x[0] - 0.7) ** 2 + 2 * (x[1] - 1.3) ** 2 + 0.3 * (x[0] - 0.7) * (x[1] - 1.3)


def _barrier_edge(x):
    if x[0] < 0 or x[1] < 0 or x[0] > 2 or x[1] > 2:
        return 1e38
    return 2.0 + (x[0] - 2.5) ** 2 + (x[1] - 0.4) ** 2


def _parabola(x):
    return 3.0 + (x[0] - 1.25) ** 2


def _cosines(x):
    return -sum(np.cos(0.7 * (v - 0.2 * (k + 1))) for k, v in enumerate(x)) + 0.05 * sum(v * v for v in x)


def _quartic(x):
    return 1.0 + sum((k + 1) * (v - 0.1 * k) ** 4 + 0.3 * (v - 0.1 * k) ** 2 for k, v in enumerate(x)) + 0.2 * x[0] * x[-1]


def _always_barrier(x):
    return 1e38


def _problems():
    """50 problems, dimensions 1 .. 6, mixed starting points"""
    rng = np.random.default_rng(20)
    fixed = {1: [_parabola, _cosines], 2: [_rosenbrock, _barrier, _barrier_edge, _cosines, _always_barrier], 3: [_quadratic, _quartic, _cosines],
             4: [_cosines, _quartic], 5: [_cosines, _quartic], 6: [_cosines, _quartic]}
    out = []
    for q in range(50):
        n = 1 + q % 6
        f = fixed[n][(q // 6) % len(fixed[n])]
        if f in (_barrier, _barrier_edge):
            p0 = rng.uniform(0.05, 1.95, n)
        elif f is _rosenbrock:
            p0 = np.array([-1.2, 1.0]) + rng.uniform(-0.2, 0.2, 2)
        else:
            p0 = rng.uniform(-2, 2, n)
        out.append((f, p0, rng.uniform(0.5, 1.5, n)))
    assert sorted({len(p) for _, p, _ in out}) == [1, 2, 3, 4, 5, 6] and any(f is _barrier for f, _, _ in out)
    return out


@pytest.mark.parametrize("capacity", [7, 1, 64])
def test_lockstep_is_the_sequential_search_bit_for_bit(xa, capacity):
    probs = _problems()
    seq = [xa.powell_minimize(f, p0, st, 0.01) for f, p0, st in probs]
    calls, seen = [], np.zeros(len(probs), np.int64)

    def batch(idx, rows):
        calls.append(len(idx))
        assert len(set(idx)) == len(idx)
        for i in idx:
            seen[i] += 1
        return [probs[i][0](r) for i, r in zip(idx, rows)]

    p, fret, it, ev = xa.powell_minimize_batch(batch, [p0 for _, p0, _ in probs], [st for _, _, st in probs], 0.01, capacity)
    for q, (ps, fs, its) in enumerate(seq):
        assert p[q].tobytes() == np.asarray(ps, np.float64).tobytes(), (q, p[q], ps)
        assert np.float64(fret[q]).tobytes() == np.float64(fs).tobytes(), (q, fret[q], fs)
        assert it[q] == its
        assert ev[q] >= 1
    assert max(calls) <= capacity and min(calls) >= 1
    if capacity == 7:
        assert max(calls) == 7 and calls[-1] < 7         # slots were refilled, and the last batches ran ragged
    # the callback never sees a finished problem: a problem appears exactly once per cost call its search made (ev is counted inside
    # the search, so a row sent after the search ended would make the count larger), which is also what the sequential search made
    seq_calls = []
    for f, p0, st in probs:
        c = [0]

        def g(x, f=f, c=c):
            c[0] += 1
            return f(x)
        xa.powell_minimize(g, p0, st, 0.01)
        seq_calls.append(c[0])
    assert list(seen) == list(ev) == seq_calls
    # a search that the barrier decides everywhere ends at its start
    for q, (f, p0, _) in enumerate(probs):
        if f is _always_barrier:
            assert fret[q] == 1e38 and p[q].shape == p0.shape


def test_lockstep_counts_cost_calls(xa):
    counts = {}

    def batch(idx, rows):
        for i in idx:
            counts[i] = counts.get(i, 0) + 1
        return [_quadratic(r) for r in rows]

    starts = [[0.0, 0.0, 0.0], [5.0, -4.0, 1.0], [1.0, 1.0, 1.0]]
    _, _, _, ev = xa.powell_minimize_batch(batch, starts, None, 0.01, 2)
    assert [counts[i] for i in range(3)] == list(ev)


def test_lockstep_callback_failure_ends_the_run(xa):
    def batch(idx, rows):
        raise ValueError("cost failed")

    with pytest.raises(ValueError, match="cost failed"):
        xa.powell_minimize_batch(batch, [[0.0, 0.0], [1.0, 1.0], [2.0, 2.0]], None, 0.01, 2)
    # and the library is still usable afterwards
    p, f, it, _ = xa.powell_minimize_batch(lambda idx, rows: [_parabola(r) for r in rows], [[0.0]], None, 0.01, 2)
    assert abs(p[0][0] - 1.25) < 1e-3


def test_lockstep_refuses_bad_arguments(xa):
    from xmipp3_amd._lib import XhError
    with pytest.raises(XhError):
        xa.powell_minimize_batch(lambda idx, rows: [0.0] * len(idx), [[0.0]], None, 0.01, 0)


# ---------------------------------------------------------------- the program
def _run(args):
    return subprocess.run([PROG] + args, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=300)


def test_help_lists_every_reference_flag_with_its_default(xa):
    assert os.path.exists(PROG)
    r = _run(["--help"])
    assert r.returncode == 0 and "Make a continuous angular assignment" in r.stderr
    for line in ("-i <arg>", "-o <arg>", "--ref <arg>", "[--max_shift <=-1>]", "[--max_scale <=0.02>]", "[--max_angular_change <=5>]",
                 "[--max_defocus_change <=500>]", "[--max_resolution <=4>]", "[--max_gray_scale <=0.05>]", "[--max_gray_shift <=0.05>]",
                 "[--sampling <=1>]", "[--Rmax <=-1>]", "[--padding <=2>]", "[--optimizeGray]", "[--optimizeShift]", "[--optimizeScale]",
                 "[--optimizeAngles]", "[--optimizeDefocus]", "[--ignoreCTF]", "[--applyTo <=image>]", "[--phaseFlipped]", "[--sameDefocus]",
                 "[--oresiduals", "[--oprojections", "[--dev <=0>]", "[--batch <=4096>]"):
        assert line in r.stderr, line
    for ignored in ("--nThreads", "--skipThreshold"):
        assert [l for l in r.stderr.splitlines() if ignored in l and "ignored" in l]
    assert "corrWeight is not computed" in r.stderr


@pytest.mark.parametrize("args,msg", [
    (["-i", "a.xmd", "-o", "o.stk", "--optimizeShift"], "--ref is mandatory"),
    (["-i", "a.xmd", "-o", "o.stk", "--ref", "v.vol", "--optimizeShift", "--noSuchFlag"], "noSuchFlag"),
    (["-i", "a.xmd", "-o", "o.stk", "--ref", "v.vol", "--optimizeShift", "--dev", "0", "1"], "several devices are not supported"),
    (["-i", "a.xmd", "-o", "o.stk", "--ref", "v.vol"], "nothing to search"),
])
def test_refusals(xa, args, msg):
    r = _run(args)
    assert r.returncode != 0 and "XMIPP_ERROR" in r.stderr and msg in r.stderr, r.stderr


def test_no_gpu_means_xmipp_error_not_fallback(xa, tmp_path):
    import torch
    if torch.cuda.is_available():
        pytest.skip("a GPU is present")
    D = 16
    rng = np.random.default_rng(0)
    xmipp_io.write_volume(str(tmp_path / "ref.vol"), rng.standard_normal((D, D, D)).astype(np.float32))
    xmipp_io.write_stack(str(tmp_path / "in.stk"), rng.standard_normal((2, D, D)).astype(np.float32))
    xmipp_io.write_xmd(str(tmp_path / "in.xmd"), [("noname", ["image", "angleRot", "angleTilt", "anglePsi"],
                                                    [[f"{i + 1}@{tmp_path / 'in.stk'}", 10.0, 20.0, 30.0] for i in range(2)])])
    r = _run(["-i", str(tmp_path / "in.xmd"), "-o", str(tmp_path / "out.stk"), "--ref", str(tmp_path / "ref.vol"), "--optimizeShift"])
    assert r.returncode != 0 and "XMIPP_ERROR" in r.stderr and "no CPU fallback" in r.stderr
    assert not (tmp_path / "out.xmd").exists()
