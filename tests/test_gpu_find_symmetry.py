"""GPU parity of xmipp_volume_find_symmetry (xh_fsym_*, FindSymmetry in api.py) against the numpy fp64 restatement
(tests/find_symmetry_ref.py): the correlation of every trial of both modes, the search's first maximum above 0, the materialised
volume_sym, independence of the batch capacity, run-to-run identity, the local modes and the program end to end.

Boxes, Z x Y x X: 16^3 (brick-aligned), 17^3 (a remainder on every axis, odd centre), 9 x 10 x 12 (every side different, fewer than two
bricks on an axis), 20 x 18 x 13, 29 x 41 x 43 (288 bricks of 8 x 8 x 4: the finish's loop over bricks t, t + 256, .. takes a second step)
and 37 x 49 x 57 (560 bricks: a third step for threads 0 .. 47).
Axis mode (R.AXIS_CASES): rot_sym 2, 3, 4 and 7, LINEAR and cubic splines, with and without a circular mask; the trials are the planted
axis, the z axis (with rot_sym 4 its coordinates are integers up to the rounding of cos 90), tilt 90 and two generic ones.
Helical mode (R.HELICAL_CASES): rises of 1.0, 4.3 and 5 voxels, Cn 1 and 3, with and without the dihedral copies, heightFraction 0.95 and
1 on an even and an odd Z (0.95 keeps 16 of 17, 19 of 20 and 28 of 29 planes; depth 1 of the recursion is reached on 16^3 and
20 x 18 x 13), a cylinder mask, and four trials the gate refuses mixed into every list. The rise of one voxel runs on every box but
37 x 49 x 57, so also where the finish takes a second step over the bricks (29 x 41 x 43, with the dihedral copies).
Every case of both modes is run at capacities 3, 1 and 64 and a second time: the same bytes from fit and search.
Not covered: the axis cases give each box two of the (rot_sym, interpolation, mask) combinations, so that every value meets every other
on some box, not all twelve on each; cubic splines, a mask and rot_sym 3 together are run on 9 x 10 x 12 alone.

Bound: R.BOUND = 1e-13 relative to max(1, |corr|). It is not taken from the device: tests/test_find_symmetry_ref.py derives it as 16 times
the largest relative difference (6.1e-15) between the restatement's own forms over every trial of every case here, rounded up to a power
of ten, and asserts the preconditions of every case on the restatement alone; 0 trials and 0 voxels are left out. Every correlation is
held to the bound against the restatement and against the exact sums (R.corr_exact). volume_sym: 1e-13 of max|V|, every voxel. The
correlation map file holds 32-bit floats, so half an ulp of them (6e-8 of the value) is added there.
Measured on one MI355X, largest over the cases: correlations 7.7e-15 from the restatement and 5.4e-15 from the exact sums (both on
9 x 10 x 12 with cubic splines under the mask of 257 voxels, where the restatement itself is 6.1e-15 from the exact sums; every other
case below 3.3e-15), volume_sym 5.2e-15 of max|V| with splines (rot_sym 7 on 16^3) and 1.6e-15 for the helix, bit-equal with linear
interpolation. The
local modes end 2.4e-7 degrees and 9.3e-8 voxels from the restatement's own Powell search."""
import os
import subprocess

import numpy as np
import pytest

from tests import find_symmetry_ref as R
from tests import xmipp_io

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PROG = os.path.join(ROOT, "xmipp3_amd", "bin", "xmipp_volume_find_symmetry")


@pytest.fixture(scope="module")
def gpu():
    import torch
    import xmipp3_amd as xa
    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    return xa, xa.Context(0), torch


def rel_to(got, want):
    live = want != R.GATED
    assert np.array_equal(got[~live], want[~live])                   # -1e38 exactly where the gate refuses
    return float((np.abs(got - want)[live] / np.maximum(1.0, np.abs(want[live]))).max())


def axis_handle(gpu, case, capacity=3):
    xa, ctx, _ = gpu
    shape, rot_sym, degree, masked = case
    r = R.axis_case(case)
    fs = xa.FindSymmetry(ctx, shape, capacity)
    fs.set_volume(r["V"], r["mask"], splines=degree == 3)
    return fs, r


def helical_handle(gpu, case, capacity=3):
    xa, ctx, _ = gpu
    r = R.helical_case(case)
    fs = xa.FindSymmetry(ctx, case[0], capacity)
    fs.set_volume(r["V"], r["mask"])
    return fs, r


CAPACITIES = (3, 1, 64, 64)       # 3: two launches of the five axis trials, the second partial; 64 twice: two runs of the same handle shape


@pytest.mark.parametrize("case", R.AXIS_CASES, ids=str)
def test_axis_fit_and_search_against_the_restatement(gpu, case):
    """every trial's correlation within R.BOUND of the restatement and of the exact sums, the chosen index the restatement's, and the
    materialised volume_sym of every trial within 1e-13 of max|V|; then the same bytes at capacities 1, 3 and 64 (5 trials: a multiple
    of neither 3 nor 64) and from a second run, for fit and search alike"""
    shape, rot_sym, degree, masked = case
    fs, r = axis_handle(gpu, case, CAPACITIES[0])
    got = fs.axis_fit(R.AXIS_TRIALS, rot_sym)
    worst = 0.0
    for (rot, tilt), want in zip(R.AXIS_TRIALS, r["vols"]):
        vol = fs.axis_volume(rot, tilt, rot_sym).cpu().numpy()
        worst = max(worst, float(np.abs(vol - want).max() / np.abs(r["V"]).max()))
    print(f"{case} ({R.bricks(shape)} bricks): device to restatement {rel_to(got, r['two']):.3e}, to exact sums {rel_to(got, r['exact']):.3e}, restatement to "
          f"exact sums {rel_to(r['two'], r['exact']):.3e} (bound {R.BOUND:.0e}); volume_sym {worst:.3e} of max|V| (bound 1e-13)")
    assert worst <= 1e-13
    assert rel_to(got, r["two"]) <= R.BOUND and rel_to(got, r["exact"]) <= R.BOUND
    gi, gb, gc = fs.axis_search(R.AXIS_TRIALS, rot_sym, corrs=True)
    assert gi == r["choice"][0] and gc.tobytes() == got.tobytes() and gb == got[gi]
    assert np.allclose(fs.stats(), R.stats(r["V"], r["mask"]), rtol=1e-13, atol=1e-11)
    for capacity in CAPACITIES[1:]:
        other, _ = axis_handle(gpu, case, capacity)
        assert other.axis_fit(R.AXIS_TRIALS, rot_sym).tobytes() == got.tobytes(), capacity
        oi, ob, oc = other.axis_search(R.AXIS_TRIALS, rot_sym, corrs=True)
        assert (oi, ob) == (gi, gb) and oc.tobytes() == got.tobytes(), capacity


@pytest.mark.parametrize("case", R.HELICAL_CASES, ids=str)
def test_helical_fit_and_search_against_the_restatement(gpu, case):
    """as for the axis; the trials the gate refuses come back as -1e38 exactly, without a launch, and are never chosen. The lists hold 3
    or 4 trials that run among 7 or 8: capacity 3 cuts them into two launches or fills one exactly, 1 and 64 do neither"""
    shape, Cn, dihedral, hf, kind = case
    fs, r = helical_handle(gpu, case, CAPACITIES[0])
    got = fs.helical_fit(r["trials"], R.HELICAL_BOX, dihedral, hf, Cn)
    worst = 0.0
    for (rot, z), want in zip(r["trials"], r["vols"]):
        if want is None:
            continue
        vol = fs.helical_volume(rot, z, dihedral, hf, Cn).cpu().numpy()
        worst = max(worst, float(np.abs(vol - want).max() / np.abs(r["V"]).max()))
    print(f"{case} ({R.bricks(shape)} bricks, depth {r['depth']}): device to restatement {rel_to(got, r['two']):.3e}, to exact sums {rel_to(got, r['exact']):.3e}, "
          f"restatement to exact sums {rel_to(r['two'], r['exact']):.3e} (bound {R.BOUND:.0e}); volume_sym {worst:.3e} of max|V| (bound 1e-13)")
    assert worst <= 1e-13
    assert rel_to(got, r["two"]) <= R.BOUND and rel_to(got, r["exact"]) <= R.BOUND
    gi, gb, gc = fs.helical_search(r["trials"], R.HELICAL_BOX, dihedral, hf, Cn, corrs=True)
    assert gi == r["choice"][0] and gc.tobytes() == got.tobytes() and gb == got[gi]
    assert int(fs.stats(clipped=True)[0]) == int((r["clipped"] != 0).sum())
    for capacity in CAPACITIES[1:]:
        other, _ = helical_handle(gpu, case, capacity)
        assert other.helical_fit(r["trials"], R.HELICAL_BOX, dihedral, hf, Cn).tobytes() == got.tobytes(), capacity
        oi, ob, oc = other.helical_search(r["trials"], R.HELICAL_BOX, dihedral, hf, Cn, corrs=True)
        assert (oi, ob) == (gi, gb) and oc.tobytes() == got.tobytes(), capacity


def test_the_first_maximum_across_chunks_and_launches(gpu):
    """600 trials drawn from the five of a case, the winner planted at 299, 300 and 599 (the last of one chunk and the first of the next of
    the choice kernel when a launch holds all 600, three to a thread; the last of one launch and the first of the next at capacity 300),
    then at 599 alone, then nowhere with the runner-up at 1 and 598: the first of the equal maxima is taken every time, at capacities
    1024, 300, 256 and 7, and the 600 correlations are the same bytes at all four"""
    case = ((9, 10, 12), 7, 1, False)
    r = R.axis_case(case)
    order = np.argsort(r["two"])
    best, second, rest = int(order[-1]), int(order[-2]), [int(o) for o in order[:-2]]
    filler = [rest[t % len(rest)] for t in range(600)]
    for planted, runner, want in (((299, 300, 599), (), 299), ((599,), (), 599), ((), (1, 598), 1)):
        pool = list(filler)
        for t in planted:
            pool[t] = best
        for t in runner:
            pool[t] = second
        tr = R.AXIS_TRIALS[pool]
        assert R.choose(r["two"][pool])[0] == want
        seen = set()
        for capacity in (1024, 300, 256, 7):
            fs, _ = axis_handle(gpu, case, capacity)
            gi, gb, gc = fs.axis_search(tr, case[1], corrs=True)
            assert gi == want and gb == gc[want], capacity
            # equal trials give equal bits wherever they sit
            for q in range(len(R.AXIS_TRIALS)):
                assert len(set(gc[np.array(pool) == q].tolist())) <= 1
            seen.add(gc.tobytes())
        assert len(seen) == 1


def test_a_search_with_no_positive_correlation_answers_no_trial(gpu):
    """a constant volume: every correlation is 0, none is above the 0 the best starts at; the handle answers (-1, 0) and the program
    rot = tilt = 0. Gated helical trials alone: no launch at all"""
    xa, ctx, _ = gpu
    fs = xa.FindSymmetry(ctx, (9, 10, 12), 2)
    fs.set_volume(np.full((9, 10, 12), 0.37))
    gi, gb, gc = fs.axis_search(R.AXIS_TRIALS, 3, corrs=True)
    assert (gi, gb) == (-1, 0.0) and gc.tolist() == [0.0] * len(R.AXIS_TRIALS)
    gi, gb, gc = fs.helical_search([(10.0, -1.0), (10.0, 9.0), (400.0, 2.0)], R.HELICAL_BOX, corrs=True)
    assert (gi, gb) == (-1, 0.0) and gc.tolist() == [R.GATED] * 3


def test_refused_trials(gpu):
    xa, ctx, _ = gpu
    fs = xa.FindSymmetry(ctx, (16, 16, 16), 2)
    with pytest.raises(xa.XhError, match="no volume"):
        fs.axis_fit(R.AXIS_TRIALS, 3)
    fs.set_volume(R.helix_phantom((16, 16, 16)))
    with pytest.raises(xa.XhError, match="not finite"):
        fs.axis_fit([(np.nan, 0.0)], 3)
    for n in (1, 100):
        with pytest.raises(xa.XhError, match="rot_sym"):
            fs.axis_fit(R.AXIS_TRIALS, n)
    with pytest.raises(xa.XhError, match="Cn = 0"):
        fs.helical_fit([R.TRUE_HELIX], cn=0)
    with pytest.raises(xa.XhError, match="not finite"):
        fs.helical_fit([(0.0, np.inf)])
    # an ungated trial the recursion bound does not admit: a rise of 0, and the dihedral copies over the whole even Z below one voxel
    with pytest.raises(xa.XhError, match="recursion has no bound"):
        fs.helical_fit([R.TRUE_HELIX, (10.0, 0.0)])
    with pytest.raises(xa.XhError, match="recursion has no bound"):
        fs.helical_fit([(10.0, 0.5)], dihedral=True, height_fraction=1.0)
    assert fs.helical_fit([(10.0, 0.5)], dihedral=True, height_fraction=0.95)[0] > 0
    with pytest.raises(xa.XhError, match="recursion has no bound"):
        fs.helical_fit([R.TRUE_HELIX], height_fraction=1.5)


def _local_case(mode):
    shape = (16, 16, 16)
    if mode == "axis":
        V = R.axis_phantom(shape, 3)
        return V, None, (lambda p: -R.axis_corr(V, p[0], p[1], 3)), np.array(R.TRUE_AXIS) + (2.0, -2.0)
    V = R.helix_phantom(shape)
    mask = R.cylinder_mask(shape, -6.0, -13.0)
    box = (1.0, 10.0, -357.0, 357.0)                              # the program's defaults
    cost = lambda p: -R.helical_corr(V, p[0], p[1], mask, box)   # noqa: E731
    return V, mask, cost, np.array(R.TRUE_HELIX) + (3.0, 0.4)


@pytest.mark.parametrize("mode", ("axis", "helical"))
def test_local_modes_land_within_the_ftol_margin(gpu, mode, tmp_path):
    """--localRot and --localHelical of the program against the same Powell search over the restatement's cost. Powell (ftol 0.01) ends
    when a sweep lowers the cost by less than 1 %, so a variable is determined no better than the step that changes the cost by 1 % of its
    minimum: R.ftol_halfwidth measures that step per variable on the restatement (the grid 1e-3 2^k), and the restatement's own spread
    under a start moved by 1e-12 must lie inside it too"""
    xa = gpu[0]
    V, mask, cost, x0 = _local_case(mode)
    best, fmin, _ = xa.powell_minimize(cost, x0, [1.0, 1.0], 0.01)
    moved, _, _ = xa.powell_minimize(cost, x0 + 1e-12, [1.0, 1.0], 0.01)
    margin = R.ftol_halfwidth(cost, best)
    print(f"{mode}: restatement ends at {best} (cost {fmin:.6f}); margin {margin}; spread under a 1e-12 move of the start {np.abs(moved - best)}")
    assert np.all(margin > 0) and np.all(np.abs(moved - best) <= margin)
    xmipp_io.write_volume(tmp_path / "v.vol", V)
    if mode == "axis":
        args = ["--sym", "rot", 3, "--localRot", x0[0], x0[1]]
    else:
        args = ["--sym", "helical", "--localHelical", x0[1], x0[0], "--mask", "cylinder", -6, -13]
    r = subprocess.run([PROG, "-i", str(tmp_path / "v.vol"), "-o", str(tmp_path / "out.xmd")] + [str(a) for a in args], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    labels, rows = xmipp_io.read_xmd(tmp_path / "out.xmd")
    row = dict(zip(labels, rows[0]))
    got = np.array([float(row["angleRot"]), float(row["angleTilt" if mode == "axis" else "shiftZ"])])
    print(f"program: {got}; differences {np.abs(got - best)}")
    assert np.all(np.abs(got - best) <= margin + 1e-6)           # the metadata carries six decimals
    assert abs(cost(got) - fmin) <= 0.01 * abs(fmin)
    assert not os.path.exists(tmp_path / "out.xmp")               # no map in the local mode (:345)


def _g(v):
    return f"{v:g}"


def test_program_end_to_end_axis(gpu, tmp_path):
    """a 3 x 3 grid around the planted axis on files, cubic splines and a circular mask: the stdout line and the -o metadata"""
    shape, rot_sym = (17, 17, 17), 3
    V = R.axis_phantom(shape, rot_sym)
    mask = R.circular_mask(shape, -7.0)
    xmipp_io.write_volume(tmp_path / "v.vol", V)
    tr, ny, nx = R.grid((35, 45, 5), (50, 60, 5))
    assert (len(tr), ny, nx) == (9, 3, 3)
    coef = R.prefilter(V)
    corrs = np.array([R.axis_corr(V, rot, tilt, rot_sym, 3, mask, coef=coef) for rot, tilt in tr])
    idx, best = R.choose(corrs)
    assert tuple(tr[idx]) == R.TRUE_AXIS and np.sort(corrs)[-1] - np.sort(corrs)[-2] >= 1e-6
    r = subprocess.run([PROG, "-i", str(tmp_path / "v.vol"), "--sym", "rot", "3", "--rot", "35", "45", "5", "--tilt", "50", "60", "5", "--useSplines", "--mask", "circular",
                        "-7", "--thr", "4", "-o", str(tmp_path / "axis.xmd")], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    axis = R.axis_of(*R.TRUE_AXIS)
    assert r.stdout.splitlines() == ["Symmetry axis (rot,tilt)= 40 55 --> " + "".join(f"{_g(v):>10} " for v in axis)]
    assert "Searching symmetry axis ..." in r.stderr
    labels, rows = xmipp_io.read_xmd(tmp_path / "axis.xmd")
    row = dict(zip(labels, rows[0]))
    assert labels == ["angleRot", "angleTilt", "direction"] and float(row["angleRot"]) == 40.0 and float(row["angleTilt"]) == 55.0
    assert row["direction"].strip("'") == "[ " + " ".join(f"{v:.6f}" for v in axis) + " ]"
    # a constant volume: no correlation above 0, the answer is rot = tilt = 0 and the axis z
    xmipp_io.write_volume(tmp_path / "flat.vol", np.full(shape, 0.37))
    r = subprocess.run([PROG, "-i", str(tmp_path / "flat.vol"), "--sym", "rot", "3", "--rot", "35", "45", "5", "--tilt", "50", "60", "5"], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    assert r.stdout.splitlines() == ["Symmetry axis (rot,tilt)= 0 0 --> " + "".join(f"{_g(v):>10} " for v in (0.0, 0.0, 1.0))]


def test_program_end_to_end_helical(gpu, tmp_path):
    """a 3 x 4 grid around the planted helix on files, sampling 2 A / voxel, helicalDihedral with C1 under a cylinder mask: the stdout line,
    the -o metadata and the correlation map. The last column of the map is gated: 13.8 A = 6.9 voxels is above 0.4 Z = 6.8. The column of
    8.6 A = 4.3 voxels, the planted rise, wins"""
    shape, Ts = (17, 17, 17), 2.0
    V = R.helix_phantom(shape)
    mask = R.cylinder_mask(shape, -7.0, -14.0)
    xmipp_io.write_volume(tmp_path / "v.vol", V)
    rz = (-55, -45, 5)
    zz = (6.0 / Ts, 13.8 / Ts, 2.6 / Ts)
    tr, ny, nx = R.grid(rz, zz)
    assert (ny, nx) == (3, 4)
    box = (zz[0], zz[1], rz[0], rz[1])
    corrs = np.array([R.helical_corr(V, rot, z, mask, box, True, 1.0, 1) for rot, z in tr])
    assert (corrs == R.GATED).sum() == 3
    idx, best = R.choose(corrs)
    live = np.sort(corrs[corrs != R.GATED])
    assert tr[idx][0] == -50 and abs(tr[idx][1] - 4.3) < 1e-12 and live[-1] - live[-2] >= 1e-6
    r = subprocess.run([PROG, "-i", str(tmp_path / "v.vol"), "--sym", "helicalDihedral", "--sampling", "2", "-z", "6", "13.8", "2.6", "--rotHelical", "-55", "-45", "5",
                        "--mask", "cylinder", "-7", "-14", "-o", str(tmp_path / "helix.xmd")], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    line = r.stdout.splitlines()
    assert len(line) == 1 and line[0].startswith(f"Symmetry parameters (z,rot)= {_g(tr[idx][1] * Ts)} -50 correlation=")
    assert abs(float(line[0].split("correlation=")[1]) - best) <= 1e-5 * abs(best)      # six significant digits
    labels, rows = xmipp_io.read_xmd(tmp_path / "helix.xmd")
    row = dict(zip(labels, rows[0]))
    assert labels == ["angleRot", "shiftZ"] and float(row["angleRot"]) == -50.0 and abs(float(row["shiftZ"]) - tr[idx][1] * Ts) <= 1e-6
    got = xmipp_io.read_volume(tmp_path / "helix.xmp").astype(np.float64)
    assert got.shape == (1, ny, nx)
    want = corrs.reshape(ny, nx)
    gated = want == R.GATED
    assert np.array_equal(got[0][gated], np.full(int(gated.sum()), np.float64(np.float32(R.GATED))))
    assert np.all(np.abs(got[0] - want)[~gated] <= (R.BOUND + 6e-8) * np.maximum(1.0, np.abs(want[~gated])))
