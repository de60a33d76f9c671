"""GPU parity of xmipp_volume_align (xh_valign_*, VolumeAlign in api.py) against the numpy fp64 restatement (tests/volume_align_ref.py):
the fit of every trial, the search's first minimum, independence of the batch capacity, run-to-run identity, the materialised
applyTransformation, the Powell branch and the program end to end.

Boxes, Z x Y x X: 16^3 (brick-aligned), 17^3 (a remainder on every axis, odd centre), 9 x 10 x 12 (every side different, fewer than two
bricks on an axis), 20 x 18 x 13, 29 x 41 x 43 (288 bricks of 8 x 8 x 4: k_va_finish's loop over bricks t, t + 256, .. takes a second
step) and 37 x 49 x 57 (560 bricks: a third step for threads 0 .. 47). Both methods, wrap on and off, with and without a circular mask, both flips, grey values other than
1 / 0 under LEAST_SQUARES. The trial lists (R.trial_list): generic poses, the identity, integer shifts, a shift larger than the box under
wrap, poses that send most of the box outside under dontWrap.

Bound: R.BOUND = 1e-14 relative to max(1, |fit|). It is not taken from the device: tests/test_volume_align_ref.py derives it as 16 times
the largest relative difference (5.0e-16) between the restatement's two-pass fit and the one-pass identity over every trial of every case
here, rounded up to a power of ten. The same CPU test asserts the preconditions of every case on the restatement alone: no tested
coordinate within 1e-9 of a threshold min - 1e-6 / max + 1e-6 or of a wrap edge, the best fit at least 1e-6 below the runner-up; 0 trials
and 0 voxels are left out. apply: 1e-13 of max|V2|, every voxel. Files: the output is float32, so half an ulp of it (6e-8 of the largest
value) is added.
The device adds the 10^5 terms of the two large boxes in another order than numpy, so every fit is also held to R.BOUND against
R.fitness_exact: the same per-voxel fp64 terms summed with math.fsum, then the device's finish in double. The same CPU test holds the
restatement to that bound against the exact sums.
Measured on one MI355X: fit, COVARIANCE 1.9e-15, LEAST_SQUARES 2.0e-16; apply 0 (the same bits).
Measured on one MI355X, fit against the restatement / against the exact sums (restatement against the exact sums), largest per box:
29 x 41 x 43 COVARIANCE 5.6e-16 / 5.6e-16 (2.8e-16), LEAST_SQUARES 2.8e-17 / 2.8e-17 (2.8e-17); 37 x 49 x 57 COVARIANCE 4.4e-16 /
1.9e-16 (4.4e-16), LEAST_SQUARES 2.8e-17 / 2.8e-17 (2.8e-17); the four small boxes against the exact sums 1.0e-15 (restatement 1.8e-15)."""
import os
import subprocess

import numpy as np
import pytest

from tests import volume_align_ref as R
from tests import xmipp_io

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PROG = os.path.join(ROOT, "xmipp3_amd", "bin", "xmipp_volume_align")


@pytest.fixture(scope="module")
def gpu():
    import torch
    import xmipp3_amd as xa
    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    return xa, xa.Context(0), torch


_REF = {}


def ref(shape, method, wrap, masked):
    """(trials, index, best, fits) of a case on the restatement, computed once"""
    key = (shape, method, wrap, masked)
    if key not in _REF:
        V1, V2 = R.volumes(shape, wrap)
        tr = R.trial_list(shape, method, wrap)
        _REF[key] = (tr,) + R.search(V1, V2, tr, method, wrap, R.case_mask(shape, masked))
    return _REF[key]


_EXACT = {}


def exact(shape, method, wrap, masked):
    """the fits of a case from exact sums (R.fitness_exact), computed once"""
    key = (shape, method, wrap, masked)
    if key not in _EXACT:
        V1, V2 = R.volumes(shape, wrap)
        mask = R.case_mask(shape, masked)
        _EXACT[key] = np.array([R.fitness_exact(V1, V2, p, method, wrap, mask) for p in R.trial_list(shape, method, wrap)])
    return _EXACT[key]


def rel_to(got, want):
    return float((np.abs(got - want) / np.maximum(1.0, np.abs(want))).max())


def loaded(gpu, shape, wrap, masked, capacity=5):
    xa, ctx, _ = gpu
    va = xa.VolumeAlign(ctx, shape, capacity)
    V1, V2 = R.volumes(shape, wrap)
    va.set_volumes(V1, V2, R.case_mask(shape, masked))
    return va


@pytest.mark.parametrize("shape,method,wrap,masked", R.parity_cases())
def test_fit_and_search_against_the_restatement(gpu, shape, method, wrap, masked):
    """every trial's fit within R.BOUND of the restatement and of the exact sums; the search's index is the restatement's. Capacity 5:
    three launches, the last one partial. (29, 41, 43): 288 bricks, threads 0 .. 31 of k_va_finish take a second step; (37, 49, 57): 560
    bricks, threads 0 .. 47 add three and the others two"""
    tr, idx, best, fits = ref(shape, method, wrap, masked)
    va = loaded(gpu, shape, wrap, masked)
    got = va.fit(tr, method, wrap)
    rel = np.abs(got - fits) / np.maximum(1.0, np.abs(fits))
    ex = exact(shape, method, wrap, masked)
    print(f"{shape} ({R.bricks(shape)} bricks) method {method} wrap {wrap} masked {masked}: largest difference {rel.max():.3e} (bound {R.BOUND:.0e}); "
          f"device to exact sums {rel_to(got, ex):.3e}, restatement to exact sums {rel_to(fits, ex):.3e}")
    assert rel_to(got, ex) <= R.BOUND
    assert rel.max() <= R.BOUND
    gi, gb, gf = va.search(tr, method, wrap, fits=True)
    assert gi == idx and gf.tobytes() == got.tobytes() and gb == got[idx]
    if not masked:
        want = R.stats(R.volumes(shape, wrap)[0], None)
        assert np.allclose(va.stats(), want, rtol=1e-13, atol=1e-11)


def test_first_of_two_identical_trials_and_a_best_in_the_second_batch(gpu):
    """the planted pose sits at 6 and again at 11 of a list searched four at a time: the second launch holds the winner, the third its twin"""
    shape, method, wrap = (16, 16, 16), R.COVARIANCE, True
    base = R.trial_list(shape, method, wrap)
    tr = np.concatenate([base[1:7], base[:1], base[7:], base[1:2], base[:1], base[2:5]])
    assert np.array_equal(tr[6], tr[11]) and np.array_equal(tr[6], R.PLANTED)
    V1, V2 = R.volumes(shape, wrap)
    idx, best, fits = R.search(V1, V2, tr, method, wrap)
    assert idx == 6 and fits[11] == fits[6] and np.sort(fits)[2] - best >= 1e-6
    va = loaded(gpu, shape, wrap, False, capacity=4)
    gi, gb, gf = va.search(tr, method, wrap, fits=True)
    assert gi == 6 and gf[6] == gf[11] == gb


@pytest.mark.parametrize("method,wrap,masked", [(R.COVARIANCE, True, True), (R.LEAST_SQUARES, False, False)])
def test_capacity_changes_no_byte_and_two_runs_agree(gpu, method, wrap, masked):
    shape = (17, 17, 17)
    tr = R.trial_list(shape, method, wrap)[:7]
    out = []
    for capacity in (1, 3, len(tr), len(tr)):
        va = loaded(gpu, shape, wrap, masked, capacity)
        gi, gb, gf = va.search(tr, method, wrap, fits=True)
        again = va.fit(tr, method, wrap)
        assert again.tobytes() == gf.tobytes()
        out.append((gi, gb, gf.tobytes()))
    assert all(o == out[0] for o in out)


@pytest.mark.parametrize("shape", R.SHAPES)
@pytest.mark.parametrize("wrap", (True, False))
def test_apply_against_the_restatement(gpu, shape, wrap):
    V1, V2 = R.volumes(shape, wrap)
    va = loaded(gpu, shape, wrap, False)
    worst = 0.0
    for p in R.trial_list(shape, R.LEAST_SQUARES, wrap):
        got = va.apply(p, wrap).cpu().numpy()
        worst = max(worst, np.abs(got - R.apply_transformation(V2, p, wrap)).max() / np.abs(V2).max())
    print(f"{shape} wrap {wrap}: apply, largest difference {worst:.3e} of max|V2| (bound 1e-13)")
    assert worst <= 1e-13


def test_refused_trials(gpu):
    xa = gpu[0]
    va = loaded(gpu, (9, 10, 12), True, False)
    with pytest.raises(xa.XhError, match="singular"):
        va.fit([[1, 1, 0, 0, 0, 0, 0.0, 0, 0, 0]])
    with pytest.raises(xa.XhError, match="not finite"):
        va.fit([[1, 1, 0, np.nan, 0, 0, 1, 0, 0, 0]])
    with pytest.raises(xa.XhError, match="method 3"):
        va.fit([R.PLANTED], method=3)
    with pytest.raises(xa.XhError, match="no volumes"):
        xa.VolumeAlign(gpu[1], (9, 10, 12), 2).fit([R.PLANTED])


def test_local_search_against_the_restatement(gpu):
    """--local with a mirror search on 16^3 from a start 2 degrees and 0.7 voxels off the planted pose: the device's costs under the
    lockstep Powell (two problems, capacity 2) against the restatement's under the plain one. The winner's flip is the restatement's and
    every variable of the winner is within the Powell tolerance of the restatement's.
    The margin: Powell (ftol 0.01) ends when a sweep lowers the fit by less than 1 %, so a variable is determined no better than the step
    that changes the fit by 1 % of its minimum. R.ftol_halfwidths measures that step per variable on the restatement (the grid 1e-3 2^k):
    2.048 degrees, 0.016 of scale and 0.256 voxels here. It is measured against the restatement's own spread: the same search from a
    start moved by 1e-12 ends up to 0.9 degrees, 0.0007 of scale and 0.03 voxels away (a comparison inside Powell flips and the search
    stops a sweep earlier), which must lie inside the margin too"""
    xa = gpu[0]
    shape, method, wrap = (16, 16, 16), R.COVARIANCE, True
    V1, V2 = R.volumes(shape, wrap)
    steps = R.local_steps(method)
    x0 = np.array(R.PLANTED[1:]) + [0, 0, 2.0, -2.0, 2.0, 0, 0.7, -0.7, 0.7]
    best, best_fit, runs = R.local(xa.powell_minimize, V1, V2, x0, method, wrap, consider_mirror=True)
    _, _, moved = R.local(xa.powell_minimize, V1, V2, x0 + 1e-12 * steps, method, wrap)
    margin = R.ftol_halfwidths(V1, V2, best, method, wrap)
    spread = np.abs(moved[0][0] - runs[0][0])
    print(f"restatement: best {best}, fit {best_fit:.6f}\nmargin {margin}\nspread under a 1e-12 move of the start {spread}")
    assert best[0] == 1.0 and np.all(margin[steps != 0] > 0) and np.all(spread <= margin)
    va = loaded(gpu, shape, wrap, False, capacity=2)

    def cost(idx, rows):
        return va.fit([[-1.0 if q else 1.0] + list(r) for q, r in zip(idx, rows)], method, wrap)
    xs, fret, _, evals = xa.powell_minimize_batch(cost, [x0, x0], [steps, steps], 0.01, capacity=2)
    win = 0 if fret[0] <= fret[1] else 1                      # fitness < best_fit || first, mirror 0 first
    diff = np.abs(xs[win] - best[1:])
    print(f"device: flip {-1.0 if win else 1.0}, fits {fret}, cost calls {evals}; differences of the variables {diff}")
    assert (-1.0 if win else 1.0) == best[0]
    assert np.all(diff <= margin)
    assert abs(fret[win] - best_fit) <= 0.01 * abs(best_fit)


def _g(v):
    return f"{v:g}"


def test_program_end_to_end(gpu, tmp_path):
    """a 3 x 3 x 3 grid of angles around the planted pose on files: the stdout block, --copyGeo, --copyGray, --store and the --apply volume"""
    shape, wrap = (17, 17, 17), True
    V1, V2 = R.volumes(shape, wrap)
    xmipp_io.write_volume(tmp_path / "v1.vol", V1)
    xmipp_io.write_volume(tmp_path / "v2.vol", V2)
    ranges = [(1, 1, 1), (0, 0, 1), (8.7, 18.7, 5), (36.3, 46.3, 5), (-32.9, -22.9, 5), (0.93, 0.93, 1), (1.3, 1.3, 1), (-2.6, -2.6, 1), (0.4, 0.4, 1)]
    tr, _ = R.trials(ranges)
    margin, edge = R.preconditions(shape, tr, wrap)
    assert len(tr) == 27 and margin >= 1e-9 and edge == 0
    idx, best, fits = R.search(V1, V2, tr, R.COVARIANCE, wrap)
    assert np.sort(fits)[1] - best >= 1e-6
    b = tr[idx]
    args = [PROG, "--i1", tmp_path / "v1.vol", "--i2", tmp_path / "v2.vol", "--rot", 8.7, 18.7, 5, "--tilt", 36.3, 46.3, 5, "--psi", -32.9, -22.9, 5,
            "--scale", 0.93, 0.93, 1, "-z", 1.3, 1.3, 1, "-y", -2.6, -2.6, 1, "-x", 0.4, 0.4, 1, "--apply", tmp_path / "out.vol",
            "--copyGeo", tmp_path / "geo.txt", "--copyGray", tmp_path / "gray.txt", "--store", tmp_path / "store.txt"]
    r = subprocess.run([str(a) for a in args], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    A = R.matrix(b)[0]
    assert r.stdout.splitlines() == [
        "The best correlation is for", "Mirroring the in X axis: 0", f"Scale                  : {_g(b[6])}",
        f"Translation (X,Y,Z)    : {_g(b[9])} {_g(b[8])} {_g(b[7])}", f"Rotation (rot,tilt,psi): {_g(b[3])} {_g(b[4])} {_g(b[5])}",
        "Best grey scale       : 1", "Best grey shift       : 0", f"Fitness value         : {_g(best)}",
        "xmipp_transform_geometry will require the following values", f"   Angles: {_g(b[3])} {_g(b[4])} {_g(b[5])}",
        f"   Shifts: {_g(A[0, 3])} {_g(A[1, 3])} {_g(A[2, 3])}"]
    assert open(tmp_path / "geo.txt").read() == "".join(_g(v) + "\n" for v in A.ravel()) + "\n"
    assert open(tmp_path / "gray.txt").read() == "1\n0\n\n"
    assert open(tmp_path / "store.txt").read() == ", ".join(_g(v) for v in (b[3], b[4], b[5], A[0, 3], A[1, 3], A[2, 3], best)) + "\n"
    out = xmipp_io.read_volume(tmp_path / "out.vol").astype(np.float64)
    want = R.apply_transformation(V2, b, wrap)
    assert np.abs(out - want).max() <= (1e-13 + 6e-8) * np.abs(want).max()
    # --show_fit on the mirror pair of the best trial: the header, every trial with its fit, Best so far where the reference prints it
    r = subprocess.run([str(a) for a in args[:5]] + ["--rot", str(b[3]), str(b[3]), "1", "--tilt", str(b[4]), str(b[4]), "1", "--psi", str(b[5]), str(b[5]), "1",
                                                      "--scale", "0.93", "0.93", "1", "-z", "1.3", "1.3", "1", "-y", "-2.6", "-2.6", "1", "-x", "0.4", "0.4", "1",
                                                      "--consider_mirror", "--show_fit", "-v", "0"], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    lines = r.stdout.splitlines()
    mirror = np.array(b)
    mirror[0] = -1.0
    fm = R.fitness(V1, V2, mirror, R.COVARIANCE, wrap)
    assert fm > best
    assert lines[:2] == ["#grey_factor rot tilt psi scale z y x fitness", "Best so far"]
    assert lines[2] == " ".join(_g(v) for v in b) + " " + _g(best) and lines[3] == " ".join(_g(v) for v in mirror) + " " + _g(fm)
    assert lines[4] == "The best correlation is for" and len(lines) == 4 + 8
