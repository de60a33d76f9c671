"""CPU checks of the xmipp_volume_align restatement (tests/volume_align_ref.py) and of the library's host-only entries: xh_valign_matrix
against numpy, xh_valign_trials against the reference's loops in Python, the restatement's search on a planted pose, the preconditions of
every device case (the boxes of 288 and 560 bricks, the tile cases, the lists of the long search and the degenerate exits among them),
the derivation of the device tests' bound, and the restatement against the exact sums (R.fitness_exact). None needs a device."""
import math

import numpy as np
import pytest

import xmipp3_amd as xa
from tests import volume_align_ref as R


@pytest.mark.parametrize("p", [
    [1, 1, 0, 0, 0, 0, 1, 0, 0, 0],                                   # the identity
    [-1, 1, 0, 0, 0, 0, 1, 2, -1, 3],                                 # flip: column 2 and z = -z + 1
    [1, 1.3, -0.2, 0, 0, 0, 0.8, 0, 0, 0],                            # scale != 1
    [-1, 1, 0, 13.7, 41.3, -27.9, 1.08, 1.3, -2.6, 0.4],              # a generic pose
    [1, 1, 0, 200.3, 100.7, -75.1, 0.93, -4.5, 0.25, 7.0],
])
def test_matrix_against_numpy(p):
    A, Ai, ident = xa.VolumeAlign.matrix(p)
    rA, rAi, rident = R.matrix(p)
    assert ident == rident == (p[3:] == [0, 0, 0, 1, 0, 0, 0] and p[0] == 1)
    assert np.abs(A - rA).max() <= 1e-14 and np.abs(Ai - rAi).max() <= 1e-14
    # against numpy's own product and inverse
    E = np.eye(4)
    E[:3, :3] = R.euler_matrix(*p[3:6])
    E[:, 2] *= p[0]
    T = np.eye(4)
    T[:3, 3] = [p[9], p[8], -p[7] + 1 if p[0] < 0 else p[7]]
    want = E @ T @ np.diag([p[6], p[6], p[6], 1.0])
    assert np.abs(A - want).max() <= 1e-14
    assert np.abs(Ai - np.linalg.inv(want)).max() <= 1e-14 * max(1.0, np.abs(np.linalg.inv(want)).max())
    assert np.array_equal(A[3], [0, 0, 0, 1]) and np.array_equal(Ai[3], [0, 0, 0, 1])


def _ranges(**kw):
    r = {"grey_scale": (1, 1, 1), "grey_shift": (0, 0, 1), "rot": (0, 0, 1), "tilt": (0, 0, 1), "psi": (0, 0, 1), "scale": (1, 1, 1),
         "z": (0, 0, 1), "y": (0, 0, 1), "x": (0, 0, 1)}
    r.update(kw)
    return [r[n] for n in R.RANGE_NAMES]


@pytest.mark.parametrize("ranges,mirror,count", [
    (_ranges(), False, 1),                                                                   # equal bounds everywhere
    (_ranges(rot=(0, 360, 15)), False, 25),
    (_ranges(rot=(0, 360, 15), tilt=(0, 180, 15), psi=(0, 360, 15)), False, 25 * 13 * 25),
    (_ranges(rot=(0, 10, 3), x=(-1, 1, 0.4)), True, 2 * 4 * 6),                              # a step that does not divide the range
    (_ranges(scale=(0.9, 1.1, 0.1), z=(-2, 2, 0)), False, None),                             # 0.9 + 0.1 + 0.1 against 1.1 in doubles; a zero step is 1
    (_ranges(grey_scale=(0.8, 1.2, 0.2), grey_shift=(-0.1, 0.1, 0.1), y=(3, 1, 1)), True, 0),   # first > last: no trial
])
def test_trials_equal_the_reference_loops(ranges, mirror, count):
    got, times = xa.valign_trials(ranges, mirror)
    want, wtimes = R.trials(ranges, mirror)
    assert got.shape == want.shape and np.array_equal(got, want)
    assert times == wtimes
    if count is not None:
        assert len(got) == count


def test_progress_count_is_not_the_trip_count():
    """-x -1 1 0.4: FLOOR(1 + 2 / 0.4) is 6 and the loop makes 6 trips only because -1 + 5 * 0.4 rounds to 1 or below; the two are kept
    apart. --rot 0 360 15 tilt 0 0: the count skips equal bounds, the loops run them once"""
    got, times = xa.valign_trials(_ranges(scale=(0.9, 1.1, 0.1)), False)
    v, n = 0.9, 0
    while v <= 1.1:
        v += 0.1
        n += 1
    assert len(got) == n and times == int(math.floor(1 + (1.1 - 0.9) / 0.1))


def test_trials_refusals():
    with pytest.raises(xa.XhError, match="more than 100 trials"):
        xa.valign_trials(_ranges(rot=(0, 360, 1)), False, limit=100)
    with pytest.raises(xa.XhError, match="never ends"):
        xa.valign_trials(_ranges(rot=(0, 360, -15)), False)


@pytest.mark.parametrize("method", (R.COVARIANCE, R.LEAST_SQUARES))
def test_search_returns_the_planted_pose(method):
    shape = (12, 12, 12)
    V2 = R.phantom(shape, 3)
    star = [1.0, 1.0, 0.0, 10.0, 20.0, -5.0, 1.0, 1.0, -1.0, 0.5]
    V1 = R.apply_transformation(V2, star, True)
    tr, _ = R.trials(_ranges(rot=(5, 15, 5), tilt=(15, 25, 5), psi=(-10, 0, 5), z=(1, 1, 1), y=(-1, -1, 1), x=(0.5, 0.5, 1)))
    assert len(tr) == 27
    idx, best, fits = R.search(V1, V2, tr, method, True)
    assert np.array_equal(tr[idx], star)
    assert np.sort(fits)[1] - best >= 1e-6
    assert abs(best - (-1.0 if method == R.COVARIANCE else 0.0)) <= 1e-12


def test_onepass_identity_and_stats():
    shape = (9, 10, 12)
    V1, V2 = R.volumes(shape, True)
    mask = R.case_mask(shape, True)
    assert 0 < mask.sum() < mask.size
    n, mean_x, sd_x, S0 = R.stats(V1, mask)
    assert n == mask.sum() and abs(S0) <= 1e-12 * n and sd_x > 0.01
    # correlationIndex(x, x) is 1: the integer N / (N - 1) makes the deviation the population's
    assert abs(R.correlation_index(V1, V1, mask) - 1.0) <= 1e-14


def _rel(a, b):
    return float((np.abs(np.asarray(a) - b) / np.maximum(1.0, np.abs(b))).max())


def test_device_cases_meet_their_preconditions_and_give_the_bound():
    """The tolerance of the device tests, and the preconditions of their cases, on the restatement alone.
    Preconditions: no tested coordinate of any trial within 1e-9 of a threshold min - 1e-6 / max + 1e-6, none within 1e-9 of a wrap edge
    (0 found: no case and no voxel is left out); the best trial beats the runner-up by at least 1e-6.
    Bound: for every trial of every case the two-pass fit and the one-pass identity form; 16 times their largest difference relative to
    max(1, |fit|), rounded up to a power of ten, is R.BOUND. The cases include the boxes of 288 and 560 bricks (R.BIG_SHAPES: smallest
    margin 1.0e-6, 0 edge voxels, largest difference 4.4e-16, under the 5.0e-16 of the smaller boxes).
    Exact sums: the device adds the 10^5 terms of those boxes in another order than numpy, so the device tests assert against
    R.fitness_exact (math.fsum); here the restatement, in both forms, must lie within R.BOUND of it too (largest: 6.1e-16)."""
    worst, exact = 0.0, {}
    for shape, method, wrap, masked in R.parity_cases():
        tr = R.trial_list(shape, method, wrap)
        margin, edge = R.preconditions(shape, tr, wrap)
        assert margin >= 1e-9 and edge == 0, (shape, method, wrap, margin, edge)
        V1, V2 = R.volumes(shape, wrap)
        mask = R.case_mask(shape, masked)
        idx, best, two = R.search(V1, V2, tr, method, wrap, mask)
        _, _, one = R.search(V1, V2, tr, method, wrap, mask, onepass=True)
        assert np.sort(two)[1] - best >= 1e-6, (shape, method, wrap, masked, two)
        worst = max(worst, float((np.abs(two - one) / np.maximum(1.0, np.abs(two))).max()))
        ex = np.array([R.fitness_exact(V1, V2, p, method, wrap, mask) for p in tr])
        exact[shape] = max(exact.get(shape, 0.0), _rel(two, ex), _rel(one, ex))
    print(f"largest relative difference of the two-pass and one-pass fits: {worst:.3e}")
    for shape, v in exact.items():
        print(f"{shape}, {R.bricks(shape)} bricks: restatement to exact sums {v:.3e}")
        assert v <= R.BOUND
    assert worst > 0
    assert R.BOUND == 10.0 ** math.ceil(math.log10(16 * worst))
    assert [R.bricks(s) for s in R.BIG_SHAPES] == [288, 560] and all(d % 8 and d % 4 for s in R.BIG_SHAPES for d in s)


def test_exact_fit_is_the_restatement_with_exact_sums():
    """on values whose sums are exact in any order (multiples of 1/8 below 2^10) the two agree to the finish's own rounding"""
    rng = np.random.default_rng(5)
    shape = (9, 10, 12)
    V1, V2 = (rng.integers(-40, 41, shape) / 8.0 for _ in range(2))
    mask = R.case_mask(shape, True)
    ident = [1.0, 1.0, 0.0, 0.0, 0.0, 0.0, 1.0, 0.0, 0.0, 0.0]
    shift = [1.0, 1.0, 0.0, 0.0, 0.0, 0.0, 1.0, 2.0, -1.0, 3.0]
    for p, method, m in ((ident, R.LEAST_SQUARES, None), (shift, R.LEAST_SQUARES, mask), (ident, R.COVARIANCE, mask), (shift, R.COVARIANCE, None)):
        a, b = R.fitness(V1, V2, p, method, True, m, onepass=True), R.fitness_exact(V1, V2, p, method, True, m)
        assert abs(a - b) <= 4 * np.finfo(float).eps, (p, method, a, b)
    assert R.fitness_exact(V1, V2, ident, R.LEAST_SQUARES, True) == math.sqrt(float(((V1 - V2) ** 2).sum()) / V1.size)
    # the exits: n = 0, n = 1, no deviation
    none, one = np.zeros(shape, np.int32), np.zeros(shape, np.int32)
    one[4, 5, 6] = 1
    for method in (R.COVARIANCE, R.LEAST_SQUARES):
        for mk in (none, one):
            assert R.fitness_exact(V1, V2, shift, method, True, mk) == R.fitness(V1, V2, shift, method, True, mk)
    assert R.fitness_exact(np.full(shape, 0.37), V2, shift, R.COVARIANCE, True) == 0


def test_tile_cases_reach_a_second_tile():
    """13 and 10 trials at capacities 8, 9, 13 and 64: launches and their tiles (blockIdx.y) as the device cuts them"""
    assert R.launches(13, 8) == [[8], [5]] and R.launches(13, 9) == [[8, 1], [4]] and R.launches(13, 13) == R.launches(13, 64) == [[8, 5]]
    assert R.launches(10, 8) == [[8], [2]] and R.launches(10, 9) == [[8, 1], [1]] and R.launches(10, 13) == R.launches(10, 64) == [[8, 2]]
    assert R.launches(13, 5) == [[5], [5], [3]]                        # the capacity of every other test: one tile per launch
    for method, wrap, masked in R.TILE_CASES:
        assert len(R.trial_list((17, 17, 17), method, wrap)) == (13 if method == R.LEAST_SQUARES else 10)
        assert ((17, 17, 17), method, wrap, masked) in R.parity_cases()     # preconditions and bound: the test above


def test_long_search_lists():
    """588 trials in one launch: preconditions (margin 1.7e-6, 0 edge voxels, the best 5.8e-3 below the runner-up) and where the copies of
    the best trial fall in k_va_select's chunks"""
    tr, fits, best, lists = R.long_search()
    assert len(tr) == 588 and np.array_equal(tr[best], R.PLANTED)
    margin, edge = R.preconditions(R.LONG_SHAPE, tr, R.LONG_WRAP)
    print(f"margin {margin:.3e}, edge voxels {edge}, best below the runner-up by {np.sort(fits)[1] - fits[best]:.3e}")
    assert margin >= 1e-9 and edge == 0 and np.sort(fits)[1] - fits[best] >= 1e-6
    at = {k: list(np.flatnonzero(v == best)) for k, v in lists.items()}
    assert at == {"planted": [4, 5, 299, 300, 301, 302, 594], "late": [297, 298, 299, 300, 592], "last": [588]}
    assert {k: len(v) for k, v in lists.items()} == {"planted": 595, "late": 593, "last": 589}
    # one launch of everything: per = 3
    assert all(R.select_chunks(len(v)) == 3 for v in lists.values())
    assert 4 // 3 == 5 // 3 and 299 // 3 + 1 == 300 // 3 and 595 % 3 == 1 and 297 // 3 == 299 // 3 and 299 // 3 + 1 == 300 // 3 and 589 % 3 == 1
    # launches of 300: per = 2 in each, the copies at 299 | 300 in two launches, local 1 | 2 of the second in two chunks
    assert R.select_chunks(300) == 2 and R.select_chunks(295) == 2 and R.select_chunks(289) == 2 and (301 - 300) // 2 + 1 == (302 - 300) // 2
    assert 297 // 2 + 1 == 298 // 2 and 295 % 2 == 1 and 289 % 2 == 1
    assert R.select_chunks(256) == 1
    # the first minimum of every list, by the reference's rule
    for name, v in lists.items():
        idx, b, f = R.search(*R.volumes(R.LONG_SHAPE, R.LONG_WRAP), tr[v[:6]], R.LONG_METHOD, R.LONG_WRAP)
        assert np.array_equal(f, fits[v[:6]])                          # a list's fits are the pool's
        assert int(np.argmin(fits[v])) == at[name][0]


def test_degenerate_cases_meet_their_preconditions():
    """margins and wrap edges of every degenerate case (the box 2 x 3 x 5 among them: margin 1.0e-6, 0 edge voxels), what each exit returns
    on the restatement, and the restatement against the exact sums"""
    cases = R.degenerate_cases()
    worst = 0.0
    for name, (shape, V1, V2, mask, _) in cases.items():
        for method in (R.COVARIANCE, R.LEAST_SQUARES):
            for wrap in (True, False):
                tr = R.degenerate_trials(name, method, wrap)
                margin, edge = R.preconditions(shape, tr, wrap)
                assert margin >= 1e-9 and edge == 0, (name, method, wrap, margin, edge)
                fits = R.search(V1, V2, tr, method, wrap, mask)[2]
                ex = np.array([R.fitness_exact(V1, V2, p, method, wrap, mask) for p in tr])
                worst = max(worst, _rel(fits, ex))
                if name == "mask of zeros" or (method == R.COVARIANCE and name in ("mask of one voxel", "constant V1")):
                    assert np.all(fits == 0), (name, method, wrap)
                if name == "constant V2" and method == R.COVARIANCE and wrap:
                    assert np.all(fits == 0)
                if name.startswith("all outside") and not wrap:
                    assert fits[-1] == (0 if method == R.COVARIANCE else R.rms(V1, np.zeros(shape), mask))
    print(f"degenerate cases: restatement to exact sums {worst:.3e}")
    assert worst <= R.BOUND
    assert cases["mask of one voxel"][3].sum() == 1 and set(np.unique(cases["mask values 2 and -1"][3])) == {-1, 0, 2}
    assert np.array_equal(cases["mask values 2 and -1"][3] != 0, R.case_mask(R.DEGENERATE_SHAPE, True) != 0)
