"""CPU checks of the xmipp_volume_align restatement (tests/volume_align_ref.py) and of the library's host-only entries: xh_valign_matrix
against numpy, xh_valign_trials against the reference's loops in Python, the restatement's search on a planted pose, the preconditions of
every device case, and the derivation of the device tests' bound. None needs a device."""
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


def test_device_cases_meet_their_preconditions_and_give_the_bound():
    """The tolerance of the device tests, and the preconditions of their cases, on the restatement alone.
    Preconditions: no tested coordinate of any trial within 1e-9 of a threshold min - 1e-6 / max + 1e-6, none within 1e-9 of a wrap edge
    (0 found: no case and no voxel is left out); the best trial beats the runner-up by at least 1e-6.
    Bound: for every trial of every case the two-pass fit and the one-pass identity form; 16 times their largest difference relative to
    max(1, |fit|), rounded up to a power of ten, is R.BOUND."""
    worst = 0.0
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
    print(f"largest relative difference of the two-pass and one-pass fits: {worst:.3e}")
    assert worst > 0
    assert R.BOUND == 10.0 ** math.ceil(math.log10(16 * worst))
