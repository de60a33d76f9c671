"""CPU checks of the xmipp_volume_find_symmetry restatement (tests/find_symmetry_ref.py) and of the library's host-only entries:
xh_fsym_axis_matrices against the restatement and against numpy, the gate, the recursion bound against the recursion depth the
restatement observes, the derivation of the device tests' bound, and the preconditions of every device case. None needs a device.

The bound: 16 times the largest relative difference (to max(1, |corr|)) over every ungated trial of R.AXIS_CASES and R.HELICAL_CASES
between the restatement's forms (two passes against one, the helix's transcendentals moved by one ulp up and down against plain, each
against the exact sums), rounded up to a power of ten. Measured: 3.3e-16, 1.8e-15 and 6.1e-15, so 16 x 6.1e-15 = 9.8e-14 and R.BOUND =
1e-13. 0 trials and 0 voxels are left out of any case."""
import math

import numpy as np
import pytest

import xmipp3_amd as xa
from tests import find_symmetry_ref as R


def rel(a, b):
    live = a != R.GATED
    assert np.array_equal(live, b != R.GATED)
    return float((np.abs(a - b)[live] / np.maximum(1.0, np.abs(b[live]))).max())


@pytest.mark.parametrize("rot,tilt,rot_sym", [(40.0, 55.0, 3), (0.0, 0.0, 4), (25.0, 90.0, 2), (200.1, 64.9, 7), (-13.0, 170.0, 99)])
def test_axis_matrices(rot, tilt, rot_sym):
    A, Ai = xa.fsym_axis_matrices(rot, tilt, rot_sym)
    want = R.axis_matrices(rot, tilt, rot_sym)
    axis = np.array(R.axis_of(rot, tilt))
    assert len(A) == rot_sym - 1
    for n in range(rot_sym - 1):
        assert np.abs(A[n] - want[n]).max() <= 1e-15
        assert np.abs(Ai[n] - np.linalg.inv(want[n])).max() <= 1e-14
        # a rotation that leaves the axis in place, by 360 (n + 1) / rot_sym degrees, and whose inverse is entry rot_sym - 2 - n
        assert np.abs(A[n] @ A[n].T - np.eye(3)).max() <= 1e-14 and abs(np.linalg.det(A[n]) - 1) <= 1e-14
        assert np.abs(A[n] @ axis - axis).max() <= 1e-14
        assert abs(np.trace(A[n]) - (1 + 2 * math.cos(2 * math.pi * (n + 1) / rot_sym))) <= 1e-13
        assert np.abs(A[n] @ A[rot_sym - 2 - n] - np.eye(3)).max() <= 1e-14
    # the sense of rotation3DMatrix(ang, 'Z') for the z axis
    Az, _ = xa.fsym_axis_matrices(0.0, 0.0, 4)
    assert np.abs(Az[0] - np.array([[0.0, 1.0, 0.0], [-1.0, 0.0, 0.0], [0.0, 0.0, 1.0]])).max() <= 1e-15


def test_axis_matrices_refusals():
    for n in (1, 0, 100):
        with pytest.raises(xa.XhError, match="rot_sym"):
            xa.fsym_axis_matrices(0, 0, n)
    with pytest.raises(xa.XhError, match="not finite"):
        xa.fsym_axis_matrices(float("nan"), 0, 3)


def test_gate():
    box = (1.0, 10.0, -357.0, 357.0)
    for Z in (16, 37):
        for z in (-0.5, 0.0, 0.99, 1.0, 0.4 * Z, np.nextafter(0.4 * Z, 100.0), 10.0, 10.5):
            for rot in (-358.0, -357.0, 0.0, 357.0, 357.5):
                assert xa.fsym_helical_gate(Z, z, rot, *box) == R.gated(Z, z, rot, box), (Z, z, rot)
    assert xa.fsym_helical_gate(20, 8.0, 0.0, *box) is False and xa.fsym_helical_gate(20, 8.01, 0.0, *box) is True


@pytest.mark.parametrize("Z", (20, 21))
def test_depth_formula_against_the_observed_recursion(Z):
    """symmetry_Helical with its mask on Z = 20 and 21 planes: the depth the restatement's recursion reaches is the formula's wherever
    the formula gives one, and the recursion runs away (the restatement stops it at 6 levels) where the formula gives -1 for a rise
    above 0. The library's formula is the restatement's"""
    shape = (Z, 7, 6)
    V = R.helix_phantom(shape)
    seen = set()
    for dihedral in (False, True):
        for hf in (0.95, 1.0):
            m = R.clip_mask(shape, None, hf)
            for zH in (0.3, 0.99, 1.0, 1.7, 4.3, 5.0, 8.0):
                want = R.helical_depth(Z, zH, hf, dihedral)
                assert xa.fsym_helical_depth(Z, zH, hf, dihedral) == want
                if want < 0:
                    with pytest.raises(RecursionError):
                        R.helical_volume(V, 33.3, zH, m, dihedral, hf, 1)
                else:
                    st = {}
                    out = R.helical_volume(V, 33.3, zH, m, dihedral, hf, 1, 0, st)
                    assert st["depth"] == want, (dihedral, hf, zH)
                    assert np.isfinite(out).all()
                seen.add(want)
    assert seen == ({-1, 0, 1} if Z == 20 else {0})
    for zH, hf in ((0.0, 1.0), (-1.0, 1.0), (float("inf"), 1.0), (4.3, 0.0), (4.3, 1.01)):
        assert xa.fsym_helical_depth(Z, zH, hf, False) == R.helical_depth(Z, zH, hf, False) == -1
    # the bound of the unmasked caller stays as it is: it refuses a rise of one voxel wholesale
    assert xa.sym_helical_depth(Z, 1.0, 1.0, False) == -1 and xa.fsym_helical_depth(Z, 1.0, 1.0, False) == 0


def test_choice_starts_at_zero():
    assert R.choose([0.2, 0.5, 0.5, 0.1]) == (1, 0.5)
    assert R.choose([-0.2, 0.0, R.GATED, float("nan")]) == (-1, 0.0)
    assert R.choose([float("nan"), 0.3]) == (1, 0.3)


def test_the_bound_and_the_preconditions_of_every_device_case():
    worst = {"two-pass against one-pass": 0.0, "nudged against plain": 0.0, "against the exact sums": 0.0}
    for case in R.AXIS_CASES:
        r = R.axis_case(case)
        # no tested coordinate within 1e-9 of a threshold min - 1e-6 / max + 1e-6
        assert r["margin"] >= 1e-9, case
        s = np.sort(r["two"])
        assert r["choice"][0] == 0 and s[-1] - s[-2] >= 1e-6 and s[-1] > 0, case
        assert np.isfinite(r["two"]).all()
        worst["two-pass against one-pass"] = max(worst["two-pass against one-pass"], rel(r["two"], r["one"]))
        worst["against the exact sums"] = max(worst["against the exact sums"], rel(r["two"], r["exact"]), rel(r["one"], r["exact"]))
    assert R.bricks((29, 41, 43)) == 288 and R.bricks((37, 49, 57)) == 560          # a second and a third step of the finish
    depths = {}
    for case in R.HELICAL_CASES:
        r = R.helical_case(case, nudged=True)
        shape, Cn, dihedral, hf, kind = case
        live = r["two"] != R.GATED
        want_live = [not R.gated(shape[0], z, rot, R.HELICAL_BOX) for rot, z in r["trials"]]
        assert live.tolist() == want_live and live.sum() >= 3 and (~live).sum() == 4, case
        s = np.sort(r["two"][live])
        # the planted helix wins where its rise is among the trials; Z = 9 gates it, and there the winner is not the first trial
        assert r["choice"][0] == (0 if shape[0] > 9 else 2) and live[r["choice"][0]] and s[-1] - s[-2] >= 1e-6 and s[-1] > 0, case
        assert np.isfinite(r["two"][live]).all()
        # kp = k + l zHelical is compared with zFirst and zLast: it is one of them exactly or at least 1e-9 away
        zFirst, zLast = R.helix_range(shape[0], hf)
        # a fraction below 1 removes planes, so that the clipping of the mask is exercised and not the same case as a fraction of 1
        planes = zLast - zFirst + 1
        assert planes == shape[0] if hf == 1.0 else planes < shape[0], case
        assert int((r["clipped"] != 0).any(axis=(1, 2)).sum()) <= planes
        for rot, z in r["trials"][live]:
            assert R.helical_depth(shape[0], z, hf, dihedral) >= 0
            l = np.arange(-3 * shape[0], 3 * shape[0] + 1, dtype=np.float64)          # rises of 1 voxel and more: |l| <= 2 Z + 1
            kp = (np.arange(shape[0], dtype=np.float64) - shape[0] // 2)[:, None] + l[None, :] * z
            for thr in (zFirst, zLast):
                dist = np.abs(kp - thr)
                assert ((dist == 0) | (dist >= 1e-9)).all(), (case, z)
        depths[case] = r["depth"]
        assert r["depth"] == max(R.helical_depth(shape[0], z, hf, dihedral) for _, z in r["trials"][live])
        worst["two-pass against one-pass"] = max(worst["two-pass against one-pass"], rel(r["two"], r["one"]))
        worst["nudged against plain"] = max(worst["nudged against plain"], rel(r["up"], r["one"]), rel(r["down"], r["one"]))
        worst["against the exact sums"] = max(worst["against the exact sums"], rel(r["two"], r["exact"]), rel(r["one"], r["exact"]))
    # depth 1 is reached (an even Z covered entirely, dihedral), and an odd Z and heightFraction 0.95 stay at 0
    assert sorted(set(depths.values())) == [0, 1]
    assert depths[((16, 16, 16), 1, True, 1.0, None)] == 1 and depths[((17, 17, 17), 3, True, 1.0, "cylinder")] == 0
    assert depths[((20, 18, 13), 1, True, 0.95, "cylinder")] == 0
    # the clipping on an even and on an odd Z, and the rise of one voxel where the finish takes a second step over the bricks
    clipped = {c[0][0] for c in R.HELICAL_CASES if c[3] < 1.0}
    assert any(z % 2 == 0 for z in clipped) and any(z % 2 == 1 for z in clipped)
    assert 1.0 in R.helical_trials((29, 41, 43))[:, 1] and R.bricks((29, 41, 43)) > 256
    print("largest relative differences between the restatement's forms:", {k: f"{v:.2e}" for k, v in worst.items()})
    derived = 10.0 ** math.ceil(math.log10(16 * max(worst.values())))
    assert derived == R.BOUND, (worst, derived)


def test_a_search_with_no_positive_correlation_answers_zero_zero():
    """a constant volume has no deviation: every correlation is 0, none is above the 0 the best starts at, and the answer is rot = tilt = 0"""
    V = np.full((9, 10, 12), 0.37)
    corrs = [R.axis_corr(V, rot, tilt, 3) for rot, tilt in R.AXIS_TRIALS]
    assert corrs == [0.0] * len(corrs) and R.choose(corrs) == (-1, 0.0)
