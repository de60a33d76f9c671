"""CPU checks of xmipp_reconstruct_significant: properties of the numpy restatement of alignImages (tests/reconstruct_significant_ref.py),
the cumulative density function and both weightings by hand on tiny arrays, the branch population of the GPU parity cases, the
preconditions of the weight populations that pass one tile of 256 and one block (ties, margins, every option at work), and the
program's option parsing, show() text and refusals, which all come before any device is touched."""
import os
import subprocess

import numpy as np
import pytest
from scipy import ndimage

from oracle import pyoracle as po
from tests import reconstruct_significant_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PROG = os.path.join(ROOT, "xmipp3_amd", "bin", "xmipp_reconstruct_significant")


# ---------------------------------------------------------------- the restatement
def _phantom2d(D=32):
    """three blobs of different size and weight off the centre: no symmetry"""
    y, x = np.mgrid[-(D // 2):D - D // 2, -(D // 2):D - D // 2].astype(np.float64)
    img = np.zeros((D, D))
    for cx, cy, s, a in ((4.0, -2.0, 2.5, 1.0), (-5.0, 3.0, 1.8, 0.7), (1.0, 6.0, 1.2, 1.4)):
        img += a * np.exp(-((x - cx) ** 2 + (y - cy) ** 2) / (2 * s * s))
    return img


def test_an_image_against_itself():
    img = _phantom2d()
    p = R.align_pair(img, R.polar_fourier(img, False), img, True)
    assert abs(p["corr"] - 1.0) <= 1e-12
    assert np.abs(p["M"] - np.eye(3)).max() <= 1e-9
    assert p["mirror"] == 0


@pytest.mark.parametrize("mirrored", (False, True))
def test_a_rotated_shifted_copy_is_brought_back(mirrored):
    """Sanity only. A noise-free copy rotated by 15 degrees and shifted by (-4, 6), mirrored or not, at D = 32: the mirror flag is the right
    one, corr rises above the unaligned pair's and the pose is nearer the truth than the identity is. Recovered by the restatement
    on this phantom, as transformationMatrix2Parameters2D of M.inv() gives them: plain corr 0.9753, psi 14.47, shift (-4.01, 5.32);
    mirrored corr 0.9753, psi 14.47, shift (4.01, 5.32). (The copy was made with cubic splines, the aligner interpolates linearly.)"""
    ref = _phantom2d()
    img = ndimage.shift(ndimage.rotate(ref, 15.0, reshape=False, order=3, mode="constant"), (6.0, -4.0), order=3, mode="constant")
    if mirrored:
        img = img[:, ::-1].copy()
    p = R.align_pair(ref, R.polar_fourier(ref, False), img, True)
    assert p["mirror"] == int(mirrored)
    assert p["corr"] > po.correlation_index(img, ref)
    # the truth as the matrix that brings the image back, estimated by what it does: the aligned image must be nearer the reference
    # than the unaligned one, and the matrix must move the image by about the applied shift and angle
    aligned = p["chains"][p["mirror"]][p["rs"][p["mirror"]]]["image"]
    assert np.abs(aligned - ref).sum() < 0.5 * np.abs((img[:, ::-1] if mirrored else img) - ref).sum()
    _, sx, sy, psi = R.shifts_of(p["M"])
    print(f"mirrored={mirrored}: corr {p['corr']:.4f}, psi {psi:.2f}, shift ({sx:.2f}, {sy:.2f})")
    assert abs(abs(psi) - 15.0) < abs(0.0 - 15.0) and np.hypot(sx, sy) > 3.0


# ---------------------------------------------------------------- cdf and weights by hand
def test_cdf_ranks_equal_values_by_position():
    assert np.array_equal(R.cdf([0.3, 0.1, 0.3, 0.2]), np.array([3, 1, 4, 2]) / 4)


def test_repeated_list_rank_closed_form_equals_a_stable_sort():
    rng = np.random.default_rng(3)
    for copies in (1, 2, 4):
        v = np.round(rng.uniform(0, 1, 9), 1)                 # one decimal: plenty of equal values
        brute = R.cdf(np.tile(v, copies))[:len(v)]
        assert np.array_equal(R.repeated_list_cdf(v, copies), brute), (copies, v)


# 5 images x 1 volume x 4 directions; directions 0 and 1 are 8 degrees apart (neighbours at --angDistance 10), the others far away
_ROT, _TILT = np.array([0., 0., 90., 180.]), np.array([30., 38., 90., 120.])
_CC = np.array([[0.80, 0.60, 0.70, 0.10],
                [0.50, 0.90, 0.40, 0.30],
                [0.65, 0.55, 0.85, 0.20],
                [0.30, 0.35, 0.25, 0.95],
                [0.75, 0.45, 0.15, 0.05]])
_IMED = np.array([[1.0, 3.0, 2.0, 4.0],
                  [3.0, 1.0, 4.0, 2.0],
                  [2.0, 3.0, 1.0, 4.0],
                  [3.0, 2.0, 4.0, 1.0],
                  [1.5, 2.5, 3.5, 4.5]])


def _matrices(shift_x_of_pair=None):
    M = np.tile(np.eye(3), (5, 4, 1, 1))
    for (n, g), s in (shift_x_of_pair or {}).items():
        M[n, g, 0, 2] = s
    return M


def test_weights_by_hand():
    one_alpha = 0.5                                            # an image keeps the directions ranked 2, 3, 4 of 4
    k = R.neighbour_counts(_ROT, _TILT, 1, 10.0)
    assert list(k) == [1, 1, 0, 0]
    w, cc, imed = R.weights(_matrices(), _CC, _IMED, 32, 1, _ROT, _TILT, 10.0, one_alpha)
    assert np.array_equal(cc, _CC) and np.array_equal(imed, _IMED)
    # image 0: cdf 4/4, 2/4, 3/4, 1/4 -> the first three directions; per image weight cdf . cc / 0.80
    wi = R.image_weights(_matrices(), _CC, _IMED, 32, one_alpha, False, False, -1.0)
    np.testing.assert_allclose(wi[0], [1.0 * 0.80 / 0.80, 0.5 * 0.60 / 0.80, 0.75 * 0.70 / 0.80, 0.0], rtol=1e-15)
    # direction 0 (one neighbour: its 5 values twice): values 0.80 0.50 0.65 0.30 0.75 -> ranks 5 2 3 1 4 of 5, cdf of the first copies
    # (2 less + 1) / 10 = 0.9 0.3 0.5 0.1 0.7; not strict: every positive weight is multiplied by cc . (1 / 0.80) . cdf
    np.testing.assert_allclose(w[:, 0], wi[:, 0] * _CC[:, 0] * (1 / 0.80) * np.array([0.9, 0.3, 0.5, 0.1, 0.7]), rtol=1e-15)
    # direction 2 (no neighbour): cdf = rank / 5
    np.testing.assert_allclose(w[:, 2], wi[:, 2] * _CC[:, 2] * (1 / 0.85) * np.array([4, 3, 5, 2, 1]) / 5, rtol=1e-15)


def test_every_option_changes_the_expected_entries():
    one_alpha = 0.5
    base = R.weights(_matrices(), _CC, _IMED, 32, 1, _ROT, _TILT, 10.0, one_alpha)[0]
    # --strictDirection: direction 0's cdfs 0.9 0.3 0.5 0.1 0.7 -> images 1 and 3 fall below 0.5 (image 3 had weight 0 there already)
    strict = R.weights(_matrices(), _CC, _IMED, 32, 1, _ROT, _TILT, 10.0, one_alpha, strict=True)[0]
    assert base[1, 0] > 0 and strict[1, 0] == 0 and strict[0, 0] == base[0, 0]
    # --useImed: times (1 - cdfimed)(bestImed / imed); the direction with the best imed has cdfimed 1/4
    imedw = R.weights(_matrices(), _CC, _IMED, 32, 1, _ROT, _TILT, 10.0, one_alpha, use_imed=True)[0]
    np.testing.assert_allclose(imedw[0, 0], base[0, 0] * (1 - 0.25) * (1.0 / 1.0), rtol=1e-15)
    np.testing.assert_allclose(imedw[0, 2], base[0, 2] * (1 - 0.5) * (1.0 / 2.0), rtol=1e-15)
    # --maxShift 3 with pair (0, 0) shifted by 5: its cc becomes 0.8 / 3 and its imed 3 before anything else, and the pair is rejected
    M = _matrices({(0, 0): 5.0})
    w, cc, imed = R.weights(M, _CC, _IMED, 32, 1, _ROT, _TILT, 10.0, one_alpha, max_shift=3.0)
    assert cc[0, 0] == 0.80 / 3 and imed[0, 0] == 3.0 and w[0, 0] == 0
    assert w[0, 2] != base[0, 2]                               # image 0's best correlation is now 0.70: the other weights move
    np.testing.assert_allclose(R.image_weights(M, cc, imed, 32, one_alpha, False, False, 3.0)[0, 2], (4 / 4) * (0.70 / 0.70), rtol=1e-15)      # 0.70 now ranks last of 4
    # the inverted Fisher switch (applyFisher = checkParam("--dontApplyFisher")): with it, cc >= tanh(atanh(best . 0.5) - 2.96 / 32) is asked too
    # image 4: best 0.75, limit tanh(atanh(0.375) - 0.0925) = 0.293; direction 2 (cc 0.15, cdf 2/4) passes the percentile but not the limit
    ccl = np.tanh(np.arctanh(0.75 * one_alpha) - 2.96 / 32)
    assert _CC[4, 2] < ccl < _CC[4, 1]
    fisher = R.weights(_matrices(), _CC, _IMED, 32, 1, _ROT, _TILT, 10.0, one_alpha, apply_fisher=True)[0]
    assert base[4, 2] > 0 and fisher[4, 2] == 0 and fisher[4, 1] == base[4, 1]
    # a best correlation times one_alpha of 1 or more makes the limit NaN, and NaN compares false: nothing is selected for that image
    cc1 = _CC.copy()
    cc1[4, 0] = 2.5                                            # best . one_alpha = 1.25: the logarithm of a negative number
    assert np.all(R.weights(_matrices(), cc1, _IMED, 32, 1, _ROT, _TILT, 10.0, one_alpha, apply_fisher=True)[0][4] == 0)
    # --angDistance 40 makes no new neighbour here but 7 does away with the pair 0 / 1
    assert list(R.neighbour_counts(_ROT, _TILT, 1, 7.0)) == [0, 0, 0, 0]


# ---------------------------------------------------------------- the population of the GPU parity test
@pytest.mark.parametrize("D", sorted(R.CASES))
def test_branch_population(D):
    ref = R.reference(D)
    chains = [c for row in ref for p in row for m in p["chains"] for c in m]
    nv, nd, N = R.CASES[D]
    assert len(chains) == 4 * N * nv * nd
    tr = np.array([c["trace"] for c in chains])
    rounds = [(tr >> (3 * r)) & 7 for r in range(3)]
    assert np.all(rounds[0] & 3 == 3), "every chain runs both steps of round one (1.95 px and 2 degrees are over the thresholds)"
    assert any(np.any(r & R.TR_SHIFT == 0) for r in rounds[1:]), "no shift step was ever skipped"
    assert any(np.any(r & R.TR_ROT == 0) for r in rounds[1:]), "no rotation step was ever skipped"
    assert any(np.any(r & R.TR_NONWRAP != 0) for r in rounds), "no non-wrapping alternative was ever taken"
    pairs = [p for row in ref for p in row]
    assert {p["mirror"] for p in pairs} == {0, 1}, "the mirror must win and lose"
    assert {p["rs"][p["mirror"]] for p in pairs} == {0, 1}, "RS must win and lose"
    near = sum(c["margin"] < 1e-9 for c in chains)
    print(f"D={D}: {len(chains)} chains, {near} with a decision below 1e-9, smallest margin {min(c['margin'] for c in chains):.3e}")
    assert near <= 0.02 * len(chains)
    assert near == 0, "expected none: fp64 correlation maps of an asymmetric phantom do not tie"


def test_the_rotation_grid_never_holds_one_degree():
    for D in R.CASES:
        nsam, _, _ = po.polar_layout(*R.rings_of(D))
        ln = 2 * int(nsam[-1]) - 1
        assert ln % 2 == 1 and all(k * (360. / ln) != 1.0 for k in range(ln))


# ---------------------------------------------------------------- the program
@pytest.fixture(scope="module")
def prog():
    import __graft_entry__ as g
    g.build()
    assert os.path.exists(PROG)
    return PROG


def _run(args):
    return subprocess.run([PROG] + args, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=120)


def test_help_lists_the_reference_options(prog):
    r = _run(["--help"])
    assert r.returncode == 0 and "USAGE" in r.stderr
    for flag in ("-i", "--numberOfVolumes", "--initvolumes", "--initgallery", "--odir", "--sym", "--iter", "--alpha0", "--alphaF", "--keepIntermediateVolumes",
                 "--angularSampling", "--maxShift", "--minTilt", "--maxTilt", "--useImed", "--strictDirection", "--angDistance", "--dontApplyFisher",
                 "--dontReconstruct", "--useForValidation", "--dontCheckMirrors"):
        assert flag in r.stderr, flag
    assert "--gpus" not in r.stderr
    assert "switches the Fisher selection ON" in r.stderr


def test_show_text_defaults_and_the_inverted_fisher_switch(prog, tmp_path):
    r = _run(["-i", str(tmp_path / "none.xmd"), "--initvolumes", "vols.xmd", "--odir", str(tmp_path / "out"), "--dontApplyFisher"])
    assert r.returncode != 0 and "cannot open" in r.stderr           # the input is read only after show()
    for line in ("Input metadata              : " + str(tmp_path / "none.xmd"), "Output directory            : " + str(tmp_path / "out"), "Initial significance        : 0.05",
                 "Final significance          : 0.005", "Number of iterations        : 10", "Keep intermediate volumes   : 0", "Angular sampling            : 5",
                 "Maximum shift               : -1", "Minimum tilt                : 0", "Maximum tilt                : 90", "Use Imed                    : 0",
                 "Angular distance            : 10", "Apply Fisher                : 1", "Reconstruct                 : 1", "useForValidation            : 0",
                 "dontCheckMirrors            : 0", "Symmetry for projections    : c1", "Initial volume              : vols.xmd"):
        assert line in r.stdout.splitlines(), line
    r = _run(["-i", "none.xmd", "--initgallery", "gal.doc", "--useForValidation", "4", "--maxShift", "7", "--useImed", "--dontCheckMirrors"])
    for line in ("Apply Fisher                : 0", "Gallery                     : gal.doc", " numOrientationsPerParticle : 4", "Maximum shift               : 7",
                 "Use Imed                    : 1", "useForValidation            : 1", "dontCheckMirrors            : 1"):
        assert line in r.stdout.splitlines(), line


@pytest.mark.parametrize("args, words", [(["--initvolumes", "v.xmd", "--sym", "c3"], "--sym c3"), ([], "neither --initvolumes nor --initgallery")])
def test_refusals_come_before_any_device(prog, args, words):
    env = dict(os.environ, HIP_VISIBLE_DEVICES="-1", ROCR_VISIBLE_DEVICES="-1")
    r = subprocess.run([PROG, "-i", "none.xmd"] + args, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=120, env=env)
    assert r.returncode != 0
    assert "XMIPP_ERROR" in r.stderr and words in r.stderr and "xmipp_transform_symmetrize" in r.stderr
    assert "Input metadata" not in r.stdout                          # nothing ran


def test_alpha_schedule_for_three_iterations(prog):
    """as the reference's loop is written, the significance goes back to alpha0 at the top of every iteration (:416)"""
    r = _run(["-i", "none.xmd", "--initvolumes", "v.xmd", "--iter", "3", "--alpha0", "0.1", "--alphaF", "0.01"])
    lines = [l.strip() for l in r.stdout.splitlines() if l.strip().startswith("iteration ")]
    assert lines == [f"iteration {k}: alpha 0.1, significance 0.9" for k in (1, 2, 3)]


def test_dont_reconstruct_forces_one_iteration(prog):
    r = _run(["-i", "none.xmd", "--initgallery", "gal.doc", "--iter", "5", "--dontReconstruct"])
    assert "Setting iterations to 1 because of --dontReconstruct" in r.stdout
    assert "Number of iterations        : 1" in r.stdout.splitlines() and "Reconstruct                 : 0" in r.stdout.splitlines()
    assert [l.strip() for l in r.stdout.splitlines() if l.strip().startswith("iteration ")] == ["iteration 1: alpha 0.05, significance 0.95"]


# ---------------------------------------------------------------- the weight populations past one tile and one block
def _ties(v):
    """(equal values inside the first 256 entries of v, an entry at 256 or later equal to one before 256)"""
    head, tail = v[:256], v[256:]
    return len(np.unique(head)) < len(head), bool(np.isin(tail, head).any())


@pytest.mark.parametrize("shape", sorted(R.WEIGHT_SHAPES))
def test_weight_populations_meet_their_preconditions(shape):
    """What the device comparison of tests/test_gpu_reconstruct_significant.py rests on, asserted on the restatement for every pair:
    equal values inside a tile of 256 and across the 255 | 256 boundary, along G (an image's ranking) and along N (a direction's); no
    correlation within 1e-9 of its image's Fisher limit, no |shift| within 1e-9 of max_shift, no two directions within 1e-9 degrees of
    ang_distance; every option changes the weights; under strict, one_alpha cuts some and keeps some in every image and direction.
    (261, 12): blocks 256 + 5 of images, tiles 256 + 5 over N. (5, 300): tiles 256 + 44 over G. (257, 256): a tile of one over N, one
    exact tile over G. The ranks are integer quotients formed the same way on both sides and need no margin"""
    N, G = shape
    M, cc0, imed0, nv, rot, tilt = R.weight_population(shape)
    assert (N > 256 or G > 256) and G == nv * (G // nv)
    assert np.all((cc0 > 0.05) & (cc0 < 0.95) & (cc0 * 64 == np.round(cc0 * 64))) and np.all((imed0 > 1) & (imed0 < 40) & (imed0 * 8 == np.round(imed0 * 8)))
    sx, sy = R.all_shifts(M)
    far = (np.abs(sx) > R.WEIGHT_MAX_SHIFT) | (np.abs(sy) > R.WEIGHT_MAX_SHIFT)
    assert 0.05 < far.mean() < 0.2
    assert min(np.abs(np.abs(sx) - R.WEIGHT_MAX_SHIFT).min(), np.abs(np.abs(sy) - R.WEIGHT_MAX_SHIFT).min()) >= 1e-9
    ang = R.direction_angles(rot, tilt, nv)
    for a in R.WEIGHT_ANG:
        assert np.abs(ang - a).min() >= 1e-9
    assert (ang < 10.0).sum() < (ang < 40.0).sum()
    for max_shift in (-1.0, R.WEIGHT_MAX_SHIFT):
        cc, imed = R.penalise(M, cc0, imed0, max_shift)
        # ties, in the values the kernels rank
        rows = [_ties(cc[n]) + _ties(imed[n]) for n in range(N)]
        cols = [_ties(cc[:, g]) for g in range(G)]
        assert any(r[0] for r in rows) and any(r[2] for r in rows) and any(c[0] for c in cols)
        if G > 256:
            assert any(r[1] for r in rows) and any(r[3] for r in rows), "no tie across the 255 | 256 boundary of an image's ranking"
        if N > 256:
            assert any(c[1] for c in cols), "no tie across the 255 | 256 boundary of a direction's ranking"
        # the Fisher limit of every image against every correlation of it
        best = cc.max(1)
        ccl = np.tanh(0.5 * np.log((1 + best * R.WEIGHT_ONE_ALPHA) / (1 - best * R.WEIGHT_ONE_ALPHA)) - 2.96 * np.sqrt(1.0 / (R.WEIGHT_D * R.WEIGHT_D)))
        assert np.all(np.isfinite(ccl)) and np.abs(cc - ccl[:, None]).min() >= 1e-9
        # one_alpha cuts some and keeps some: in every image, and under strict in every direction for both neighbour counts
        for n in range(N):
            keep = R.cdf(cc[n]) >= R.WEIGHT_ONE_ALPHA
            assert 0 < keep.sum() < G
        for a in R.WEIGHT_ANG:
            k = R.neighbour_counts(rot, tilt, nv, a)
            for g in range(G):
                keep = R.repeated_list_cdf(cc[:, g], 1 + int(k[g])) >= R.WEIGHT_ONE_ALPHA
                assert 0 < keep.sum() < N
    # every option, flipped alone in each of the compared sets (at 40 degrees), changes the weights; so does ang_distance under strict
    a = R.WEIGHT_ANG[1]
    for fisher, use_imed, strict, max_shift in R.WEIGHT_OPTIONS:
        w = R.weights_of(shape, a, (fisher, use_imed, strict, max_shift))[0]
        assert 0 < np.count_nonzero(w) < w.size
        for other in ((not fisher, use_imed, strict, max_shift), (fisher, not use_imed, strict, max_shift), (fisher, use_imed, not strict, max_shift),
                      (fisher, use_imed, strict, -1.0 if max_shift > 0 else R.WEIGHT_MAX_SHIFT)):
            assert not np.array_equal(R.weights_of(shape, a, other)[0], w), (shape, a, other)
    for options in R.WEIGHT_OPTIONS:
        if options[2]:
            assert not np.array_equal(R.weights_of(shape, 10.0, options)[0], R.weights_of(shape, 40.0, options)[0]), options
    # the shared stages are weights() itself
    o = R.WEIGHT_OPTIONS[1]
    plain = R.weights(M, cc0, imed0, R.WEIGHT_D, nv, rot, tilt, 40.0, R.WEIGHT_ONE_ALPHA, *o)
    for x, y in zip(plain, R.weights_of(shape, 40.0, o)):
        assert np.array_equal(x, y)
