"""GPU tests of xmipp_reconstruct_significant's device side (xh_rsig.hip) past one lap of 256: the compaction of a batch's chains
(k_rs_select, laps of 256 with base[k] carried along) and the rankings of the two weighting stages (k_rs_image_weights: LDS tiles of
256 over G; k_rs_direction_weights: tiles of 256 over N in blocks of 256 images).

Chains: the D = 20 case (5 images, 7 projections) with its images stacked three times (six without mirrors), 420 chains, in batches of
420, 260 and 256. Copy c of image n must give the bytes of image n in the run of tests/test_gpu_reconstruct_significant.py in batches of
8 chains, which that module holds to the restatement chain by chain: no new tolerance, 0 chains excluded.
Weights: hand-made arrays (R.weight_population) against R.weights at (N, G) = (261, 12), (5, 300), (257, 256); the preconditions (ties
inside a tile and across the 255 | 256 boundary, margins of the Fisher limit, max_shift and ang_distance, every option at work) are
asserted for every pair by tests/test_reconstruct_significant_host.py; 0 pairs excluded. Zero pattern equal, 1e-12 relative on weight,
cc and imed, as in the weight test of the small shapes.
Measured on one MI355X: chains, the same bytes in all six runs; weights, cc and imed, largest relative difference 0 (the same bits) over
the 70 424 pairs of the three shapes, eight option sets each.
Mutation check (not committed): without `base[k] +` in k_rs_select (the list zeroed at creation, so that no stale index is read) the
batches of 420 and 260 chains fail and the full lap of 256 passes; with `k < g` for `t0 + k < g` in k_rs_image_weights (5, 300)
fails; no test from before these fails under either."""
import numpy as np
import pytest

from tests import reconstruct_significant_ref as R
from tests.test_gpu_reconstruct_significant import _align, gpu  # noqa: F401

pytestmark = pytest.mark.gpu

_D = 20


@pytest.mark.parametrize("mirrors,copies,batch_chains", [(True, 3, 420), (True, 3, 260), (True, 3, 256), (False, 6, 420), (False, 6, 260), (False, 6, 256)])
def test_a_batch_of_more_than_256_chains(gpu, mirrors, copies, batch_chains):
    """420 chains (15 images x 7 x 4, or 30 x 7 x 2 without mirrors). Laps of k_rs_select per batch: batch_chains 420 -> one batch,
    256 + 164; 260 -> batches of 260 (256 + 4) and 160; 256 -> batches of 256 (one full lap) and 164. M, corr, imed, trace and the
    four chain arrays are the bytes of the run in batches of 8 chains, tiled; the stats count the traces' steps"""
    xa, ctx, torch = gpu
    nv, nd, N = R.CASES[_D]
    G, cpp = nv * nd, 4 if mirrors else 2
    assert copies * N * G * cpp == 420
    batches = [min(batch_chains, 420 - c0) for c0 in range(0, 420, batch_chains)]
    laps = [[min(256, m - b0) for b0 in range(0, m, 256)] for m in batches]
    assert batches[0] >= 256 and all(m % cpp == 0 for m in batches)
    small, _ = _align(gpu, _D, 8, mirrors)
    gallery, _, _, images = R.population(_D)
    h = xa.ReconstructSignificant(ctx, _D, G, batch_chains=batch_chains)
    h.load_gallery(torch.from_numpy(gallery).cuda())
    M, corr, imed, tr, ch = h.align(torch.from_numpy(np.concatenate([images] * copies)).cuda(), check_mirrors=mirrors, trace=True, chains=True)
    stats = h.stats()
    h.close()
    got = {"M": M, "corr": corr, "imed": imed, "trace": tr}
    got.update({"chain_" + k: v for k, v in ch.items()})
    print(f"mirrors {mirrors}, {copies} copies, batch_chains {batch_chains}: batches {batches}, laps {laps}, stats {stats}")
    for k, v in got.items():
        v = v.cpu().numpy()
        assert v.shape[0] == copies * N
        for c in range(copies):
            assert v[c * N:(c + 1) * N].tobytes() == small[k].tobytes(), f"{k} of copy {c} differs from the run in batches of 8 chains"
    t = small["chain_trace"].astype(np.int64)
    for rnd in range(3):
        assert stats[f"shift_round{rnd + 1}"] == copies * int(((t >> (3 * rnd)) & 1).sum())
        assert stats[f"rotation_round{rnd + 1}"] == copies * int(((t >> (3 * rnd + 1)) & 1).sum())
    assert stats["shift_round1"] > 0 and stats["rotation_round1"] > 0


@pytest.mark.parametrize("shape", sorted(R.WEIGHT_SHAPES))
def test_weights_past_one_tile_and_one_block(gpu, shape):
    """(261, 12): two blocks of images, tiles 256 + 5 over N. (5, 300): tiles 256 + 44 over G. (257, 256): a tile of one over N, one
    exact tile over G. Four option sets at ang_distance 10 and 40 against R.weights"""
    xa, ctx, torch = gpu
    N, G = shape
    M, cc0, imed0, nv, rot, tilt = R.weight_population(shape)
    h = xa.ReconstructSignificant(ctx, R.WEIGHT_D, G, batch_chains=8)
    dM = torch.from_numpy(M).cuda()
    worst = 0.0
    for ang in R.WEIGHT_ANG:
        for options in R.WEIGHT_OPTIONS:
            apply_fisher, use_imed, strict, max_shift = options
            cc, imed = torch.from_numpy(cc0).cuda(), torch.from_numpy(imed0).cuda()
            w = h.weights(dM, cc, imed, nv, rot, tilt, ang, R.WEIGHT_ONE_ALPHA, apply_fisher=apply_fisher, use_imed=use_imed, strict=strict, max_shift=max_shift).cpu().numpy()
            ew, ecc, eimed = R.weights_of(shape, ang, options)
            what = (shape, ang, options)
            assert 0 < np.count_nonzero(ew) < ew.size
            assert np.array_equal(w == 0, ew == 0), what
            worst = max(worst, float((np.abs(w - ew)[ew != 0] / np.abs(ew[ew != 0])).max()))
            assert np.all(np.abs(w - ew) <= 1e-12 * np.abs(ew)), what
            assert np.all(np.abs(cc.cpu().numpy() - ecc) <= 1e-12 * np.abs(ecc)) and np.all(np.abs(imed.cpu().numpy() - eimed) <= 1e-12 * np.abs(eimed)), what
    h.close()
    print(f"{shape}: {N * G} pairs, 0 excluded, largest relative difference of a weight {worst:.3e} (bound 1e-12)")
