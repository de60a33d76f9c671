"""GPU tests of xmipp_volume_align (xh_valign.hip) past the first iteration of its strided loops, against the numpy fp64 restatement
(tests/volume_align_ref.py) and the exact sums (R.fitness_exact). tests/test_volume_align_ref.py asserts the preconditions of every case
here on the restatement alone (margins to the thresholds, 0 wrap-edge voxels, the tie positions of the long search); 0 trials and 0
voxels are left out.

  tiles     k_va_fit gives a workgroup VA_TILE = 8 trials: 13 (10) trials at capacities 8, 9, 13 and 64 reach blockIdx.y = 1 with a second
            tile of 5 (2) or 1 trials and write partials for trial indices 8 .. 12.
  bricks    k_va_finish adds bricks t, t + 256, ..: (29, 41, 43) has 288 bricks and (37, 49, 57) 560. They are parity cases of
            tests/test_gpu_volume_align.py (capacity 5, and apply); here capacity 13 puts two tiles on top of the second and third step.
  select    k_va_select cuts m fits into 256 chunks of per = ceil(m / 256): 589 .. 595 trials at capacity 1024 (per = 3), 300 (per = 2,
            the best carried from launch to launch) and 256 (per = 1), with copies of the best trial inside a chunk, across two chunks,
            across two launches and alone in the last short chunk.
  exits     n = 0, n = 1, a deviation below 1e-6, a box sent wholly outside, mask values other than 0 / 1, the box 2 x 3 x 5, and a
            handle given a mask first and none afterwards.

Bound: R.BOUND = 1e-14 relative to max(1, |fit|), derived on the CPU (tests/test_volume_align_ref.py), against the exact sums and against
the restatement.
Measured on one MI355X, largest difference to the restatement: tiles 2.8e-16; 288 and 560 bricks at capacity 13, COVARIANCE 5.6e-16
(5.6e-16 to the exact sums), LEAST_SQUARES 2.8e-17; the long search 1.7e-15; the exits 1.9e-15 on 9 x 10 x 12 and 8.7e-15 on 2 x 3 x 5
(COVARIANCE, wrap, masked; the restatement is 5.7e-15 from the exact sums there and the device 1.1e-14: the phantom's 30 voxels have
mean 3.5 and deviation 0.54, so sum y^2 / n - mean_y^2 multiplies every rounding by 2 mean^2 / var = 84 in all three).
Mutation check (not committed; each changed the library alone): blockIdx.y * VA_TILE -> 0 fails the tile, brick and long-search tests;
one step of k_va_finish's loop fails the 288- and 560-brick cases; <= in k_va_select's merge fails the planted and late lists and the
all-zero exits; no test from before these fails under any of them."""
import numpy as np
import pytest

from tests import volume_align_ref as R
from tests.test_gpu_volume_align import exact, gpu, loaded, ref, rel_to  # noqa: F401

pytestmark = pytest.mark.gpu

BOX17 = (17, 17, 17)


@pytest.mark.parametrize("method,wrap,masked", R.TILE_CASES)
def test_more_than_one_tile_of_trials(gpu, method, wrap, masked):
    """17^3, 13 trials (LEAST_SQUARES) or 10 (COVARIANCE). Launches and their tiles: capacity 8 -> [8], [5]; 9 -> [8, 1], [4];
    13 and 64 -> [8, 5] (10 trials: [8], [2]; [8, 1], [1]; [8, 2]). Every fit within R.BOUND of the restatement; fit, search index and best
    byte-equal to the capacity-5 run ([5], [5], [3]: one tile per launch)"""
    tr, idx, best, fits = ref(BOX17, method, wrap, masked)
    va = loaded(gpu, BOX17, wrap, masked, capacity=5)
    base = va.fit(tr, method, wrap)
    bi, bb, bf = va.search(tr, method, wrap, fits=True)
    assert bi == idx and bf.tobytes() == base.tobytes() and bb == base[idx]
    for capacity in R.TILE_CAPACITIES:
        tiles = R.launches(len(tr), capacity)
        va = loaded(gpu, BOX17, wrap, masked, capacity)
        got = va.fit(tr, method, wrap)
        print(f"method {method} wrap {wrap} masked {masked} capacity {capacity}: tiles {tiles}, largest difference {rel_to(got, fits):.3e}")
        assert max(len(t) for t in tiles) == (1 if capacity == R.TILE else 2) and tiles[0][0] == R.TILE      # a full tile, then more
        assert rel_to(got, fits) <= R.BOUND
        assert got.tobytes() == base.tobytes(), capacity
        gi, gb, gf = va.search(tr, method, wrap, fits=True)
        assert gi == bi and gf.tobytes() == base.tobytes() and np.float64(gb).tobytes() == np.float64(bb).tobytes(), capacity


@pytest.mark.parametrize("shape,method,wrap,masked", [c for c in R.parity_cases() if c[0] in R.BIG_SHAPES])
def test_two_tiles_over_more_than_256_bricks(gpu, shape, method, wrap, masked):
    """288 and 560 bricks at capacity 13: one launch, tiles [8, 5] ([8, 2] under COVARIANCE), so that the second tile's partials lie
    behind 8 x 288 (560) x NK doubles. Within R.BOUND of the exact sums and of the restatement; the bytes of the capacity-5 run"""
    tr, idx, best, fits = ref(shape, method, wrap, masked)
    ex = exact(shape, method, wrap, masked)
    assert R.bricks(shape) > 256 and R.launches(len(tr), 13) == [[8, len(tr) - 8]]
    small = loaded(gpu, shape, wrap, masked, capacity=5).fit(tr, method, wrap)
    gi, gb, gf = loaded(gpu, shape, wrap, masked, capacity=13).search(tr, method, wrap, fits=True)
    print(f"{shape} method {method} wrap {wrap} masked {masked} capacity 13: device to exact sums {rel_to(gf, ex):.3e}, to the restatement {rel_to(gf, fits):.3e}")
    assert rel_to(gf, ex) <= R.BOUND
    assert rel_to(gf, fits) <= R.BOUND
    assert gf.tobytes() == small.tobytes() and gi == idx and gb == gf[idx]


@pytest.mark.parametrize("name", ("planted", "late", "last"))
def test_search_of_more_than_256_trials(gpu, name):
    """9 x 10 x 12, COVARIANCE, wrap: 588 trials with copies of the best one planted (R.long_search).
    planted, 595 trials: capacity 1024 -> one launch, per = 3, 199 chunks, the last of one trial, 57 empty; copies at 4 | 5 in chunk 1,
             299 | 300 in chunks 99 | 100. Capacity 300 -> launches of 300 and 295, per = 2 in both; 299 | 300 in two launches, 301 | 302
             in chunks 0 | 1 of the second. Capacity 256 -> 256, 256, 83, per = 1. The winner is 4.
    late, 593 trials: the winner 297 is the first of 297 .. 300 (per = 3: chunk 99 and chunk 100; per = 2: chunks 148 | 149 and the next launch).
    last, 589 trials: the winner 588 is alone in the last chunk (per = 3: 589 = 196 . 3 + 1; per = 2: 289 = 144 . 2 + 1).
    The index is the restatement's first minimum, the fits' bytes do not depend on the capacity, best is the winner's fit"""
    tr, pool, best, lists = R.long_search()
    order = lists[name]
    trials, fits = tr[order], pool[order]
    want = int(np.argmin(fits))                       # numpy's argmin is the first minimum
    V1, V2 = R.volumes(R.LONG_SHAPE, R.LONG_WRAP)
    runs = []
    for capacity in R.LONG_CAPACITIES:
        xa, ctx, _ = gpu
        va = xa.VolumeAlign(ctx, R.LONG_SHAPE, capacity)
        va.set_volumes(V1, V2)
        gi, gb, gf = va.search(trials, R.LONG_METHOD, R.LONG_WRAP, fits=True)
        per = [R.select_chunks(min(capacity, len(order) - t0)) for t0 in range(0, len(order), capacity)]
        print(f"{name}: {len(order)} trials, capacity {capacity}, per {per}: index {gi} (restatement {want}), largest difference {rel_to(gf, fits):.3e}")
        assert rel_to(gf, fits) <= R.BOUND
        assert gi == want and gb == gf[gi]
        assert np.all(gf[order == best] == gb) and np.all(gf[order != best] > gb)
        runs.append(gf.tobytes())
    assert runs[0] == runs[1] == runs[2]


@pytest.mark.parametrize("name", sorted(R.degenerate_cases()))
def test_degenerate_exits(gpu, name):
    """each early exit of the finish against the restatement, both methods, wrap on and off, capacity 5; zeros are compared as numbers, so
    that the -0.0 of minus a zero correlation equals 0"""
    xa, ctx, _ = gpu
    shape, V1, V2, mask, _ = R.degenerate_cases()[name]
    va = xa.VolumeAlign(ctx, shape, 5)
    va.set_volumes(V1, V2, mask)
    want = R.stats(V1, mask)
    assert va.stats()[0] == want[0] and np.allclose(va.stats(), want, rtol=1e-13, atol=1e-11)
    for method in (R.COVARIANCE, R.LEAST_SQUARES):
        for wrap in (True, False):
            tr = R.degenerate_trials(name, method, wrap)
            fits = R.search(V1, V2, tr, method, wrap, mask)[2]
            ex = np.array([R.fitness_exact(V1, V2, p, method, wrap, mask) for p in tr])
            got = va.fit(tr, method, wrap)
            print(f"{name} method {method} wrap {wrap}: largest difference {rel_to(got, fits):.3e}, device to exact sums {rel_to(got, ex):.3e}, "
                  f"restatement to exact sums {rel_to(fits, ex):.3e}")
            assert np.all(np.isfinite(got))
            assert np.array_equal(got == 0, fits == 0), (name, method, wrap, got, fits)
            assert rel_to(got, fits) <= R.BOUND, (name, method, wrap)
            gi, gb, gf = va.search(tr, method, wrap, fits=True)
            assert gf.tobytes() == got.tobytes() and gi == int(np.argmin(got)) and gb == got[gi]
    if name == "mask values 2 and -1":
        # the same voxels as the 0 / 1 mask of the parity cases: the same bytes
        plain = loaded(gpu, shape, True, True)
        tr = R.trial_list(shape, R.COVARIANCE, True)
        assert va.fit(tr, R.COVARIANCE, True).tobytes() == plain.fit(tr, R.COVARIANCE, True).tobytes() and va.stats() == plain.stats()


def test_a_handle_forgets_its_mask(gpu):
    """set_volumes with a mask, then other volumes without one on the same handle: fits and stats() are a fresh handle's"""
    xa, ctx, _ = gpu
    shape = R.DEGENERATE_SHAPE
    V1, V2 = R.volumes(shape, True)
    W1, W2 = R.volumes(shape, False)
    assert not np.array_equal(V1, W1)
    used = xa.VolumeAlign(ctx, shape, 5)
    used.set_volumes(V1, V2, R.case_mask(shape, True))
    masked_stats = used.stats()
    used.fit(R.trial_list(shape, R.COVARIANCE, True))
    used.set_volumes(W1, W2)
    fresh = xa.VolumeAlign(ctx, shape, 5)
    fresh.set_volumes(W1, W2)
    assert used.stats() == fresh.stats() and used.stats()[0] == W1.size != masked_stats[0]
    for method in (R.COVARIANCE, R.LEAST_SQUARES):
        for wrap in (True, False):
            tr = R.trial_list(shape, method, wrap)
            a, b = used.search(tr, method, wrap, fits=True), fresh.search(tr, method, wrap, fits=True)
            assert a[0] == b[0] and a[1] == b[1] and a[2].tobytes() == b[2].tobytes()
            assert rel_to(a[2], R.search(W1, W2, tr, method, wrap)[2]) <= R.BOUND
