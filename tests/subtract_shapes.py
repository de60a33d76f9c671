"""The shapes at which the device tests of xmipp_subtract_projection leave the 16-pixel case (one lap of every grid-stride loop of
xh_sub.hip, one workgroup of k_sub_fit, one chunk of projections in xh_rsp.hip), and a restatement of the quantities each shape is
in the list for: the loop lengths against the 256 threads of a workgroup, the cells of a wi bin, the padded size, the block counts of
k_sub_fit and k_sub_translate, the chunk and the tile count of rsp_run. check_reach() asserts from the restatement the property each
shape is there for: a change of a block size or of a chunk constant that takes a shape off its path fails there by name, not by
silently un-covering the path."""
import numpy as np

from tests import subtract_projection_ref as ref

THREADS = 256                # xh_sub.hip: k_sub_prepare, k_sub_bins, k_sub_models run 256 threads and stride their loops by 256
FIT_THREADS = 64             # xh_sub.hip: k_sub_fit, a thread per particle, (m + 63) / 64 blocks
TRANSLATE_THREADS = 64       # xh_sub.hip: k_sub_translate, a thread per row of a particle, (m D + 63) / 64 blocks
RSP_CHUNK = 4096             # xh_rsp.hip: rsp_run uploads the constants of at most 4096 projections per launch
RSP_TILE = 8                 # xh_rsp.hip: a workgroup of k_rsp_project covers 8 x 8 pixels

# D of the pipeline
SMALL = (16, 17)             # the sizes of the older tests: one lap everywhere
LAP_MODELS = 22              # the smallest D whose half spectrum (264 cells) takes k_sub_models into a second lap
LAPS = 40                    # 840 half-spectrum cells: three full laps and a tail of 72; D D = 1600: six full laps and a tail of 64
COMPOSITE = 41               # padded to 81 = 3^4; the older sizes pad to 31 (prime) and 33 (3 x 11), 22 and 40 to 43 and 79 (prime)
BIN = 168                    # the largest wi bin holds 269 cells: the second lap of k_sub_bins; with padding 1 the window is 168 = 2^3 3 7
BIN_BELOW = 160              # no bin above 256 cells
CHUNK_M = 65                 # particles in one chunk: two workgroups of k_sub_fit, blockIdx.y = 64 in k_sub_bins, p = t / D past 64

# the ray projector: n rows over six orientations, so that the seam between the chunks (rows 4095 | 4096) lies between two of them
RSP_D = 8
RSP_N = 4099
RSP_ORIENTATIONS = 6


def half_cells(D):
    """the cells k_sub_models walks: for (n = tid; n < D * xh; n += 256)"""
    return D * (D // 2 + 1)


def full_cells(D):
    """the cells each of the two loops of k_sub_prepare walks: for (n = tid; n < DD; n += 256)"""
    return D * D


def laps(cells, threads=THREADS):
    """(laps of a grid-stride loop over `cells` in which some thread works, the threads that work in the last of them)"""
    n = -(-cells // threads)
    return n, cells - (n - 1) * threads


def bin_cells(D, sampling=1.0, max_resolution=-1.0):
    """cells per wi bin as xh_sub_create groups them (binStart): counted from freq_map, only 0 < wi < maxwi; [maxwi + 1]"""
    wi, maxwi = ref.freq_map(D, sampling, max_resolution)
    return np.bincount(wi[(wi > 0) & (wi < maxwi)], minlength=maxwi + 1)


def padded(D, padding=2.0):
    """Np of xh_sub_create: the window from (int)padding STARTING to (int)padding FINISHING"""
    return int(padding) * (D - 1) + 1


def fit_blocks(m):
    return (m + FIT_THREADS - 1) // FIT_THREADS


def translate_blocks(m, D):
    return (m * D + TRANSLATE_THREADS - 1) // TRANSLATE_THREADS


def rsp_chunks(n):
    """the projections of each launch of rsp_run: for (p0 = 0; p0 < n; p0 += chunk), chunk = min(n, 4096)"""
    return [min(RSP_CHUNK, n - p0) for p0 in range(0, n, RSP_CHUNK)]


def rsp_blocks(m, D):
    """workgroups of one launch of k_rsp_project: m projections of ((D + 7) / 8)^2 tiles"""
    tiles = (D + RSP_TILE - 1) // RSP_TILE
    return m * tiles * tiles


def rsp_rows(n=RSP_N):
    """which of the six orientations each row of the projector test carries"""
    return np.arange(n) % RSP_ORIENTATIONS


def rsp_angles():
    """three orientations with an exact Euler matrix and three generic ones"""
    return [ref.EXACT_ANGLES[1], ref.EXACT_ANGLES[3], ref.EXACT_ANGLES[4]] + ref.generic_angles(3)


def factors(n):
    out, p = [], 2
    while p * p <= n:
        while n % p == 0:
            out.append(p)
            n //= p
        p += 1
    return out + ([n] if n > 1 else [])


def check_reach():
    """every shape reaches what it is listed for; the sizes of the older tests reach none of it"""
    for D in SMALL:
        assert laps(half_cells(D))[0] == 1                                     # 144 and 153 cells: threads 153 .. 255 never work
        assert laps(full_cells(D))[0] <= 2 and full_cells(D) <= THREADS + 33   # one lap, or one lap and 33 threads
        assert bin_cells(D).max() <= THREADS
        assert len(factors(padded(D))) <= 2                                    # 31, and 33 = 3 x 11
    assert (half_cells(16), half_cells(17)) == (144, 153)

    # the second lap of k_sub_models
    assert half_cells(LAP_MODELS) == 264 and laps(264) == (2, 8)
    assert all(half_cells(D) <= THREADS for D in range(4, LAP_MODELS)), "22 is the smallest D with D * xh > 256"
    assert laps(full_cells(LAP_MODELS)) == (2, 228)

    # several laps and a tail in k_sub_models and in both loops of k_sub_prepare
    assert half_cells(LAPS) == 840 and laps(840) == (4, 72)
    assert full_cells(LAPS) == 1600 and laps(1600) == (7, 64)
    assert bin_cells(LAPS).max() == 59 and bin_cells(64).max() == 101          # far from a second lap of a bin

    # composite padded sizes
    assert padded(COMPOSITE) == 81 and factors(81) == [3, 3, 3, 3]
    assert padded(BIN, 1.0) == 168 and factors(168) == [2, 2, 2, 3, 7]
    assert factors(padded(LAP_MODELS)) == [43] and factors(padded(LAPS)) == [79]

    # the second lap of k_sub_bins
    cells = bin_cells(BIN)
    assert cells.max() == 269 and laps(269) == (2, 13)
    assert int((cells > THREADS).sum()) >= 1
    assert bin_cells(BIN_BELOW).max() <= THREADS, "160 has no bin above 256 cells"
    assert cells[0] == 0 and cells[-1] == 0                                    # wi = 0 and wi = maxwi are no bins of the fit

    # a chunk of more than 64 particles
    assert fit_blocks(64) == 1 and fit_blocks(CHUNK_M) == 2
    assert translate_blocks(CHUNK_M, 16) == 17 and translate_blocks(64, 16) == 16
    assert (CHUNK_M * 16 - 1) // 16 == 64                                      # the last thread of k_sub_translate: p = t / D = 64
    assert all(fit_blocks(m) == 1 for m in (2, 3, 5))                          # the chunks of the older tests

    # two chunks of projections
    assert rsp_chunks(RSP_N) == [4096, 3] and rsp_chunks(4096) == [4096] and rsp_chunks(18) == [18]
    assert rsp_blocks(4096, RSP_D) == 4096 and rsp_blocks(3, RSP_D) == 3 and rsp_blocks(1, 17) == 9
    rows, ang = rsp_rows(), rsp_angles()
    assert len(ang) == RSP_ORIENTATIONS and len(set(ang)) == RSP_ORIENTATIONS
    assert rows[RSP_CHUNK - 1] != rows[RSP_CHUNK] and ang[rows[RSP_CHUNK - 1]] != ang[rows[RSP_CHUNK]]
    assert set(rows[RSP_CHUNK:]) != set(rows[:RSP_N - RSP_CHUNK])              # the second chunk does not repeat the head of the first
