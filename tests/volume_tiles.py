"""The volume shapes at which the device tests of LocalDeblur (xh_ldb.hip) and MonoRes (xh_mono.hip) leave the tile of the small shapes
(8 rows or lines of a Bluestein length per workgroup, one output per thread, one lap of every grid-stride loop), and a restatement of the
constructors' tile choices. check_reach() asserts from the restatement the property each shape is in the list for: a change of the tiling
that takes a shape off its path fails there by name, not by silently un-covering the path."""
from types import SimpleNamespace

# (Z, Y, X)
POW2_X = (40, 36, 64)        # x lines of a power of two: bit-reversed placement in the row kernels; two register slots in k_ldb_rows
POW2_ZY = (64, 32, 48)       # y and z lines of powers of two: bit-reversed placement in both line passes
X160 = (21, 19, 160)         # Bluestein x with M = 512: four register slots, rpb = 6 with a tail, ppc = 1; MonoRes rpb = 2 with a tail
X300 = (20, 19, 300)         # M = 1024: rpb = 3 with a tail, ppc = 1; MonoRes rpb = 1
Y130 = (36, 130, 40)         # y lines: 8 lines of M = 512, 64 KiB of dynamic LDS
Z130 = (130, 24, 34)         # z lines: 8 lines of M = 512, 64 KiB of dynamic LDS
Z260 = (260, 16, 18)         # z lines of M = 1024: lpb = 4; 33 bands, so a batch of 3 (nbuf 4) ends on a band without a partner
TILE_SHAPES = [POW2_X, POW2_ZY, X160, X300, Y130, Z130, Z260]
BIG = (81, 80, 82)           # NF = 272 160 > 256 * 4 * CUs on 256 CUs, N = 531 360: the shape and the guard of test_gpu_halves_restoration.py
SHELLS = (520, 8, 10)        # 262 shells: a thread of k_mn_shell_planes takes two, k_mn_shell_final takes several workgroups

LDB_EPT = 4                  # xh_ldb.hip: LDB_EPT
CD = 16                      # sizeof(xh_cd)


def is_pow2(n):
    return n & (n - 1) == 0


def plan_M(n):
    """xh_plan_create (xh_plan.h): the LDS stride of a line of n points, n itself for a power of two and else the power of two >= 2 n - 1"""
    M = 1
    while M < (n if is_pow2(n) else 2 * n - 1):
        M <<= 1
    return M


def plan_lpb(n, budget=64 * 1024, max_lines=8):
    """xh_plan_lpb (xh_plan.h) as ldb_filter (xh_ldb.hip) and fft3d_yz (xh_fft3d.h, the batch of four of xh_mono.hip) call it: 64 KiB, at most 8 lines"""
    return max(1, min(max_lines, budget // (CD * plan_M(n))))


def tiling(shape, batch=8):
    """The tile values of a shape. LocalDeblur: nbuf, rpb, ppc as xh_ldb_create (xh_ldb.hip) sets h->nbuf, h->rpb, h->ppc; lpy, lpz and the
    LDS bytes of the three launches as ldb_filter computes them. MonoRes: mono_rpb as xh_mono_create (xh_mono.hip) sets h->rpb from
    rowBytes; nshell as xh_mono_num_shells"""
    Z, Y, X = shape
    t = SimpleNamespace()
    t.Mx, t.My, t.Mz = plan_M(X), plan_M(Y), plan_M(Z)
    t.nbuf = (batch + 1) & ~1
    line_bytes = CD * t.Mx
    t.rpb = max(1, min(8, 256 * LDB_EPT // X))
    t.ppc = max(1, min(t.nbuf // 2, 32 * 1024 // (line_bytes * t.rpb)))
    t.rows_lds = t.rpb * t.ppc * line_bytes
    t.nrows = Z * Y
    t.lpy, t.lpz = plan_lpb(Y), plan_lpb(Z)
    t.y_lds, t.z_lds = t.lpy * CD * t.My, t.lpz * CD * t.Mz
    row_bytes = 2 * CD * t.Mx
    t.mono_rpb = max(1, min(8, 32 * 1024 // row_bytes))
    t.nshell = int(((Z // 2) ** 2 + (Y // 2) ** 2 + (X // 2) ** 2) ** 0.5) + 2
    t.NF, t.N = Z * Y * (X // 2 + 1), Z * Y * X
    return t


def slots(shape):
    """the register slots u of k_ldb_rows (q = tid + 256 u) that hold a voxel in a full workgroup. Whether a slot holds a voxel whose
    value is compared depends on the input: ldb_compared()"""
    t = tiling(shape)
    return (t.rpb * shape[2] + 255) // 256


# The synthetic pair of local_sharpening_ref.synth has its resolution map inside a small sphere about the centre and 0 elsewhere, and
# k_ldb_rows leaves every voxel of the outside set at 0: such a voxel compares 0 with 0 whatever the workgroup did. Rolled by these
# (z, y, x) steps the sphere's centre lies on the last row (k = Z - 1, i = Y - 1), inside the tail workgroup, and at X300 at x = 212,
# where rows 0, 1 and 2 of a workgroup put it in slots 0, 1 and 2, and 3
ROLLS = {(21, 21, 21): (10, 10, 0), X160: (10, 9, 0), X300: (9, 9, 62)}


def ldb_compared(shape, inside):
    """how many voxels of the inside set (a bool volume: res >= 2 sampling, where k_ldb_rows accumulates) each register slot of
    k_ldb_rows holds over all workgroups, and how many the tail workgroup (nr < rpb) holds; (per-slot list, tail count or None)"""
    import numpy as np
    t = tiling(shape)
    X = shape[2]
    rows = np.asarray(inside, bool).reshape(t.nrows, X)
    q = (np.arange(t.nrows) % t.rpb)[:, None] * X + np.arange(X)[None, :]       # the output index inside its workgroup
    per_slot = [int(rows[q // 256 == u].sum()) for u in range(slots(shape))]
    ntail = t.nrows % t.rpb
    return per_slot, (int(rows[t.nrows - ntail:].sum()) if ntail else None)


def check_reach():
    """every shape reaches what it is listed for; the small shapes of the older tests reach none of it"""
    for s in [(24, 20, 18), (21, 21, 21), (24, 24, 24)]:
        t = tiling(s)
        assert not any(is_pow2(n) for n in s) and slots(s) == 1 and t.rpb == 8 and t.ppc == 4 and t.lpy == t.lpz == 8 and t.mono_rpb == 8 and t.nshell <= 256
        assert max(t.y_lds, t.z_lds, t.rows_lds) <= 32 * 1024

    t = tiling(POW2_X)
    assert is_pow2(POW2_X[2]) and t.Mx == 64                                  # bit-reversed placement in k_ldb_rows and k_mn_rows_amp
    assert t.rpb == 8 and t.rpb * POW2_X[2] == 512 and slots(POW2_X) == 2     # u = 0, 1 of k_ldb_rows
    assert t.ppc == 4 and t.mono_rpb == 8

    t = tiling(POW2_ZY)
    assert is_pow2(POW2_ZY[0]) and is_pow2(POW2_ZY[1]) and t.Mz == 64 and t.My == 32        # bit-reversed placement in k_ldb_lines<0>, <1>
    assert not is_pow2(POW2_ZY[2])

    t = tiling(X160)
    assert t.Mx == 512 and t.rpb == 6 and t.rpb * X160[2] > 768 and slots(X160) == 4         # u = 0 .. 3 of k_ldb_rows
    assert t.nrows % t.rpb == 3                                               # a tail workgroup with rpb < 8
    assert t.ppc == 1 and t.nbuf // 2 == 4 and t.rows_lds == 48 * 1024        # the p0 loop runs 4 times per batch, LDS reused between chunks
    assert all(tiling(X160, b).ppc == 1 for b in (1, 2, 8, 16))
    assert t.mono_rpb == 2 and t.nrows % 2 == 1                               # k_mn_rows_amp: rpb 2 with a tail

    t = tiling(X300)
    assert t.Mx == 1024 and t.rpb == 3 and t.nrows % t.rpb == 2 and t.ppc == 1 and slots(X300) == 4
    # (that the slots and the tail rows hold voxels whose values are compared is a property of the input: ROLLS, ldb_compared)
    assert t.mono_rpb == 1                                                    # k_mn_rows_amp: one row per workgroup

    t = tiling(Y130)
    assert t.My == 512 and t.lpy == 8 and t.y_lds == 64 * 1024                # k_ldb_lines<0> at 64 KiB of dynamic LDS plus base[]
    t = tiling(Z130)
    assert t.Mz == 512 and t.lpz == 8 and t.z_lds == 64 * 1024                # k_ldb_lines<1> at 64 KiB of dynamic LDS plus base[]

    t = tiling(Z260, 3)
    assert t.Mz == 1024 and t.lpz == 4 and t.nbuf == 4                        # lpb < 8 needs M >= 1024

    t = tiling(BIG)
    assert t.NF == 272160 and t.N == 531360                                   # against 256 * 4 * CUs: asserted on the device by the tests

    t = tiling(SHELLS)
    assert t.nshell == 262 and (3 * t.nshell + 255) // 256 > 1                # r += 256 in k_mn_shell_planes; k_mn_shell_final's grid
