"""GPU tests of the transforms every module builds on, path by path, against numpy's double-precision FFT of the same input:
the LDS line transform of xh_plan.h (radix 2 and Bluestein, float and double, the three line layouts the callers use), the
2-D transform of xh_fft2d.hip one axis at a time and whole (direct lines, small odd factor times a power of two, four-step
with power-of-two and Bluestein factors, degenerate shapes, whole detector frames), and FlexAlign's two row entries that
transform a real frame two rows at a time.

Error model. One rounding level costs at most eps = 2^-24 (fp32) or 2^-53 (fp64) of the largest coefficient; a radix-2 line of
M points has log2(M) levels, a Bluestein line three M-point transforms and three products (chirp, kernel spectrum, chirp), a
direct DFT of n1 <= 64 points ceil(log2(n1)) + 1 and a four-step line the levels of its two factors plus the twiddle product.
Every comparison asserts max |got - exp| <= C * eps * levels * max |exp| with C of its path class within 10x of the worst
ratio measured over the sweep (printed at the end of the module under -s). A table rounded to float inside the double plan
(about 1e-8 relative) is five orders of magnitude above these bounds."""
import math
from collections import defaultdict

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

EPS = {32: 2.0 ** -24, 64: 2.0 ** -53}
# C of every path class; the worst ratio to eps * levels * max |X| measured over the sweep on an MI355X was radix2 0.85 (fp32) /
# 0.72 (fp64), bluestein 0.22 / 0.34, probe 0.38 / 1.46, 2d-direct 0.76, 2d-small 0.29, 2d-fourstep 0.25, 2d-frame 0.27,
# rows-pairs 0.10, rows-kept 0.26 (the module's report prints it again)
C = {"radix2/32": 2.5, "radix2/64": 2.5, "bluestein/32": 0.6, "bluestein/64": 1.0, "probe/32": 1.0, "probe/64": 4.0,
     "2d-direct": 2.0, "2d-small": 0.8, "2d-fourstep": 0.8, "2d-frame": 0.8, "rows-pairs": 0.3, "rows-kept": 0.8}
WORST = defaultdict(float)
SENTINEL = -7777.25 + 3333.5j


@pytest.fixture(scope="module")
def gpu():
    import torch
    import xmipp3_amd as xa
    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    return xa, xa.Context(0), torch


@pytest.fixture(scope="module", autouse=True)
def report():
    yield
    print("\nworst measured error / (eps * levels * max|X|) per path class (asserted <= C):")
    for k in sorted(WORST):
        print(f"  {k:12s} {WORST[k]:.3g}   C = {C[k]:g}")


def is_pow2(n):
    return n > 0 and n & (n - 1) == 0


def lds_len(n):
    """M: the LDS length of a line of n points (n for powers of two, else the power of two >= 2n - 1)."""
    if is_pow2(n):
        return n
    M = 1
    while M < 2 * n - 1:
        M <<= 1
    return M


def levels(n):
    lg = lds_len(n).bit_length() - 1
    return max(1, lg) if is_pow2(n) else 3 * lg + 3


def check(cls, got, exp, prec, lev):
    """max |got - exp| <= C[cls] eps lev max |exp|; records the ratio."""
    scale = np.abs(exp).max()
    err = np.abs(got - exp).max()
    bound = EPS[prec] * lev * scale
    ratio = err / bound if bound > 0 else (0.0 if err == 0 else math.inf)
    WORST[cls] = max(WORST[cls], ratio)
    assert ratio <= C[cls], f"{cls}: error {err:.3g} is {ratio:.3g} x eps*levels*max|X| ({bound:.3g}); C = {C[cls]}"


# ---------------------------------------------------------------------------------------------- line transforms (xh_plan.h)
def lpb_of(n, prec, max_lines):
    line = (8 if prec == 32 else 16) * lds_len(n)
    return max(1, min(max_lines, 65536 // line))


def layout(kind, n, nlines):
    """(inner, outerStride, innerStride, elemStride, max_lines) of the three layouts the callers use, with gaps between lines."""
    if kind == "rows":              # contiguous lines, 3 elements apart (fp x lines, rf rows, fft2d rows)
        return 1, n + 3, 0, 1, 16
    if kind == "columns":           # neighbouring columns of a stack of images: 5 of 7 columns, images one element apart
        return 5, n * 7 + 1, 1, 7, 16
    return nlines, 0, 1, nlines + 2, 8          # z lines: outerStride 0 (fp z lines)


def line_index(n, nlines, inner, outer, istr, estr):
    l = np.arange(nlines)[:, None]
    e = np.arange(n)[None, :]
    return (l // inner) * outer + (l % inner) * istr + e * estr


def run_lines(gpu, x, prec, kind, inverse):
    """x [nlines, n] -> the device transform of its lines laid out as `kind`, after checking that nothing else changed."""
    xa, ctx, torch = gpu
    nlines, n = x.shape
    inner, outer, istr, estr, ml = layout(kind, n, nlines)
    idx = line_index(n, nlines, inner, outer, istr, estr)
    total = int(idx.max()) + 1 + 9
    buf = np.full(total, SENTINEL, np.complex64 if prec == 32 else np.complex128)
    buf[idx] = x
    d = torch.from_numpy(buf).cuda()
    xa.debug_fft_lines(ctx, d, n, nlines, inner, outer, istr, estr, ml, inverse)
    out = d.cpu().numpy()
    rest = np.ones(total, bool)
    rest[idx] = False
    assert np.all(out[rest] == buf[rest]), f"{kind}: the transform wrote outside its lines"
    return out[idx]


def reference(x, inverse):
    x = x.astype(np.complex128)
    n = x.shape[-1]
    return n * np.fft.ifft(x, axis=-1) if inverse else np.fft.fft(x, axis=-1)


def sweep_lines(gpu, n, prec):
    rng = np.random.default_rng(n * 131 + prec)
    cdt = np.complex64 if prec == 32 else np.complex128
    lev = levels(n)
    cls = ("radix2/" if is_pow2(n) else "bluestein/") + str(prec)
    for kind in ("rows", "columns", "z"):
        ml = layout(kind, n, 1)[4]
        lpb = lpb_of(n, prec, ml)
        for nlines in (2 * lpb - 1, 2 * lpb, 2 * lpb + 1):
            x = (rng.standard_normal((nlines, n)) + 1j * rng.standard_normal((nlines, n))).astype(cdt)
            for inverse in (False, True):
                got = run_lines(gpu, x, prec, kind, inverse)
                check(cls, got, reference(x, inverse), prec, lev)
    # exact probes: an impulse at j gives exp(-+2 pi i j k / n); a constant gives n at DC and nothing else
    js = sorted({0, min(1, n - 1), n // 3, n // 2, n - 1})
    x = np.zeros((len(js) + 1, n), cdt)
    for r, j in enumerate(js):
        x[r, j] = 1
    x[-1] = 0.75
    k = np.arange(n)
    for inverse in (False, True):
        got = run_lines(gpu, x, prec, "rows", inverse)
        sgn = 1 if inverse else -1
        for r, j in enumerate(js):
            check(f"probe/{prec}", got[r], np.exp(sgn * 2j * np.pi * ((j * k) % n) / n), prec, lev)
        dc = np.zeros(n)
        dc[0] = 0.75 * n
        check(f"probe/{prec}", got[-1], dc, prec, lev)


@pytest.mark.parametrize("prec", [32, 64])
@pytest.mark.parametrize("n", list(range(1, 131)))
def test_lines_every_short_length(gpu, n, prec):
    sweep_lines(gpu, n, prec)


@pytest.mark.parametrize("prec,n", [(p, n) for p in (32, 64) for n in (256, 512, 1024, 2048)] + [(32, 4096)] +
                         [(p, n) for p in (32, 64) for n in (511, 513, 1000, 1021, 1023, 1025, 1200, 1500, 2047)])
def test_lines_long_lengths(gpu, n, prec):
    """Powers of two up to the largest each precision's callers use, Bluestein lines on both sides of every M edge: from 1025
    points M = 4096, one double line per workgroup (the gridder's k_rf_c2r_window at P > 1024)."""
    sweep_lines(gpu, n, prec)


@pytest.mark.parametrize("prec,n", [(64, 2049), (32, 4097)])
def test_lines_refuse_what_does_not_fit(gpu, n, prec):
    xa, ctx, torch = gpu
    d = torch.zeros(4 * n, dtype=torch.complex64 if prec == 32 else torch.complex128, device="cuda")
    with pytest.raises(xa.XhError):
        xa.debug_fft_lines(ctx, d, n, 1, 1, n, 0, 1, 16, False)


# ---------------------------------------------------------------------------------------------- the 2-D transform (xh_fft2d.hip)
def odd_part(n):
    while n % 2 == 0:
        n //= 2
    return n


def path_of(n, n1, n2):
    assert n1 * n2 == n
    if n2 == 1:
        return "direct"
    if n1 == odd_part(n) and n1 <= 64 and is_pow2(n2):
        return "small"
    return "fourstep-pow2" if is_pow2(n1) and is_pow2(n2) else "fourstep-bluestein"


def axis_levels(n, n1, n2):
    p = path_of(n, n1, n2)
    if p == "direct":
        return levels(n)
    first = math.ceil(math.log2(n1)) + 1 if p == "small" else levels(n1)
    return first + 1 + levels(n2)


CLASS = {"direct": "2d-direct", "small": "2d-small", "fourstep-pow2": "2d-fourstep", "fourstep-bluestein": "2d-fourstep"}

SMALL = [o * 2 ** k for o, ks in ((3, (9, 11)), (5, (8, 11)), (7, (8, 11)), (9, (7, 8, 11)), (15, (7, 11)), (45, (5, 8, 11)),
                                  (63, (5, 11))) for k in ks]
SHAPES = ([(1024, 1000, "direct", "direct"), (1023, 2048, "direct", "direct"), (96, 100, "direct", "direct")] +
          [(5, n, "direct", "small") for n in SMALL] + [(n, 7, "small", "direct") for n in SMALL] +
          [(6, 4096, "direct", "fourstep-pow2"), (5, 8192, "direct", "fourstep-pow2"), (4096, 6, "fourstep-pow2", "direct"),
           (8192, 3, "fourstep-pow2", "direct")] +
          [(4, n, "direct", "fourstep-bluestein") for n in (2042, 3710, 3838, 4092)] +
          [(n, 5, "fourstep-bluestein", "direct") for n in (2042, 3710, 3838, 4092)] +
          [(1, 1000, "direct", "direct"), (1, 5760, "direct", "small"), (1536, 1, "small", "direct"), (4092, 1, "fourstep-bluestein", "direct"),
           (1, 1, "direct", "direct")])


def plan(gpu, ny, nx, py, px):
    xa, ctx, torch = gpu
    f = xa.Fft2D(ctx, ny, nx)
    ny1, ny2, nx1, nx2 = f.factors
    assert (path_of(ny, ny1, ny2), path_of(nx, nx1, nx2)) == (py, px), f.factors
    return f, axis_levels(ny, ny1, ny2), axis_levels(nx, nx1, nx2)


@pytest.mark.parametrize("ny,nx,py,px", SHAPES)
def test_fft2d_each_axis_and_both(gpu, ny, nx, py, px):
    """exec_axis 0 (the rows, along x) and 1 (the columns, along y) un-normalised both ways, exec forward and inverse (divided
    by ny nx), every path on rows and on columns."""
    xa, ctx, torch = gpu
    f, ly, lx = plan(gpu, ny, nx, py, px)
    rng = np.random.default_rng(ny * 31 + nx)
    x = (rng.standard_normal((ny, nx)) + 1j * rng.standard_normal((ny, nx))).astype(np.complex64)
    x64 = x.astype(np.complex128)
    for axis, npaxis, lev, p in ((0, 1, lx, px), (1, 0, ly, py)):
        for inverse in (False, True):
            got = f(torch.from_numpy(x).cuda(), inverse=inverse, axis=axis).cpu().numpy()
            n = x.shape[npaxis]
            exp = n * np.fft.ifft(x64, axis=npaxis) if inverse else np.fft.fft(x64, axis=npaxis)
            check(CLASS[p], got, exp, 32, lev)
    cls = CLASS[px if lx >= ly else py]
    for inverse in (False, True):
        got = f(torch.from_numpy(x).cuda(), inverse=inverse).cpu().numpy()
        exp = np.fft.ifft2(x64) if inverse else np.fft.fft2(x64)
        check(cls, got, exp, 32, lx + ly)
    f.close()


@pytest.mark.parametrize("ny,nx,py,px", [(3710, 3838, "fourstep-bluestein", "fourstep-bluestein"),
                                         (4096, 4096, "fourstep-pow2", "fourstep-pow2"),
                                         (8184, 11520, "fourstep-bluestein", "small")])
def test_fft2d_whole_detector_frames(gpu, ny, nx, py, px):
    """K2 (3710 x 3838), Falcon (4096 x 4096) and K3 super-resolution (8184 x 11520) frames: forward against numpy, then the
    inverse of that spectrum against the input."""
    xa, ctx, torch = gpu
    f, ly, lx = plan(gpu, ny, nx, py, px)
    rng = np.random.default_rng(ny + nx)
    x = np.empty((ny, nx), np.complex64)
    x.real = rng.standard_normal((ny, nx), dtype=np.float32)
    x.imag = rng.standard_normal((ny, nx), dtype=np.float32)
    d = torch.from_numpy(x).cuda()
    f(d)
    got = d.cpu().numpy()
    exp = np.fft.fft2(x.astype(np.complex128))
    check("2d-frame", got, exp, 32, lx + ly)
    del got, exp
    f(d, inverse=True)
    check("2d-frame", d.cpu().numpy(), x, 32, lx + ly)
    f.close()


# ---------------------------------------------------------------------------------------------- FlexAlign's row entries
def frame_input(rng, Y, X, cg):
    frame = (rng.standard_normal((Y, X)) * 3 + 10).astype(np.float32)
    dark = (rng.standard_normal((Y, X)) * 0.5).astype(np.float32) if cg else None
    gain = rng.uniform(0.8, 1.25, (Y, X)).astype(np.float32) if cg else None
    a = frame
    if cg:
        a = (frame - dark) * gain          # float32 arithmetic, like loadFrame
    return frame, dark, gain, a.astype(np.float64)


def packed_rows(a):
    Y = a.shape[0]
    z = np.zeros(((Y + 1) // 2, a.shape[1]), np.complex128)
    z.real = a[0::2]
    z[: Y // 2].imag = a[1::2]
    return z


def device(torch, a):
    return None if a is None else torch.from_numpy(a).cuda()


@pytest.mark.parametrize("cg", [False, True])
@pytest.mark.parametrize("Y", [9, 10])
@pytest.mark.parametrize("X,n1,n2", [(1440, 45, 32), (1536, 3, 512), (1920, 15, 128), (2880, 45, 64), (3840, 15, 256), (4032, 63, 64),
                                     (5760, 45, 128), (11520, 45, 256)])
def test_rows_of_real_pairs(gpu, X, n1, n2, Y, cg):
    """form 0 (k_fft2d_small_pairs, k_fft2d_45_pairs + the n2-point lines): the transform of row[2r] + i row[2r + 1] (the lone last
    row of an odd Y alone) at n2 (k % n1) + k / n1."""
    xa, ctx, torch = gpu
    rng = np.random.default_rng(X + Y + cg)
    frame, dark, gain, a = frame_input(rng, Y, X, cg)
    f = xa.Fft2D(ctx, (Y + 1) // 2, X)
    ny = (Y + 1) // 2
    out = torch.full((ny * X + 64,), SENTINEL, dtype=torch.complex64, device="cuda")
    _, info = f.debug_real_rows(device(torch, frame), device(torch, dark), device(torch, gain), form=0, out=out)
    assert info == (n1, n2, 1)
    o = out.cpu().numpy()
    assert np.all(o[ny * X:] == np.complex64(SENTINEL)), "written past the end"
    k = np.arange(X)
    got = o[: ny * X].reshape(ny, X)[:, n2 * (k % n1) + k // n1]
    exp = np.fft.fft(packed_rows(a), axis=1)
    check("rows-pairs", got, exp, 32, math.ceil(math.log2(n1)) + 2 + levels(n2))
    f.close()


@pytest.fixture(scope="module")
def k3_rows():
    """One 5760-wide frame (11 rows: the lone last one too), with and without dark / gain, and the spectra of its packed and real rows."""
    rng = np.random.default_rng(5760)
    out = {}
    for cg in (False, True):
        frame, dark, gain, a = frame_input(rng, 11, 5760, cg)
        out[cg] = (frame, dark, gain, np.fft.fft(a, axis=1), np.abs(np.fft.fft(packed_rows(a), axis=1)).max())
    return out


@pytest.mark.parametrize("cg", [False, True])
@pytest.mark.parametrize("nc", [1, 44, 45, 46, 359, 719, 720])
def test_rows_kept(gpu, k3_rows, nc, cg):
    """form 1 (k_fft2d_45x128_rows_kept): the first nc frequencies of every real row of a 5760-wide frame."""
    xa, ctx, torch = gpu
    frame, dark, gain, F, zmax = k3_rows[cg]
    Y, X = frame.shape
    f = xa.Fft2D(ctx, (Y + 1) // 2, X)
    out = torch.full((Y * nc + 64,), SENTINEL, dtype=torch.complex64, device="cuda")
    _, info = f.debug_real_rows(device(torch, frame), device(torch, dark), device(torch, gain), form=1, nc=nc, out=out)
    assert info == (45, 128, 1)
    o = out.cpu().numpy()
    assert np.all(o[Y * nc:] == np.complex64(SENTINEL)), "written past the end"
    got = o[: Y * nc].reshape(Y, nc)
    # error of the packed transform (scale: its largest coefficient), then the separation's two sums
    err = np.abs(got - F[:, :nc]).max()
    ratio = err / (EPS[32] * (math.ceil(math.log2(45)) + 2 + levels(128)) * zmax)
    WORST["rows-kept"] = max(WORST["rows-kept"], ratio)
    assert ratio <= C["rows-kept"], ratio
    f.close()


def test_rows_kept_declines_beyond_720(gpu, k3_rows):
    xa, ctx, torch = gpu
    frame = k3_rows[False][0]
    Y, X = frame.shape
    f = xa.Fft2D(ctx, (Y + 1) // 2, X)
    out = torch.full((Y * 721,), SENTINEL, dtype=torch.complex64, device="cuda")
    _, info = f.debug_real_rows(device(torch, frame), form=1, nc=721, out=out)
    assert info[2] == 0
    assert bool((out == SENTINEL).all())
    f.close()
