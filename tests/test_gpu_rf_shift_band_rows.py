"""k_rf_shift_band with the band's row quantities worked out once per wave (xh_rf.hip): lane k of a wave evaluates row k's source
ordinate, footprint start and four B-spline weights, and the wave reads them back lane by lane as scalars, where every thread used
to evaluate them for all sixteen rows.  The expressions are the ones k_rf_shift evaluates per thread (the file is built without
contraction), so the output must equal k_rf_shift's (option shift_bands 0, which tests/test_gpu_rf.py holds to the oracle) as bytes.

256 px is the only box the kernel serves; eight images per case.  The cases are the paths the rows can take: no shift (the copy),
whole and fractional shifts of both signs, shifts whose row wrap falls inside a band (that band goes pixel by pixel, the others
through LDS) or exactly between two bands, shifts beyond half a box and beyond a whole one (d_realwrap), each mirrored and not.
"""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

D, N = 256, 8

CASES = {
    # (shiftX, shiftY) per image
    "none": [(0.0, 0.0)] * N,
    "whole": [(3.0, -2.0), (-3.0, 2.0), (1.0, 0.0), (0.0, 1.0), (0.0, -1.0), (-7.0, -5.0), (12.0, 9.0), (0.0, 0.0)],
    "fractional": [(0.25, -0.75), (-1.5, 2.5), (2.125, 0.0), (0.0, -3.375), (1e-3, -1e-3), (-4.7, -6.1), (8.9, 7.3), (0.5, 0.5)],
    # the wrap of the rows inside a band (|shiftY| not a multiple of 16), on a band's edge (16, 32), next to it
    "row_wrap": [(0.0, 20.3), (0.0, -20.3), (1.5, 16.0), (-1.5, -32.0), (0.25, 15.999), (0.25, -16.001), (3.0, 100.5), (-3.0, -127.25)],
    # beyond half a box and beyond a whole one
    "far": [(130.25, -131.5), (-130.25, 131.5), (128.0, 128.0), (-128.0, -128.0), (300.5, -290.25), (-300.5, 290.25), (0.0, 255.5), (256.0, 256.0)],
}


@pytest.fixture(scope="module")
def gpu():
    import torch
    import xmipp3_amd as xa
    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    return xa, xa.Context(0), torch


@pytest.fixture(scope="module")
def images(gpu):
    xa, ctx, torch = gpu
    rng = np.random.default_rng(77)
    imgs = torch.from_numpy(rng.standard_normal((N, D, D)).astype(np.float32)).cuda()
    # any array serves as "the coefficients the caller has": either kernel interpolates what it is given
    coefs = torch.from_numpy(rng.standard_normal((N, D, D)).astype(np.float32)).cuda()
    return imgs, coefs


@pytest.fixture(scope="module")
def gridders(gpu):
    """one gridder per kernel, shared by every case: shift_images keeps no state between calls"""
    xa, ctx, torch = gpu
    rfs = {}
    for bands in (1, 0):
        rfs[bands] = xa.RecFourier(ctx, D)
        rfs[bands].set_option("shift_bands", bands)
    return rfs


def _shift(gridders, imgs, shifts, flips, bands, coefs):
    rf = gridders[bands]
    return rf.shift_images(imgs, shifts, flips=flips, coefs=coefs.data_ptr() if coefs is not None else None).cpu().numpy()


@pytest.mark.parametrize("with_coefs", [False, True], ids=["prefiltered_here", "coefs_given"])
@pytest.mark.parametrize("flipped", ["plain", "mirrored", "mixed"])
@pytest.mark.parametrize("case", list(CASES))
def test_band_rows_once_per_wave_gives_the_bits_of_the_plain_kernel(gpu, gridders, images, case, flipped, with_coefs):
    xa, ctx, torch = gpu
    imgs, coefs = images
    shifts = np.array(CASES[case], np.float32)
    flips = {"plain": np.zeros(N, np.uint8), "mirrored": np.ones(N, np.uint8), "mixed": (np.arange(N) % 2).astype(np.uint8)}[flipped]
    c = coefs if with_coefs else None
    band = _shift(gridders, imgs, shifts, flips, 1, c)
    plain = _shift(gridders, imgs, shifts, flips, 0, c)
    assert np.isfinite(plain).all()
    assert band.tobytes() == plain.tobytes()
    if case == "none":
        for i in range(N):
            if not flips[i]:
                assert band[i].tobytes() == imgs[i].cpu().numpy().tobytes()      # the copy path
    else:
        assert not np.array_equal(band, imgs.cpu().numpy())


def test_device_side_shifts_take_the_same_kernel(gpu, gridders, images):
    """shifts and flips as device tensors (what ProjectionMatcher.translate returns): the same bits as the plain kernel"""
    xa, ctx, torch = gpu
    imgs, coefs = images
    sh = np.array(CASES["row_wrap"][:4] + CASES["fractional"][:2] + CASES["far"][:2], np.float64)
    flips = torch.from_numpy((np.arange(N) % 2).astype(np.uint8)).cuda()
    dev = (torch.from_numpy(sh[:, 0].copy()).cuda(), torch.from_numpy(sh[:, 1].copy()).cuda())
    outs = []
    for bands in (1, 0):
        outs.append(gridders[bands].shift_images(imgs, dev, flips=flips, coefs=coefs.data_ptr()).cpu().numpy())
    assert outs[0].tobytes() == outs[1].tobytes()
