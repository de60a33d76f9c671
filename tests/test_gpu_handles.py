"""Lifetimes of the library's handles: every destroy returns all the device memory its handle held (xh_device_bytes_held),
failed creates leave nothing behind, and the gridder's record buffer grown between two calls stays finite."""
import ctypes as C
import gc

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

from tests import synth  # noqa: E402


@pytest.fixture(scope="module")
def gpu():
    import torch
    import xmipp3_amd as xa
    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    ctx = xa.Context(0)
    return xa, ctx, torch


def held():
    from xmipp3_amd import _lib
    v = C.c_int64()
    assert _lib.lib().xh_device_bytes_held(C.byref(v)) == 0
    return v.value


def _rf(xa, ctx, torch):
    D = 32
    rf = xa.RecFourier(ctx, D)
    rf.insert_images(torch.randn((6, D, D), device="cuda"), synth.random_angles(6, np.random.default_rng(1)))
    return rf


def _rf2(xa, ctx, torch):
    D = 32
    rf2 = xa.RecFourier2(ctx, D)
    rf2.insert(torch.randn((4, D, D), device="cuda"), synth.random_angles(4, np.random.default_rng(2)))
    rf2.finish()
    return rf2


def _fft2d(xa, ctx, torch):
    f = xa.Fft2D(ctx, 48, 90)
    f(torch.randn((48, 90), dtype=torch.complex64, device="cuda"))
    return f


def _fa(xa, ctx, torch):
    fa = xa.FlexAlign(ctx, 128, 128, 1.0, 8.0)
    fa.global_alignment(torch.randn((3, 128, 128), device="cuda"), 10.0)
    return fa


def _shiftcorr(xa, ctx, torch):
    est = xa.ShiftCorrEstimator(ctx, 32, 32, 8)
    est.load_reference(torch.randn((32, 32), device="cuda"))
    est.compute_shifts(torch.randn((5, 32, 32), device="cuda"))
    return est


def _align_sig(xa, ctx, torch):
    al = xa.AlignSignificant(ctx, 32, 2, batch_pairs=4)
    al.load_references(torch.randn((2, 32, 32), device="cuda"))
    al.align(torch.randn((3, 32, 32), device="cuda"))
    return al


def _halves(xa, ctx, torch):
    h = xa.HalvesRestoration(ctx, (16, 16, 16))
    h.load(torch.randn((16, 16, 16), dtype=torch.float64, device="cuda"), torch.randn((16, 16, 16), dtype=torch.float64, device="cuda"))
    h.denoise(1)
    return h


def _ctfops(xa, ctx, torch):
    from xmipp3_amd.api import ctf_params
    op = xa.CtfOps(ctx, 32, 32, pad=2.0)
    op.wiener2d(torch.randn((2, 32, 32), device="cuda"), [ctf_params(kV=300.0, Cs=2.7, Q0=0.07, K=1.0, DeltafU=15000.0, DeltafV=15500.0)] * 2)
    return op


def _fp(xa, ctx, torch):
    fp = xa.FourierProjector(ctx, torch.randn((16, 16, 16), device="cuda"))
    fp.project(synth.random_angles(3, np.random.default_rng(3)))
    return fp


def _pm(xa, ctx, torch):
    pm = xa.ProjectionMatcher(ctx, torch.randn((8, 32, 32), device="cuda"))
    pm.match(torch.randn((4, 32, 32), device="cuda"))
    return pm


@pytest.mark.parametrize("make", [_rf, _rf2, _fft2d, _fa, _shiftcorr, _align_sig, _halves, _ctfops, _fp, _pm],
                         ids=lambda f: f.__name__.lstrip("_"))
def test_destroy_returns_every_byte(gpu, make):
    """Create a handle, run one call that grows its scratch, destroy it: the library holds exactly what it held before."""
    xa, ctx, torch = gpu
    gc.collect()
    ctx.sync()
    before = held()
    h = make(xa, ctx, torch)
    ctx.sync()
    assert held() > before
    h.close()
    assert held() == before


def test_failed_create_leaves_nothing(gpu):
    """Creates that refuse their arguments after their first allocation (the line plans of the double-precision transform are made
    before their length is checked against the LDS) free what they had allocated."""
    xa, ctx, torch = gpu
    gc.collect()
    before = held()
    with pytest.raises(xa.XhError):
        xa.ShiftCorrEstimator(ctx, 2050, 64, 8)
    assert held() == before
    with pytest.raises(xa.XhError):
        xa.AlignSignificant(ctx, 2050, 1, batch_pairs=1)
    assert held() == before


def test_grown_record_buffer_gives_the_one_call_result(gpu):
    """xh_rf_insert_images reserves its record buffer per call and zeroes it whenever the reservation grows: a small batch, then a
    larger one, on one handle equal the same images in one call on a fresh handle, within the tolerance of
    test_gpu_rf.py::test_linearity_of_insertion (the gridding adds with atomics in no fixed order), and nothing is NaN.  This test
    cannot force the allocator to hand back memory that holds NaN; the guarantee is that the zeroing is keyed on the growth the
    reservation reports, not on the address it returns."""
    xa, ctx, torch = gpu
    D, n1, n = 32, 3, 24
    g = torch.Generator(device="cuda").manual_seed(5)
    imgs = torch.randn((n, D, D), generator=g, device="cuda")
    ang = synth.random_angles(n, np.random.default_rng(5))
    a = xa.RecFourier(ctx, D)
    a.insert_images(imgs[:n1].contiguous(), ang[:n1])
    a.insert_images(imgs[n1:].contiguous(), ang[n1:])
    b = xa.RecFourier(ctx, D)
    b.insert_images(imgs, ang)
    assert not torch.isnan(a.temp).any() and not torch.isnan(b.temp).any()
    assert b.temp.abs().max().item() > 0
    assert (a.temp - b.temp).abs().max().item() <= 2e-6 * b.temp.abs().max().item()
    a.mirror_and_crop()
    b.mirror_and_crop()
    va, vb = a.finish(), b.finish()
    assert np.isfinite(va).all() and np.isfinite(vb).all()
    # finished volumes of one data set gridded in different groupings: test_gpu_rf.py::test_half_sets_sum_to_the_full_reconstruction
    assert np.abs(va - vb).max() <= 1e-5 * np.abs(vb).max()
    a.close()
    b.close()
