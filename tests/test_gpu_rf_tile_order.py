"""The gridding kernel's tile list (xmipp3_amd/csrc/xh_rf_tiles.h: heavy tiles around the origin first in every class) on the device,
at a box whose volume is no multiple of the tile size: every voxel is still written, once, and the stream counters start from
zero at every launch."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

from tests import synth  # noqa: E402


def _compare(rf, o):
    ev, ew = o.temp()
    gv, gw = rf.temp_spaces()
    gv, gw = gv.cpu().numpy(), gw.cpu().numpy()
    assert (ew != 0).sum() > 1000
    assert np.array_equal(gw != 0, ew != 0)
    assert np.abs(gw - ew).max() <= 2e-6 * np.abs(ew).max()
    assert np.abs(gv - ev).max() <= 2e-6 * np.abs(ev).max()


def test_box_40_against_the_oracle_twice_on_one_handle(oracle):
    import torch
    import xmipp3_amd as xa
    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    ctx = xa.Context(0)
    D = 40
    rf = xa.RecFourier(ctx, D)
    assert rf.mv == 80
    o = oracle.RF(D)
    rng = np.random.default_rng(11)
    # 48 random orientations, the three axis-aligned ones, and 17 others for the second launch
    ang = np.concatenate([synth.random_angles(48, rng), np.array([[0.0, 0.0, 0.0], [0.0, 90.0, 0.0], [90.0, 90.0, 0.0]]),
                          synth.random_angles(17, rng)])
    n = len(ang)
    ffts = np.stack([o.prepare_image(im) for im in rng.standard_normal((n, D, D)).astype(np.float32)])
    ctf = (rng.uniform(0.5, 2.0, ffts.shape[:3]) * rng.choice([-1, 1], ffts.shape[:3])).astype(np.float32)
    mod = rng.uniform(0.0, 1.0, ffts.shape[:3]).astype(np.float32)

    def insert(o_, lo, hi):
        for i in range(lo, hi):
            o_.insert(ffts[i], synth.euler_matrix(*ang[i]).T, ctf=ctf[i], modulator=mod[i])
        rf.insert(torch.from_numpy(ffts[lo:hi]).cuda(), ang[lo:hi], ctf=torch.from_numpy(ctf[lo:hi]).cuda(),
                  modulator=torch.from_numpy(mod[lo:hi]).cuda())

    insert(o, 0, 51)
    _compare(rf, o)
    # a second launch on the same handle: the ring's stream counters are cleared per launch
    rf.reset()
    o2 = oracle.RF(D)
    insert(o2, 51, n)
    _compare(rf, o2)
