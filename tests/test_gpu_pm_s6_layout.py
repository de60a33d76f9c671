"""The fp32 chain of S6 (xh_pm_translate) with w column-major between its line passes (xh_pm.hip, S6Cm; option "s6_layout" 1, the
default) against the row-major kernels it replaces (option 0): only addresses and lane maps differ, every butterfly, twiddle
product, cross-power term and reduction keeps its operands and order, so everything the chain leaves must be equal as bytes.

Sizes 64, 128 and 256 px are the three instantiations of the chain; batches of 1, 2 and 5 (an odd batch pairs its last particle
with itself).  The particles are those of tests/test_gpu_pm_s6_planes.py (flips mixed, entry 3 without a reference) with two of them
replaced: entry 1, a plain particle, is rolled by half a box along x, so the maximum of its map lies at the wrap seam of the centred
map, and entry 2 is blank (all zero: a constant map, shift (0, 0), maxCC undefined in the oracle as well).
Compared per case: shifts, maxCC and the number of particles repeated in double precision with the default margin (a particle
flagged under one layout only would come back with the other precision's bits); the same with the margin at zero, where the fp32
pass alone speaks; the fp32 correlation maps themselves (s6_capture 32).  Layout 1 against the CPU oracle keeps the bounds of
tests/test_gpu_pm_s6_planes.py: shifts 1e-3 px, maxCC 1e-5.
"""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

from tests.test_gpu_pm_s6_planes import MAX_SHIFT, _case  # noqa: E402

SIZES = [64, 128, 256]


@pytest.fixture(scope="module")
def gpu():
    import torch
    import xmipp3_amd as xa
    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    return xa, xa.Context(0), torch


_built = {}


def _data(oracle, D):
    """the case of the planes test with the seam particle and the blank one; the oracle's translation of the five, once per size"""
    if D in _built:
        return _built[D]
    refs, parts, er, ep, ef, _ = _case(oracle, D)
    parts, er, ep, ef = parts.copy(), er.copy(), ep.copy(), ef.copy()
    assert ef[1] == 0 and er[3] == -1 and ef[0] == 1 and ef[4] == 1
    parts[1] = np.roll(parts[1], D // 2, axis=1)
    parts[2] = 0.0
    ef[2] = 0
    expect = oracle.PM(refs).translate(parts, er, ep, ef, MAX_SHIFT)
    _built[D] = refs, parts, er, ep, ef, [np.asarray(v) for v in expect]
    return _built[D]


def _matcher(gpu, refs, layout, eps=None, capture=0):
    xa, ctx, torch = gpu
    pm = xa.ProjectionMatcher(ctx, torch.from_numpy(refs).cuda())
    pm.set_option("s6_layout", layout)
    assert pm.get_option("s6_layout") == layout
    if eps is not None:
        pm.set_option("s6_eps", eps)
    if capture:
        pm.set_option("s6_capture", capture)
    return pm


def _translate(gpu, pm, data, m, max_shift=MAX_SHIFT):
    xa, ctx, torch = gpu
    refs, parts, er, ep, ef, _ = data
    out = pm.translate(torch.from_numpy(parts[:m]).cuda(), torch.from_numpy(er[:m]).cuda(), torch.from_numpy(ep[:m]).cuda(),
                       torch.from_numpy(ef[:m]).cuda(), max_shift)
    return [t.cpu().numpy() for t in out]


def _close(a, b, tol):
    """|a - b| <= tol, NaN only against NaN (the blank particle's maxCC)"""
    return bool(np.all((np.isnan(a) & np.isnan(b)) | (np.abs(a - b) <= tol)))


def test_the_option_defaults_to_the_new_layout(gpu, oracle):
    xa, ctx, torch = gpu
    pm = xa.ProjectionMatcher(ctx, torch.from_numpy(_data(oracle, 64)[0]).cuda())
    assert pm.get_option("s6_layout") == 1
    pm.close()


@pytest.mark.parametrize("m", [1, 2, 5])
@pytest.mark.parametrize("D", SIZES)
def test_both_layouts_give_the_same_bytes_and_the_oracles_values(gpu, oracle, D, m):
    data = _data(oracle, D)
    er = data[2]
    expect = [v[:m] for v in data[5]]
    for eps in (None, 0.0):                          # the default margin (some particles repeated in double), the fp32 pass alone
        res = {}
        for layout in (1, 0):
            pm = _matcher(gpu, data[0], layout, eps)
            res[layout] = _translate(gpu, pm, data, m), pm.translate_repeated()
            if layout == 1:
                again = _translate(gpu, pm, data, m)
                for a, b in zip(res[1][0], again):
                    assert a.tobytes() == b.tobytes()
                wide = _translate(gpu, pm, data, m, -1.0), pm.translate_repeated()      # max_shift D/2: the seam particle's shift is kept
            else:
                wide0 = _translate(gpu, pm, data, m, -1.0), pm.translate_repeated()
            pm.close()
        (new, rep1), (old, rep0) = res[1], res[0]
        print("D", D, "m", m, "eps", eps, "repeated", rep1, rep0, "max |dsx|", np.nanmax(np.abs(new[0] - expect[0])), "|dsy|",
              np.nanmax(np.abs(new[1] - expect[1])), "|dcc|", np.nanmax(np.abs(new[2] - expect[2])))
        assert rep1 == rep0 and wide[1] == wide0[1]
        if eps == 0.0:
            assert rep1 == 0
        for a, b in zip(new + wide[0], old + wide0[0]):
            assert a.tobytes() == b.tobytes()
        assert _close(new[0], expect[0], 1e-3) and _close(new[1], expect[1], 1e-3)
        assert _close(new[2], expect[2], 1e-5)
        if m == 5:
            assert new[0][3] == 0 and new[1][3] == 0 and new[2][3] == 0          # refno = -1
            assert new[0][2] == 0 and new[1][2] == 0                             # the blank particle
        assert int((er[:m] >= 0).sum()) >= rep1


@pytest.mark.parametrize("D", SIZES)
def test_the_fp32_maps_are_the_same_bytes(gpu, oracle, D):
    """the correlation maps the fp32 chain leaves for bestShift (s6_capture 32), five particles: every element, not only what the
    arg-max and the fit look at"""
    data = _data(oracle, D)
    maps = {}
    for layout in (1, 0):
        pm = _matcher(gpu, data[0], layout, capture=32)
        _translate(gpu, pm, data, 5)
        maps[layout] = pm.debug_s6_maps(5)
        pm.close()
    assert np.isfinite(maps[0]).all() and np.ptp(maps[0][0]) > 0
    assert maps[1].tobytes() == maps[0].tobytes()
    # the rolled particle's maximum lies half a box from where the unrolled particles have theirs (within the +-3 px they were shifted by)
    c0 = np.unravel_index(np.argmax(maps[1][0]), (D, D))[1]
    c1 = np.unravel_index(np.argmax(maps[1][1]), (D, D))[1]
    d = abs(int(c1) - int(c0))
    assert abs(min(d, D - d) - D // 2) <= 6, (c0, c1)


def test_a_smaller_batch_after_a_larger_one_reads_nothing_stale(gpu, oracle):
    """translate with five particles, then with two on the same handle: w, the maps and the block statistics of the first call are
    still in the scratch buffers, and the second call must give the bytes of a fresh handle's"""
    D = 128
    data = _data(oracle, D)
    pm = _matcher(gpu, data[0], 1)
    _translate(gpu, pm, data, 5)
    second = _translate(gpu, pm, data, 2)
    pm.close()
    pm = _matcher(gpu, data[0], 1)
    fresh = _translate(gpu, pm, data, 2)
    pm.close()
    pm = _matcher(gpu, data[0], 0)
    old = _translate(gpu, pm, data, 2)
    pm.close()
    for a, b, c in zip(second, fresh, old):
        assert a.tobytes() == b.tobytes() == c.tobytes()
