"""GPU tests of xmipp_reconstruct_significant's device side (xh_rsig_*): alignImagesConsideringMirrors of every (image, projection)
pair against the numpy restatement (tests/reconstruct_significant_ref.py) chain by chain, the two weighting stages against their
restatement, and the handle's argument checks. Batches of more than 256 chains and weights past one tile of 256 and one block of
images: tests/test_gpu_reconstruct_significant_laps.py.

Parity bound of align. A chain is about 10^2 reductions of D^2 fp64 terms; device and restatement differ in the order of every sum
(trees against serial loops), in the line transforms (radix 2 / Bluestein against the oracle's) and in applyGeometry's source
coordinate (computed directly against added along the row). Measured on an MI355X over the three cases, the largest
|device - restatement| / max(1, |restatement|) of M, corr and imed over all 464 chains and 116 pairs was 4.6e-15 (1.9e-15 at D = 20,
3.4e-15 at D = 32, 4.6e-15 at D = 48), with no chain excluded as a near-tie; the bound is 16 times that rounded up to a power of ten."""
import itertools

import numpy as np
import pytest

from tests import reconstruct_significant_ref as R

pytestmark = pytest.mark.gpu

_BOUND = 1e-13
_TIE = 1e-9          # decisions taken by less than this are near-ties and are not compared


@pytest.fixture(scope="module")
def gpu():
    import torch
    import __graft_entry__ as g
    g.build()
    import xmipp3_amd as xa
    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    return xa, xa.Context(0), torch


_runs = {}


def _align(gpu, D, batch_chains, mirrors=True):
    """One device run of a case, kept: dict of numpy arrays plus the stats"""
    key = (D, batch_chains, mirrors)
    if key not in _runs:
        xa, ctx, torch = gpu
        gallery, _, _, images = R.population(D)
        h = xa.ReconstructSignificant(ctx, D, len(gallery), batch_chains=batch_chains)
        h.load_gallery(torch.from_numpy(gallery).cuda())
        M, corr, imed, tr, ch = h.align(torch.from_numpy(images).cuda(), check_mirrors=mirrors, trace=True, chains=True)
        out = {"M": M, "corr": corr, "imed": imed, "trace": tr}
        out.update({"chain_" + k: v for k, v in ch.items()})
        _runs[key] = ({k: v.cpu().numpy() for k, v in out.items()}, h.stats())
        h.close()
    return _runs[key]


def _rel(got, ref):
    ref = np.asarray(ref, np.float64)
    return float(np.max(np.abs(got - ref) / np.maximum(1.0, np.abs(ref))))


@pytest.mark.parametrize("D", sorted(R.CASES))
def test_align_matches_the_restatement_chain_by_chain(gpu, D):
    nv, nd, N = R.CASES[D]
    G = nv * nd
    got, stats = _align(gpu, D, 8)
    ref = R.reference(D)
    # a batch of 8 chains is two pairs: N G / 2 batches, the last one partial where N G is odd; one batch of everything gives the same bytes
    whole, _ = _align(gpu, D, 4 * N * G)
    for k in got:
        assert np.array_equal(got[k], whole[k], equal_nan=True), f"{k} depends on the batch size"
    worst, excluded, chains = 0.0, 0, 0
    for n, g, m, o in itertools.product(range(N), range(G), range(2), range(2)):
        c = ref[n][g]["chains"][m][o]
        chains += 1
        if c["margin"] < _TIE:
            excluded += 1
            continue
        assert int(got["chain_trace"][n, g, m, o]) == c["trace"], f"chain {(n, g, m, o)}: steps {got['chain_trace'][n, g, m, o]:#x}, restatement {c['trace']:#x}"
        worst = max(worst, _rel(got["chain_M"][n, g, m, o], c["M"]), _rel(got["chain_corr"][n, g, m, o], c["corr"]), _rel(got["chain_imed"][n, g, m, o], c["imed"]))
    for n, g in itertools.product(range(N), range(G)):
        p = ref[n][g]
        if p["margin"] < _TIE:
            continue
        assert int(got["trace"][n, g]) == p["trace"], f"pair {(n, g)}: trace {got['trace'][n, g]:#x}, restatement {p['trace']:#x}"
        worst = max(worst, _rel(got["M"][n, g], p["M"]), _rel(got["corr"][n, g], p["corr"]), _rel(got["imed"][n, g], p["imed"]))
    print(f"D={D}: {chains} chains, {excluded} excluded as near-ties, largest relative difference {worst:.3e}, stats {stats}")
    assert excluded <= 0.02 * chains
    assert worst <= _BOUND
    # the stats count what the traces say ran
    tr = got["chain_trace"].astype(np.int64)
    for rnd in range(3):
        assert stats[f"shift_round{rnd + 1}"] == int(((tr >> (3 * rnd)) & 1).sum())
        assert stats[f"rotation_round{rnd + 1}"] == int(((tr >> (3 * rnd + 1)) & 1).sum())


@pytest.mark.parametrize("D", sorted(R.CASES))
def test_without_mirrors_is_the_plain_half_of_the_mirrored_run(gpu, D):
    both, _ = _align(gpu, D, 8)
    plain, _ = _align(gpu, D, 8, mirrors=False)
    for k in ("chain_M", "chain_corr", "chain_imed", "chain_trace"):
        assert plain[k].shape[2] == 1
        assert np.array_equal(plain[k][:, :, 0], both[k][:, :, 0], equal_nan=True), k
    # alignImages alone: corrRS > corrSR picks the pair's answer
    rs = plain["chain_corr"][:, :, 0, 1] > plain["chain_corr"][:, :, 0, 0]
    pick = np.where(rs, plain["chain_corr"][:, :, 0, 1], plain["chain_corr"][:, :, 0, 0])
    assert np.array_equal(plain["corr"], pick)
    assert np.array_equal(plain["trace"] & 3, rs.astype(np.int32) << 1)


_ANGLES = {  # per volume: directions 0 and 1 are 8 degrees apart, 2 is 30 degrees from 0, the rest far away
    6: (np.array([0., 0., 0., 90., 180., 270.]), np.array([20., 28., 50., 90., 90., 120.])),
}


@pytest.mark.parametrize("apply_fisher, ang_distance, validation", list(itertools.product((False, True), (10.0, 40.0), (False, True))))
def test_weights_match_the_restatement(gpu, apply_fisher, ang_distance, validation):
    xa, ctx, torch = gpu
    D = 32
    nv, nd, N = R.CASES[D]
    got, _ = _align(gpu, D, 8)
    rot, tilt = (np.tile(a, nv) for a in _ANGLES[nd])
    if validation:                      # --useForValidation 3: alpha = numOrientationsPerParticle / Ndirs, deltaAlpha2 = 1 / (2 Ndirs) (:704-739)
        one_alpha = 1 - 3.0 / nd - 1.0 / (2 * nd)
    else:
        one_alpha = 1 - 0.05 - 0.0
    h = xa.ReconstructSignificant(ctx, D, nv * nd, batch_chains=8)
    for use_imed, strict, max_shift in itertools.product((False, True), (False, True), (-1.0, 3.0)):
        cc, imed = torch.from_numpy(got["corr"]).cuda(), torch.from_numpy(got["imed"]).cuda()
        w = h.weights(torch.from_numpy(got["M"]).cuda(), cc, imed, nv, rot, tilt, ang_distance, one_alpha, apply_fisher=apply_fisher, use_imed=use_imed, strict=strict,
                      max_shift=max_shift).cpu().numpy()
        ew, ecc, eimed = R.weights(got["M"], got["corr"], got["imed"], D, nv, rot, tilt, ang_distance, one_alpha, apply_fisher, use_imed, strict, max_shift)
        what = (apply_fisher, ang_distance, validation, use_imed, strict, max_shift)
        assert np.array_equal(w == 0, ew == 0), what
        assert np.all(np.abs(w - ew) <= 1e-12 * np.abs(ew)), what
        assert np.all(np.abs(cc.cpu().numpy() - ecc) <= 1e-12 * np.abs(ecc)) and np.all(np.abs(imed.cpu().numpy() - eimed) <= 1e-12 * np.abs(eimed)), what
    h.close()


def test_weights_paths_differ_on_this_population(gpu):
    """the parity above would say nothing if an option left the weights as they were"""
    D = 32
    nv, nd, N = R.CASES[D]
    got, _ = _align(gpu, D, 8)
    rot, tilt = (np.tile(a, nv) for a in _ANGLES[nd])
    base = R.weights(got["M"], got["corr"], got["imed"], D, nv, rot, tilt, 10.0, 0.5)[0]
    assert np.count_nonzero(base) > 0
    # (the Fisher limit lies below every correlation of this population; tests/test_reconstruct_significant_host.py has a case where it cuts)
    for kw in ({"use_imed": True}, {"strict": True}, {"max_shift": 3.0}):
        assert not np.array_equal(R.weights(got["M"], got["corr"], got["imed"], D, nv, rot, tilt, 10.0, 0.5, **kw)[0], base), kw
    assert not np.array_equal(R.weights(got["M"], got["corr"], got["imed"], D, nv, rot, tilt, 40.0, 0.5, strict=True)[0],
                              R.weights(got["M"], got["corr"], got["imed"], D, nv, rot, tilt, 10.0, 0.5, strict=True)[0])


def test_fisher_limit_and_its_nan_on_the_device(gpu):
    """The population above never meets the Fisher limit (it lies below every correlation, or only the best direction is selected), so the
    limit is checked on hand-made arrays: 5 images x 4 directions where the limit cuts some selected pairs and passes others, and one
    image whose best correlation times one_alpha is above 1, which makes the limit NaN: nothing of that image is selected."""
    from tests.test_reconstruct_significant_host import _CC, _IMED, _ROT, _TILT, _matrices
    xa, ctx, torch = gpu
    D, one_alpha = 32, 0.5
    cc0 = _CC.copy()
    cc0[3, 3] = 2.5                                            # image 3: best . one_alpha = 1.25, the logarithm of a negative number
    M0 = _matrices({(0, 0): 5.0})
    h = xa.ReconstructSignificant(ctx, D, 4, batch_chains=8)

    def device(apply_fisher, use_imed, strict, max_shift):
        cc, imed = torch.from_numpy(cc0).cuda(), torch.from_numpy(_IMED.copy()).cuda()
        w = h.weights(torch.from_numpy(M0).cuda(), cc, imed, 1, _ROT, _TILT, 10.0, one_alpha, apply_fisher=apply_fisher, use_imed=use_imed, strict=strict, max_shift=max_shift)
        return w.cpu().numpy(), cc.cpu().numpy(), imed.cpu().numpy()
    for use_imed, strict, max_shift in itertools.product((False, True), (False, True), (-1.0, 3.0)):
        got = {f: device(f, use_imed, strict, max_shift) for f in (False, True)}
        for f in (False, True):
            ew, ecc, eimed = R.weights(M0, cc0, _IMED, D, 1, _ROT, _TILT, 10.0, one_alpha, f, use_imed, strict, max_shift)
            w, cc, imed = got[f]
            what = (f, use_imed, strict, max_shift)
            assert np.array_equal(w == 0, ew == 0), what
            assert np.all(np.abs(w - ew) <= 1e-12 * np.abs(ew)), what
            assert np.array_equal(cc, ecc) and np.array_equal(imed, eimed), what
        off, on = got[False][0], got[True][0]
        assert on[4, 2] == 0, "image 4, direction 2 (cc 0.15) lies below the limit 0.293"
        if not strict:                                          # (--strictDirection drops image 4 from directions 1 and 2 by itself)
            assert off[4, 2] > 0, "image 4, direction 2 passes the percentile"
            assert on[4, 1] == off[4, 1] > 0, "image 4, direction 1 (cc 0.45) is above the limit"
        assert np.count_nonzero(off[3]) > 0 and np.all(on[3] == 0), "a NaN limit selects nothing"
    h.close()


def test_handle_hygiene(gpu):
    xa, ctx, torch = gpu
    D = 20
    gallery, _, _, images = R.population(D)
    full, _ = _align(gpu, D, 8)
    h = xa.ReconstructSignificant(ctx, D, len(gallery), batch_chains=8)
    # a gallery of 3, then the whole one: the second load replaces the first
    h.load_gallery(torch.from_numpy(gallery[:3]).cuda())
    M3, corr3, imed3 = h.align(torch.from_numpy(images[:1]).cuda())
    assert tuple(M3.shape) == (1, 3, 3, 3)
    assert np.array_equal(corr3.cpu().numpy(), full["corr"][:1, :3]) and np.array_equal(M3.cpu().numpy(), full["M"][:1, :3])
    h.load_gallery(torch.from_numpy(gallery).cuda())
    M, corr, imed = h.align(torch.from_numpy(images[2:3]).cuda())              # N = 1
    assert np.array_equal(corr.cpu().numpy(), full["corr"][2:3]) and np.array_equal(imed.cpu().numpy(), full["imed"][2:3])
    h.close()
    for bad in ((21, 4, 8), (14, 4, 8), (20, 4, 0), (20, 0, 8)):
        with pytest.raises(xa.XhError, match=r"xmipp_hip error -1: xh_rsig_create"):          # XH_ERR_ARG
            xa.ReconstructSignificant(ctx, *bad[:2], batch_chains=bad[2])
    h = xa.ReconstructSignificant(ctx, D, 4, batch_chains=8)
    with pytest.raises(xa.XhError):
        h.load_gallery(torch.from_numpy(gallery[:5]).cuda())                    # more than max_gallery
    with pytest.raises(xa.XhError):
        h.align(torch.from_numpy(images[:1]).cuda())                            # nothing loaded
    h.close()


# ---------------------------------------------------------------- the program end to end
import os            # noqa: E402
import subprocess    # noqa: E402

from tests import synth, xmipp_io    # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIN = os.path.join(ROOT, "xmipp3_amd", "bin")


def _prog(name, args, cwd):
    return subprocess.run([os.path.join(BIN, name)] + args, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=300, cwd=str(cwd))


@pytest.fixture(scope="module")
def program_case(gpu, tmp_path_factory):
    """D = 32, one phantom, 24 noisy images from 6 directions; the two-iteration runs with and without --keepIntermediateVolumes, and the
    first iteration's gallery made once more by xmipp_angular_project_library with the program's arguments (the program deletes its own)"""
    from scipy import ndimage
    tmp = tmp_path_factory.mktemp("rsig")
    D = 32
    vol = R._asymmetric_phantom(D, 3)
    rng = np.random.default_rng(11)
    imgs = []
    for r, t in synth.fibonacci_directions(12)[:6]:                 # the upper hemisphere: the gallery covers tilt 0 .. 90
        p = synth.project(vol, r, t, 0.0)
        for _ in range(4):
            q = ndimage.shift(ndimage.rotate(p, float(rng.uniform(0, 360)), reshape=False, order=3, mode="constant"), rng.uniform(-2, 2, 2), order=1, mode="constant")
            imgs.append(q + 0.5 * q.std() * rng.standard_normal(q.shape))
    xmipp_io.write_stack(str(tmp / "imgs.stk"), np.array(imgs))
    xmipp_io.write_xmd(str(tmp / "imgs.xmd"), [("noname", ["itemId", "image"], [[100 + i, f"{i + 1:06d}@imgs.stk"] for i in range(24)])])
    xmipp_io.write_volume(str(tmp / "init.vol"), vol)
    xmipp_io.write_xmd(str(tmp / "vols.xmd"), [("noname", ["image"], [["init.vol"]])])
    common = ["-i", "imgs.xmd", "--initvolumes", "vols.xmd", "--angularSampling", "30", "--iter", "2"]
    runs = {}
    for odir, extra in (("keep", ["--keepIntermediateVolumes"]), ("nokeep", [])):
        runs[odir] = _prog("xmipp_reconstruct_significant", common + extra + ["--odir", odir], tmp)
        assert runs[odir].returncode == 0, runs[odir].stderr
    r = _prog("xmipp_angular_project_library", ["-i", "keep/volume_iter000_00.vol", "-o", "gal.stk", "--sampling_rate", "30.000000", "--sym", "c1", "--compute_neighbors",
                                                "--angular_distance", "-1", "--experimental_images", "keep/angles_iter000_00.xmd", "--min_tilt_angle", "0.000000",
                                                "--max_tilt_angle", "90.000000", "-v", "0"], tmp)
    assert r.returncode == 0, r.stderr
    return tmp, np.array(imgs), runs


def _files(d):
    return sorted(os.listdir(str(d)))


def test_program_file_sets(program_case):
    tmp, _, runs = program_case
    per_iter = lambda it: [f"angles_iter{it:03d}_00.xmd", f"images_iter{it:03d}_00.xmd", f"images_significant_iter{it:03d}_00.xmd", f"volume_iter{it:03d}_00.vol"]  # noqa: E731
    assert _files(tmp / "keep") == sorted(["angles_iter000_00.xmd", "volume_iter000_00.vol"] + per_iter(1) + per_iter(2))       # galleries deleted
    assert _files(tmp / "nokeep") == sorted(per_iter(2))                                                                        # and the earlier iterations
    for name in per_iter(2):
        assert (tmp / "keep" / name).read_bytes() == (tmp / "nokeep" / name).read_bytes(), name
    assert runs["keep"].stdout.count("Current significance: 0.95") == 2 and "Iteration 2" in runs["keep"].stdout


def _expected_angle_rows(gpu, tmp, imgs, **opt):
    """angles_iter001_00.xmd from the binding and the restatement's row rules: a row per pair with a positive final weight, image after
    image, direction after direction"""
    xa, ctx, torch = gpu
    labels, rows = xmipp_io.read_xmd(str(tmp / "gal.doc"))
    col = {l: k for k, l in enumerate(labels)}
    rot, tilt = np.array([float(r[col["angleRot"]]) for r in rows]), np.array([float(r[col["angleTilt"]]) for r in rows])
    gallery = xmipp_io.read_stack(str(tmp / "gal.stk")).astype(np.float64)
    assert len(gallery) == len(rows) >= 6
    h = xa.ReconstructSignificant(ctx, 32, len(gallery))
    h.load_gallery(torch.from_numpy(gallery).cuda())
    M, cc, imed = h.align(torch.from_numpy(imgs.astype(np.float32).astype(np.float64)).cuda())
    w = h.weights(M, cc, imed, 1, rot, tilt, 10.0, 1 - 0.05 - 0.0, **opt).cpu().numpy()
    h.close()
    M, cc, imed = M.cpu().numpy(), cc.cpu().numpy(), imed.cpu().numpy()
    out = []
    for n in range(len(imgs)):
        for g in range(len(gallery)):
            if not w[n, g] > 0:
                continue
            flip, sx, sy, psi = R.shifts_of(M[n, g])
            if flip:
                sx *= -1
            out.append({"image": f"{n + 1:06d}@imgs.stk", "itemId": str(100 + n), "enabled": "1", "maxCC": cc[n, g], "cost": imed[n, g], "angleRot": rot[g], "angleTilt": tilt[g],
                        "anglePsi": psi, "shiftX": -sx, "shiftY": -sy, "flip": str(int(flip)), "imageIndex": str(n), "ref": str(g), "ref3d": "0", "weight": w[n, g],
                        "weightSignificant": w[n, g]})
    return out


def _check_angle_rows(path, expected):
    labels, rows = xmipp_io.read_xmd(str(path))
    assert set(labels) == set(expected[0]), labels
    assert len(rows) == len(expected)
    col = {l: k for k, l in enumerate(labels)}
    for r, e in zip(rows, expected):
        for l, v in e.items():
            assert r[col[l]] == (v if isinstance(v, str) else f"{v:.6f}"), (l, r, e)


def test_program_angles_are_the_binding_plus_the_row_rules(gpu, program_case):
    tmp, imgs, _ = program_case
    expected = _expected_angle_rows(gpu, tmp, imgs)
    assert 24 <= len(expected)                                       # alpha 0.05: at least every image's best direction
    _check_angle_rows(tmp / "keep" / "angles_iter001_00.xmd", expected)
    # images_significant: the rows of images_iter whose image occurs in angles
    la, ra = xmipp_io.read_xmd(str(tmp / "keep" / "angles_iter001_00.xmd"))
    li, ri = xmipp_io.read_xmd(str(tmp / "keep" / "images_iter001_00.xmd"))
    ls, rs = xmipp_io.read_xmd(str(tmp / "keep" / "images_significant_iter001_00.xmd"))
    names = {r[la.index("image")] for r in ra}
    assert len(ri) == 24 and ls == li and rs == [r for r in ri if r[li.index("image")] in names]


def test_program_volume_is_reconstruct_fourier_then_the_mask(program_case):
    tmp, _, _ = program_case
    r = _prog("xmipp_reconstruct_fourier", ["-i", "keep/angles_iter001_00.xmd", "-o", "sep.vol", "--sym", "c1", "--weight", "-v", "0"], tmp)
    assert r.returncode == 0, r.stderr
    sep = xmipp_io.read_volume(str(tmp / "sep.vol")).copy()
    z, y, x = np.mgrid[-16:16, -16:16, -16:16]
    sep[z * z + y * y + x * x > 16 * 16] = 0
    got = xmipp_io.read_volume(str(tmp / "keep" / "volume_iter001_00.vol"))
    assert got.tobytes() == sep.tobytes()
    assert np.count_nonzero(got) > 0 and got[0, 0, 0] == 0
    assert os.path.getsize(str(tmp / "sep.vol")) == os.path.getsize(str(tmp / "keep" / "volume_iter001_00.vol"))


def test_program_with_a_gallery_and_no_reconstruction(program_case):
    tmp, _, _ = program_case
    r = _prog("xmipp_reconstruct_significant", ["-i", "imgs.xmd", "--initgallery", "gal.doc", "--dontReconstruct", "--iter", "4", "--odir", "galrun", "-v", "2"], tmp)
    assert r.returncode == 0, r.stderr
    # -v 2 (:566-572): the correlations and the weights of the iteration as volumes [image][volume][direction]
    ccv, wv = (xmipp_io.read_volume(str(tmp / "galrun" / f"{n}_iter001.vol")) for n in ("cc", "weight"))
    for n in ("cc", "weight"):
        os.remove(str(tmp / "galrun" / f"{n}_iter001.vol"))
    la, ra = xmipp_io.read_xmd(str(tmp / "galrun" / "angles_iter001_00.xmd"))
    ngal = len(xmipp_io.read_xmd(str(tmp / "gal.doc"))[1])
    assert ccv.shape == wv.shape == (24, 1, ngal)
    at = {(int(x[la.index("imageIndex")]), int(x[la.index("ref")])): x for x in ra}
    assert {(int(n), int(g)) for n, _, g in zip(*np.nonzero(wv > 0))} == set(at)
    for (n, g), x in at.items():
        assert abs(ccv[n, 0, g] - float(x[la.index("maxCC")])) <= 1e-6 and abs(wv[n, 0, g] - float(x[la.index("weight")])) <= 1e-6
    # no volume; and without --keepIntermediateVolumes iteration 1 deletes iteration 0's files (:557-563), angles_iter000 among them
    assert _files(tmp / "galrun") == ["angles_iter001_00.xmd", "images_iter001_00.xmd", "images_significant_iter001_00.xmd"]
    assert os.path.exists(str(tmp / "gal.doc")) and os.path.exists(str(tmp / "gal.stk"))       # a gallery that was given is not deleted
    # the same gallery as the first iteration of the other runs, projection for projection: the same rows, but for the gallery's path
    a, b = xmipp_io.read_xmd(str(tmp / "galrun" / "angles_iter001_00.xmd")), xmipp_io.read_xmd(str(tmp / "keep" / "angles_iter001_00.xmd"))
    assert a == b
