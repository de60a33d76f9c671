"""GPU tests of xmipp_align_significant: the many-to-many alignment (xh_align_sig_align) pair for pair against the one-reference chain
and the oracle's restatement of it, the significance weights and the reference update against numpy restatements of
computeWeightsAndSave and updateRefs, and the program end to end against the same chain through the Python binding."""
import os
import subprocess

import numpy as np
import pytest

from tests import xmipp_io

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PROG = os.path.join(ROOT, "xmipp3_amd", "bin", "xmipp_align_significant")


@pytest.fixture(scope="module")
def gpu():
    import torch
    import __graft_entry__ as g
    g.build()
    import xmipp3_amd as xa
    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    return xa, xa.Context(0), torch


def _arm(D):
    c = D // 2
    arm = int((D - c) / 1.5)
    ref = np.zeros((D, D), np.float32)
    ref[c:c + arm, c] = 1
    ref[c, c:c + arm] = 1
    return ref


def _population(oracle, D, R, N, seed):
    """R references (the clock arm rotated), N images (the arm shifted and rotated by oracle.es_test_make_others)"""
    rng = np.random.default_rng(seed)
    refs = oracle.es_test_make_others(_arm(D), np.zeros((R, 2), np.float32), (np.arange(R) * 360.0 / R + 7).astype(np.float32))
    sh = rng.uniform(-D / 10, D / 10, (N, 2)).astype(np.float32)
    rot = rng.uniform(0, 360, N).astype(np.float32)
    return refs, oracle.es_test_make_others(_arm(D), sh, rot)


def _inv(m):
    """M3x3_INV of float matrices [..., 3, 3]: float cofactors, the reciprocal of the determinant in double, stored as floats"""
    m = np.asarray(m, np.float32)
    a = lambda i, j: m[..., i, j]
    o = np.stack([a(2, 2) * a(1, 1) - a(2, 1) * a(1, 2), -(a(2, 2) * a(0, 1) - a(2, 1) * a(0, 2)), a(1, 2) * a(0, 1) - a(1, 1) * a(0, 2),
                  -(a(2, 2) * a(1, 0) - a(2, 0) * a(1, 2)), a(2, 2) * a(0, 0) - a(2, 0) * a(0, 2), -(a(1, 2) * a(0, 0) - a(1, 0) * a(0, 2)),
                  a(2, 1) * a(1, 0) - a(2, 0) * a(1, 1), -(a(2, 1) * a(0, 0) - a(2, 0) * a(0, 1)), a(1, 1) * a(0, 0) - a(1, 0) * a(0, 1)], -1).astype(np.float32)
    det = (a(0, 0) * o[..., 0] + a(1, 0) * o[..., 1] + a(2, 0) * o[..., 2]).astype(np.float32)
    return (o.astype(np.float64) * (1.0 / det.astype(np.float64))[..., None]).astype(np.float32).reshape(m.shape)


@pytest.mark.parametrize("D", [64, 128])
def test_alignment_pair_for_pair(gpu, oracle, D):
    xa, ctx, torch = gpu
    R, N = 5, 37
    refs, imgs = _population(oracle, D, R, N, D)
    al = xa.AlignSignificant(ctx, D, R, batch_pairs=16)          # 185 pairs: the last batch is partial
    al.load_references(torch.from_numpy(refs).cuda())
    poses, merit = al.align(torch.from_numpy(imgs).cuda())
    poses, merit = poses.cpu().numpy(), merit.cpu().numpy()
    assert poses.shape == (R, N, 3, 3) and merit.shape == (R, N)
    dimgs = torch.from_numpy(imgs).cuda()
    for r in range(R):
        p1, m1 = xa.iterative_alignment(ctx, torch.from_numpy(refs[r]).cuda(), dimgs, D // 4, 3)
        np.testing.assert_allclose(poses[r], p1, rtol=0, atol=1e-5)
        np.testing.assert_allclose(merit[r], m1, rtol=0, atol=1e-6)
        ep, em = oracle.es_iterative_alignment(refs[r], imgs, D // 4, 3)
        for i in range(N):
            if np.allclose(poses[r, i], ep[i], rtol=0, atol=1e-5):
                assert abs(merit[r, i] - em[i]) <= 1e-4, (r, i)
            else:                            # a shift step met an arg-max tie
                reach = oracle.es_iterative_reachable(refs[r], imgs[i], D // 4, 3)
                assert any(t > 0 and np.allclose(poses[r, i], p_, rtol=0, atol=1e-5) and abs(merit[r, i] - m_) <= 1e-4 for p_, m_, t in reach), (r, i)


def _directions(rot, tilt):
    a, b = np.radians(np.asarray(rot, np.float64)), np.radians(np.asarray(tilt, np.float64))
    return np.stack([np.sin(b) * np.cos(a), np.sin(b) * np.sin(a), np.cos(b)], -1)


def weights_numpy(merit, rot, tilt, ang):
    """computeWeightsAndSave (aalign_significant.cpp:233-311), ties ranked by (reference, image) index"""
    R, N = merit.shape
    d = _directions(rot, tilt)
    angle = np.degrees(np.arccos(np.clip(d @ d.T, -1, 1)))
    out = np.zeros((R, N), np.float32)
    for r in range(R):
        sel = [q for q in range(R) if q == r or angle[r, q] <= ang]
        vals = np.concatenate([merit[q] for q in sel])
        order = np.argsort(vals, kind="stable")
        rank = np.empty(len(vals), np.int64)
        rank[order] = np.arange(len(vals))
        at = sel.index(r) * N
        inv = np.float32(1) / np.float32(vals.max())
        for s in range(N):
            m = np.float32(merit[r, s])
            cdf = np.float32(rank[at + s]) / np.float32(len(vals) - 1)
            out[r, s] = m * inv * cdf if m > 0 else 0
    return out


@pytest.mark.parametrize("ang", [0.0, 20.0, 60.0, 180.0])
def test_weights(gpu, ang):
    xa, ctx, torch = gpu
    rng = np.random.default_rng(3)
    R, N = 9, 300
    merit = rng.uniform(0.05, 1.0, (R, N)).astype(np.float32)
    rot = np.linspace(0, 80, R).astype(np.float32)
    tilt = np.linspace(0, 50, R).astype(np.float32)
    al = xa.AlignSignificant(ctx, 32, 2)
    got = al.weights(rot, tilt, ang, torch.from_numpy(merit).cuda()).cpu().numpy()
    exp = weights_numpy(merit, rot, tilt, ang)
    np.testing.assert_allclose(got, exp, rtol=1e-6, atol=0)
    if ang == 0.0:                           # only r itself: the rank is within the reference's own merits
        assert np.allclose(got.max(1), 1.0, atol=1e-6)


def test_weights_of_non_positive_merits_are_zero(gpu):
    xa, ctx, torch = gpu
    rng = np.random.default_rng(4)
    merit = rng.uniform(-1, 1, (4, 50)).astype(np.float32)
    merit[1, 7] = 0
    al = xa.AlignSignificant(ctx, 32, 2)
    got = al.weights(np.zeros(4, np.float32), np.zeros(4, np.float32), 10, torch.from_numpy(merit).cuda()).cpu().numpy()
    assert np.all(got[merit <= 0] == 0)
    np.testing.assert_allclose(got, weights_numpy(merit, np.zeros(4), np.zeros(4), 10), rtol=1e-6, atol=0)


def test_weight_of_a_lone_merit_is_zero(gpu):
    """one image and a reference that selects only itself: count N - 1 = 0 (the reference program writes NaN), the weight is 0"""
    xa, ctx, torch = gpu
    merit = np.array([[0.5], [0.7], [0.2]], np.float32)
    al = xa.AlignSignificant(ctx, 32, 2)
    got = al.weights(np.array([0, 90, 180], np.float32), np.array([0, 90, 90], np.float32), 0.0, torch.from_numpy(merit).cuda()).cpu().numpy()
    assert np.array_equal(got, np.zeros((3, 1), np.float32))


def test_more_images_than_the_handle_has_references(gpu, oracle):
    """the handle is sized by the references it loads; the images are any number, and the reference update takes its count"""
    xa, ctx, torch = gpu
    D, R, N = 32, 2, 300
    refs, imgs = _population(oracle, D, R, N, 21)
    al = xa.AlignSignificant(ctx, D, R)
    al.load_references(torch.from_numpy(refs).cuda())
    dimgs = torch.from_numpy(imgs).cuda()
    poses, merit = al.align(dimgs)
    for r in range(R):
        p1, m1 = xa.iterative_alignment(ctx, torch.from_numpy(refs[r]).cuda(), dimgs, D // 4, 3)
        np.testing.assert_allclose(poses[r].cpu().numpy(), p1, rtol=0, atol=1e-5)
        np.testing.assert_allclose(merit[r].cpu().numpy(), m1, rtol=0, atol=1e-6)
    # seven references updated through a handle that holds two
    rng = np.random.default_rng(8)
    k = 40
    ref_idx, img_idx = rng.integers(0, 7, k), rng.integers(0, N, k)
    weight = rng.uniform(0.1, 1, k).astype(np.float32)
    pose = np.tile(np.eye(3, dtype=np.float32), (k, 1, 1))
    pose[:, :2, 2] = rng.integers(-3, 4, (k, 2))
    got = al.update_refs(dimgs, ref_idx, img_idx, weight, pose, n_refs=7).cpu().numpy()
    exp = update_refs_numpy(oracle, imgs, 7, ref_idx, img_idx, weight, pose)
    assert got.shape == (7, D, D) and np.abs(got - exp).max() <= 1e-5 * np.abs(exp).max()


def update_refs_numpy(oracle, imgs, R, ref_idx, img_idx, weight, pose):
    """updateRefs: the weighted sum of the assigned images through the inverse pose, divided by the running sum of the weights of
    references 0 .. r; zeros where that sum is 0"""
    D = imgs.shape[-1]
    out = np.zeros((R, D, D))
    norm = 0.0
    for r in range(R):
        ks = [k for k in range(len(ref_idx)) if ref_idx[k] == r]
        for k in ks:
            out[r] += weight[k] * oracle.apply_geometry2d(imgs[img_idx[k]], _inv(pose[k]), 1, True, False)
        norm += sum(weight[k] for k in ks)
        out[r] = out[r] / norm if norm != 0 else 0
    return out


@pytest.mark.parametrize("empty", [None, 0, 2])
def test_update_refs(gpu, oracle, empty):
    xa, ctx, torch = gpu
    D, R, N = 32, 4, 11
    rng = np.random.default_rng(5)
    imgs = rng.standard_normal((N, D, D)).astype(np.float32)
    ref_idx = rng.integers(0, R, 20)
    if empty is not None:
        ref_idx[ref_idx == empty] = (empty + 1) % R
    img_idx = rng.integers(0, N, 20)
    weight = rng.uniform(0.1, 1, 20).astype(np.float32)
    ang = np.radians(rng.uniform(0, 360, 20))
    pose = np.zeros((20, 3, 3), np.float32)
    pose[:, 0, 0] = pose[:, 1, 1] = np.cos(ang)
    pose[:, 0, 1], pose[:, 1, 0] = np.sin(ang), -np.sin(ang)
    pose[:, :2, 2] = rng.uniform(-4, 4, (20, 2))
    pose[:, 2, 2] = 1
    al = xa.AlignSignificant(ctx, D, R)
    al.load_references(torch.zeros((R, D, D), dtype=torch.float32, device="cuda"))
    got = al.update_refs(torch.from_numpy(imgs).cuda(), ref_idx, img_idx, weight, pose).cpu().numpy()
    exp = update_refs_numpy(oracle, imgs, R, ref_idx, img_idx, weight, pose)
    assert np.all(np.isfinite(got))
    assert np.abs(got - exp).max() <= 1e-5 * np.abs(exp).max()
    if empty is not None:
        assert np.all(got[empty] == 0)


# ---- the program end to end


def _run(args, timeout=600):
    return subprocess.run([PROG] + args, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=timeout)


def _write_inputs(tmp, refs, imgs, rot, tilt):
    xmipp_io.write_stack(str(tmp / "refs.stk"), refs)
    xmipp_io.write_stack(str(tmp / "imgs.stk"), imgs)
    xmipp_io.write_xmd(str(tmp / "refs.xmd"), [("noname", ["image", "ref", "angleRot", "angleTilt"],
                                                [[f"{i + 1}@{tmp}/refs.stk", 10 + i, float(rot[i]), float(tilt[i])] for i in range(len(refs))])])
    xmipp_io.write_xmd(str(tmp / "imgs.xmd"), [("noname", ["itemId", "image"], [[100 + i, f"{i + 1}@{tmp}/imgs.stk"] for i in range(len(imgs))])])


def _expected(xa, ctx, torch, refs, imgs, rot, tilt, ang, keep, use_weight, swap):
    """the chain through the binding plus computeAssignment / storeAlignedImages in numpy: rows (ref, psi, shiftX, shiftY, flip, weight,
    maxCC) in output order, and the assignments"""
    D = refs.shape[-1]
    R0, N0 = len(refs), len(imgs)
    transposed = swap and R0 > N0
    a, b = (imgs, refs) if transposed else (refs, imgs)
    al = xa.AlignSignificant(ctx, D, len(a))
    al.load_references(torch.from_numpy(np.ascontiguousarray(a)).cuda())
    poses, merit = al.align(torch.from_numpy(np.ascontiguousarray(b)).cuda())
    poses, merit = poses.cpu().numpy(), merit.cpu().numpy()
    if transposed:
        merit, poses = merit.T.copy(), _inv(poses.transpose(1, 0, 2, 3))
    w = al.weights(rot, tilt, ang, torch.from_numpy(np.ascontiguousarray(merit)).cuda()).cpu().numpy()
    assign = []
    for i in range(N0):
        votes = (w if use_weight else merit)[:, i].copy()
        for _ in range(keep):
            r = int(np.argmax(votes))
            val = votes[r]
            votes[r] = np.finfo(np.float32).min
            if val <= 0:
                continue
            assign.append((r, i, w[r, i], val, poses[r, i]))
    assign.sort(key=lambda t: (t[1], -(t[2] if use_weight else t[3])))
    rows, best = [], {}
    for r, i, wt, val, p in assign:
        best.setdefault(i, val)
        A = _inv(p)
        flip = A[0, 0] * A[1, 1] - A[0, 1] * A[1, 0] < 0
        sg = -1 if flip else 1
        scale = np.hypot(A[0, 0], A[0, 1])
        rows.append((10 + r, np.degrees(np.arctan2(sg * A[0, 1], sg * A[0, 0])), -A[0, 2] / scale, -A[1, 2] / scale, int(flip), wt, best[i], i))
    return rows, assign, al


def _check_rows(path, rows):
    labels, got = xmipp_io.read_xmd(path)
    col = {l: k for k, l in enumerate(labels)}
    assert len(got) == len(rows)
    for g, e in zip(got, rows):
        assert int(g[col["ref"]]) == e[0] and int(g[col["flip"]]) == e[4] and int(g[col["itemId"]]) == 100 + e[7]
        assert int(g[col["imageIndex"]]) == e[7] + 1 and int(g[col["enabled"]]) == 1
        dpsi = (float(g[col["anglePsi"]]) - e[1] + 180) % 360 - 180
        assert abs(dpsi) < 1e-3, (g, e)
        for lab, v in (("shiftX", e[2]), ("shiftY", e[3]), ("weight", e[5]), ("weightSignificant", e[5]), ("maxCC", e[6])):
            assert abs(float(g[col[lab]]) - v) < 2e-5, (lab, g, e)


def _program_case(gpu, oracle, tmp, R, N, D, keep=1, use_weight=False, swap=False, odd=False, update=False):
    xa, ctx, torch = gpu
    refs, imgs = _population(oracle, D, R, N, 11 + R + N)
    rot = np.linspace(0, 40, R).astype(np.float32)
    tilt = np.linspace(0, 30, R).astype(np.float32)
    if odd:         # one more row and column: the program crops them
        pad = lambda x: np.pad(x, ((0, 0), (0, 1), (0, 1)), constant_values=3.0)
        _write_inputs(tmp, pad(refs), pad(imgs), rot, tilt)
    else:
        _write_inputs(tmp, refs, imgs, rot, tilt)
    args = ["-i", str(tmp / "imgs.xmd"), "-r", str(tmp / "refs.xmd"), "-o", "out.xmd", "--odir", str(tmp), "--angDistance", "15",
            "--keepBestN", str(keep)]
    args += ["--useWeightInsteadOfCC"] * use_weight + ["--allowInputSwap"] * swap + ["--oUpdatedRefs", "upd"] * update
    r = _run(args)
    assert r.returncode == 0, r.stderr
    rows, assign, al = _expected(xa, ctx, torch, refs, imgs, rot, tilt, 15, keep, use_weight, swap)
    assert rows
    _check_rows(str(tmp / "out.xmd"), rows)
    if odd:
        assert "Input will be cropped" in r.stderr
    if swap:
        assert "We are swapping reference images" in r.stderr
    return refs, imgs, assign, al


def test_program_rows(gpu, oracle, tmp_path):
    _program_case(gpu, oracle, tmp_path, 4, 9, 32)


def test_program_keep_best_two(gpu, oracle, tmp_path):
    _program_case(gpu, oracle, tmp_path, 4, 9, 32, keep=2)


def test_program_weight_criterion(gpu, oracle, tmp_path):
    _program_case(gpu, oracle, tmp_path, 4, 9, 32, keep=2, use_weight=True)


def test_program_input_swap(gpu, oracle, tmp_path):
    _program_case(gpu, oracle, tmp_path, 7, 3, 32, swap=True)


def test_program_odd_size_is_cropped(gpu, oracle, tmp_path):
    _program_case(gpu, oracle, tmp_path, 4, 6, 32, odd=True)


def test_program_updated_references(gpu, oracle, tmp_path):
    xa, ctx, torch = gpu
    refs, imgs, assign, al = _program_case(gpu, oracle, tmp_path, 5, 8, 32, keep=2, update=True)
    R = len(refs)
    exp = al.update_refs(torch.from_numpy(imgs).cuda(), [a[0] for a in assign], [a[1] for a in assign], [a[2] for a in assign],
                         np.stack([a[4] for a in assign]), n_refs=R).cpu().numpy()
    got = xmipp_io.read_stack(str(tmp_path / "upd.stk"))
    assert got.shape == (R, 32, 32)
    np.testing.assert_allclose(got, exp, rtol=0, atol=1e-6 * max(1.0, np.abs(exp).max()))
    labels, rows = xmipp_io.read_xmd(str(tmp_path / "upd.xmd"), "classes")
    col = {l: k for k, l in enumerate(labels)}
    counts = np.bincount([a[0] for a in assign], minlength=R)
    assert [int(r[col["ref"]]) for r in rows] == [10 + r for r in range(R)]
    assert [int(r[col["classCount"]]) for r in rows] == list(counts)
    assert [r[col["image"]] for r in rows] == [f"{r + 1:06d}@{tmp_path}/upd.stk" for r in range(R)]
    for r in range(R):
        if counts[r] == 0:
            continue
        lb, rr = xmipp_io.read_xmd(str(tmp_path / "upd.xmd"), f"class{10 + r:06d}_images")
        c = {l: k for k, l in enumerate(lb)}
        assert [int(x[c["itemId"]]) for x in rr] == sorted(100 + a[1] for a in assign if a[0] == r)
        assert all(int(x[c["ref"]]) == 10 + r for x in rr)


def test_program_with_more_images_than_a_grid_dimension(gpu, tmp_path):
    """66 000 images (more than 65 535) against two references: the handle holds the references, not the images"""
    xa, ctx, torch = gpu
    D, R, N = 16, 2, 66000
    rng = np.random.default_rng(9)
    refs = rng.standard_normal((R, D, D)).astype(np.float32)
    imgs = (refs[rng.integers(0, R, N)] + 0.5 * rng.standard_normal((N, D, D))).astype(np.float32)
    rot, tilt = np.array([0, 40], np.float32), np.array([0, 30], np.float32)
    _write_inputs(tmp_path, refs, imgs, rot, tilt)
    r = _run(["-i", str(tmp_path / "imgs.xmd"), "-r", str(tmp_path / "refs.xmd"), "-o", "out.xmd", "--odir", str(tmp_path), "--angDistance", "15"])
    assert r.returncode == 0, r.stderr
    rows, _, _ = _expected(xa, ctx, torch, refs, imgs, rot, tilt, 15, 1, False, False)
    assert len(rows) > 60000
    _check_rows(str(tmp_path / "out.xmd"), rows)


def test_program_empty_assignment_writes_empty_metadata(gpu, tmp_path):
    D = 32
    _write_inputs(tmp_path, np.zeros((3, D, D), np.float32), np.zeros((2, D, D), np.float32), np.zeros(3), np.zeros(3))
    r = _run(["-i", str(tmp_path / "imgs.xmd"), "-r", str(tmp_path / "refs.xmd"), "-o", "out.xmd", "--odir", str(tmp_path)])
    assert r.returncode == 0, r.stderr
    labels, rows = xmipp_io.read_xmd(str(tmp_path / "out.xmd"))
    assert rows == []
