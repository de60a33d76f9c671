"""Throughput of the many-to-many alignment of xmipp_align_significant (xh_align_sig_align) against the loop it replaces, one
xa.iterative_alignment call per reference. R references, N images of D px, iters rounds; prints one JSON line with pairs/s of both.
The baseline runs on the first --baseline-refs references only (its rate per pair does not depend on R). weights_all_selected_s times the
significance weights with every reference selected, the worst case of their counting rank."""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--refs", type=int, default=64)
    ap.add_argument("--images", type=int, default=4096)
    ap.add_argument("--size", type=int, default=128)
    ap.add_argument("--iters", type=int, default=3)
    ap.add_argument("--batch", type=int, default=1024)
    ap.add_argument("--baseline-refs", type=int, default=4)
    a = ap.parse_args()
    import torch
    import __graft_entry__ as g
    g.build()
    import xmipp3_amd as xa
    from tests import synth
    D, R, N = a.size, a.refs, a.images
    from scipy import ndimage
    base = synth.phantom(D, seed=1, nblobs=10).sum(0)          # one projection, turned in-plane: R distinct references, quickly
    refs = np.stack([ndimage.rotate(base, 360.0 * r / R, reshape=False, order=1) for r in range(R)]).astype(np.float32)
    imgs, _ = synth.make_particles(refs, N, np.random.default_rng(0), snr=0.5, max_shift=3)
    dref = torch.from_numpy(np.ascontiguousarray(refs, np.float32)).cuda()
    dimg = torch.from_numpy(np.ascontiguousarray(imgs, np.float32)).cuda()
    ctx = xa.Context(0)
    al = xa.AlignSignificant(ctx, D, R, batch_pairs=a.batch, iters=a.iters)
    al.load_references(dref[:1])
    al.align(dimg[:64])                                   # warm-up: code objects, buffers
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    al.load_references(dref)
    poses, merit = al.align(dimg)
    torch.cuda.synchronize()
    t_new = time.perf_counter() - t0
    # the significance weights with every reference selected (angDistance 180): the counting rank's worst case, O(R N^2) per reference
    rot, tilt = np.zeros(R, np.float32), np.zeros(R, np.float32)
    al.weights(rot, tilt, 180.0, merit)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    al.weights(rot, tilt, 180.0, merit)
    torch.cuda.synchronize()
    t_w = time.perf_counter() - t0
    B = min(a.baseline_refs, R)
    xa.iterative_alignment(ctx, dref[0], dimg[:64], D // 4, a.iters)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for r in range(B):
        p1, m1 = xa.iterative_alignment(ctx, dref[r], dimg, D // 4, a.iters)
    torch.cuda.synchronize()
    t_old = time.perf_counter() - t0
    same = bool(np.allclose(poses[B - 1].cpu().numpy(), p1, rtol=0, atol=1e-5) and np.allclose(merit[B - 1].cpu().numpy(), m1, rtol=0, atol=1e-6))
    print(json.dumps({"bench": "align_significant", "refs": R, "images": N, "size": D, "iters": a.iters, "batch_pairs": a.batch,
                      "new_s": round(t_new, 3), "new_pairs_per_s": round(R * N / t_new, 1), "weights_all_selected_s": round(t_w, 4),
                      "baseline_refs": B, "baseline_s": round(t_old, 3), "baseline_pairs_per_s": round(B * N / t_old, 1),
                      "speedup": round((R * N / t_new) / (B * N / t_old), 2), "last_baseline_ref_matches": same}))


if __name__ == "__main__":
    main()
