"""Timing of xmipp_transform_symmetrize's device side (xh_sym_*, Symmetrize) on the phantom of tests/symmetrize_ref.py:
 - a volume at 128^3 and 256^3 through c5, d7, o and i1, with spline 1 and 3 and with wrap on and off: ms per volume (median of five runs
   after a warm-up, with the smallest and the largest), the stage times by events (coefficients, outside mean, the pass), (voxel, matrix)
   pairs per second, next to the pass's HBM byte bound (the source read once, the output written once, at 8 TB/s) and its fp64 flop bound
   (per pair and tap one multiply-add for the row sum, the weights' ~40 operations per axis; at 78.6 TFLOP/s vector fp64);
 - the helix at 128^3 for two pitches, with and without the dihedral: trilinear samples per second;
 - a stack of 1024 images of 128 x 128, order 6.
The reference cannot be built here: its time is not measured, no speed-up is claimed and no rate is a condition.
Prints one JSON line per case; --out writes them to a file."""
import argparse
import json
import math
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

HBM = 8e12
FP64 = 78.6e12


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", type=int, nargs="+", default=[128, 256])
    ap.add_argument("--groups", nargs="+", default=["c5", "d7", "o", "i1"])
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import numpy as np
    import torch
    import __graft_entry__ as g
    g.build()
    import xmipp3_amd as xa
    from tests import symmetrize_ref as R
    ctx = xa.Context(0)
    lines = []

    def wall(f):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        f()
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e3

    def five(f):
        f()
        t = sorted(wall(f) for _ in range(5))
        return {"median": round(statistics.median(t), 4), "min": round(t[0], 4), "max": round(t[-1], 4)}

    def emit(line):
        line["reference_speedup"] = "not measured"
        line["library"] = os.path.basename(xa.lib_path())
        print(json.dumps(line), flush=True)
        lines.append(line)

    for D in a.sizes:
        shape = (D, D, D)
        v = torch.from_numpy(R.phantom(shape, 1)).cuda()
        h = xa.Symmetrize(ctx, shape)
        N = D ** 3
        for sym in a.groups:
            mats = R.group_matrices(sym)
            h.set_matrices(mats)
            for degree in (1, 3):
                for wrap in (True, False):
                    ms = five(lambda: h.symmetrize(v, degree, wrap, False))
                    h.set_timing(True)
                    h.symmetrize(v, degree, wrap, False)
                    st = h.stage_ms()
                    h.set_timing(False)
                    pairs = N * len(mats)
                    taps = 8 if degree == 1 else 64
                    flops = pairs * (2 * taps + 3 * 40 + 18)
                    emit({"bench": "symmetrize", "shape": list(shape), "sym": sym, "matrices": len(mats), "spline": degree, "wrap": wrap, "ms_per_volume": ms,
                          "stage_ms": {k: round(t, 4) for k, t in st.items()}, "pairs_per_s": round(pairs / (st["pass"] * 1e-3), 1),
                          "pass_hbm_bound_ms": round(2 * 8 * N / HBM * 1e3, 4), "pass_fp64_bound_ms": round(flops / FP64 * 1e3, 4)})
        if D == 128:
            for zh, rot in ((5.0, 27.0), (7.31 / 1.7, -41.5)):
                for dihedral in (False, True):
                    cn = 3
                    ms = five(lambda: h.helical(v, zh, math.radians(rot), 0.0, cn, dihedral, 0.95, 3))
                    h.set_timing(True)
                    h.helical(v, zh, math.radians(rot), 0.0, cn, dihedral, 0.95, 3)
                    st = h.stage_ms()
                    h.set_timing(False)
                    # every voxel has about 0.95 Z / zHelical terms in range, each Cn samples, twice with the dihedral
                    samples = N * (0.95 * D / zh) * cn * (2 if dihedral else 1)
                    emit({"bench": "symmetrize_helix", "shape": list(shape), "zHelical": round(zh, 4), "Cn": cn, "dihedral": dihedral, "ms_per_volume": ms,
                          "stage_ms": {k: round(t, 4) for k, t in st.items()}, "samples_per_s": round(samples / (ms["median"] * 1e-3), 1)})
        h.close()
    n, D, order = 1024, 128, 6
    imgs = torch.from_numpy(np.tile(R.phantom((D, D), 2), (n, 1, 1))).cuda()
    h = xa.Symmetrize(ctx, (1, D, D))
    for degree in (1, 3):
        for wrap in (True, False):
            ms = five(lambda: h.symmetrize_images(imgs, order, degree, wrap, False))
            emit({"bench": "symmetrize_stack", "images": n, "D": D, "order": order, "spline": degree, "wrap": wrap, "ms_per_stack": ms,
                  "images_per_s": round(n / (ms["median"] * 1e-3), 1)})
    h.close()
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            for l in lines:
                f.write(json.dumps(l) + "\n")


if __name__ == "__main__":
    main()
