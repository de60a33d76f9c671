"""Timing of xmipp_resolution_fso's device side (xh_fso_*, FSO in api.py) on the synthetic pair of tests/fso_ref.py at size^3 with its
mask, 321 directions and a cone of 17 degrees: seconds of a full run (load, cones, host decisions, 3DFSC) after a warm-up run, and with
per-stage events the transforms, the layout (with the global sums), the cones, the segment reduction and the 3DFSC, each next to the time
its HBM bytes take at 8 TB/s (the bound of a stage that only moves data). The cone stage also lists its lane-iteration count,
Ncomps x ceil(ndir / 64) x 64, and the rate that gives. `seg` (the coefficients a workgroup of the cone stage takes) is swept.
--numpy-size times the numpy restatement's cone sums and 3DFSC at that size: for scale only, numpy on one core is not the reference.
Prints one JSON line per (size, seg); --out writes them to a file."""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

HBM = 8e12


def stage_bytes(n, ncomps, nseg, ndir):
    """HBM bytes of the stages, each array read or written once per kernel that touches it"""
    N, xh = n ** 3, n // 2 + 1
    NF, L = n * n * xh, n // 2 + 1
    c, d = 16, 8
    nchunks = -(-NF // 4096)
    return {
        "transforms": 2 * (3 * N * d + (NF * c) + 4 * NF * c),            # mask multiply, r2c rows, y and z passes, per half map
        "layout": 4 * L * nchunks * 4 + 2 * NF * c + 8 * ncomps * 4 + ncomps * (4 + 2 * c),    # counts, the spectra once, the layout, the sums' gather
        "cones": 6 * ncomps * 4 + nseg * ndir * 28,                      # the layout's six float arrays once, the partials
        "segment_reduce": nseg * ndir * 28 + L * ndir * 32,
        "threedfsc": 5 * ncomps * 4 + NF * d * 2 + ncomps * d + NF * d + N * d,
    }


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", type=int, nargs="+", default=[128, 256, 384])
    ap.add_argument("--segs", type=int, nargs="+", default=[256, 512, 1024, 2048])
    ap.add_argument("--numpy-size", type=int, default=128)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import torch
    import __graft_entry__ as g
    g.build()
    import xmipp3_amd as xa
    from tests import fso_ref as R
    ctx = xa.Context(0)
    ang = xa.fso_directions(3)
    dirs = xa.fso_unit_vectors(ang)
    cosA, aux = xa.fso_cone(17.0)
    ndir = len(dirs)
    lines = []
    for n in a.sizes:
        shape = (n, n, n)
        need = 2 * n * n * (n // 2 + 1) * 16 + 6 * n ** 3 * 8
        free = torch.cuda.mem_get_info()[0]
        if need > 0.5 * free:
            print(json.dumps({"bench": "resolution_fso", "size": n, "skipped": f"needs {need >> 20} MiB, {free >> 20} MiB free"}), flush=True)
            continue
        h1, h2, m = (torch.from_numpy(v).cuda() for v in R.synth(shape, 1))
        for seg in a.segs:
            f = xa.FSO(ctx, shape, seg=seg)

            def timed(fn, reps):
                fn()
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                for _ in range(reps):
                    r = fn()
                torch.cuda.synchronize()
                return (time.perf_counter() - t0) / reps, r
            t_run, out = timed(lambda: f.run(h1, h2, m, threedfsc=True, distribution=False), 2)
            t_cones, _ = timed(lambda: f.directional(dirs, cosA, aux), 5)
            f.set_timing(True)
            f.run(h1, h2, m, threedfsc=True, distribution=False)
            ms = f.stage_ms()
            f.set_timing(False)
            info = f.info()
            by = stage_bytes(n, info["ncomps"], info["nseg"], ndir)
            lane_iter = info["ncomps"] * (-(-ndir // 64)) * 64
            line = {"bench": "resolution_fso", "size": n, "seg": info["seg"], "directions": ndir, "ncomps": info["ncomps"], "segments": info["nseg"],
                    "run_s": round(t_run, 4), "directional_call_ms": round(t_cones * 1e3, 3),
                    "stage_ms": {k: round(x, 4) for k, x in ms.items()}, "stage_hbm_bound_ms": {k: round(by[k] / HBM * 1e3, 4) for k in ms},
                    "cone_lane_iterations": lane_iter, "cone_lane_iterations_per_ns": round(lane_iter / (ms["cones"] * 1e6), 2),
                    "in_cone_pairs": int(out["counts"].sum()), "library": os.path.basename(xa.lib_path())}
            print(json.dumps(line), flush=True)
            lines.append(line)
            f.close()
        del h1, h2, m
    if a.numpy_size:
        n = a.numpy_size
        shape = (n, n, n)
        h1, h2, m = R.synth(shape, 1)
        lay = R.layout(shape, *R.spectra(h1, h2, m))
        rc, raux = R.cone(17.0)
        t0 = time.perf_counter()
        ds, _ = R.cone_sums(lay, dirs, rc, raux)
        t1 = time.perf_counter()
        R.threedfsc(shape, lay, dirs, rc, raux, R.dir_fsc(ds))
        t2 = time.perf_counter()
        line = {"bench": "resolution_fso", "size": n, "numpy_restatement_one_core": True, "cone_sums_s": round(t1 - t0, 2), "threedfsc_s": round(t2 - t1, 2)}
        print(json.dumps(line), flush=True)
        lines.append(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            for l in lines:
                f.write(json.dumps(l) + "\n")


if __name__ == "__main__":
    main()
