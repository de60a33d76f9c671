"""Timing of xmipp_volume_local_sharpening's device side (xh_ldb_*, LocalDeblur) on the synthetic volume of tests/local_sharpening_ref.py
at size^3, sampling 1, with a resolution map that reaches 10 A: ms per localfiltering call and per iteration, seconds of a full run (after
a warm-up run) with its band and iteration counts, and with per-stage events the split of a localfiltering call into forward transform,
split, the y and z line passes, the row pass and finishing, each next to the time its HBM bytes take at 8 TB/s (the bound of a stage that
only moves data; the bytes count the kept lines and columns only). The kept-line fraction of the y and z passes is listed per band.
batch = 1 (one pair of bands at a time) is the baseline. Prints one JSON line per (size, batch); --out writes them to a file."""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

HBM = 8e12


def stage_bytes(n, bands, nbuf):
    """HBM bytes of one localfiltering call's stages, each array read or written once per kernel that touches it"""
    N, xh = n ** 3, n // 2 + 1
    NF = n * n * xh
    c, d = 16, 8
    nbatch = (len(bands) + nbuf - 1) // nbuf
    cols = sum(b["jcount"] for b in bands) * n * n                       # spectrum elements of the kept columns, all bands
    ylines = sum(b["kcount"] * b["jcount"] for b in bands) * n
    zlines = sum(b["jcount"] for b in bands) * n * n
    return {
        "forward": (N * d + NF * c) + 4 * NF * c,                        # r2c rows, y and z passes
        "split": nbatch * NF * c + cols * c,                             # the spectrum read once per batch (at most), the kept columns written
        "yz": 2 * (ylines + zlines) * c,                                 # each kept line read and written
        "rows": cols * c + nbatch * N * d + (2 * nbatch - 1) * N * d,    # kept columns, the map's rows, the accumulator
        "finish": 3 * N * d,
    }


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", type=int, nargs="+", default=[128, 256])
    ap.add_argument("--batches", type=int, nargs="+", default=[1, 8])
    ap.add_argument("--niter", type=int, default=50)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import torch
    import __graft_entry__ as g
    g.build()
    import xmipp3_amd as xa
    from tests import local_sharpening_ref as R
    ctx = xa.Context(0)
    lines = []
    for n in a.sizes:
        shape = (n, n, n)
        v, rm = R.synth(shape, 1)
        rm = np.where(rm > 0, 3 + (rm - 3) * 7 / 4, 0.0)                 # 3 + 7 r / R: reaches 10 A
        dv, dr = torch.from_numpy(v).cuda(), torch.from_numpy(rm).cuda()
        for batch in a.batches:
            m = xa.LocalDeblur(ctx, shape, batch=batch)
            m.load(dv, dr, 1.0, 0.025)
            info = m.info()
            bands = info["bands"]

            def timed(f, reps):
                f()
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                for _ in range(reps):
                    r = f()
                torch.cuda.synchronize()
                return (time.perf_counter() - t0) / reps, r
            t_lf, _ = timed(lambda: m.localfilter(dv), 5)
            t_run, (_, lam, its) = timed(lambda: m.run(1.0, a.niter), 1)
            m.set_timing(True)
            m.localfilter(dv)
            ms = m.stage_ms()
            m.set_timing(False)
            nbuf = (batch + 1) // 2 * 2
            by = stage_bytes(n, bands, nbuf)
            xh = n // 2 + 1
            line = {"bench": "volume_local_sharpening", "size": n, "batch": batch, "bands": len(bands), "max_res": round(info["maxRes"], 3),
                    "localfilter_ms": round(t_lf * 1e3, 3), "iterations": len(its), "stopped": bool(its[-1]["stop"]), "lambda": round(lam, 4),
                    "run_s": round(t_run, 4), "ms_per_iteration": round(t_run * 1e3 / len(its), 3),
                    "stage_ms_per_localfilter": {k: round(x, 4) for k, x in ms.items()},
                    "stage_hbm_bound_ms": {k: round(by[k] / HBM * 1e3, 4) for k in ms},
                    "kept_y_lines": [round(b["kcount"] * b["jcount"] / (n * xh), 4) for b in bands],
                    "kept_z_lines": [round(b["jcount"] / xh, 4) for b in bands],
                    "band_res": [round(b["res"], 1) for b in bands], "library": os.path.basename(xa.lib_path())}
            print(json.dumps(line), flush=True)
            lines.append(line)
            m.close()
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            for l in lines:
                f.write(json.dumps(l) + "\n")


if __name__ == "__main__":
    main()
