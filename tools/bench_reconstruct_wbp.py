"""Timing of xmipp_reconstruct_wbp's device side (xh_wbp_*, ReconstructWbp) on random images with fractional shifts and random directions:
 - images per second at D = 64, 128 and 256 against the batch capacity (1 is the baseline: one image per launch of every kernel), for
   direction lists of 100, 1 000 and 10 000 entries;
 - the stage times by events (prepare, both transforms, filter, back-projection) per image, next to each stage's HBM byte bound at 8 TB/s
   and its fp64 issue bound at 39.3e12 instructions/s (78.6 TFLOP/s vector fp64 counts a fused multiply-add as two; these kernels are
   built without contraction). Filter: D (D / 2 + 1) no_mats look-ups per image, about 10 fp64 instructions each (argum 3, the quotient
   and its test 4, the product and the sum 2, conversions 1), and 8 bytes each if every look-up of the table missed every cache (the
   table is 80 000 D bytes: it does not). Back-projection: the volume read and written once per batch plus the images, and about 30 fp64
   instructions per voxel of the sphere and image, plus one dependent add per voxel of the row before a thread's segment of 16 voxels
   ((D - 16) / 2 on average per thread, so (D - 16) / 32 per voxel). Transforms:
   two passes forward and two back over 16 D^2 bytes, read and written. Prepare: the image, its coefficients twice, the output;
 - the filter's look-ups per second;
 - one full run of 5 000 images of 128 pixels under --use_each_image (5 000 directions) in seconds, capacity 64.
Every rate is the median of three windows of at least --window seconds after a warm-up. The reference cannot be built here: its time is
not measured, no speed-up is claimed and no rate is a condition. Prints one JSON line per case; --out writes them to a file."""
import argparse
import json
import math
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

HBM = 8e12
FP64_INSTR = 78.6e12 / 2
FILTER_OPS = 10
BACKPROJECT_OPS = 30
SEG = 16


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", type=int, nargs="+", default=[64, 128, 256])
    ap.add_argument("--capacities", type=int, nargs="+", default=[1, 64])
    ap.add_argument("--no_mats", type=int, nargs="+", default=[100, 1000, 10000])
    ap.add_argument("--full", type=int, default=5000, help="images of the full run at 128 pixels (0: none)")
    ap.add_argument("--window", type=float, default=0.3)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import numpy as np
    import xmipp3_amd as xa
    ctx = xa.Context(0)
    lines = []
    rng = np.random.default_rng(3)

    def emit(line):
        line["reference_speedup"] = "not measured"
        line["library"] = os.path.basename(xa.lib_path())
        print(json.dumps(line), flush=True)
        lines.append(line)

    def population(D, n):
        images = rng.standard_normal((n, D, D)).astype(np.float32)
        angles = np.stack([rng.uniform(0, 360, n), rng.uniform(0, 180, n), rng.uniform(0, 360, n)], axis=1)
        rows = np.zeros((n, 22))
        g = np.zeros((n, 4))
        for k, (rot, tilt, psi) in enumerate(angles):
            d, F, B = xa.wbp_image_matrices(rot, tilt, psi)
            rows[k, 0:2] = rng.uniform(-3, 3, 2)
            rows[k, 3] = 1.0
            rows[k, 4:13], rows[k, 13:22] = F.reshape(9), B.reshape(9)
            g[k, :3], g[k, 3] = d, 1.0
        return images, rows, g

    def windows(f, per_call):
        f()
        rates = []
        for _ in range(3):
            n, t0 = 0, time.perf_counter()
            while True:
                f()
                n += per_call
                dt = time.perf_counter() - t0
                if dt >= a.window:
                    break
            rates.append(n / dt)
        return statistics.median(rates), min(rates), max(rates)

    for D in a.sizes:
        DD = D * D
        sphere = math.pi / 6 * D ** 3
        for nm in a.no_mats:
            v = rng.standard_normal((nm, 3))
            v /= np.linalg.norm(v, axis=1)[:, None]
            g = np.concatenate([v, np.ones((nm, 1))], axis=1)
            lookups = D * (D // 2 + 1) * nm
            base = None
            for cap in a.capacities:
                m = 64 if cap > 1 else 8
                images, rows, _ = population(D, m)
                w = xa.ReconstructWbp(ctx, D, cap)
                w.set_directions(g, 0.005 * nm, D)
                rate, lo, hi = windows(lambda: w.add(images, rows), m)
                w.set_timing(True)
                w.add(images, rows)
                st = w.stage_ms()
                w.close()
                base = base or rate
                batch = min(cap, m)
                us = {k: round(t / m * 1e3, 3) for k, t in st.items() if k != "finish"}
                emit({"bench": "reconstruct_wbp_add", "D": D, "no_mats": nm, "capacity": cap, "images_per_call": m, "images_per_s": round(rate, 1),
                      "images_per_s_min_max": [round(lo, 1), round(hi, 1)], "against_capacity_1": round(rate / base, 2), "stage_us_per_image": us,
                      "filter_lookups_per_s": round(lookups / (st["filter"] / m * 1e-3), 0) if st["filter"] > 0 else None,
                      "bounds_us_per_image": {
                          "prepare_hbm": round((4 + 8 * 3 + 16) * DD / HBM * 1e6, 3),
                          "transforms_hbm": round(4 * 2 * 16 * DD / HBM * 1e6, 3),
                          "filter_hbm_if_every_lookup_missed": round(lookups * 8 / HBM * 1e6, 3),
                          "filter_fp64_issue": round(lookups * FILTER_OPS / FP64_INSTR * 1e6, 3),
                          "backprojection_hbm": round((16 * D ** 3 / batch + 8 * DD) / HBM * 1e6, 3),
                          "backprojection_fp64_issue": round(sphere * (BACKPROJECT_OPS + max(0, D - SEG) / 2 / SEG) / FP64_INSTR * 1e6, 3)}})
    if a.full:
        D, n = 128, a.full
        images, rows, g = population(D, n)
        w = xa.ReconstructWbp(ctx, D, 64)
        w.set_directions(g, 0.005 * n, D)
        w.add(images[:64], rows[:64])
        t = []
        for _ in range(2):
            w.reset()
            t0 = time.perf_counter()
            w.add(images, rows)
            w.finish()
            vol = w.volume()
            ctx.sync()
            t.append(time.perf_counter() - t0)
        emit({"bench": "reconstruct_wbp_full", "D": D, "images": n, "no_mats": n, "capacity": 64, "seconds": round(statistics.median(t), 3),
              "seconds_min_max": [round(min(t), 3), round(max(t), 3)], "count_thr": w.count_thr(), "finite": bool(vol.isfinite().all().item())})
        w.close()
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            for l in lines:
                f.write(json.dumps(l) + "\n")


if __name__ == "__main__":
    main()
