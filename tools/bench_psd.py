"""Timing of the PSD stage's device side (xh_psd_*, PsdEstimator) on random micrographs:
 - pieces per second and micrographs per second for micrographs of 4096 x 4096 and 4092 x 5760 (K3) with pieces of 256, 384 and 512 at
   overlap 0.5 and skipBorders 2 (the defaults of xmipp_ctf_estimate_from_micrograph), in double, against the batch capacity (1 is the
   baseline: one piece per launch of every kernel), and in float (xmipp_psd_estimate's patches at overlap 0.4) at capacity 64;
 - the stage times by events (statistics, rows, columns + accumulate, finish) per piece, next to each stage's HBM byte bound at 8 TB/s:
   statistics read the window once per pass (4 P^2 bytes, three passes in double, one in float) if no pass hit a cache, rows read it once
   more and write the half spectrum (2 e P (P / 2 + 1), e the element size), columns read the half spectrum, and per batch the sums;
 - a resident micrograph (load once, add many times) against one streamed from page-locked host memory and from pageable memory (load +
   add per micrograph), which settles whether the program is bound by reading the micrograph over the host link or by the kernels.
Every rate is the median of three windows of at least --window seconds after a warm-up. The reference cannot be built here: its time is
not measured, no speed-up is claimed and no rate is a condition. Prints one JSON line per case; --out writes them to a file."""
import argparse
import json
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

HBM = 8e12


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", type=int, nargs="+", default=[4096, 4096, 4092, 5760], help="rows columns, pairs")
    ap.add_argument("--pieces", type=int, nargs="+", default=[256, 384, 512])
    ap.add_argument("--capacities", type=int, nargs="+", default=[1, 8, 64])
    ap.add_argument("--window", type=float, default=0.3)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import numpy as np
    import torch
    import xmipp3_amd as xa
    ctx = xa.Context(0)
    lines = []
    rng = np.random.default_rng(3)

    def emit(line):
        line["reference_speedup"] = "not measured"
        line["library"] = os.path.basename(xa.lib_path())
        print(json.dumps(line), flush=True)
        lines.append(line)

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

    for Y, X in zip(a.shapes[0::2], a.shapes[1::2]):
        mic = (1000 + 5 * rng.standard_normal((Y, X))).astype(np.float32)
        pinned = torch.from_numpy(mic).pin_memory()
        for P in a.pieces:
            hx = P // 2 + 1
            for dtype, name in ((np.float64, "double"), (np.float32, "float")):
                e = 8 if dtype == np.float64 else 4
                if dtype == np.float64:
                    corners, _, _ = xa.psd_pieces(Y, X, P, 0.5, 2, "micrograph")
                else:
                    corners = xa.psd_patches(Y, X, P, P, 0, 0, 0.4)
                n = len(corners)
                base = None
                for cap in (a.capacities if dtype == np.float64 else a.capacities[-1:]):
                    est = xa.PsdEstimator(ctx, Y, X, P, P, cap, dtype)
                    est.load(mic)
                    rate, lo, hi = windows(lambda: est.add(corners), n)
                    est.set_timing(True)
                    est.reset()
                    est.add(corners)
                    est.result()
                    st = est.stage_ms()
                    est.set_timing(False)
                    base = base or rate
                    line = {"bench": "psd_add", "Y": Y, "X": X, "piece": P, "type": name, "capacity": cap, "pieces": n, "pieces_per_s": round(rate, 1),
                            "pieces_per_s_min_max": [round(lo, 1), round(hi, 1)], "micrographs_per_s_resident": round(rate / n, 2),
                            "against_capacity_1": round(rate / base, 2),
                            "stage_us_per_piece": {k: round(t / n * 1e3, 3) for k, t in st.items() if k != "finish"}, "finish_us": round(st["finish"] * 1e3, 3),
                            "bounds_us_per_piece": {"statistics_hbm": round((3 if dtype == np.float64 else 1) * 4 * P * P / HBM * 1e6, 4),
                                                    "rows_hbm": round((4 * P * P + 2 * e * P * hx) / HBM * 1e6, 4),
                                                    "columns_hbm": round((2 * e * P * hx + 4 * e * P * hx / min(cap, n)) / HBM * 1e6, 4)}}
                    if cap == a.capacities[-1]:
                        def streamed(src):
                            est.reset()
                            est.load(src)
                            est.add(corners)
                            est.result()
                        for src, key in ((pinned, "page_locked"), (mic, "pageable")):
                            r, _, _ = windows(lambda: streamed(src), 1)
                            line[f"micrographs_per_s_streamed_{key}"] = round(r, 2)
                        t0 = time.perf_counter()
                        for _ in range(5):
                            est.load(pinned)
                        line["load_page_locked_GB_per_s"] = round(5 * mic.nbytes / (time.perf_counter() - t0) / 1e9, 2)
                    emit(line)
                    est.close()
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            for l in lines:
                f.write(json.dumps(l) + "\n")


if __name__ == "__main__":
    main()
