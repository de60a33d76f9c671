"""Timing of xmipp_volume_align's device side (xh_valign_*, VolumeAlign) on the phantom of tests/symmetrize_ref.py:
 - trials per second and ms per trial at 64^3, 128^3 and 256^3 against the batch capacity (1 is the baseline: one trial per pass over V1),
   at 128^3 for both methods, wrap on and off, masked and not; the other sizes with COVARIANCE, wrap, no mask;
 - next to the fit kernel's HBM byte bound (V1 and the mask once per tile of 8 trials, V2 once per trial by the gather, at 8 TB/s) and its
   fp64 bound (about 60 operations per voxel and trial: 18 for the source point, 36 for the trilinear rule, 6 for the sums; at
   78.6 TFLOP/s vector fp64), with the stage times by events (gather and workgroup sums, finish, choice);
 - a full --rot 0 360 15 --tilt 0 180 15 --psi 0 360 15 search in seconds (8 125 trials: both ends of every range are visited).
Every figure is the median of five windows of at least half a second after a warm-up. The staged-against-gather A/B of the issue is not
here: no staged kernel was built. The reference cannot be built here: its time is not measured, no speed-up is claimed and no rate is a
condition. Prints one JSON line per case; --out writes them to a file."""
import argparse
import json
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

HBM = 8e12
FP64 = 78.6e12
TILE = 8
FLOPS = 60


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", type=int, nargs="+", default=[64, 128, 256])
    ap.add_argument("--capacities", type=int, nargs="+", default=[1, 8, 64])
    ap.add_argument("--full", type=int, nargs="*", default=[64, 128], help="sizes of the full global search")
    ap.add_argument("--window", type=float, default=0.5)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import numpy as np
    import __graft_entry__ as g
    g.build()
    import xmipp3_amd as xa
    from tests import volume_align_ref as R
    ctx = xa.Context(0)
    lines = []
    rng = np.random.default_rng(3)

    def emit(line):
        line["reference_speedup"] = "not measured"
        line["library"] = os.path.basename(xa.lib_path())
        print(json.dumps(line), flush=True)
        lines.append(line)

    def poses(n):
        p = np.zeros((n, 10))
        p[:, 0] = 1
        p[:, 1] = 1
        p[:, 3:6] = rng.uniform(-180, 180, (n, 3))
        p[:, 6] = rng.uniform(0.9, 1.1, n)
        p[:, 7:] = rng.uniform(-3, 3, (n, 3))
        return p

    def windows(f, per_call):
        """median trials per second of five windows of at least a.window seconds, after a warm-up"""
        f()
        rates = []
        for _ in range(5):
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
        shape = (D, D, D)
        N = D ** 3
        V2 = R.phantom(shape, 1)
        V1 = R.phantom(shape, 2)
        mask = R.circular_mask(shape, -(D // 2 - 2.0))
        combos = [(m, w, k) for m in (1, 2) for w in (True, False) for k in (False, True)] if D == 128 else [(1, True, False)]
        for method, wrap, masked in combos:
            base = None
            for cap in a.capacities:
                h = xa.VolumeAlign(ctx, shape, cap)
                h.set_volumes(V1, V2, mask if masked else None)
                m = max(cap, 16)
                tr = poses(m)
                rate, lo, hi = windows(lambda: h.fit(tr, method, wrap), m)
                h.set_timing(True)
                h.fit(tr, method, wrap)
                st = h.stage_ms()
                h.close()
                base = base or rate
                tiles = -(-min(m, cap) // TILE) * -(-m // cap)
                bytes_ = tiles * N * (8 + (4 if masked else 0)) + m * N * 8
                emit({"bench": "volume_align_fit", "shape": list(shape), "method": "covariance" if method == 1 else "least_squares", "wrap": wrap, "masked": masked,
                      "capacity": cap, "trials_per_call": m, "trials_per_s": round(rate, 1), "trials_per_s_min_max": [round(lo, 1), round(hi, 1)],
                      "ms_per_trial": round(1e3 / rate, 5), "against_capacity_1": round(rate / base, 2),
                      "stage_ms_per_trial": {k: round(t / m, 5) for k, t in st.items()},
                      "gather_hbm_bound_ms_per_trial": round(bytes_ / m / HBM * 1e3, 5), "gather_fp64_bound_ms_per_trial": round(FLOPS * N / FP64 * 1e3, 5)})
    ranges = [(1, 1, 1), (0, 0, 1), (0, 360, 15), (0, 180, 15), (0, 360, 15), (1, 1, 1), (0, 0, 1), (0, 0, 1), (0, 0, 1)]
    tr, _ = xa.valign_trials(ranges)
    for D in a.full:
        shape = (D, D, D)
        h = xa.VolumeAlign(ctx, shape, 256)
        h.set_volumes(R.phantom(shape, 2), R.phantom(shape, 1))
        h.search(tr[:256])
        t = []
        for _ in range(3):
            t0 = time.perf_counter()
            idx, best = h.search(tr)
            t.append(time.perf_counter() - t0)
        h.close()
        emit({"bench": "volume_align_global_search", "shape": list(shape), "ranges": "rot 0 360 15, tilt 0 180 15, psi 0 360 15", "trials": len(tr), "capacity": 256,
              "seconds": round(statistics.median(t), 4), "seconds_min_max": [round(min(t), 4), round(max(t), 4)], "best_index": idx})
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            for l in lines:
                f.write(json.dumps(l) + "\n")


if __name__ == "__main__":
    main()
