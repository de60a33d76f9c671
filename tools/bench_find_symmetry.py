"""Timing of xmipp_volume_find_symmetry's device side (xh_fsym_*, FindSymmetry) on the phantom of tests/symmetrize_ref.py:
 - trials per second and ms per trial at 64^3, 128^3 and 256^3 against the batch capacity (1 is the baseline: one trial per pass over
   the volume). Axis mode: rot_sym 3 and 7, linear and cubic splines at 128^3, rot_sym 3 linear at the other sizes, no mask. Helical
   mode: a rise of 5 voxels, C1, with and without the dihedral copies, under a cylinder mask;
 - next to the gather's HBM byte bound (V and the mask once per tile of 8 trials, V once per trial and copy by the gather, at 8 TB/s) and
   its fp64 bound at 78.6 TFLOP/s vector fp64 (an estimate of the operations per voxel, trial and copy: axis 15 for the source point and
   its tests, 36 for the trilinear rule or 150 for the 64 spline taps and their weights; helix 60 for sin, cos and the weights of a term
   and 40 per interpolated copy; 6 per trial for the sums), with the stage times by events (gather and workgroup sums, finish, choice);
 - one full default search of each mode in seconds: --rot 0 355 5 --tilt 0 90 5 (1368 trials, rot_sym 3) and --rotHelical -357 357 3
   -z 1 10 0.5 (4541 trials, C1, cylinder mask), beside the numpy restatement's seconds per trial on this host's CPU at 32^3 and 64^3 (the
   reference cannot be built here: the restatement is vectorised numpy, not the reference's scalar loop, so the figure is a scale, not a
   speed-up).
Every rate is the median of five windows of at least --window seconds after a warm-up. No staged-source kernel was built, so there is no
A/B against one. Prints one JSON line per case; --out writes them to a file."""
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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", type=int, nargs="+", default=[64, 128, 256])
    ap.add_argument("--capacities", type=int, nargs="+", default=[1, 8, 64])
    ap.add_argument("--full", type=int, nargs="*", default=[64, 128], help="sizes of the full default searches")
    ap.add_argument("--cpu", type=int, nargs="*", default=[32, 64], help="sizes of the restatement's time per trial")
    ap.add_argument("--window", type=float, default=0.3)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import numpy as np
    import __graft_entry__ as g
    g.build()
    import xmipp3_amd as xa
    from tests import find_symmetry_ref as R
    from tests.symmetrize_ref import phantom
    ctx = xa.Context(0)
    lines = []
    rng = np.random.default_rng(3)

    def emit(line):
        line["reference_speedup"] = "not measured"
        line["library"] = os.path.basename(xa.lib_path())
        print(json.dumps(line), flush=True)
        lines.append(line)

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

    def series(kind, shape, V, mask, label, run, copies, flops_copy, flops_trial, splines=False):
        N = shape[0] * shape[1] * shape[2]
        live = N if mask is None else int((mask != 0).sum())
        base = None
        for cap in a.capacities:
            h = xa.FindSymmetry(ctx, shape, cap)
            h.set_volume(V, mask, splines=splines)
            m = max(cap, 16)
            rate, lo, hi = windows(lambda: run(h, m), m)
            h.set_timing(True)
            run(h, m)
            st = h.stage_ms()
            h.close()
            base = base or rate
            tiles = -(-min(m, cap) // TILE) * -(-m // cap)
            bytes_ = tiles * N * 12 + m * copies * live * 8
            line = {"bench": kind, "shape": list(shape), "masked_voxels": live, "capacity": cap, "trials_per_call": m, "trials_per_s": round(rate, 1),
                    "trials_per_s_min_max": [round(lo, 1), round(hi, 1)], "ms_per_trial": round(1e3 / rate, 5), "against_capacity_1": round(rate / base, 2),
                    "stage_ms_per_trial": {k: round(t / m, 5) for k, t in st.items()}, "gather_hbm_bound_ms_per_trial": round(bytes_ / m / HBM * 1e3, 5),
                    "gather_fp64_bound_ms_per_trial": round((copies * flops_copy + flops_trial) * live / FP64 * 1e3, 5)}
            line.update(label)
            emit(line)

    for D in a.sizes:
        shape = (D, D, D)
        V = phantom(shape, 1)
        combos = [(n, s) for n in (3, 7) for s in (False, True)] if D == 128 else [(3, False)]
        for rot_sym, splines in combos:
            tr = {}

            def run(h, m, rot_sym=rot_sym, tr=tr):
                if m not in tr:
                    tr[m] = np.stack([rng.uniform(0, 355, m), rng.uniform(0, 90, m)], axis=1)
                h.axis_fit(tr[m], rot_sym)
            series("find_symmetry_axis_fit", shape, V, None, {"rot_sym": rot_sym, "splines": splines}, run, rot_sym - 1, 15 + (150 if splines else 36), 6, splines)
        mask = R.cylinder_mask(shape, -(D // 2 - 2.0), -(D - 4.0))
        for dihedral in (False, True):
            tr = {}

            def run(h, m, dihedral=dihedral, tr=tr):
                if m not in tr:
                    tr[m] = np.stack([rng.uniform(-357, 357, m), np.full(m, 5.0)], axis=1)
                h.helical_fit(tr[m], None, dihedral, 1.0, 1)
            terms = -(-D // 5) + 1
            series("find_symmetry_helical_fit", shape, V, mask, {"z_helical": 5.0, "cn": 1, "dihedral": dihedral}, run, terms * (2 if dihedral else 1), 40,
                   6 + 60 * terms)
    axis_tr, _, _ = xa.fsym_grid((0, 355, 5), (0, 90, 5))
    hel_tr, ny, nx = xa.fsym_grid((-357, 357, 3), (1, 10, 0.5))
    for D in a.full:
        shape = (D, D, D)
        V = phantom(shape, 1)
        for kind, tr, mask, f in (("axis", axis_tr, None, lambda h, t: h.axis_search(t, 3)),
                                  ("helical", hel_tr, R.cylinder_mask(shape, -(D // 2 - 2.0), -(D - 4.0)),
                                   lambda h, t: h.helical_search(t, (1.0, 10.0, -357.0, 357.0), False, 1.0, 1))):
            h = xa.FindSymmetry(ctx, shape, 256)
            h.set_volume(V, mask)
            f(h, tr[:256])
            t = []
            while len(t) < 3 and sum(t) < 20.0:               # three runs, fewer where one takes many seconds
                t0 = time.perf_counter()
                idx, best = f(h, tr)
                t.append(time.perf_counter() - t0)
            h.close()
            emit({"bench": "find_symmetry_default_search", "mode": kind, "shape": list(shape), "trials": len(tr), "capacity": 256,
                  "ranges": "rot 0 355 5, tilt 0 90 5, rot_sym 3, linear" if kind == "axis" else "rotHelical -357 357 3, z 1 10 0.5, C1, cylinder mask",
                  "seconds": round(statistics.median(t), 4), "seconds_min_max": [round(min(t), 4), round(max(t), 4)], "runs": len(t), "best_index": idx})
    for D in a.cpu:
        shape = (D, D, D)
        V = phantom(shape, 1)
        mask = R.clip_mask(shape, R.cylinder_mask(shape, -(D // 2 - 2.0), -(D - 4.0)), 1.0)
        t0 = time.perf_counter()
        R.axis_corr(V, 40.0, 55.0, 3)
        t1 = time.perf_counter()
        for z in (1.0, 5.0, 10.0):
            R.correlation_index(V, R.helical_volume(V, 33.0, z, mask), mask)
        t2 = time.perf_counter()
        emit({"bench": "find_symmetry_restatement_cpu", "shape": list(shape), "axis_seconds_per_trial": round(t1 - t0, 4),
              "helical_seconds_per_trial_mean_of_rises_1_5_10": round((t2 - t1) / 3, 4), "note": "vectorised numpy on one host thread, not the reference's scalar loop"})
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            for l in lines:
                f.write(json.dumps(l) + "\n")


if __name__ == "__main__":
    main()
