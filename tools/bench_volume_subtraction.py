"""Timing of xmipp_volume_subtraction's device side (xh_vsub_*, VolumeSubtraction) on the synthetic volumes of
tests/volume_subtraction_ref.py, with the mask, at 128^3, 256^3 and 200 x 180 x 160 (no power of two), in both amplitude modes, with
and without --cutFreq 0.3: ms per iteration (the difference of a 6- and a 1-iteration adjust, over 5), seconds of a full run
(set_reference and a 5-iteration adjust, after a warm-up), and with per-stage events the split of an iteration into transforms, spectrum
steps, real-space steps and filter (again 6 iterations minus 1, over 5), each next to the time its HBM bytes take at 8 TB/s: the bound
of a stage that only moves data. The reference cannot be built here: its time is not measured and no speed-up is claimed.
Prints one JSON line per case; --out writes them to a file."""
import argparse
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

HBM = 8e12
CUT = 0.3


def stage_bytes(shape, radavg, cut):
    """HBM bytes of one iteration's stages, each array read or written once per kernel that touches it"""
    Z, Y, X = shape
    vb = 8 * Z * Y * X                                   # a volume of doubles
    fb = 16 * Z * Y * (X // 2 + 1)                       # a half spectrum of complex doubles
    transform = vb + 5 * fb                              # the row pass (volume and spectrum once each), the y and z passes in place
    return {
        "transforms": 4 * transform,
        # amplitude: F read and written, V1FourierMag read (the quotient table stays in cache); phase: F read and written, the phases read
        "spectrum": (2 * fb + (0 if radavg else fb // 2)) + 3 * fb,
        # clip and mask: V read and written, the mask read; max(0, .) with the moments: V read and written
        "real": 3 * vb + 2 * vb,
        "filter": (2 * transform + 2 * fb) if cut else 0,
    }


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", type=int, nargs="+", default=[128, 128, 128, 256, 256, 256, 200, 180, 160], help="Z Y X of every box, one after the other")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import torch
    import __graft_entry__ as g
    g.build()
    import xmipp3_amd as xa
    from tests import volume_subtraction_ref as R
    ctx = xa.Context(0)
    lines = []
    shapes = [tuple(a.shapes[i:i + 3]) for i in range(0, len(a.shapes), 3)]
    for shape in shapes:
        v1, v, mask = R.synth(shape, 1)
        d1, dv, dm = (torch.from_numpy(t).cuda() for t in (v1, v, mask))
        h = xa.VolumeSubtraction(ctx, shape)
        for radavg in (False, True):
            if radavg and R.radial_overflows(shape):
                continue
            for cut in (0.0, CUT):
                def wall(f):
                    torch.cuda.synchronize()
                    t0 = time.perf_counter()
                    f()
                    torch.cuda.synchronize()
                    return time.perf_counter() - t0

                def full():
                    h.set_reference(d1, dm, radavg)
                    h.adjust(dv, 5, 1.0, radavg, cut)
                full()
                t_full = min(wall(full) for _ in range(3))
                t1 = min(wall(lambda: h.adjust(dv, 1, 1.0, radavg, cut)) for _ in range(3))
                t6 = min(wall(lambda: h.adjust(dv, 6, 1.0, radavg, cut)) for _ in range(3))
                h.set_timing(True)
                h.adjust(dv, 1, 1.0, radavg, cut)
                s1 = h.stage_ms()
                h.adjust(dv, 6, 1.0, radavg, cut)
                s6 = h.stage_ms()
                h.set_timing(False)
                by = stage_bytes(shape, radavg, cut)
                line = {"bench": "volume_subtraction", "shape": list(shape), "radavg": radavg, "cutFreq": cut,
                        "ms_per_iteration": round((t6 - t1) * 1e3 / 5, 4), "full_run_s": round(t_full, 5), "reference_speedup": "not measured",
                        "stage_ms_per_iteration": {k: round((s6[k] - s1[k]) / 5, 4) for k in s6},
                        "stage_hbm_bound_ms": {k: round(by[k] / HBM * 1e3, 4) for k in s6}, "library": os.path.basename(xa.lib_path())}
                print(json.dumps(line), flush=True)
                lines.append(line)
        h.close()
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            for l in lines:
                f.write(json.dumps(l) + "\n")


if __name__ == "__main__":
    main()
