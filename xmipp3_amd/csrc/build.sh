#!/bin/bash
# Builds libxmipp_hip.so for gfx950 (MI355X). hipcc cross-compiles without a GPU.
set -e
cd "$(dirname "$0")"
HIPCC=${HIPCC:-/opt/rocm/bin/hipcc}
COMMON="--offload-arch=gfx950 -O3 -std=c++17 -fPIC -munsafe-fp-atomics -Wall -Wno-unused-function -Wno-unused-result"
mkdir -p build
pids=()
# geometry of the gridding must round like the reference's scalar code: no FMA contraction
$HIPCC $COMMON -ffp-contract=off -c xh_rf.hip -o build/xh_rf.o & pids+=($!)
$HIPCC $COMMON -c xh_ctx.hip -o build/xh_ctx.o & pids+=($!)
if [ -f xh_pm.hip ]; then $HIPCC $COMMON -c xh_pm.hip -o build/xh_pm.o & pids+=($!); fi
$HIPCC $COMMON -c xh_fp.hip -o build/xh_fp.o & pids+=($!)
$HIPCC $COMMON -c xh_fft2d.hip -o build/xh_fft2d.o & pids+=($!)
$HIPCC $COMMON -c xh_ctfops.hip -o build/xh_ctfops.o & pids+=($!)
$HIPCC $COMMON -c xh_flexalign.hip -o build/xh_flexalign.o & pids+=($!)
$HIPCC $COMMON -c xh_estimators.hip -o build/xh_estimators.o & pids+=($!)
$HIPCC $COMMON -c xh_align_sig.hip -o build/xh_align_sig.o & pids+=($!)
$HIPCC $COMMON -c xh_ca2.hip -o build/xh_ca2.o & pids+=($!)
# shell membership of the FSC is decided in double arithmetic that must round like the scalar code
$HIPCC $COMMON -ffp-contract=off -c xh_fsc.hip -o build/xh_fsc.o & pids+=($!)
# frequency-band and resolution-limit membership (R2 against w^2, 0.25) must round like the reference's scalar double code
$HIPCC $COMMON -ffp-contract=off -c xh_halves.hip -o build/xh_halves.o & pids+=($!)
$HIPCC $COMMON -c xh_vds.hip -o build/xh_vds.o & pids+=($!)
$HIPCC $COMMON -c xh_asa.hip -o build/xh_asa.o & pids+=($!)
$HIPCC $COMMON -c xh_faz.hip -o build/xh_faz.o & pids+=($!)
# Powell's line searches compare costs that differ in the last bits: the minimiser keeps the rounding it was validated with, no FMA contraction
$HIPCC $COMMON -ffp-contract=off -c xh_powell.hip -o build/xh_powell.o & pids+=($!)
# which voxel a ray enters next is decided by comparing doubles that differ in the last bits: the walk must round like the reference's scalar code
$HIPCC $COMMON -ffp-contract=off -c xh_rsp.hip -o build/xh_rsp.o & pids+=($!)
# the fit runs the same code on the host and on the device; its quotients must round alike
$HIPCC $COMMON -ffp-contract=off -c xh_sub.hip -o build/xh_sub.o & pids+=($!)
# band membership (freqH <= un && un <= freq) and the threshold comparisons must round like the reference's scalar double code
$HIPCC $COMMON -ffp-contract=off -c xh_mono.hip -o build/xh_mono.o & pids+=($!)
# band membership (w_inf <= un && un <= wL) must round like the reference's scalar double code; the weighted sum rounds product and add separately
$HIPCC $COMMON -ffp-contract=off -c xh_ldb.hip -o build/xh_ldb.o & pids+=($!)
# cone membership (cosine >= cosAngle) is a float comparison of a three-term dot product that must round like the reference's scalar code
$HIPCC $COMMON -ffp-contract=off -c xh_fso.hip -o build/xh_fso.o & pids+=($!)
# mod > 1e-10 of the amplitude step and the radial bin index (round, floor of w X) must round like the reference's scalar double code
$HIPCC $COMMON -ffp-contract=off -c xh_vsub.hip -o build/xh_vsub.o & pids+=($!)
# the chain's thresholds, arg-max picks, corr > bestCorr, RS against SR and the mirror pick compare doubles that must round like the reference's scalar code
$HIPCC $COMMON -ffp-contract=off -c xh_rsig.hip -o build/xh_rsig.o & pids+=($!)
# the source coordinates feed the wrap / outside thresholds, the (int) and ceil of the taps and the helix's kp range: they must round like the scalar code
$HIPCC $COMMON -ffp-contract=off -c xh_sym.hip -o build/xh_sym.o & pids+=($!)
# the same source coordinates and range tests as xh_sym.hip (xh_applygeo.h), and fits whose last bits decide the search's first minimum
$HIPCC $COMMON -ffp-contract=off -c xh_valign.hip -o build/xh_valign.o & pids+=($!)
# the same source coordinates, range tests and helix as xh_sym.hip (xh_applygeo.h, xh_helix.h), and correlations whose last bits decide the search's first maximum
$HIPCC $COMMON -ffp-contract=off -c xh_fsym.hip -o build/xh_fsym.o & pids+=($!)
# the sinc table's index is the (int) of a quotient, the back-projection's taps the (int) of a coordinate, and the threshold, sphere and image cuts compare doubles: they must round like the scalar code
$HIPCC $COMMON -ffp-contract=off -c xh_wbp.hip -o build/xh_wbp.o & pids+=($!)
# the deviation of normalize_ramp feeds a comparison (> 1e-6) and every value before the transform is formed with the reference's roundings
$HIPCC $COMMON -ffp-contract=off -c xh_psd.hip -o build/xh_psd.o & pids+=($!)
fail=0
for p in "${pids[@]}"; do wait $p || fail=1; done
if [ $fail -ne 0 ]; then echo "build.sh: compilation FAILED" >&2; exit 1; fi
$HIPCC --offload-arch=gfx950 -shared -fPIC -o ../libxmipp_hip.so build/xh_rf.o build/xh_ctx.o build/xh_pm.o build/xh_fp.o build/xh_fft2d.o build/xh_fsc.o build/xh_ctfops.o build/xh_flexalign.o build/xh_estimators.o build/xh_align_sig.o build/xh_halves.o build/xh_ca2.o build/xh_vds.o build/xh_asa.o build/xh_faz.o build/xh_powell.o build/xh_rsp.o build/xh_sub.o build/xh_mono.o build/xh_ldb.o build/xh_fso.o build/xh_vsub.o build/xh_rsig.o build/xh_sym.o build/xh_valign.o build/xh_fsym.o build/xh_wbp.o build/xh_psd.o
echo "built $(cd .. && pwd)/libxmipp_hip.so"
