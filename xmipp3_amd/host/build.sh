#!/bin/bash
# Builds the host programs against libxmipp_hip.so (plain g++: the host side has no HIP code).
set -e
cd "$(dirname "$0")"
mkdir -p ../bin
CXX=${CXX:-g++}
FLAGS="-O2 -std=c++17 -pthread -Wall -Wno-unused-function"
LINK="-L.. -lxmipp_hip -Wl,-rpath,\$ORIGIN/.. -Wl,-rpath,/opt/rocm/lib"
$CXX $FLAGS angular_projection_matching_main.cpp -o ../bin/xmipp_angular_projection_matching $LINK &
$CXX $FLAGS reconstruct_fourier_accel_main.cpp -o ../bin/xmipp_reconstruct_fourier_accel $LINK &
$CXX $FLAGS reconstruct_fourier_main.cpp -o ../bin/xmipp_reconstruct_fourier $LINK &
$CXX $FLAGS angular_project_library_main.cpp -o ../bin/xmipp_angular_project_library $LINK &
$CXX $FLAGS resolution_fsc_main.cpp -o ../bin/xmipp_resolution_fsc $LINK &
$CXX $FLAGS ctf_phase_flip_main.cpp -o ../bin/xmipp_ctf_phase_flip $LINK &
$CXX $FLAGS ctf_correct_wiener2d_main.cpp -o ../bin/xmipp_ctf_correct_wiener2d $LINK &
$CXX $FLAGS movie_alignment_correlation_main.cpp -o ../bin/xmipp_movie_alignment_correlation $LINK &
$CXX $FLAGS movie_filter_dose_main.cpp -o ../bin/xmipp_movie_filter_dose $LINK &
$CXX $FLAGS align_significant_main.cpp -o ../bin/xmipp_align_significant $LINK &
$CXX $FLAGS volume_halves_restoration_main.cpp -o ../bin/xmipp_volume_halves_restoration $LINK &
$CXX $FLAGS angular_continuous_assign2_main.cpp -o ../bin/xmipp_angular_continuous_assign2 $LINK &
$CXX $FLAGS volume_deform_sph_main.cpp -o ../bin/xmipp_volume_deform_sph $LINK &
$CXX $FLAGS angular_sph_alignment_main.cpp -o ../bin/xmipp_angular_sph_alignment $LINK &
$CXX $FLAGS forward_art_zernike3d_main.cpp -o ../bin/xmipp_forward_art_zernike3d $LINK &
$CXX $FLAGS subtract_projection_main.cpp -o ../bin/xmipp_subtract_projection $LINK &
$CXX $FLAGS resolution_monogenic_signal_main.cpp -o ../bin/xmipp_resolution_monogenic_signal $LINK &
$CXX $FLAGS volume_local_sharpening_main.cpp -o ../bin/xmipp_volume_local_sharpening $LINK &
$CXX $FLAGS resolution_fso_main.cpp -o ../bin/xmipp_resolution_fso $LINK &
$CXX $FLAGS volume_subtraction_main.cpp -o ../bin/xmipp_volume_subtraction $LINK &
$CXX $FLAGS reconstruct_significant_main.cpp -o ../bin/xmipp_reconstruct_significant $LINK &
$CXX $FLAGS transform_symmetrize_main.cpp -o ../bin/xmipp_transform_symmetrize $LINK &
$CXX $FLAGS volume_align_main.cpp -o ../bin/xmipp_volume_align $LINK &
$CXX $FLAGS volume_find_symmetry_main.cpp -o ../bin/xmipp_volume_find_symmetry $LINK &
$CXX $FLAGS reconstruct_wbp_main.cpp -o ../bin/xmipp_reconstruct_wbp $LINK &
$CXX $FLAGS ctf_estimate_from_micrograph_main.cpp -o ../bin/xmipp_ctf_estimate_from_micrograph $LINK &
$CXX $FLAGS psd_estimate_main.cpp -o ../bin/xmipp_psd_estimate $LINK &
wait
echo "built $(cd ../bin && pwd)/xmipp_{angular_projection_matching,reconstruct_fourier_accel,reconstruct_fourier,angular_project_library,resolution_fsc,ctf_phase_flip,ctf_correct_wiener2d,movie_alignment_correlation,movie_filter_dose,align_significant,volume_halves_restoration,angular_continuous_assign2,volume_deform_sph,angular_sph_alignment,forward_art_zernike3d,subtract_projection,resolution_monogenic_signal,volume_local_sharpening,resolution_fso,volume_subtraction,reconstruct_significant,transform_symmetrize,volume_align,volume_find_symmetry,reconstruct_wbp,ctf_estimate_from_micrograph,psd_estimate}"
