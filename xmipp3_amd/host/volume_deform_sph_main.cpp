// xmipp_volume_deform_sph -- same main as the reference's applications/programs/cuda_volume_deform_sph (ProgVolumeDeformSphGpu);
// a missing mandatory parameter prints the usage after its message
#include "volume_deform_sph.h"
int main(int argc, char **argv)
{
    mc::ProgVolumeDeformSph program;
    program.read(argc, argv);
    if (program.errorCode == mc::ERR_ARG_MISSING) program.showUsage();
    return program.tryRun();
}
