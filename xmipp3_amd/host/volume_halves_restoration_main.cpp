// xmipp_volume_halves_restoration -- same main as the reference's applications/programs/cuda_volume_halves_restoration
// (ProgVolumeHalvesRestorationGpu<double>)
#include "volume_halves_restoration.h"
int main(int argc, char **argv)
{
    mc::ProgVolumeHalvesRestoration program;
    program.read(argc, argv);
    return program.tryRun();
}
