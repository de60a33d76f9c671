// xmipp_volume_subtraction -- same main as the reference's applications/programs/volume_subtraction
#include "volume_subtraction.h"
int main(int argc, char **argv)
{
    mc::ProgVolumeSubtraction program;
    program.read(argc, argv);
    return program.tryRun();
}
