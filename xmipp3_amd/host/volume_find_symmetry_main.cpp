// xmipp_volume_find_symmetry -- drop-in for the Xmipp program of the same name:
// applications/programs/volume_find_symmetry/volume_find_symmetry_main.cpp
#include "volume_find_symmetry.h"
int main(int argc, char **argv)
{
    mc::ProgVolumeFindSymmetry program;
    program.read(argc, argv);
    return program.tryRun();
}
