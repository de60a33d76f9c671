// xmipp_volume_align -- drop-in for the Xmipp program of the same name:
// applications/programs/volume_align/volume_align_main.cpp
#include "volume_align.h"
int main(int argc, char **argv)
{
    mc::ProgAlignVolumes program;
    program.read(argc, argv);
    return program.tryRun();
}
