// xmipp_transform_symmetrize -- drop-in for the Xmipp program of the same name:
// applications/programs/transform_symmetrize/transform_symmetrize_main.cpp
#include "transform_symmetrize.h"
int main(int argc, char **argv)
{
    mc::ProgSymmetrize program;
    program.read(argc, argv);
    return program.tryRun();
}
