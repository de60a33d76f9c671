// xmipp_angular_sph_alignment -- same main as the reference's applications/programs/angular_sph_alignment
#include "angular_sph_alignment.h"
int main(int argc, char **argv)
{
    mc::ProgAngularSphAlignment program;
    program.read(argc, argv);
    return program.tryRun();
}
