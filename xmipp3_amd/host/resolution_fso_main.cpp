// xmipp_resolution_fso -- same main as the reference's applications/programs/resolution_fso
#include "resolution_fso.h"
int main(int argc, char **argv)
{
    mc::ProgFSO program;
    program.read(argc, argv);
    return program.tryRun();
}
