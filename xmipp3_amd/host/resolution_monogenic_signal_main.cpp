// xmipp_resolution_monogenic_signal -- same main as the reference's applications/programs/resolution_monogenic_signal
#include "resolution_monogenic_signal.h"
int main(int argc, char **argv)
{
    mc::ProgMonogenicSignalRes program;
    program.read(argc, argv);
    return program.tryRun();
}
