// xmipp_psd_estimate -- drop-in for the Xmipp program of the same name:
// applications/programs/psd_estimate/psd_estimate_main.cpp
#include "psd_programs.h"
int main(int argc, char **argv)
{
    mc::ProgPSDEstimate program;
    program.read(argc, argv);
    return program.tryRun();
}
