// xmipp_ctf_estimate_from_micrograph -- drop-in for the PSD stage of the Xmipp program of the same name:
// applications/programs/ctf_estimate_from_micrograph/ctf_estimate_from_micrograph_main.cpp
#include "psd_programs.h"
int main(int argc, char **argv)
{
    mc::ProgCTFEstimateFromMicrograph program;
    program.read(argc, argv);
    return program.tryRun();
}
