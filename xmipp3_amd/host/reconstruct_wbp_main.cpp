// xmipp_reconstruct_wbp -- drop-in for the Xmipp program of the same name:
// applications/programs/reconstruct_wbp/reconstruct_wbp_main.cpp
#include "reconstruct_wbp.h"
int main(int argc, char **argv)
{
    mc::ProgRecWbp program;
    program.read(argc, argv);
    return program.tryRun();
}
