// xmipp_reconstruct_significant -- same main as the reference's applications/programs/reconstruct_significant (ProgReconstructSignificant),
// without the MPI variant
#include "reconstruct_significant.h"
int main(int argc, char **argv)
{
    mc::ProgReconstructSignificant program;
    program.read(argc, argv);
    return program.tryRun();
}
