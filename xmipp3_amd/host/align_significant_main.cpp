// xmipp_align_significant -- same main as the reference's applications/programs/cuda_align_significant (ProgAlignSignificantGPU<float>)
#include "align_significant.h"
int main(int argc, char **argv)
{
    // --dev takes a list of devices in the reference; the references are not sharded over devices here, so more than one is refused
    for (int i = 1; i < argc; ++i)
        if (std::string(argv[i]) == "--dev" && i + 2 < argc && argv[i + 2][0] != '-') {
            std::cerr << "XMIPP_ERROR " << mc::ERR_NOT_IMPLEMENTED << ": --dev: several devices are not supported, give one device id" << std::endl;
            return mc::ERR_NOT_IMPLEMENTED;
        }
    mc::ProgAlignSignificant program;
    program.read(argc, argv);
    return program.tryRun();
}
