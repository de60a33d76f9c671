// xmipp_subtract_projection -- same main as the reference's applications/programs/subtract_projection
#include "subtract_projection.h"
int main(int argc, char **argv)
{
    // one device per run: the particles are not sharded over devices, so a list of ids is refused (as xmipp_angular_continuous_assign2 does)
    for (int i = 1; i < argc; ++i)
        if (std::string(argv[i]) == "--dev" && i + 2 < argc && argv[i + 2][0] != '-') {
            std::cerr << "XMIPP_ERROR " << mc::ERR_NOT_IMPLEMENTED << ": --dev: several devices are not supported, give one device id" << std::endl;
            return mc::ERR_NOT_IMPLEMENTED;
        }
    mc::ProgSubtractProjection program;
    program.read(argc, argv);
    return program.tryRun();
}
