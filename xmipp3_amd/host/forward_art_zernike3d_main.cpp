// xmipp_forward_art_zernike3d -- same main as the reference's applications/programs/cuda11_forward_art_zernike3d
#include "forward_art_zernike3d.h"
int main(int argc, char **argv)
{
    // one device per run: the sweep is sequential in the volume, so a list of ids is refused (as xmipp_align_significant does)
    for (int i = 1; i < argc; ++i)
        if (std::string(argv[i]) == "--dev" && i + 2 < argc && argv[i + 2][0] != '-') {
            std::cerr << "XMIPP_ERROR " << mc::ERR_NOT_IMPLEMENTED << ": --dev: several devices are not supported, give one device id" << std::endl;
            return mc::ERR_NOT_IMPLEMENTED;
        }
    mc::ProgForwardArtZernike3D program;
    program.read(argc, argv);
    return program.tryRun();
}
