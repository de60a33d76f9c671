// xmipp_volume_local_sharpening -- same main as the reference's applications/programs/volume_local_sharpening
#include "volume_local_sharpening.h"
int main(int argc, char **argv)
{
    mc::ProgLocSharpening program;
    program.read(argc, argv);
    return program.tryRun();
}
