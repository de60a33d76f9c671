// Test probe for the host normalisation of xmipp_psd_estimate (xmipp3_amd/host/psd_programs.h, no device needed): reads float32 values from
// a file, runs psdNormalize (10 log10, the floor for the values that are not positive, reject_outliers) and writes the float32 result to
// stdout, so that tests/test_psd_host.py can compare it with the restatement.
#include "../../xmipp3_amd/host/psd_programs.h"
using namespace mc;

int main(int argc, char **argv)
{
    if (argc < 2) {
        fprintf(stderr, "usage: psd_probe <float32 file>\n");
        return 1;
    }
    std::ifstream f(argv[1], std::ios::binary);
    std::vector<char> raw((std::istreambuf_iterator<char>(f)), std::istreambuf_iterator<char>());
    std::vector<float> v(raw.size() / 4);
    memcpy(v.data(), raw.data(), v.size() * 4);
    psdNormalize(v);
    fwrite(v.data(), 4, v.size(), stdout);
    return 0;
}
