// Test probe for the CTF model the host programs share with the device code (xmipp3_amd/csrc/xh_ctf.h through
// xmipp3_amd/host/ctf_model.h; no device and no library needed): prints what side_info + d_ctf_at and the matcher's gallery-filter
// table give, %.17g, so that tests/test_host_ctf.py can compare them with an independent evaluation.
//   ctf_probe value <phaseShiftInDegrees 0|1> <the 19 xh_ctf_params fields> <X Y>...   the pure value with damping, one per line
//   ctf_probe table <the 19 xh_ctf_params fields> <paddim> <phase_flipped 0|1>         ctfFilterTable, one row per line
#include "../../xmipp3_amd/host/ctf_model.h"
using namespace mc;

static void readParams(char **argv, xh_ctf_params &c)
{
    double *f = reinterpret_cast<double *>(&c);
    for (int i = 0; i < 19; ++i) f[i] = atof(argv[i]);
}

int main(int argc, char **argv)
{
    static_assert(sizeof(xh_ctf_params) == 19 * sizeof(double), "xh_ctf_params is 19 doubles");
    const std::string mode = argc > 1 ? argv[1] : "";
    xh_ctf_params c;
    if (mode == "value" && argc >= 3 + 19 + 2 && (argc - 3 - 19) % 2 == 0) {
        readParams(argv + 3, c);
        const CtfSide s = side_info(c, atoi(argv[2]) != 0);
        for (int a = 3 + 19; a + 1 < argc; a += 2) printf("%.17g\n", d_ctf_at(s, atof(argv[a]), atof(argv[a + 1]), true));
        return 0;
    }
    if (mode == "table" && argc == 2 + 19 + 2) {
        readParams(argv + 2, c);
        const int paddim = atoi(argv[2 + 19]);
        const std::vector<double> M = ctfFilterTable(c, paddim, atoi(argv[2 + 19 + 1]) != 0);
        for (int i = 0; i < paddim; ++i) {
            for (int j = 0; j < paddim; ++j) printf("%.17g ", M[(size_t)i * paddim + j]);
            printf("\n");
        }
        return 0;
    }
    fprintf(stderr, "usage: ctf_probe value <deg> <19 fields> <X Y>... | table <19 fields> <paddim> <phase_flipped>\n");
    return 1;
}
