// volume_deform_sph.h -- xmipp_volume_deform_sph: ProgVolumeDeformSphGpu (reconstruction_adapt_cuda/volume_deform_sph_gpu.cpp; CPU
// counterpart reconstruction/volume_deform_sph.cpp) with the cost, the search, the output volume and the strain analysis on the device
// behind the C ABI (xh_vds_*). Same flags, defaults and output files as the reference program; it runs on the default device.
// --thr is accepted and ignored (no host thread pool); --optimizeRadius is accepted and ignored, as the reference reads it and never
// uses it. An empty --sigma, and the single value 0, mean no filtered pairs. Degrees above l1 = 5, l2 = 4 are refused.
#ifndef XMIPP3_AMD_VOLUME_DEFORM_SPH_H
#define XMIPP3_AMD_VOLUME_DEFORM_SPH_H
#include <sstream>
#include "programs.h"

namespace mc {

class ProgVolumeDeformSph : public XmippProgram {
public:
    std::string fnVolI, fnVolR, fnVolOut, fnRoot;
    std::vector<double> sigma;
    bool analyzeStrain = false;
    int L1 = 3, L2 = 2;
    double lambda = 0.00025, Rmax = -1;

    void defineParams() override
    {
        addUsageLine("Compute the deformation that properly fits two volumes using spherical harmonics");
        addParamsLine("   -i <volume>                         : Volume to deform");
        addParamsLine("   -r <volume>                         : Reference volume");
        addParamsLine("  [-o <volume=\"\">]                   : Output volume which is the deformed input volume");
        addParamsLine("  [--oroot <rootname=\"Volumes\">]     : Root name for output files");
        addParamsLine("                                       : By default, the input file is rewritten");
        addParamsLine("  [--sigma <Matrix1D=\"\">]            : Sigma values to filter the volume to perform a multiresolution analysis");
        addParamsLine("  [--analyzeStrain]                    : Save the deformation of each voxel for local strain and rotation analysis");
        addParamsLine("  [--optimizeRadius]                   : Optimize the radius of each spherical harmonic");
        addParamsLine("  [--l1 <l1=3>]                        : Degree Zernike Polynomials=1,2,3,...");
        addParamsLine("  [--l2 <l2=2>]                        : Harmonical depth of the deformation=1,2,3,...");
        addParamsLine("  [--regularization <l=0.00025>]       : Regularization weight");
        addParamsLine("  [--Rmax <r=-1>]                      : Maximum radius for the transformation");
        addParamsLine("  [--thr <N=-1>]                       : Maximal number of the processing CPU threads");
        addExampleLine("xmipp_volume_deform_sph -i vol1.vol -r vol2.vol -o vol1DeformedTo2.vol");
    }

    void readParams() override
    {
        fnVolI = getParam("-i");
        fnVolR = getParam("-r");
        L1 = (int)getIntParam("--l1");
        L2 = (int)getIntParam("--l2");
        fnRoot = getParam("--oroot");
        std::stringstream ss(getParam("--sigma"));
        std::string tok;
        while (ss >> tok) {
            char *end = nullptr;
            const double v = strtod(tok.c_str(), &end);
            if (end == tok.c_str() || *end) REPORT_ERROR(ERR_ARG_INCORRECT, "--sigma: '" + tok + "' is not a number");
            sigma.push_back(v);
        }
        fnVolOut = getParam("-o");
        if (fnVolOut == "") fnVolOut = fnVolI;
        analyzeStrain = checkParam("--analyzeStrain");
        lambda = getDoubleParam("--regularization");
        Rmax = getDoubleParam("--Rmax");
        int32_t n = 0;
        if (xh_vds_num_terms(L1, L2, &n) != XH_OK) REPORT_ERROR(ERR_ARG_INCORRECT, std::string("--l1 / --l2: ") + xh_last_error());
    }

    void show() const
    {
        if (verbose == 0) return;
        std::cout << "Volume to deform:     " << fnVolI << std::endl
                  << "Reference volume:     " << fnVolR << std::endl
                  << "Output volume:        " << fnVolOut << std::endl
                  << "Zernike Degree:       " << L1 << std::endl
                  << "SH Degree:            " << L2 << std::endl
                  << "Save deformation:     " << analyzeStrain << std::endl
                  << "Regularization:       " << lambda << std::endl;
    }

    static void readVolume(const std::string &fn, std::vector<double> &v, ImageInfo &I)
    {
        std::vector<float> f;
        readImage(fn, f, I);
        v.assign(f.begin(), f.end());
    }

    // writeVector: every value followed by a space, in the stream's default formatting
    static void writeVector(const std::string &path, const std::vector<double> &v, bool append)
    {
        std::ofstream f(path, append ? std::ios_base::app : std::ios_base::out);
        if (!f.good()) REPORT_ERROR(ERR_IO_NOREAD, "cannot write " + path);
        for (double x : v) f << x << " ";
        f << std::endl;
    }

    static std::string withoutExtension(const std::string &fn)
    {
        const size_t slash = fn.rfind('/'), dot = fn.rfind('.');
        return (dot == std::string::npos || (slash != std::string::npos && dot < slash)) ? fn : fn.substr(0, dot);
    }

    void run() override
    {
        show();
        std::vector<double> VI, VR;
        ImageInfo II, IR;
        readVolume(fnVolI, VI, II);
        readVolume(fnVolR, VR, IR);
        if (II.x != IR.x || II.y != IR.y || II.z != IR.z) REPORT_ERROR(ERR_MATRIX_DIM, "Input and reference volumes have different dimensions");
        const size_t X = II.x, Y = II.y, Z = II.z, N = X * Y * Z;

        xh_ctx *ctx = nullptr;
        xhCheck(xh_ctx_create_private(0, &ctx));
        XhOwner<xh_ctx> ctxOwner(ctx);
        xh_vds *h = nullptr;
        xhCheck(xh_vds_create(ctx, (int)Z, (int)Y, (int)X, L1, L2, Rmax, lambda, &h));
        XhOwner<xh_vds> hOwner(h);
        int32_t vecSize = 0;
        xhCheck(xh_vds_info(h, &Rmax, &vecSize, nullptr));

        // pair 0: the normalised volumes; one more pair per sigma: the raw volumes low-passed, then normalised
        const bool filtered = sigma.size() > 1 || (sigma.size() == 1 && sigma[0] != 0);
        const size_t npairs = 1 + (filtered ? sigma.size() : 0);
        std::vector<double> pI(npairs * N), pR(npairs * N);
        std::copy(VI.begin(), VI.end(), pI.begin());
        std::copy(VR.begin(), VR.end(), pR.begin());
        for (size_t p = 1; p < npairs; ++p) {
            xhCheck(xh_vds_gauss(h, sigma[p - 1], VI.data(), pI.data() + p * N));
            xhCheck(xh_vds_gauss(h, sigma[p - 1], VR.data(), pR.data() + p * N));
        }
        for (size_t p = 0; p < npairs; ++p) {
            xhCheck(xh_vds_normalize_robust(pI.data() + p * N, N, 1.3284));
            xhCheck(xh_vds_normalize_robust(pR.data() + p * N, N, 1.3284));
        }
        xhCheck(xh_vds_set_pairs(h, (int)npairs, pI.data(), pR.data()));

        std::vector<double> x(3 * (size_t)vecSize, 0.0);
        double out[4] = {0, 0, 0, 0};
        const double count = (double)npairs * (double)N;
        for (int st = 0; st <= L2; ++st) {
            std::cout << std::endl;
            std::cout << "-------------------------- Basis Degrees: (" << L1 << "," << st << ") --------------------------" << std::endl;
            double fitness = 0;
            int32_t iter = 0;
            int64_t evals = 0;
            xhCheck(xh_vds_refine_stage(h, st, x.data(), &fitness, &iter, &evals));
            xhCheck(xh_vds_cost(h, x.data(), out));
            const double deformation = std::sqrt(out[3] / count);
            std::cout << std::endl;
            std::cout << "Deformation " << deformation << std::endl;
            std::ofstream deformFile(fnRoot + "_deformation.txt");
            deformFile << deformation;
        }
        writeVector(fnRoot + "_clnm.txt", {(double)L1, (double)L2, Rmax}, false);
        writeVector(fnRoot + "_clnm.txt", x, true);

        std::vector<double> VO(N), G;
        if (analyzeStrain) G.resize(3 * N);
        xhCheck(xh_vds_apply(h, VI.data(), x.data(), VO.data(), analyzeStrain ? G.data() : nullptr));
        writeVolume(fnVolOut, VO.data(), X, Y, Z);
        if (analyzeStrain) {
            std::vector<double> LS(N), LR(N);
            xhCheck(xh_vds_strain(h, G.data(), LS.data(), LR.data()));
            static const char *axis[3] = {"x", "y", "z"};
            for (int c = 0; c < 3; ++c) writeVolume(fnRoot + "_PPPG" + axis[c] + ".vol", G.data() + c * N, X, Y, Z);
            const std::string base = withoutExtension(fnVolOut);
            writeVolume(base + "_strain.mrc", LS.data(), X, Y, Z);
            writeVolume(base + "_rotation.mrc", LR.data(), X, Y, Z);
        }
    }
};

}  // namespace mc
#endif
