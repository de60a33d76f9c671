// volume_halves_restoration.h -- xmipp_volume_halves_restoration: ProgVolumeHalvesRestorationGpu<double>
// (reconstruction_adapt_cuda/volume_halves_restoration_gpu.cpp) with VolumeHalvesRestorator's stages on the device behind the C ABI
// (xh_halves_*). Same flags, defaults, error messages and output files as the reference program; it runs on the default device.
//
// Masks: minicore has no Mask class, so two of Mask's types are supported:
//   --mask binary_file <file>  a volume read as int (truncated), nonzero = inside
//   --mask circular <R>        BinaryCircularMask about the Xmipp origin (plus --center): R < 0 keeps r <= |R|, R > 0 keeps r >= R
// Every other mask type is refused with ERR_NOT_IMPLEMENTED and its name. The reference program builds its mask only when Mask's
// fn_mask is set, which Mask::readParams does for file masks alone, so it ignores a circular mask; here a circular mask is applied.
#ifndef XMIPP3_AMD_VOLUME_HALVES_RESTORATION_H
#define XMIPP3_AMD_VOLUME_HALVES_RESTORATION_H
#include "programs.h"

namespace mc {

class ProgVolumeHalvesRestoration : public XmippProgram {
public:
    std::string fnV1, fnV2, fnRoot;
    int denoisingIters = 0, deconvolutionIters = 0, differenceIters = 0, weightFun = 1;
    double sigma = 0.2, lambda = 0.001, Kdiff = 1.5, bankStep = 0, bankOverlap = 0.5, weightPower = 3;
    std::string maskType, maskArg;
    double R1 = 0, x0 = 0, y0 = 0, z0 = 0;
    bool useMask = false;

    void defineParams() override
    {
        // volume_halves_restoration_gpu.cpp defineParams
        addUsageLine("Given two halves of a volume (and an optional mask), produce a better estimate of the volume underneath");
        addParamsLine("   --i1 <volume1>              : First half");
        addParamsLine("   --i2 <volume2>              : Second half");
        addParamsLine("  [--oroot <root=\"volumeRestored\">] : Output rootname");
        addParamsLine("  [--denoising <N=0>]          : Number of iterations of denoising in real space");
        addParamsLine("  [--deconvolution <N=0> <sigma0=0.2> <lambda=0.001>]   : Number of iterations of deconvolution in Fourier space, initial sigma and lambda");
        addParamsLine("  [--filterBank <step=0> <overlap=0.5> <weightFun=1> <weightPower=3>] : Frequency step for the filter bank (typically, 0.01; between 0 and 0.5)");
        addParamsLine("                                        : filter overlap is between 0 (no overlap) and 1 (full overlap)");
        addParamsLine("                                : Weight function (0=mean, 1=min, 2=mean*diff");
        addParamsLine("  [--difference <N=0> <K=1.5>]  : Number of iterations of difference evaluation in real space");
        // Mask::defineParams(this, INT_MASK), the two supported types
        addParamsLine("  [--mask <mask_type=circular> <arg=\"\">] : binary_file <file> or circular <R> (R < 0: inside, R > 0: outside); other types are refused");
        addParamsLine("  [--center <x0=0> <y0=0> <z0=0>]: mask center");
    }

    void readParams() override
    {
        fnV1 = getParam("--i1");
        fnV2 = getParam("--i2");
        fnRoot = getParam("--oroot");
        denoisingIters = (int)getIntParam("--denoising");
        if (denoisingIters < 0) REPORT_ERROR(ERR_ARG_BADCMDLINE, "`denoising N` has to be non-negative integer");
        deconvolutionIters = (int)getIntParam("--deconvolution");
        sigma = getDoubleParam("--deconvolution", 1);
        lambda = getDoubleParam("--deconvolution", 2);
        if (deconvolutionIters < 0) REPORT_ERROR(ERR_ARG_BADCMDLINE, "`deconvolution N` has to be non-negative integer");
        bankStep = getDoubleParam("--filterBank", 0);
        bankOverlap = getDoubleParam("--filterBank", 1);
        weightFun = (int)getIntParam("--filterBank", 2);
        weightPower = getDoubleParam("--filterBank", 3);
        if (bankStep < 0 || bankStep > 0.5001) REPORT_ERROR(ERR_ARG_BADCMDLINE, "`filterBank step` parameter has to be in interval [0, 0.5].");
        if (bankOverlap < 0 || bankOverlap > 1.001) REPORT_ERROR(ERR_ARG_BADCMDLINE, "`filterBank overlap` parameter has to be in interval [0, 1]");
        // the reference's message names 0, 1 or 2 while its check admits 3
        if (weightFun < 0 || weightFun > 3) REPORT_ERROR(ERR_ARG_BADCMDLINE, "`filterBank weightFun` parameter has to be 0, 1 or 2");
        differenceIters = (int)getIntParam("--difference");
        Kdiff = getDoubleParam("--difference", 1);
        if (differenceIters < 0) REPORT_ERROR(ERR_ARG_BADCMDLINE, "`difference N` has to be non-negative integer");
        if (checkParam("--mask")) readMaskParams();
    }

    void readMaskParams()
    {
        // Mask::readParams
        x0 = getDoubleParam("--center", 0);
        y0 = getDoubleParam("--center", 1);
        z0 = getDoubleParam("--center", 2);
        maskType = getParam("--mask");
        if (maskType == "circular") {
            R1 = getDoubleParam("--mask", 1);
            if (R1 == 0) REPORT_ERROR(ERR_ARG_INCORRECT, "MaskProgram: circular mask with radius 0");
        } else if (maskType == "binary_file") {
            maskArg = getParam("--mask", 1);
            if (maskArg.empty()) REPORT_ERROR(ERR_ARG_MISSING, "--mask binary_file needs a file name");
        } else {
            REPORT_ERROR(ERR_NOT_IMPLEMENTED, "--mask " + maskType + ": only the binary_file and circular mask types are supported");
        }
        useMask = true;
    }

    void show() const
    {
        if (!verbose) return;
        std::cout << "Input/Ouput filenames:" << std::endl
                  << "    Volume1:  " << fnV1 << std::endl
                  << "    Volume2:  " << fnV2 << std::endl
                  << "    Rootname: " << fnRoot << std::endl
                  << "VolumeHalvesRestoration parameters:" << std::endl
                  << "    Denoising Iterations:" << denoisingIters << std::endl
                  << "    Deconvolution Iterations: " << deconvolutionIters << std::endl
                  << "    Sigma0:   " << sigma << std::endl
                  << "    Lambda:   " << lambda << std::endl
                  << "    Bank step:" << bankStep << std::endl
                  << "    Bank overlap:" << bankOverlap << std::endl
                  << "    Weight fun:" << weightFun << std::endl
                  << "    Weight power:" << weightPower << std::endl
                  << "    Difference Iterations: " << differenceIters << std::endl
                  << "    Kdiff: " << Kdiff << std::endl;
    }

    void run() override
    {
        show();
        std::vector<double> v1, v2;
        ImageInfo I1, I2;
        readDoubles(fnV1, v1, I1);
        readDoubles(fnV2, v2, I2);
        sameShape(I1, I2, "Input volumes");
        const size_t X = I1.x, Y = I1.y, Z = I1.z, N = X * Y * Z;
        std::vector<int32_t> mask;
        if (useMask) {
            if (maskType == "binary_file") {
                std::vector<float> f;
                ImageInfo IM;
                readImage(maskArg, f, IM);
                sameShape(IM, I1, "Mask and input volumes");
                mask.resize(N);
                xhCheck(xh_halves_binary_mask(f.data(), N, mask.data()));
            } else {
                mask.resize(N);
                xhCheck(xh_halves_circular_mask((int)Z, (int)Y, (int)X, R1, x0, y0, z0, mask.data()));
            }
        }

        xh_ctx *ctx = nullptr;
        xhCheck(xh_ctx_create_private(0, &ctx));
        XhOwner<xh_ctx> ctxOwner(ctx);
        xh_halves *h = nullptr;
        xhCheck(xh_halves_create(ctx, (int)Z, (int)Y, (int)X, &h));
        XhOwner<xh_halves> hOwner(h);
        DeviceBuffer dV1, dV2, dMask, dOut;
        dV1.upload(ctx, v1.data(), sizeof(double) * N);
        dV2.upload(ctx, v2.data(), sizeof(double) * N);
        const int32_t *m = nullptr;
        if (!mask.empty()) {
            dMask.upload(ctx, mask.data(), sizeof(int32_t) * N);
            m = dMask.as<int32_t>();
        }
        xhCheck(xh_halves_load(h, dV1.as<double>(), dV2.as<double>()));
        // VolumeHalvesRestorator::apply
        xhCheck(xh_halves_denoise(h, denoisingIters, m));
        std::vector<double> sig(2 * (size_t)std::max(1, deconvolutionIters));
        xhCheck(xh_halves_deconvolve(h, deconvolutionIters, sigma, lambda, sig.data()));
        if (verbose > 0)
            for (int i = 0; i < deconvolutionIters; ++i) std::cout << "   Deconvolving with sigma=" << sig[2 * i] << " " << sig[2 * i + 1] << std::endl;
        xhCheck(xh_halves_filter_bank(h, bankStep, bankOverlap, weightFun, weightPower));
        xhCheck(xh_halves_difference(h, differenceIters, Kdiff, m));
        // saveResults: an output whose stage did not run is empty and not written
        static const char *suffix[6] = {"_restored1.vol", "_restored2.vol", "_filterBank.vol", "_deconvolved.vol", "_convolved.vol", "_avgDiff.vol"};
        std::vector<double> out(N);
        dOut.reserve(ctx, sizeof(double) * N);
        for (int w = 0; w < 6; ++w) {
            int32_t present = 0;
            xhCheck(xh_halves_output(h, w, dOut.as<double>(), &present));
            if (!present) continue;
            xhCheck(xh_memcpy_d2h(ctx, out.data(), dOut.p, sizeof(double) * N));
            writeVolume(fnRoot + suffix[w], out.data(), X, Y, Z);
        }
    }
};

}  // namespace mc
#endif
