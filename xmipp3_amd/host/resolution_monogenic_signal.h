// resolution_monogenic_signal.h -- xmipp_resolution_monogenic_signal, MonoRes: ProgMonogenicSignalRes
// (reconstruction/resolution_monogenic_signal.{h,cpp}) with the sweep on the device behind the C ABI (xh_mono_*). The options of
// defineParams (:51-87) plus --dev; --threads is accepted and ignored. Outputs go into the -o folder under the reference's names:
// meanMap.mrc (half maps only), refinedMask.mrc, monoresResolutionChimera.mrc, monoresResolutionMap.mrc. The reference writes the
// refined mask as an int image; minicore writes float MRC, so it is written as floats 0 / 1.
// A missing --mask is an error (the reference prints its message and calls exit(0); here the exit code is not 0).
#ifndef XMIPP3_AMD_RESOLUTION_MONOGENIC_SIGNAL_H
#define XMIPP3_AMD_RESOLUTION_MONOGENIC_SIGNAL_H
#include "programs.h"

namespace mc {

class ProgMonogenicSignalRes : public XmippProgram {
public:
    std::string fnVol, fnVol2, fnMask, fnMaskExl, fnOut;
    xh_mono_params prm;
    int nthrs = 4, device = 0;

    void defineParams() override
    {
        addUsageLine("MONORES: This algorithm estimates the local resolution map from a single reconstruction");
        addUsageLine("or two half maps.");
        addUsageLine("Reference: J.L. Vilas et al, MonoRes: Automatic and Accurate Estimation of ");
        addUsageLine("Local Resolution for Electron Microscopy Maps, Structure, 26, 337-344, (2018).");
        addParamsLine("  --vol <vol_file=\"\">         : Input map to estimate its local resolution map; with --vol2, the first half map");
        addParamsLine("  --mask <vol_file=\"\">        : Mask defining the region where the protein is.");
        addParamsLine("  --minRes <s=30>               : Lowest resolution in (A) for the resolution range to be analyzed.");
        addParamsLine("  --maxRes <s=1>                : Highest resolution in (A) for the resolution range to be analyzed.");
        addParamsLine("  --sampling_rate <s=1>         : Sampling rate (A/px)");
        addParamsLine("  -o <output_folder=\"\">         : Folder where the results will be stored.");
        addParamsLine("  [--vol2 <vol_file=\"\">]      : (Optional but recommended) Second half map");
        addParamsLine("  [--maskExcl <vol_file=\"\">]  : (Optional) This mask excludes the masked region in the estimation of the local resolution.");
        addParamsLine("  [--step <s=0.25>]             : (Optional) The resolution is computed from low to high frequency in steps of this parameter in (A).");
        addParamsLine("  [--significance <s=0.95>]     : (Optional) The level of confidence for the hypothesis test between signal and noise.");
        addParamsLine("  [--threads <s=4>]             : (Optional) accepted and ignored: the sweep runs on the device");
        addParamsLine("  [--noiseonlyinhalves]         : (Optional) The noise estimation is only performed inside the mask (two half maps only).");
        addParamsLine("  [--gaussian]                  : (Optional) This flag assumes than the noise is gaussian.");
        addParamsLine("  [--dev <id=0>]                : GPU device to use (one device only)");
    }

    void readParams() override
    {
        xh_mono_defaults(&prm);
        fnVol = getParam("--vol");
        fnVol2 = getParam("--vol2");
        prm.minRes = getDoubleParam("--minRes");
        prm.maxRes = getDoubleParam("--maxRes");
        prm.freq_step = getDoubleParam("--step");
        fnMask = getParam("--mask");
        fnMaskExl = getParam("--maskExcl");
        prm.sampling = getDoubleParam("--sampling_rate");
        prm.significance = getDoubleParam("--significance");
        fnOut = getParam("-o");
        prm.gaussian = checkParam("--gaussian");
        prm.noise_only_in_halves = checkParam("--noiseonlyinhalves");
        nthrs = (int)getIntParam("--threads");
        if (checkParam("--dev")) device = parseGpuDevice(getParam("--dev"));
        // produceSideInfo :122-127, :162-163
        if (fnMask.empty()) REPORT_ERROR(ERR_ARG_MISSING, "Error: a mask ought to be provided");
        if (prm.freq_step < 0.25) prm.freq_step = 0.25;
    }

    void show() const
    {
        if (!verbose) return;
        std::cout << "vol: " << fnVol << std::endl
                  << "vol2: " << fnVol2 << std::endl
                  << "mask: " << fnMask << std::endl
                  << "maskExcl: " << fnMaskExl << std::endl
                  << "output folder: " << fnOut << std::endl
                  << "minRes: " << prm.minRes << std::endl
                  << "maxRes: " << prm.maxRes << std::endl
                  << "step: " << prm.freq_step << std::endl
                  << "sampling_rate: " << prm.sampling << std::endl
                  << "significance: " << prm.significance << std::endl
                  << "gaussian: " << prm.gaussian << std::endl
                  << "noiseonlyinhalves: " << prm.noise_only_in_halves << std::endl;
    }

    // Image<int>::read: the file's values truncated to int
    static void readInts(const std::string &fn, std::vector<int32_t> &v, const ImageInfo &ref, const char *what)
    {
        std::vector<float> f;
        ImageInfo I;
        readImage(fn, f, I);
        sameShape(I, ref, std::string(what) + " and input volume");
        v.resize(f.size());
        for (size_t i = 0; i < f.size(); ++i) v[i] = (int32_t)f[i];
    }

    void run() override
    {
        show();
        std::cout << "Starting..." << std::endl;
        std::vector<double> v1, v2;
        ImageInfo I1, I2;
        readDoubles(fnVol, v1, I1);
        const bool halves = !fnVol2.empty();
        if (halves) {
            readDoubles(fnVol2, v2, I2);
            sameShape(I1, I2, "Input volumes");
        }
        std::vector<int32_t> mask, excl;
        readInts(fnMask, mask, I1, "Mask");
        if (!fnMaskExl.empty()) readInts(fnMaskExl, excl, I1, "Exclusion mask");
        const size_t X = I1.x, Y = I1.y, Z = I1.z, N = X * Y * Z;

        xh_ctx *ctx = nullptr;
        xhCheck(xh_ctx_create_private(device, &ctx));
        XhOwner<xh_ctx> ctxOwner(ctx);
        xh_mono *h = nullptr;
        xhCheck(xh_mono_create(ctx, (int)Z, (int)Y, (int)X, &h));
        XhOwner<xh_mono> hOwner(h);
        DeviceBuffer dV1, dV2, dMask, dExcl, dMean, dRef, dChim, dRes;
        const size_t vb = sizeof(double) * N, mb = sizeof(int32_t) * N;
        dV1.upload(ctx, v1.data(), vb);
        if (halves) {
            dV2.upload(ctx, v2.data(), vb);
            dMean.reserve(ctx, vb);
        }
        dMask.upload(ctx, mask.data(), mb);
        if (!excl.empty()) {
            dExcl.upload(ctx, excl.data(), mb);
        }
        dRef.reserve(ctx, mb);
        dChim.reserve(ctx, vb);
        dRes.reserve(ctx, vb);
        std::vector<xh_mono_step> steps(4096);
        int32_t n = 0, stop = 0;
        xhCheck(xh_mono_run(h, dV1.as<double>(), halves ? dV2.as<double>() : nullptr, dMask.as<int32_t>(), excl.empty() ? nullptr : dExcl.as<int32_t>(), &prm,
                            steps.data(), (int32_t)steps.size(), &n, &stop, halves ? dMean.as<double>() : nullptr, dRef.as<int32_t>(), dChim.as<double>(),
                            dRes.as<double>()));
        int32_t radius = 0, radiuslimit = 0;
        xhCheck(xh_mono_info(h, &radius, &radiuslimit, nullptr, nullptr));
        std::cout << "                                     " << std::endl;
        std::cout << "The protein has a radius of " << radius << " px " << std::endl;
        std::cout << "There is no noise beyond a radius of " << radiuslimit << " px " << std::endl;
        std::cout << "Regions with a radius greater than " << radiuslimit << " px will not be considered" << std::endl;
        if ((double)radiuslimit <= (double)radius)
            std::cout << "Warning: the boxsize is very close to the protein size please provide a greater box" << std::endl;
        std::cout << "Analyzing frequencies" << std::endl;
        for (int32_t k = 0; k < std::min<int32_t>(n, (int32_t)steps.size()); ++k) std::cout << "resolution = " << steps[k].resolution << std::endl;
        switch (stop) {
            case XH_MONO_STOP_MASK_DONE: std::cout << "Search of resolutions stopped due to mask has been completed" << std::endl; break;
            case XH_MONO_STOP_NO_POINTS:
                std::cout << "There are no points to compute inside the mask" << std::endl;
                std::cout << "If the number of computed frequencies is low, perhaps the provided"
                             "mask is not enough tight to the volume, in that case please try another mask" << std::endl;
                break;
            case XH_MONO_STOP_LOW_SIGNAL: std::cout << "Search of resolutions stopped due to too low signal" << std::endl; break;
            case XH_MONO_STOP_ZTEST: std::cout << "Search stopped due to z>Z (hypothesis test)" << std::endl; break;
            default: break;
        }
        std::vector<double> out(N);
        if (halves) {
            xhCheck(xh_memcpy_d2h(ctx, out.data(), dMean.p, vb));
            writeVolume(fnOut + "/meanMap.mrc", out.data(), X, Y, Z);
        }
        std::vector<int32_t> rm(N);
        xhCheck(xh_memcpy_d2h(ctx, rm.data(), dRef.p, mb));
        for (size_t i = 0; i < N; ++i) out[i] = (double)rm[i];
        writeVolume(fnOut + "/refinedMask.mrc", out.data(), X, Y, Z);
        xhCheck(xh_memcpy_d2h(ctx, out.data(), dChim.p, vb));
        writeVolume(fnOut + "/monoresResolutionChimera.mrc", out.data(), X, Y, Z);
        xhCheck(xh_memcpy_d2h(ctx, out.data(), dRes.p, vb));
        writeVolume(fnOut + "/monoresResolutionMap.mrc", out.data(), X, Y, Z);
    }
};

}  // namespace mc
#endif
