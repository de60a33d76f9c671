// volume_subtraction.h -- xmipp_volume_subtraction: ProgVolumeSubtraction (reconstruction/volume_subtraction.{h,cpp}) with the
// adjustment and the subtraction on the device behind the C ABI (xh_vsub_*). The options of defineParams (:35-84) with the reference's
// defaults, plus --dev. With --sub the intermediate volumes go to --saveV1 and --saveV2, whose empty defaults stand for
// volume1_filtered.mrc and volume2_adjusted.mrc as in readParams (:101-106). With --computeEnergy one line per iteration is printed; the
// reference forms the same values and prints nothing.
// Refused before any device is touched, each where the reference writes past an array or divides by zero: volumes or masks of
// different shapes, --radavg on a box whose radial bins overflow, lambda outside [0, 1], cutFreq outside [0, 0.5], a negative --iter or
// --sigma.
#ifndef XMIPP3_AMD_VOLUME_SUBTRACTION_H
#define XMIPP3_AMD_VOLUME_SUBTRACTION_H
#include "programs.h"

namespace mc {

class ProgVolumeSubtraction : public XmippProgram {
public:
    std::string fnVol1, fnVol2, fnOutVol, fnMask1, fnMask2, fnMaskSub, fnVol1F, fnVol2A;
    bool performSubtraction = false, radavg = false, computeE = false;
    int iter = 5, sigma = 3, device = 0;
    double cutFreq = 0, lambda = 1;

    void defineParams() override
    {
        addUsageLine("This program modifies a volume as much as possible in order to assimilate it to another one, without loosing the important information in it");
        addUsageLine("('adjustment process'). Then, the subtraction of the two volumes can be optionally calculated.");
        addParamsLine("--i1 <volume>            : Reference volume");
        addParamsLine("--i2 <volume>            : Volume to modify");
        addParamsLine("[-o <structure=\"\">]    : Volume 2 modified or volume difference. If no name is given, then output_volume.mrc");
        addParamsLine("[--sub]                  : Perform the subtraction of the volumes. Output will be the difference");
        addParamsLine("[--sigma <s=3>]          : Decay of the filter (sigma) to smooth the mask transition");
        addParamsLine("[--iter <n=5>]           : Number of iterations for the adjustment process");
        addParamsLine("[--mask1 <mask=\"\">]    : Mask for volume 1");
        addParamsLine("[--mask2 <mask=\"\">]    : Mask for volume 2");
        addParamsLine("[--maskSub <mask=\"\">]  : Mask for subtraction region");
        addParamsLine("[--cutFreq <f=0>]        : Filter both volumes with a filter which specified cutoff frequency (i.e. resolution inverse, <0.5)");
        addParamsLine("[--lambda <l=1>]         : Relaxation factor for Fourier Amplitude POCS, between 1 (full modification, recommended) and 0 (no modification)");
        addParamsLine("[--radavg]               : Match the radially averaged Fourier amplitudes instead of taking them directly from the reference volume");
        addParamsLine("[--computeEnergy]        : Compute the energy difference between each step and print one line per iteration");
        addParamsLine("[--saveV1 <structure=\"\">] : Save subtraction intermediate file (vol1 filtered) just when option --sub is passed");
        addParamsLine("[--saveV2 <structure=\"\">] : Save subtraction intermediate file (vol2 adjusted) just when option --sub is passed");
        addParamsLine("[--dev <id=0>]           : GPU device to use (one device only)");
    }

    void readParams() override
    {
        fnVol1 = getParam("--i1");
        fnVol2 = getParam("--i2");
        fnOutVol = getParam("-o");
        if (fnOutVol.empty()) fnOutVol = "output_volume.mrc";
        performSubtraction = checkParam("--sub");
        iter = (int)getIntParam("--iter");
        sigma = (int)getIntParam("--sigma");
        fnMask1 = getParam("--mask1");
        fnMask2 = getParam("--mask2");
        fnMaskSub = getParam("--maskSub");
        cutFreq = getDoubleParam("--cutFreq");
        lambda = getDoubleParam("--lambda");
        fnVol1F = getParam("--saveV1");
        if (fnVol1F.empty()) fnVol1F = "volume1_filtered.mrc";
        fnVol2A = getParam("--saveV2");
        if (fnVol2A.empty()) fnVol2A = "volume2_adjusted.mrc";
        radavg = checkParam("--radavg");
        computeE = checkParam("--computeEnergy");
        if (checkParam("--dev")) device = parseGpuDevice(getParam("--dev"));
        if (iter < 0) REPORT_ERROR(ERR_ARG_INCORRECT, "--iter " + std::to_string(iter) + ": a negative number of iterations");
        if (sigma < 0) REPORT_ERROR(ERR_ARG_INCORRECT, "--sigma " + std::to_string(sigma) + ": a negative sigma");
        if (!(lambda >= 0 && lambda <= 1)) REPORT_ERROR(ERR_ARG_INCORRECT, "--lambda " + std::to_string(lambda) + " is outside [0, 1]");
        if (!(cutFreq >= 0 && cutFreq <= 0.5)) REPORT_ERROR(ERR_ARG_INCORRECT, "--cutFreq " + std::to_string(cutFreq) + " is outside [0, 0.5]");
    }

    void show() const
    {
        if (!verbose) return;
        std::cout << "Input volume 1: " << fnVol1 << std::endl
                  << "Input volume 2: " << fnVol2 << std::endl
                  << "Input mask 1: " << fnMask1 << std::endl
                  << "Input mask 2: " << fnMask2 << std::endl
                  << "Input mask sub: " << fnMaskSub << std::endl
                  << "Sigma: " << sigma << std::endl
                  << "Iterations: " << iter << std::endl
                  << "Cutoff frequency: " << cutFreq << std::endl
                  << "Relaxation factor: " << lambda << std::endl
                  << "Match radial averages: " << radavg << std::endl
                  << "Subtraction: " << performSubtraction << std::endl
                  << "Save volume 1 filtered: " << fnVol1F << std::endl
                  << "Save volume 2 adjusted: " << fnVol2A << std::endl
                  << "Output: " << fnOutVol << std::endl;
    }

    void run() override
    {
        show();
        std::vector<double> V1, V, mask, maskSub;
        ImageInfo I1, I2, IM;
        readDoubles(fnVol1, V1, I1);
        readDoubles(fnVol2, V, I2);
        sameShape(I2, I1, "The volume to modify and the reference volume");
        // createMask :317-330: both masks or none
        const bool haveMask = !fnMask1.empty() && !fnMask2.empty();
        if (haveMask) {
            std::vector<double> m2;
            readDoubles(fnMask1, mask, IM);
            sameShape(IM, I1, "Mask 1 and the reference volume");
            readDoubles(fnMask2, m2, IM);
            sameShape(IM, I1, "Mask 2 and the reference volume");
            for (size_t n = 0; n < mask.size(); ++n) mask[n] *= m2[n];
        }
        if (performSubtraction && !fnMaskSub.empty()) {
            readDoubles(fnMaskSub, maskSub, IM);
            sameShape(IM, I1, "The subtraction mask and the reference volume");
        }
        const size_t X = I1.x, Y = I1.y, Z = I1.z, N = X * Y * Z;
        if (X < 2 || Y < 2 || Z < 2) REPORT_ERROR(ERR_MATRIX_DIM, "A box of " + std::to_string(X) + " x " + std::to_string(Y) + " x " + std::to_string(Z) + " is no volume");
        if (radavg) {
            int32_t nbins = 0, maxbin = 0;
            xhCheck(xh_vsub_radial_bins((int)Z, (int)Y, (int)X, &nbins, &maxbin));
            if (maxbin >= nbins)
                REPORT_ERROR(ERR_MATRIX_DIM, "--radavg on a " + std::to_string(Z) + " x " + std::to_string(Y) + " x " + std::to_string(X) + " box: the radial average's largest bin " +
                                                 std::to_string(maxbin) + " reaches its " + std::to_string(nbins) + " bins");
        }

        xh_ctx *ctx = nullptr;
        xhCheck(xh_ctx_create_private(device, &ctx));
        XhOwner<xh_ctx> ctxOwner(ctx);
        xh_vsub *h = nullptr;
        xhCheck(xh_vsub_create(ctx, (int)Z, (int)Y, (int)X, &h));
        XhOwner<xh_vsub> hOwner(h);
        const size_t vb = sizeof(double) * N;
        DeviceBuffer dV1, dV, dMask, dAdj, dSub, dV1F, dOut;
        dV1.upload(ctx, V1.data(), vb);
        dV.upload(ctx, V.data(), vb);
        if (haveMask) {
            dMask.upload(ctx, mask.data(), vb);
        }
        dAdj.reserve(ctx, vb);
        xhCheck(xh_vsub_set_reference(h, dV1.as<double>(), haveMask ? dMask.as<double>() : nullptr, radavg ? 1 : 0));
        std::vector<xh_vsub_energy> energies(computeE ? (size_t)iter : 0);
        xhCheck(xh_vsub_adjust(h, dV.as<double>(), iter, lambda, radavg ? 1 : 0, cutFreq, computeE && iter > 0 ? energies.data() : nullptr, dAdj.as<double>()));
        for (size_t n = 0; n < energies.size(); ++n) {
            const xh_vsub_energy &e = energies[n];
            std::cout << "Energy iteration " << n << ": amplitude " << e.amplitude << " minmax " << e.minmax << " mask " << e.mask << " phase " << e.phase << " nonnegative "
                      << e.nonneg << " scale " << e.scale;
            if (cutFreq != 0) std::cout << " filter " << e.filter;
            std::cout << std::endl;
        }
        std::vector<double> out(N);
        if (!performSubtraction) {
            xhCheck(xh_memcpy_d2h(ctx, out.data(), dAdj.p, vb));
            writeVolume(fnOutVol, out.data(), X, Y, Z);
            return;
        }
        // getSubtractionMask :347-357
        dSub.reserve(ctx, vb);
        if (!fnMaskSub.empty()) xhCheck(xh_memcpy_h2d(ctx, dSub.p, maskSub.data(), vb));
        else {
            if (!haveMask) mask.assign(N, 1.0);
            xhCheck(xh_memcpy_h2d(ctx, dSub.p, mask.data(), vb));
            xhCheck(xh_vsub_smooth_mask(h, dSub.as<double>(), (double)sigma, dSub.as<double>()));
        }
        // :445-446: V1 as read, not the masked one
        dV1F.reserve(ctx, vb);
        dOut.reserve(ctx, vb);
        xhCheck(xh_vsub_subtract(h, dV1.as<double>(), dAdj.as<double>(), dSub.as<double>(), cutFreq, dV1F.as<double>(), dOut.as<double>()));
        xhCheck(xh_memcpy_d2h(ctx, out.data(), dV1F.p, vb));
        writeVolume(fnVol1F, out.data(), X, Y, Z);
        xhCheck(xh_memcpy_d2h(ctx, out.data(), dAdj.p, vb));
        writeVolume(fnVol2A, out.data(), X, Y, Z);
        xhCheck(xh_memcpy_d2h(ctx, out.data(), dOut.p, vb));
        writeVolume(fnOutVol, out.data(), X, Y, Z);
    }
};

}  // namespace mc
#endif
