// resolution_fso.h -- xmipp_resolution_fso, the Fourier Shell Occupancy: ProgFSO (reconstruction/resolution_fso.{h,cpp}) with the sweep
// over the Fourier coefficients on the device behind the C ABI (xh_fso_*). The options of defineParams (:74-87) plus --dev; --threads is
// accepted and unused. Everything that is O(directions x shells) is done on the host with one thread, as the reference does it
// (xh_fso_decide, xh_fso_resolution_distribution: host-only functions of the library, so that the Python class takes the same decisions).
// Files, all in the output folder: GlobalFSC.xmd (:323-343), fso.xmd (:1035-1053), Resolution_Distribution.xmd (:1194-1261); with
// --threedfsc_filter also threeD_FSC.mrc (:1542-1544), 3dFSC.mrc (:1556-1557) and filteredHalfMap{1,2}.mrc (:1187-1190).
// Labels: resolutionFreqFourier, resolutionFRC, resolutionFreqReal, angleRot and angleTilt as the resolution_fsc writer and SURVEY.md
// Appendix B have them; resolutionFSO and resolutionAnisotropy (MDL_RESOLUTION_FSO, MDL_RESOLUTION_ANISOTROPY) are parity unpinned.
// The 321 directions come from xh_fso_directions (the reference's table is the same set to 5.3e-4 degrees).
// Deviations:
//  - the reference writes threeD_FSC.mrc to the working directory; here it goes to the output folder;
//  - the device sums in fp64, where the reference's float den1 den2 (:468) can overflow on un-normalised spectra;
//  - directionalFilterHalves multiplies both spectra by 1 (:1130-1131) between a forward and an inverse transform: the filtered half maps
//    are the masked half maps, and those are written.
// Refused: an empty -o (the reference would write to /), half maps or a mask of different shapes, --anglecone outside (0, 90), X < 8 (and
// what xh_fso_create refuses), --threedfsc_filter with a box that is not cubic (createFullFourier passes (X, Y, Z) to a (Z, Y, X) resize).
#ifndef XMIPP3_AMD_RESOLUTION_FSO_H
#define XMIPP3_AMD_RESOLUTION_FSO_H
#include "programs.h"
#include <filesystem>

namespace mc {

class ProgFSO : public XmippProgram {
public:
    std::string fnhalf1, fnhalf2, fnmask, fnOut;
    double sampling = 1, ang_con = 17, thrs = 0.143;
    bool do_3dfsc_filter = false;
    int Nthreads = 1, device = 0;

    void defineParams() override
    {
        addUsageLine("Calculate Fourier Shell Occupancy - FSO curve - via directional FSC measurements.");
        addParamsLine("   --half1 <input_file>               : Input Half map 1");
        addParamsLine("   --half2 <input_file>               : Input Half map 2");
        addParamsLine("   [-o <output_folder=\"\">]          : Folder where the results will be stored.");
        addParamsLine("   [--sampling <Ts=1>]                : (Optical) Pixel size (Angstrom). If it is not provided by default will be 1 A/px.");
        addParamsLine("   [--mask <input_file=\"\">]         : (Optional) Smooth mask to remove noise. If it is not provided, the computation will be carried out without mask.");
        addParamsLine("   [--anglecone <ang_con=17>]         : (Optional) Angle Cone (angle between the axis and the  generatrix) for estimating the directional FSC");
        addParamsLine("   [--threshold <thrs=0.143>]         : (Optional) Threshold for the FSC/directionalFSC estimation ");
        addParamsLine("   [--threedfsc_filter]               : (Optional) Put this flag to estimate the 3DFSC, and apply it as low pass filter to obtain a directionally filtered map. It mean to apply an anisotropic filter.");
        addParamsLine("   [--threads <Nthreads=1>]           : (Optional) Number of threads to be used (accepted and unused: the sweep runs on the device)");
        addParamsLine("   [--dev <id=0>]                     : GPU device to use (one device only)");
    }

    void readParams() override
    {
        fnhalf1 = getParam("--half1");
        fnhalf2 = getParam("--half2");
        fnOut = getParam("-o");
        sampling = getDoubleParam("--sampling");
        fnmask = getParam("--mask");
        ang_con = getDoubleParam("--anglecone");
        thrs = getDoubleParam("--threshold");
        do_3dfsc_filter = checkParam("--threedfsc_filter");
        Nthreads = (int)getIntParam("--threads");
        if (checkParam("--dev")) device = parseGpuDevice(getParam("--dev"));
        if (fnOut.empty()) REPORT_ERROR(ERR_ARG_MISSING, "-o is empty: the results need an output folder");
        if (!(ang_con > 0 && ang_con < 90)) REPORT_ERROR(ERR_ARG_INCORRECT, "--anglecone " + std::to_string(ang_con) + ": the cone angle must lie inside (0, 90) degrees");
    }

    void show() const
    {
        if (!verbose) return;
        std::cout << "half1: " << fnhalf1 << std::endl
                  << "half2: " << fnhalf2 << std::endl
                  << "output: " << fnOut << std::endl
                  << "sampling: " << sampling << std::endl
                  << "mask: " << fnmask << std::endl
                  << "anglecone: " << ang_con << std::endl
                  << "threshold: " << thrs << std::endl
                  << "threedfsc_filter: " << (do_3dfsc_filter ? 1 : 0) << std::endl
                  << "threads: " << Nthreads << std::endl;
    }

    // fscInterpolation :352-374
    void fscInterpolation(const std::vector<double> &freq, const std::vector<double> &frc) const
    {
        for (size_t i = 0; i < freq.size(); ++i) {
            const double ff = frc[i];
            if (ff <= thrs && i > 2) {
                const double y1 = ff, x1 = freq[i], y2 = frc[i - 1], x2 = freq[i - 1];
                const double slope = (y2 - y1) / (x2 - x1);
                const double ny = y2 - slope * x2;
                const double fscResolution = (thrs - ny) / slope;
                std::cout << "Resolution " << 1 / fscResolution << std::endl;
                break;
            }
        }
    }

    void run() override
    {
        show();
        std::cout << "Starting ... " << std::endl << std::endl;
        std::vector<double> half1, half2, mask;
        ImageInfo I1, I2, IM;
        readDoubles(fnhalf1, half1, I1);
        readDoubles(fnhalf2, half2, I2);
        sameShape(I1, I2, "The half maps");
        if (!fnmask.empty()) {
            readDoubles(fnmask, mask, IM);
            sameShape(IM, I1, "The mask and the half maps");
        }
        const size_t X = I1.x, Y = I1.y, Z = I1.z, N = X * Y * Z, L = X / 2 + 1;
        if (X < 8 || Y < 8 || Z < 8) REPORT_ERROR(ERR_MATRIX_DIM, "A box of " + std::to_string(X) + " x " + std::to_string(Y) + " x " + std::to_string(Z) + ": sides below 8 are refused");
        if (do_3dfsc_filter && !(X == Y && Y == Z)) REPORT_ERROR(ERR_MATRIX_DIM, "--threedfsc_filter needs a cubic box");
        std::error_code ec;
        if (!std::filesystem::exists(fnOut) && !std::filesystem::create_directories(fnOut, ec)) REPORT_ERROR(ERR_IO_NOREAD, "cannot create " + fnOut);

        xh_ctx *ctx = nullptr;
        xhCheck(xh_ctx_create_private(device, &ctx));
        XhOwner<xh_ctx> ctxOwner(ctx);
        xh_fso *h = nullptr;
        xhCheck(xh_fso_create(ctx, (int)Z, (int)Y, (int)X, 0, &h));
        XhOwner<xh_fso> hOwner(h);
        const size_t vb = sizeof(double) * N;
        std::vector<double> gsums(3 * L);
        {
            DeviceBuffer d1, d2, dm;
            d1.upload(ctx, half1.data(), vb);
            d2.upload(ctx, half2.data(), vb);
            if (!mask.empty()) {
                dm.upload(ctx, mask.data(), vb);
            }
            xhCheck(xh_fso_load(h, d1.as<double>(), d2.as<double>(), mask.empty() ? nullptr : dm.as<double>(), gsums.data(), nullptr, nullptr));
        }

        // arrangeFSC_and_fscGlobal :323-346
        std::vector<double> freq(L), frc(L);
        {
            MetaDataVec mdRes;
            for (size_t i = 0; i < L; ++i) {
                frc[i] = gsums[3 * i] / sqrt(gsums[3 * i + 1] * gsums[3 * i + 2]);
                freq[i] = (float)i / (X * sampling);
                if (i > 0) {
                    const size_t id = mdRes.addObject();
                    mdRes.setValue("resolutionFreqFourier", freq[i], id);
                    mdRes.setValue("resolutionFRC", frc[i], id);
                    mdRes.setValue("resolutionFreqReal", 1. / freq[i], id);
                }
            }
            mdRes.write(fnOut + "/GlobalFSC.xmd");
            fscInterpolation(freq, frc);
        }

        // run :1343-1414
        int32_t ndir = 0;
        xhCheck(xh_fso_directions(3, nullptr, 0, &ndir));
        std::vector<float> angles(2 * (size_t)ndir), dirs(3 * (size_t)ndir);
        xhCheck(xh_fso_directions(3, angles.data(), ndir, &ndir));
        xhCheck(xh_fso_unit_vectors(angles.data(), ndir, dirs.data()));
        float cosAngle = 0, aux = 0;
        xhCheck(xh_fso_cone(ang_con, &cosAngle, &aux));
        std::vector<double> dsums(3 * L * (size_t)ndir), resDirFSC((size_t)ndir), isotropyMatrix(L);
        std::vector<int64_t> counts((size_t)ndir);
        xhCheck(xh_fso_directional(h, dirs.data(), ndir, cosAngle, aux, dsums.data(), counts.data()));
        std::vector<float> fsc(L * (size_t)ndir), aniParam(L);
        xhCheck(xh_fso_decide(dsums.data(), dirs.data(), ndir, (int)L, (int)X, sampling, thrs, fsc.data(), resDirFSC.data(), aniParam.data(), isotropyMatrix.data()));
        if (verbose)
            for (int k = 0; k < ndir; ++k) printf("Direction %d/%d -> %.2f A \n", k, ndir, resDirFSC[(size_t)k]);
        std::cout << "----- Directional resolution estimated -----" << std::endl << std::endl;
        std::cout << "Preparing results ..." << std::endl;

        {   // saveAnisotropyToMetadata :1035-1053
            MetaDataVec mdani;
            for (size_t i = 1; i < L; ++i) {
                const size_t id = mdani.addObject();
                mdani.setValue("resolutionFreqFourier", freq[i], id);
                mdani.setValue("resolutionFSO", (double)aniParam[i], id);
                mdani.setValue("resolutionFreqReal", 1.0 / freq[i], id);
                mdani.setValue("resolutionAnisotropy", xh_fso_incomplete_gamma(isotropyMatrix[i]), id);
            }
            mdani.write(fnOut + "/fso.xmd");
        }
        {   // resolutionDistribution :1194-1261
            std::vector<double> dist(360 * 91);
            xhCheck(xh_fso_resolution_distribution(dirs.data(), ndir, resDirFSC.data(), ang_con, dist.data()));
            MetaDataVec mdOut;
            for (int i = 0; i < 360; ++i)
                for (int j = 0; j < 91; ++j) {
                    const size_t id = mdOut.addObject();
                    mdOut.setValue("angleRot", (double)i, id);
                    mdOut.setValue("angleTilt", (double)j, id);
                    mdOut.setValue("resolutionFRC", dist[(size_t)i * 91 + j], id);
                }
            mdOut.write(fnOut + "/Resolution_Distribution.xmd");
        }

        if (do_3dfsc_filter) {   // run :1483-1558
            DeviceBuffer dHalf, dFull;
            const size_t hb = sizeof(double) * Z * Y * L;
            dHalf.reserve(ctx, hb);
            dFull.reserve(ctx, vb);
            xhCheck(xh_fso_threedfsc(h, dirs.data(), ndir, cosAngle, aux, fsc.data(), dHalf.as<double>(), dFull.as<double>()));
            std::vector<double> out(N);
            xhCheck(xh_memcpy_d2h(ctx, out.data(), dHalf.p, hb));
            writeVolume(fnOut + "/threeD_FSC.mrc", out.data(), L, Y, Z);
            xhCheck(xh_memcpy_d2h(ctx, out.data(), dFull.p, vb));
            writeVolume(fnOut + "/3dFSC.mrc", out.data(), X, Y, Z);
            // directionalFilterHalves :1084-1192: both spectra times 1
            if (!mask.empty())
                for (size_t n = 0; n < N; ++n) { half1[n] *= mask[n]; half2[n] *= mask[n]; }
            writeVolume(fnOut + "/filteredHalfMap1.mrc", half1.data(), X, Y, Z);
            writeVolume(fnOut + "/filteredHalfMap2.mrc", half2.data(), X, Y, Z);
        }
        std::cout << "-------------Finished-------------" << std::endl;
    }
};

}  // namespace mc
#endif
