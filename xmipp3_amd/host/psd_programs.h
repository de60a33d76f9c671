// psd_programs.h -- the two programs that estimate the power spectrum of a micrograph, with the pieces on the device behind the C ABI
// (xh_psd_*):
//   xmipp_ctf_estimate_from_micrograph   ProgCTFEstimateFromMicrograph (reconstruction/ctf_estimate_from_micrograph.cpp): the option set
//       of defineParams (:91-141) with the ARMA and CTF fit options it pulls in, so that existing command lines parse; run() :289-584 up
//       to the PSD. The "+" that marks expert options is not part of their names.
//   xmipp_psd_estimate                   PSDEstimatorProgram (applications/programs/psd_estimate/psd_estimate_main.cpp) and
//       PSDEstimator<float>::estimatePSD (reconstruction/psd_estimator.cpp:74-148); its normalisation (:123-141) runs here on the host,
//       on the one patch-sized result.
// Refused before any device is opened, each with its reason: a run without --dont_estimate_ctf (the CTF fit is not built yet),
// --psd_estimator ARMA, --bootstrapFit, --Nsubpiece other than 1 (that branch normalises the large piece instead of the small one and needs
// xmippCore's scaleToSize), a micrograph smaller than a piece, a piece side outside 2 .. 1024, a mode and --skipBorders that leave no piece
// (the reference divides by zero), regions mode with fewer than 2 skipBorders + 1 divisions (the reference's own error), a particle nearer
// than pieceDim / 2 to the left or top edge (the reference's unsigned subtraction wraps), a micrograph stack outside micrograph mode,
// several devices; for xmipp_psd_estimate a patch larger than the micrograph and an overlap outside [0, 1).
// Outputs: <oroot>.psd in micrograph mode; <oroot>.psdstk in the other modes with piece N at 1-based slot N and zero images in the skipped
// slots (xmippCore's stack extension on write, unpinned); in particles mode the psd column goes back into the position file. Image files
// hold 32-bit floats, as Image<double>::write stores them.
// reject_outliers and statisticsAdjust are xmippCore code outside the reference tree: INTEGRATION.md states the reading used.
#ifndef XMIPP3_AMD_PSD_PROGRAMS_H
#define XMIPP3_AMD_PSD_PROGRAMS_H
#include "programs.h"
#include <limits>

namespace mc {

// xmippCore's reject_outliers(v, 0.25): a 200-bin histogram between the extremes, the values clamped to its percentiles 0.125 and 99.875,
// a percentile interpolated linearly inside its bin
inline void psdRejectOutliers(std::vector<float> &v, double percentil_out = 0.25, int steps = 200)
{
    if (v.empty()) return;
    double hmin = v[0], hmax = v[0];
    for (float x : v) { hmin = std::min(hmin, (double)x); hmax = std::max(hmax, (double)x); }
    if (hmax == hmin) return;
    const double step = (hmax - hmin) / steps, istep = 1.0 / step;
    std::vector<double> hist((size_t)steps, 0.);
    for (float x : v) hist[(size_t)std::min<long>((long)(((double)x - hmin) * istep), steps - 1)] += 1;
    double total = 0;
    for (double c : hist) total += c;
    auto percentil = [&](double mass) {
        const double required = total * mass / 100.0;
        double acc = 0;
        int i = 0;
        while (acc < required) acc += hist[(size_t)i++];
        --i;
        if (i < 0) return hmin;
        return hmin + (i + (required - (acc - hist[(size_t)i])) / hist[(size_t)i]) * step;
    };
    const double lo = percentil(percentil_out / 2), hi = percentil(100 - percentil_out / 2);
    for (float &x : v) {
        if ((double)x < lo) x = (float)lo;
        else if ((double)x > hi) x = (float)hi;
    }
}

// psd_estimator.cpp:123-141
inline void psdNormalize(std::vector<float> &psd)
{
    float min_val = std::numeric_limits<float>::max();
    for (float p : psd)
        if (p > 0 && p < min_val) min_val = p;
    min_val = (float)(10 * std::log10((double)min_val));
    for (float &p : psd) p = p > 0 ? (float)(10 * std::log10((double)p)) : min_val;
    psdRejectOutliers(psd);
}

inline int psdSingleDevice(const std::string &dev)
{
    if (dev.find(',') != std::string::npos) REPORT_ERROR(ERR_ARG_INCORRECT, "--device " + dev + ": this program runs on one device");
    return parseGpuDevice(dev);
}

class ProgCTFEstimateFromMicrograph : public XmippProgram {
public:
    std::string fn_micrograph, fn_root, fn_pos, mode;
    int pieceDim = 512, skipBorders = 2, Nsubpiece = 1, device = 0;
    double overlap = 0.5;

    void defineParams() override
    {
        addUsageLine("Estimate the CTF from a micrograph.");
        addUsageLine("The PSD of the micrograph is first estimated using periodogram averaging. ");
        addUsageLine("Only the PSD stage is built: --dont_estimate_ctf is required.");
        addParamsLine("   --micrograph <file>         : File with the micrograph");
        addParamsLine("  [--oroot <rootname=\"\">]    : Rootname for output");
        addParamsLine("                               : If not given, the micrograph without extensions is taken");
        addParamsLine("                               : rootname.psd or .psdstk contains the PSD or PSDs");
        addParamsLine("  [--psd_estimator <method=periodogram>] : Method for estimating the PSD (periodogram; ARMA is refused)");
        addParamsLine("  [--pieceDim <d=512>]       : Size of the piece");
        addParamsLine("  [--overlap <o=0.5>]        : Overlap (0=no overlap, 1=full overlap)");
        addParamsLine("  [--skipBorders <s=2>]      : Number of pieces around the border to skip");
        addParamsLine("  [--Nsubpiece <N=1>]        : Each piece is further subdivided into NxN subpieces (only 1)");
        addParamsLine("  [--mode <mode=micrograph> <file=\"\">]  : How many PSDs are to be estimated: micrograph, regions <file>, particles <file>");
        addParamsLine("  [--dont_estimate_ctf]       : Do not fit a CTF to PSDs");
        addParamsLine("  [--acceleration1D]          : Accelerate PSD estimation");
        // accepted so that existing command lines parse: ARMA_parameters, ProgCTFEstimateFromPSD, ProgCTFBasicParams, CTFDescription
        for (const char *o : {"--N_AR <N=24>", "--M_AR <N=24>", "--N_MA <N=20>", "--M_MA <N=20>", "--downSamplingPerformed <F=1>", "--min_freq <fmin=0.03>",
                              "--max_freq <fmax=0.35>", "--fastDefocus <lambda=2> <size=10>", "--noDefocus", "--defocus_range <D=8000>",
                              "--refine_amplitude_contrast", "--show_optimization", "--radial_noise", "--enhance_weight <w=1>", "--model_simplification <s=0>",
                              "--bootstrapFit <N=-1>", "--ctfmodelSize <size=256>", "--enhance_min_freq <f1=0>", "--enhance_max_freq <f2=0>", "--selfEstimation",
                              "--ctf_similar_to <ctfFile=\"\">", "--sampling_rate <Tm=1>", "--voltage <kV=100>", "--spherical_aberration <Cs=0>",
                              "--defocusU <Defocus=0>", "--defocusV <DeltafV=0>", "--azimuthal_angle <ang=0>", "--chromatic_aberration <Ca=0>", "--energy_loss <espr=0>",
                              "--lens_stability <ispr=0>", "--convergence_cone <alpha=0>", "--longitudinal_displace <DeltaF=0>", "--transversal_displace <DeltaR=0>",
                              "--Q0 <Q0=0>", "--K <K=0>", "--phase_shift <phase_shift=0>", "--VPP_radius <VPP_radius=0>"})
            addParamsLine(std::string("  [") + o + "] : CTF fit option, accepted and unused");
        addParamsLine("  [--device <id=0>]           : HIP device (one device only)");
        addExampleLine("xmipp_ctf_estimate_from_micrograph --micrograph micrograph.mrc --dont_estimate_ctf");
    }

    void readParams() override
    {
        // :43-89
        fn_micrograph = getParam("--micrograph");
        fn_root = getParam("--oroot");
        if (fn_root == "") fn_root = FileName(fn_micrograph).removeAllExtensions();
        pieceDim = (int)getIntParam("--pieceDim");
        skipBorders = (int)getIntParam("--skipBorders");
        overlap = getDoubleParam("--overlap");
        Nsubpiece = (int)getIntParam("--Nsubpiece");
        mode = getParam("--mode");
        fn_pos = getParam("--mode", 1);
        device = psdSingleDevice(getParam("--device"));
        if (getParam("--psd_estimator") == "ARMA") REPORT_ERROR(ERR_NOT_IMPLEMENTED, "--psd_estimator ARMA: only the periodogram is built");
        if (getParam("--psd_estimator") != "periodogram") REPORT_ERROR(ERR_ARG_INCORRECT, "--psd_estimator " + getParam("--psd_estimator") + ": periodogram is expected");
        if (!checkParam("--dont_estimate_ctf"))
            REPORT_ERROR(ERR_NOT_IMPLEMENTED, "the CTF fit is not built yet: run with --dont_estimate_ctf, which writes the PSD");
        if (getIntParam("--bootstrapFit") != -1) REPORT_ERROR(ERR_NOT_IMPLEMENTED, "--bootstrapFit belongs to the CTF fit, which is not built yet");
        if (Nsubpiece != 1)
            REPORT_ERROR(ERR_NOT_IMPLEMENTED, "--Nsubpiece " + std::to_string(Nsubpiece) + ": only 1 is built (the reference's other branch normalises the large piece "
                                              "instead of the small one and needs xmippCore's scaleToSize)");
        if (mode != "micrograph" && mode != "regions" && mode != "particles") REPORT_ERROR(ERR_ARG_INCORRECT, "--mode " + mode + ": micrograph, regions or particles");
        if (mode == "particles" && fn_pos == "") REPORT_ERROR(ERR_ARG_MISSING, "--mode particles needs the file with the positions");
        if (pieceDim < 2 || pieceDim > 1024) REPORT_ERROR(ERR_ARG_INCORRECT, "--pieceDim " + std::to_string(pieceDim) + ": piece sides of 2 .. 1024 are supported");
        if (!(overlap >= 0 && overlap < 1)) REPORT_ERROR(ERR_ARG_INCORRECT, "--overlap " + getParam("--overlap") + ": 0 <= overlap < 1 is expected");
        if (skipBorders < 0) REPORT_ERROR(ERR_ARG_INCORRECT, "--skipBorders " + std::to_string(skipBorders));
    }

    void run() override
    {
        const int m = mode == "micrograph" ? 0 : mode == "regions" ? 1 : 2;
        MetaDataVec posFile;
        std::vector<int64_t> pos;
        if (m == 2) {
            posFile.read(fn_pos);
            if (!posFile.containsLabel("xcoor") || !posFile.containsLabel("ycoor")) REPORT_ERROR(ERR_MD_MISSINGLABEL, fn_pos + " has no xcoor / ycoor columns");
            for (size_t r = 0; r < posFile.size(); ++r) {
                long x = 0, y = 0;
                posFile.getValue("xcoor", x, r);
                posFile.getValue("ycoor", y, r);
                pos.push_back(x);
                pos.push_back(y);
            }
        }
        const ImageInfo I = readInfo(fn_micrograph);
        const size_t Ndim = I.isStack ? I.n : 1;
        if (I.z != 1 && !I.isStack) REPORT_ERROR(ERR_MATRIX_DIM, fn_micrograph + " is a volume");
        if (Ndim > 1 && m != 0) REPORT_ERROR(ERR_ARG_INCORRECT, "a stack of " + std::to_string(Ndim) + " micrographs is taken in --mode micrograph only");
        if ((size_t)pieceDim > I.x || (size_t)pieceDim > I.y)
            REPORT_ERROR(ERR_MATRIX_DIM, "the micrograph of " + std::to_string(I.y) + " x " + std::to_string(I.x) + " is smaller than a piece of " + std::to_string(pieceDim));
        // the piece list: every refusal of it comes from the library's host-only call, before a device is opened
        int32_t n = 0, div = 0;
        const int64_t *pp = pos.empty() ? nullptr : pos.data();
        xhCheck(xh_psd_pieces((int)I.y, (int)I.x, pieceDim, overlap, skipBorders, m, pp, (int)(pos.size() / 2), nullptr, nullptr, 0, &n, &div));
        std::vector<int32_t> corners(2 * (size_t)n), slots((size_t)n);
        xhCheck(xh_psd_pieces((int)I.y, (int)I.x, pieceDim, overlap, skipBorders, m, pp, (int)(pos.size() / 2), corners.data(), slots.data(), n, &n, &div));

        const std::string fn_psd = fn_root + (m == 0 ? ".psd" : ".psdstk");
        std::remove(fn_psd.c_str());
        std::remove((fn_root + ".ctfparam").c_str());
        if (verbose) std::cerr << "Computing models of each piece ...\n";

        xh_ctx *ctx = nullptr;
        xhCheck(xh_ctx_create_private(device, &ctx));
        XhOwner<xh_ctx> ctxOwner(ctx);
        const size_t PP = (size_t)pieceDim * pieceDim;
        const int capacity = (int)std::max<size_t>(1, std::min<size_t>({(size_t)n, (size_t)256, ((size_t)1 << 28) / (PP * 16)}));
        xh_psd *h = nullptr;
        xhCheck(xh_psd_create(ctx, (int)I.y, (int)I.x, pieceDim, pieceDim, capacity, 1, &h));
        XhOwner<xh_psd> hOwner(h);
        std::vector<float> mic;
        ImageInfo J;
        std::vector<double> stack;
        if (m != 0) stack.resize(PP * (size_t)n);
        for (size_t nIm = 1; nIm <= Ndim; ++nIm) {
            readImage(I.isStack ? std::to_string(nIm) + "@" + fn_micrograph : fn_micrograph, mic, J);
            std::cout << "Micrograph number: " << nIm << std::endl;
            xhCheck(xh_psd_load(h, mic.data()));
            xhCheck(xh_psd_add(h, corners.data(), n, 3, m == 0 ? nullptr : stack.data()));
        }
        if (m == 0) {
            std::vector<double> avg(PP), sd(PP);
            int64_t added = 0;
            xhCheck(xh_psd_result(h, avg.data(), sd.data(), &added));
            writeVolume(fn_psd, avg.data(), pieceDim, pieceDim, 1);
            return;
        }
        // piece N goes to slot N of the stack; the slots of skipped pieces are zero images
        std::vector<float> out(PP * (size_t)slots.back(), 0.f);
        for (int k = 0; k < n; ++k)
            for (size_t e = 0; e < PP; ++e) out[(size_t)(slots[k] - 1) * PP + e] = (float)stack[(size_t)k * PP + e];
        writeStack(fn_psd, out.data(), pieceDim, pieceDim, (size_t)slots.back());
        if (m == 2) {
            for (int k = 0; k < n; ++k) {
                char b[32];
                snprintf(b, sizeof(b), "%06d@", slots[k]);
                posFile.setValue("psd", std::string(b) + fn_psd, (size_t)k);
            }
            posFile.write(fn_pos);
        }
    }
};

class ProgPSDEstimate : public XmippProgram {
public:
    std::string fn_in, fn_out;
    float overlap = 0.4f;
    int px = 384, py = 384, device = 0;
    bool normalize = true;

    void defineParams() override
    {
        addUsageLine("Estimate the PSD of a micrograph as the sum of the amplitudes of overlapping patches.");
        addParamsLine("-i <input_file>             : Micrograph to be analyzed");
        addParamsLine("-o <output_file>            : PSD to be stored");
        addParamsLine("[--overlap <o=0.4>]         : overlap of the patches");
        addParamsLine("[--patches <x=384> <y=384>] :  size of the patches");
        addParamsLine("[--threads <t=4>]           : for FFT (accepted and ignored: the transforms run on the device)");
        addParamsLine("[--skipNormalization]       : if not present, FFT will be centered, and log_10 applied");
        addParamsLine("[--device <id=0>]           : HIP device (one device only)");
    }

    void readParams() override
    {
        fn_in = getParam("-i");
        fn_out = getParam("-o");
        overlap = (float)getDoubleParam("--overlap");
        px = (int)getIntParam("--patches", 0);
        py = (int)getIntParam("--patches", 1);
        (void)getIntParam("--threads");
        normalize = !checkParam("--skipNormalization");
        device = psdSingleDevice(getParam("--device"));
        if (!(overlap >= 0.f && overlap < 1.f)) REPORT_ERROR(ERR_ARG_INCORRECT, "--overlap " + getParam("--overlap") + ": 0 <= overlap < 1 is expected");
        if (px < 2 || px > 1024 || py < 2 || py > 1024)
            REPORT_ERROR(ERR_ARG_INCORRECT, "--patches " + std::to_string(px) + " " + std::to_string(py) + ": patch sides of 2 .. 1024 are supported");
    }

    void run() override
    {
        std::vector<float> mic;
        ImageInfo I;
        readImage(fn_in, mic, I);
        if ((size_t)px > I.x || (size_t)py > I.y)
            REPORT_ERROR(ERR_MATRIX_DIM, "the patch of " + std::to_string(py) + " x " + std::to_string(px) + " is larger than the micrograph of " + std::to_string(I.y) + " x " + std::to_string(I.x));
        int32_t n = 0;
        xhCheck(xh_psd_patches((int)I.y, (int)I.x, py, px, 0, 0, overlap, nullptr, 0, &n));
        std::vector<int32_t> corners(2 * (size_t)n);
        xhCheck(xh_psd_patches((int)I.y, (int)I.x, py, px, 0, 0, overlap, corners.data(), n, &n));
        xh_ctx *ctx = nullptr;
        xhCheck(xh_ctx_create_private(device, &ctx));
        XhOwner<xh_ctx> ctxOwner(ctx);
        const size_t PP = (size_t)py * px;
        const int capacity = (int)std::max<size_t>(1, std::min<size_t>({(size_t)n, (size_t)256, ((size_t)1 << 28) / (PP * 8)}));
        xh_psd *h = nullptr;
        xhCheck(xh_psd_create(ctx, (int)I.y, (int)I.x, py, px, capacity, 0, &h));
        XhOwner<xh_psd> hOwner(h);
        xhCheck(xh_psd_load(h, mic.data()));
        xhCheck(xh_psd_add(h, corners.data(), n, 1, nullptr));
        std::vector<float> psd(PP);
        xhCheck(xh_psd_result(h, psd.data(), nullptr, nullptr));
        if (normalize) psdNormalize(psd);
        std::vector<double> out(psd.begin(), psd.end());
        writeVolume(fn_out, out.data(), px, py, 1);
    }
};

}  // namespace mc
#endif
