// volume_align.h -- xmipp_volume_align: ProgAlignVolumes (reconstruction/volume_align_prog.cpp) with the fitness of every trial on the
// device behind the C ABI (xh_valign_*). The option lines, defaults, messages and output text of volume_align_prog.cpp:154-195 and
// :499-575, plus --device. The exhaustive search enumerates its trials on the host with the reference's ten loops (xh_valign_trials) and
// hands the list to xh_valign_search in that order; --local runs the reference's Powell search over nine variables, the two mirror
// searches in lockstep (xh_powell_minimize_batch), each cost call one xh_valign_fit of the live rows.
// Masks: --mask circular <R> and --mask binary_file <file> with --center, as volume_halves_restoration.h reads them.
// Refused before any device is touched, each with a message naming the option:
//  - --frm: it calls the external Python package sh_alignment, which is not part of this project;
//  - every other mask type; a mask of another shape, or one that selects no voxel;
//  - --i1 / --i2 of different shapes; sides above 1024 (or below 2); several devices;
//  - --grey_scale / --grey_shift without --least_squares (the reference's `requires` lines);
//  - an exhaustive search of more than kMaxTrials trials: the list is materialised on the host, 80 bytes a trial and 8 for its fit, and
//    2^21 trials are 185 MB; the reference's typical global search is 7 800. Split the ranges.
// Not pinned: `std::cout << trial` under --show_fit prints a Matrix1D through xmippCore's operator<<, which is not in the reference tree;
// here the ten values follow each other on one line, separated by spaces, in the stream's default formatting.
#ifndef XMIPP3_AMD_VOLUME_ALIGN_H
#define XMIPP3_AMD_VOLUME_ALIGN_H
#include "programs.h"

namespace mc {

class ProgAlignVolumes : public XmippProgram {
public:
    static constexpr int64_t kMaxTrials = (int64_t)1 << 21;
    static constexpr int kCapacity = 256;              // trials of one launch; no result depends on it
    enum { COVARIANCE = 1, LEAST_SQUARES = 2 };

    std::string fn1, fn2, fnOut, fnGeo, fnGray, fnStore;
    // grey_scale, grey_shift, rot, tilt, psi, scale, z, y, x: first, last, step (the order of xh_valign_trials)
    double ranges[9][3] = {};
    bool consider_mirror = false, tell = false, apply = false, usePowell = false, onlyShift = false, useFRM = false, copyGeo = false, copyGray = false,
         store = false, wrap = true, dontScale = false, useMask = false;
    int alignment_method = COVARIANCE, device = 0;
    std::string maskType, maskArg;
    double R1 = 0, x0c = 0, y0c = 0, z0c = 0;

    void defineParams() override
    {
        addUsageLine("Align two volumes varying orientation, position and scale");
        addParamsLine("   --i1 <volume1>        : the first volume to align");
        addParamsLine("   --i2 <volume2>        : the second one");
        addParamsLine("  [--rot   <rot0=0>  <rotF=0>  <step_rot=1>]  : in degrees");
        addParamsLine("  [--tilt  <tilt0=0> <tiltF=0> <step_tilt=1>] : in degrees");
        addParamsLine("  [--psi   <psi0=0>  <psiF=0>  <step_psi=1>]  : in degrees");
        addParamsLine("  [--scale <sc0=1>   <scF=1>   <step_sc=1>]   : size scale margin");
        addParamsLine("  [--grey_scale <sc0=1> <scF=1> <step_sc=1>]  : grey scale margin");
        addParamsLine("    requires --least_squares;");
        addParamsLine("  [--grey_shift <sh0=0> <shF=0> <step_sh=1>]  : grey shift margin");
        addParamsLine("    requires --least_squares;");
        addParamsLine("  [-z <z0=0> <zF=0> <step_z=1>] : Z position in pixels");
        addParamsLine("  [-y <y0=0> <yF=0> <step_y=1>] : Y position in pixels");
        addParamsLine("  [-x <x0=0> <xF=0> <step_x=1>] : X position in pixels");
        addParamsLine("  [--consider_mirror] : Consider the mirror volume");
        addParamsLine("  [--show_fit]      : Show fitness values");
        addParamsLine("  [--apply <file=\"\">] : Apply best movement to --i2 and store results in this file");
        addParamsLine("  [--covariance]    : Covariance fitness criterion");
        addParamsLine("  [--least_squares] : LS fitness criterion");
        addParamsLine("  [--local]         : Use local optimizer instead of exhaustive search");
        addParamsLine("  [--frm <maxFreq=0.25> <maxShift=10> <tilt0=-90> <tiltF=90>] : Use Fast Rotational Matching, if tilt0 and tiltF are left as -90 and 90 they do not effect the results of the alignment");
        addParamsLine("                    : Maximum frequency is in digital frequencies (<0.5)");
        addParamsLine("                    : Maximum shift is in pixels");
        addParamsLine("                    :+ See Y. Chen, et al. Fast and accurate reference-free alignment of subtomograms. JSB, 182: 235-245 (2013)");
        addParamsLine("  [--onlyShift]     : Only shift");
        addParamsLine("  [--dontScale]     : Do not look for scale changes");
        addParamsLine("  [--copyGeo <file=\"\">] : copy transformation matrix in a txt file. ('A' matrix elements)");
        addParamsLine("  [--copyGray <file=\"\">] : copy gray scale and shift txt file.)");
        addParamsLine("  [--store <file=\"\">] : copy angles and shifts to a txt file.");
        addParamsLine("  [--dontWrap] : Do not wrap input2 when aligning to input1");
        addParamsLine(" == Mask Options == ");
        // Mask::defineParams(this, INT_MASK), the two supported types
        addParamsLine("  [--mask <mask_type=circular> <arg=\"\">] : binary_file <file> or circular <R> (R < 0: inside, R > 0: outside); other types are refused");
        addParamsLine("  [--center <x0=0> <y0=0> <z0=0>]: mask center");
        addParamsLine("  [--device <id=0>]     : HIP device (one device only)");
        addExampleLine("Typically you first look for a rough approximation of the alignment using exhaustive search. For instance, for a global rotational alignment use", false);
        addExampleLine("xmipp_volume_align --i1 volume1.vol --i2 volume2.vol --rot 0 360 15 --tilt 0 180 15 --psi 0 360 15");
        addExampleLine("Then, assume the best alignment is obtained for rot=45, tilt=60, psi=90", false);
        addExampleLine("Now you perform a local search to refine the estimation and apply", false);
        addExampleLine("xmipp_volume_align --i1 volume1.vol --i2 volume2.vol --rot 45 --tilt 60 --psi 90 --local --apply volume2aligned.vol");
        addSeeAlsoLine("xmipp_volumeset_align");
    }

    void readParams() override
    {
        fn1 = getParam("--i1");
        fn2 = getParam("--i2");
        static const char *opt[9] = {"--grey_scale", "--grey_shift", "--rot", "--tilt", "--psi", "--scale", "-z", "-y", "-x"};
        for (int a = 0; a < 9; ++a) {
            for (int c = 0; c < 3; ++c) ranges[a][c] = getDoubleParam(opt[a], c);
            if (ranges[a][2] == 0) ranges[a][2] = 1;
        }
        consider_mirror = checkParam("--consider_mirror");
        useMask = checkParam("--mask");
        if (useMask) readMaskParams();
        usePowell = checkParam("--local");
        useFRM = checkParam("--frm");
        onlyShift = checkParam("--onlyShift");
        wrap = !checkParam("--dontWrap");
        tell = checkParam("--show_fit");
        apply = checkParam("--apply");
        fnOut = getParam("--apply");
        copyGeo = checkParam("--copyGeo");
        copyGray = checkParam("--copyGray");
        fnGeo = getParam("--copyGeo");
        fnGray = getParam("--copyGray");
        store = checkParam("--store");
        fnStore = getParam("--store");
        dontScale = checkParam("--dontScale");
        alignment_method = checkParam("--covariance") ? COVARIANCE : (checkParam("--least_squares") ? LEAST_SQUARES : COVARIANCE);
        const std::string dev = getParam("--device");
        // refused before any device is touched
        if (dev.find(',') != std::string::npos) REPORT_ERROR(ERR_ARG_INCORRECT, "--device " + dev + ": this program runs on one device");
        device = parseGpuDevice(dev);
        if (useFRM)
            REPORT_ERROR(ERR_NOT_IMPLEMENTED, "--frm: Fast Rotational Matching calls the external Python package sh_alignment, which is not part of this project");
        for (const char *o : {"--grey_scale", "--grey_shift"})
            if (checkParam(o) && !checkParam("--least_squares")) REPORT_ERROR(ERR_ARG_MISSING, std::string(o) + " requires --least_squares");
    }

    void readMaskParams()
    {
        // Mask::readParams
        x0c = getDoubleParam("--center", 0);
        y0c = getDoubleParam("--center", 1);
        z0c = getDoubleParam("--center", 2);
        maskType = getParam("--mask");
        if (maskType == "circular") {
            R1 = getDoubleParam("--mask", 1);
            if (R1 == 0) REPORT_ERROR(ERR_ARG_INCORRECT, "MaskProgram: circular mask with radius 0");
        } else if (maskType == "binary_file") {
            maskArg = getParam("--mask", 1);
            if (maskArg.empty()) REPORT_ERROR(ERR_ARG_MISSING, "--mask binary_file needs a file name");
        } else
            REPORT_ERROR(ERR_NOT_IMPLEMENTED, "--mask " + maskType + ": only the binary_file and circular mask types are supported");
    }

    struct LocalCost {
        xh_valign *h;
        int method, wrap;
        std::vector<double> p;
        std::string error;
    };

    // rows of nine variables -> trials of ten (flip by the problem: 0 as it is, 1 the mirror) -> one xh_valign_fit
    static int32_t localCost(int32_t m, const int32_t *problem, const double *x, double *cost, void *user)
    {
        LocalCost *L = (LocalCost *)user;
        L->p.resize(10 * (size_t)m);
        for (int r = 0; r < m; ++r) {
            L->p[10 * (size_t)r] = problem[r] ? -1.0 : 1.0;
            std::copy_n(x + 9 * (size_t)r, 9, L->p.begin() + 10 * (size_t)r + 1);
        }
        if (xh_valign_fit(L->h, L->p.data(), m, L->method, L->wrap, cost) != XH_OK) {
            L->error = xh_last_error();
            return 1;
        }
        return 0;
    }

    static void printTrial(const double *p, double fit)
    {
        for (int c = 0; c < 10; ++c) std::cout << p[c] << " ";
        std::cout << fit << std::endl;
    }

    void run() override
    {
        // ---- everything that can be refused, from the headers and the options alone
        const ImageInfo I1 = readInfo(fn1), I2 = readInfo(fn2);
        if (I1.x != I2.x || I1.y != I2.y || I1.z != I2.z)
            REPORT_ERROR(ERR_MATRIX_DIM, "--i1 and --i2 have different dimensions (" + dims(I1) + " and " + dims(I2) + ")");
        const size_t X = I1.x, Y = I1.y, Z = I1.z, N = X * Y * Z;
        if (X < 2 || Y < 2 || Z < 2 || X > 1024 || Y > 1024 || Z > 1024)
            REPORT_ERROR(ERR_MATRIX_DIM, "--i1: a box of " + dims(I1) + " is not supported (2 .. 1024 a side)");
        std::vector<int32_t> mask;
        if (useMask) {
            mask.resize(N);
            if (maskType == "binary_file") {
                std::vector<float> f;
                ImageInfo IM;
                readImage(maskArg, f, IM);
                if (IM.x != X || IM.y != Y || IM.z != Z) REPORT_ERROR(ERR_MATRIX_DIM, "--mask " + maskArg + " is " + dims(IM) + ", the volumes " + dims(I1));
                xhCheck(xh_halves_binary_mask(f.data(), N, mask.data()));
            } else
                xhCheck(xh_halves_circular_mask((int)Z, (int)Y, (int)X, R1, x0c, y0c, z0c, mask.data()));
            if (std::all_of(mask.begin(), mask.end(), [](int32_t v) { return v == 0; })) REPORT_ERROR(ERR_VALUE_INCORRECT, "--mask selects no voxel");
        }
        std::vector<double> trials;
        int64_t ntrials = 0, times = 1;
        if (!usePowell) {
            if (xh_valign_trials(&ranges[0][0], consider_mirror ? 1 : 0, kMaxTrials, nullptr, &ntrials, &times) != XH_OK)
                REPORT_ERROR(ERR_ARG_INCORRECT, std::string("the search ranges (--rot .. -x): ") + xh_last_error() + "; at most " + std::to_string(kMaxTrials) +
                                                " trials are enumerated, split the ranges");
            trials.resize(10 * (size_t)ntrials);
            xhCheck(xh_valign_trials(&ranges[0][0], consider_mirror ? 1 : 0, kMaxTrials, trials.data(), &ntrials, nullptr));
        }

        // ---- the device
        std::vector<double> V1, V2;
        ImageInfo J;
        readDoubles(fn1, V1, J);
        readDoubles(fn2, V2, J);
        xh_ctx *ctx = nullptr;
        xhCheck(xh_ctx_create_private(device, &ctx));
        XhOwner<xh_ctx> ctxOwner(ctx);
        xh_valign *h = nullptr;
        xhCheck(xh_valign_create(ctx, (int)Z, (int)Y, (int)X, usePowell ? 2 : kCapacity, &h));
        XhOwner<xh_valign> hOwner(h);
        xhCheck(xh_valign_set_volumes(h, V1.data(), V2.data(), useMask ? mask.data() : nullptr));

        double best_fit = 1e38;
        double best_align[10] = {};
        bool first = true;
        if (!usePowell) {
            // :327-405. The progress bar's count is not the loops' trip count; both are kept
            if (!tell) init_progress_bar((size_t)times);
            else std::cout << "#grey_factor rot tilt psi scale z y x fitness\n";
            if (ntrials > 0) {
                int64_t idx = 0;
                std::vector<double> fits(tell ? (size_t)ntrials : 0);
                xhCheck(xh_valign_search(h, trials.data(), ntrials, alignment_method, wrap ? 1 : 0, &idx, &best_fit, tell ? fits.data() : nullptr));
                std::copy_n(trials.data() + 10 * (size_t)idx, 10, best_align);
                first = false;
                if (tell) {
                    double running = 0;
                    for (int64_t t = 0; t < ntrials; ++t) {
                        if (t == 0 || fits[t] < running) {
                            running = fits[t];
                            std::cout << "Best so far\n";
                        }
                        printTrial(trials.data() + 10 * (size_t)t, fits[t]);
                    }
                }
            }
            if (!tell) progress_bar((size_t)times);
        } else {
            // :406-446
            double steps9[9];
            for (double &s : steps9) s = 1;
            if (onlyShift) for (int c = 0; c < 6; ++c) steps9[c] = 0;
            if (alignment_method == COVARIANCE) steps9[0] = steps9[1] = 0;
            if (dontScale) steps9[5] = 0;
            const int nprob = consider_mirror ? 2 : 1;
            std::vector<double> x(9 * (size_t)nprob), st(9 * (size_t)nprob), fret((size_t)nprob);
            std::vector<int32_t> n((size_t)nprob, 9), iter((size_t)nprob);
            for (int q = 0; q < nprob; ++q)
                for (int c = 0; c < 9; ++c) {
                    x[9 * (size_t)q + c] = ranges[c][0];
                    st[9 * (size_t)q + c] = steps9[c];
                }
            LocalCost L{h, alignment_method, wrap ? 1 : 0, {}, ""};
            const int rc = xh_powell_minimize_batch(nprob, n.data(), 9, x.data(), st.data(), 0.01, nprob, &localCost, &L, fret.data(), iter.data(), nullptr);
            if (rc != XH_OK) REPORT_ERROR(ERR_GPU, "--local: " + (L.error.empty() ? std::string(xh_last_error()) : L.error));
            for (int mirror = 0; mirror < nprob; ++mirror) {
                if (fret[mirror] < best_fit || first) {
                    best_align[0] = mirror ? -1.0 : 1.0;
                    std::copy_n(x.data() + 9 * (size_t)mirror, 9, best_align + 1);
                    best_fit = fret[mirror];
                }
                first = false;
            }
        }

        // ---- the report (:499-575)
        if (!first)
            std::cout << "The best correlation is for\n"
                      << "Mirroring the in X axis: " << (best_align[0] < 0) << std::endl
                      << "Scale                  : " << best_align[6] << std::endl
                      << "Translation (X,Y,Z)    : " << best_align[9] << " " << best_align[8] << " " << best_align[7] << std::endl
                      << "Rotation (rot,tilt,psi): " << best_align[3] << " " << best_align[4] << " " << best_align[5] << std::endl
                      << "Best grey scale       : " << best_align[1] << std::endl
                      << "Best grey shift       : " << best_align[2] << std::endl
                      << "Fitness value         : " << best_fit << std::endl;
        // A = Euler (column 2 times flip) * translation (x, y, z as they are: no z = -z + 1 here) * scale. The Euler block comes from
        // xh_valign_matrix at scale 1; the products with the translation and scale matrices are written out with their zero terms left out
        const double pm[10] = {best_align[0], 1, 0, best_align[3], best_align[4], best_align[5], 1, 0, 0, 0};
        double M[16], Mi[16];
        int32_t ident = 0;
        xhCheck(xh_valign_matrix(pm, M, Mi, &ident));
        double A[4][4] = {};
        for (int i = 0; i < 3; ++i) {
            for (int j = 0; j < 3; ++j) A[i][j] = M[i * 4 + j] * best_align[6];
            A[i][3] = M[i * 4 + 0] * best_align[9] + M[i * 4 + 1] * best_align[8] + M[i * 4 + 2] * best_align[7];
        }
        A[3][3] = 1;
        if (verbose != 0)
            std::cout << "xmipp_transform_geometry will require the following values"
                      << "\n   Angles: " << best_align[3] << " " << best_align[4] << " " << best_align[5] << "\n   Shifts: " << A[0][3] << " " << A[1][3] << " " << A[2][3]
                      << std::endl;
        if (copyGeo) {
            std::ofstream outputGeo(fnGeo.c_str());
            for (int i = 0; i < 4; ++i)
                for (int j = 0; j < 4; ++j) outputGeo << A[i][j] << "\n";
            outputGeo << std::endl;
        }
        if (copyGray) {
            std::ofstream outputGray(fnGray.c_str());
            outputGray << best_align[1] << "\n" << best_align[2] << "\n" << std::endl;
        }
        if (store) {
            std::ofstream outputStore(fnStore.c_str());
            outputStore << best_align[3] << ", " << best_align[4] << ", " << best_align[5] << ", " << A[0][3] << ", " << A[1][3] << ", " << A[2][3] << ", " << best_fit
                        << std::endl;
        }
        if (apply) {
            DeviceBuffer dOut;
            dOut.reserve(ctx, sizeof(double) * N);
            xhCheck(xh_valign_apply(h, best_align, wrap ? 1 : 0, dOut.as<double>()));
            std::vector<double> out(N);
            xhCheck(xh_memcpy_d2h(ctx, out.data(), dOut.p, sizeof(double) * N));
            writeVolume(fnOut, out.data(), X, Y, Z);
        }
    }

    static std::string dims(const ImageInfo &I) { return std::to_string(I.x) + " x " + std::to_string(I.y) + " x " + std::to_string(I.z); }
};

}  // namespace mc
#endif
