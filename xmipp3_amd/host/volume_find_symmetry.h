// volume_find_symmetry.h -- xmipp_volume_find_symmetry: ProgVolumeFindSymmetry (reconstruction/volume_find_symmetry.cpp) with the cost of
// every trial on the device behind the C ABI (xh_fsym_*). The usage lines, options, defaults and output text of :58-162, :255-347, plus
// --device. The exhaustive searches enumerate their trials on the host with the reference's two loops (xh_fsym_grid) and hand the list to
// xh_fsym_axis_search / xh_fsym_helical_search in that order; the answer is the first maximum above 0 in trial order, the reference's
// with --thr 1, and rot = tilt = 0 (rot = z = 0) where no correlation is above 0. --thr is accepted and ignored. --localRot and
// --localHelical run powell.h's optimiser (ftol 0.01, steps 1) with the device as the cost function, one trial per evaluation; a trial the
// gate refuses (:396-399) costs 1e38 without a launch.
// Masks: --mask circular <R>, binary_file <file>, cylinder <R> <H> and tube <R1> <R2> <H> with --center, as Mask::readParams reads them
// (data/mask.cpp:1318-1431); without --mask every voxel counts.
// Refused before any device is touched, each with a message naming the option:
//  - every other mask type; a mask of another shape, or one that selects no voxel (for the helix: after the clipping to
//    [zFirst, zLast] of --heightFraction);
//  - a flat input (Z = 1), sides above 1024 (or below 2); several devices;
//  - --sym rot <n> with n < 2 or n > 99; --sym2 that is not C<n> with n in 1 .. 99;
//  - ranges that are not finite, a loop that would never end (a step <= 0), an empty grid, a grid of more than kMaxTrials trials;
//  - --sampling <= 0, --heightFraction outside (0, 1], and a helical search with any trial that passes the gate but not the recursion
//    bound (xh_fsym_helical_depth: zHelical = 0 divides by zero in the reference).
// Not pinned (xmippCore is not in the reference tree): `std::cout << sym_axis` prints a Matrix1D through xmippCore's operator<<; here the
// three values follow each other in fields of ten characters, as the usage text shows them. MDL_DIRECTION is written as the label
// `direction` with the value '[ x y z ]', six decimals. The correlation map <root>.xmp is a Spider image, whose samples are 32-bit floats:
// a gated entry reads back as float(-1e38) = -9.99999968e37, not as -1e38.
#ifndef XMIPP3_AMD_VOLUME_FIND_SYMMETRY_H
#define XMIPP3_AMD_VOLUME_FIND_SYMMETRY_H
#include "programs.h"
#include "powell.h"
#include <iomanip>

namespace mc {

class ProgVolumeFindSymmetry : public XmippProgram {
public:
    static constexpr int64_t kMaxTrials = (int64_t)1 << 21;
    static constexpr int kCapacity = 256;              // trials of one launch; no result depends on it

    int rot_sym = 0, Cn = 1, device = 0;
    bool useSplines = false, local = false, helical = false, helicalDihedral = false, useMask = false;
    std::string fn_input, fn_output, sym2, maskType, maskArg;
    double rot0 = 0, rotF = 0, step_rot = 0, rotLocal = 0, tilt0 = 0, tiltF = 0, step_tilt = 0;
    double z0 = 0, zF = 0, step_z = 0, zLocal = 0, Ts = 1, heightFraction = 1;
    double R1 = 0, R2 = 0, H = 0, x0c = 0, y0c = 0, z0c = 0;

    void defineParams() override
    {
        addUsageLine("Find a symmetry rotational axis.");
        addUsageLine("The output is of the form");
        addUsageLine("Symmetry axis (rot,tilt)= 10 20 -->    0.33682   0.059391    0.93969");
        addUsageLine("The angles represent the rot and tilt angles of the symmetry axis ");
        addUsageLine("see [[http://xmipp.cnb.csic.es/twiki/bin/view/Xmipp/Conventions#Euler_Angles][the note on Euler angles]] ");
        addUsageLine("convention in Xmipp). The rest of the numbers is the axis itself in X, Y, Z ");
        addUsageLine("coordinates. In this way, the symmetry axis is a line that passes through the ");
        addUsageLine("center of the volume and whose direction is this vector.");
        addUsageLine("It is important that the volume is correctly centered.");
        addSeeAlsoLine("volume_center, transform_geometry");
        addParamsLine(" -i <volumeFile>                : Volume to process");
        addParamsLine("[-o <file=\"\">]                : Metadata with the orientation of the symmetry axis");
        addParamsLine("                                : In helical mode, there is a file called output.xmp ");
        addParamsLine("                                : with the correlation map (vertical axis is the rotation, ");
        addParamsLine("                                : horizontal axis is the translation)");
        addParamsLine("[--thr <N=1>]                   : Number of threads");
        // --sym <mode>, where <mode> is rot <n> | helical | helicalDihedral
        addParamsLine("--sym <mode> <n=0>              : Symmetry mode: rot <n> (Order of the rotational axis), helical (Helical symmetry.), helicalDihedral (Helical-Dihedral symmetry.)");
        addParamsLine("[--sym2 <Cn=C1>]                : Additional Cn symmetry. Only for helical and helicalDihedral");
        addParamsLine("==Locate rotational axis==");
        addParamsLine("[--rot  <rot0=0>  <rotF=355> <step=5>]: Limits for rotational angle search");
        addParamsLine("[--tilt <tilt0=0> <tiltF=90> <step=5>]: Limits for tilt angle search");
        addParamsLine("[--localRot <rot0> <tilt0>]     : Perform a local search around this angle");
        addParamsLine("[--useSplines]                  : Use cubic B-Splines for the interpolations");
        addParamsLine("==Locate helical parameters==");
        addParamsLine("[-z <z0=1> <zF=10> <zstep=0.5>] : Search space for the shift in Z (in Angstroms)");
        addParamsLine("[--sampling <T=1>]              : Sampling rate in A/pix");
        addParamsLine("[--rotHelical <rot0=-357> <rotF=357> <step=3>]: Search space for rotation around Z");
        addParamsLine("[--localHelical <z> <rot>]      : Perform a local search around this angle and shift");
        addParamsLine("[--heightFraction <f=1>]        : Use this fraction of the volume");
        // Mask::defineParams(this, INT_MASK, nullptr, "Restrict the comparison to the mask area.", true), the four supported types
        addParamsLine("[--mask <mask_type=circular> <a=\"\"> <b=\"\"> <c=\"\">] : Restrict the comparison to the mask area. binary_file <file>, circular <R>, "
                      "cylinder <R> <H> or tube <R1> <R2> <H> (all negative: inside, all positive: outside); other types are refused");
        addParamsLine("[--center <x0=0> <y0=0> <z0=0>] : mask center");
        addParamsLine("[--device <id=0>]               : HIP device (one device only)");
        addExampleLine("A typical application for a rotational symmetry axis is ", false);
        addExampleLine("xmipp_volume_center -i volume.vol");
        addExampleLine("xmipp_volume_find_symmetry -i volume.vol --sym rot 3");
        addExampleLine("Presume the symmetry axis is in rot=20, tilt=10. To align vertically the axis use", false);
        addExampleLine("xmipp_transform_geometry -i volume.vol --rotate_volume euler 20 10 0");
        addExampleLine("For locating the helical parameters use", false);
        addExampleLine("xmipp_volume_find_symmetry -i volume --sym helical -z 0 6 1 --mask circular -32 --thr 2 -o parameters.xmd");
    }

    static void finite(const char *opt, std::initializer_list<double> v)
    {
        for (double x : v)
            if (!std::isfinite(x)) REPORT_ERROR(ERR_ARG_INCORRECT, std::string(opt) + ": a value is not finite");
    }

    void readParams() override
    {
        fn_input = getParam("-i");
        fn_output = getParam("-o");
        const std::string mode = getParam("--sym");
        if (mode == "helical") helical = true;
        else if (mode == "helicalDihedral") helicalDihedral = true;
        else {
            if (mode != "rot") REPORT_ERROR(ERR_ARG_INCORRECT, "--sym " + mode + ": the modes are rot <n>, helical and helicalDihedral");
            rot_sym = (int)getIntParam("--sym", 1);
            if (rot_sym < 2 || rot_sym > 99) REPORT_ERROR(ERR_ARG_INCORRECT, "--sym rot " + getParam("--sym", 1) + ": the order of the axis must be 2 .. 99");
        }
        useSplines = checkParam("--useSplines");
        if (helical || helicalDihedral) {
            Ts = getDoubleParam("--sampling");
            if (!(Ts > 0) || !std::isfinite(Ts)) REPORT_ERROR(ERR_ARG_INCORRECT, "--sampling " + getParam("--sampling") + ": the sampling rate must be above 0");
            heightFraction = getDoubleParam("--heightFraction");
            if (!(heightFraction > 0 && heightFraction <= 1))
                REPORT_ERROR(ERR_ARG_INCORRECT, "--heightFraction " + getParam("--heightFraction") + ": the fraction must be in (0, 1]");
            local = checkParam("--localHelical");
            if (local) {
                zLocal = getDoubleParam("--localHelical", 0) / Ts;
                rotLocal = getDoubleParam("--localHelical", 1);
                finite("--localHelical", {zLocal, rotLocal});
            }
            z0 = getDoubleParam("-z", 0) / Ts;
            zF = getDoubleParam("-z", 1) / Ts;
            step_z = getDoubleParam("-z", 2) / Ts;
            rot0 = getDoubleParam("--rotHelical", 0);
            rotF = getDoubleParam("--rotHelical", 1);
            step_rot = getDoubleParam("--rotHelical", 2);
            finite("-z", {z0, zF, step_z});
            finite("--rotHelical", {rot0, rotF, step_rot});
            sym2 = getParam("--sym2");
            // Cn = std::stoi(sym2.substr(1))
            bool ok = sym2.size() >= 2 && sym2.size() <= 3 && (sym2[0] == 'C' || sym2[0] == 'c');
            for (size_t c = 1; ok && c < sym2.size(); ++c) ok = isdigit((unsigned char)sym2[c]) != 0;
            if (ok) Cn = std::stoi(sym2.substr(1));
            if (!ok || Cn < 1) REPORT_ERROR(ERR_ARG_INCORRECT, "--sym2 " + sym2 + ": C<n> with n in 1 .. 99");
        } else {
            local = checkParam("--localRot");
            if (local) {
                rot0 = getDoubleParam("--localRot", 0);
                tilt0 = getDoubleParam("--localRot", 1);
                finite("--localRot", {rot0, tilt0});
            } else {
                rot0 = getDoubleParam("--rot", 0);
                rotF = getDoubleParam("--rot", 1);
                step_rot = getDoubleParam("--rot", 2);
                tilt0 = getDoubleParam("--tilt", 0);
                tiltF = getDoubleParam("--tilt", 1);
                step_tilt = getDoubleParam("--tilt", 2);
                finite("--rot", {rot0, rotF, step_rot});
                finite("--tilt", {tilt0, tiltF, step_tilt});
            }
        }
        useMask = checkParam("--mask");
        if (useMask) readMaskParams();
        (void)getIntParam("--thr");                      // accepted and ignored
        const std::string dev = getParam("--device");
        if (dev.find(',') != std::string::npos) REPORT_ERROR(ERR_ARG_INCORRECT, "--device " + dev + ": this program runs on one device");
        device = parseGpuDevice(dev);
    }

    void readMaskParams()
    {
        // Mask::readParams (data/mask.cpp:1318-1431), the binary types this program supports
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
        } else if (maskType == "cylinder") {
            R1 = getDoubleParam("--mask", 1);
            H = getDoubleParam("--mask", 2);
            if (!((R1 < 0 && H < 0) || (R1 > 0 && H > 0))) REPORT_ERROR(ERR_ARG_INCORRECT, "MaskProgram: cannot determine mode for cylinder (--mask cylinder <R> <H>)");
        } else if (maskType == "tube") {
            R1 = getDoubleParam("--mask", 1);
            R2 = getDoubleParam("--mask", 2);
            H = getDoubleParam("--mask", 3);
            if (!((R1 < 0 && R2 < 0 && H < 0) || (R1 > 0 && R2 > 0 && H > 0)))
                REPORT_ERROR(ERR_ARG_INCORRECT, "MaskProgram: cannot determine mode for tube (--mask tube <R1> <R2> <H>)");
        } else
            REPORT_ERROR(ERR_NOT_IMPLEMENTED, "--mask " + maskType + ": only the binary_file, circular, cylinder and tube mask types are supported");
    }

    struct LocalCost {
        ProgVolumeFindSymmetry *prog;
        xh_fsym *h;
        std::string error;
    };

    // evaluateSymmetryWrapper: x[1], x[2] = (rot, tilt) or (rotHelical, zHelical); minus the correlation, 1e38 where the gate refuses
    static double localCost(double *x, void *user)
    {
        LocalCost *L = (LocalCost *)user;
        ProgVolumeFindSymmetry *P = L->prog;
        if (!L->error.empty()) return 1e38;
        const double p[2] = {x[1], x[2]};
        double corr = 0;
        int rc;
        if (P->helical || P->helicalDihedral) {
            const double box[4] = {P->z0, P->zF, P->rot0, P->rotF};
            rc = xh_fsym_helical_fit(L->h, p, 1, box, P->helicalDihedral ? 1 : 0, P->heightFraction, P->Cn, &corr);
        } else
            rc = xh_fsym_axis_fit(L->h, p, 1, P->rot_sym, &corr);
        if (rc != XH_OK) {
            L->error = xh_last_error();
            return 1e38;
        }
        return -corr;
    }

    void run() override
    {
        // ---- everything that can be refused, from the header and the options alone
        const ImageInfo I = readInfo(fn_input);
        const size_t X = I.x, Y = I.y, Z = I.z, N = X * Y * Z;
        if (Z == 1) REPORT_ERROR(ERR_MATRIX_DIM, "-i " + fn_input + " is an image (" + dims(I) + "): this program needs a volume");
        if (X < 2 || Y < 2 || Z < 2 || X > 1024 || Y > 1024 || Z > 1024)
            REPORT_ERROR(ERR_MATRIX_DIM, "-i: a box of " + dims(I) + " is not supported (2 .. 1024 a side)");
        const bool hel = helical || helicalDihedral;
        std::vector<int32_t> mask;
        if (useMask) {
            mask.resize(N);
            if (maskType == "binary_file") {
                std::vector<float> f;
                ImageInfo IM;
                readImage(maskArg, f, IM);
                if (IM.x != X || IM.y != Y || IM.z != Z) REPORT_ERROR(ERR_MATRIX_DIM, "--mask " + maskArg + " is " + dims(IM) + ", the volume " + dims(I));
                xhCheck(xh_halves_binary_mask(f.data(), N, mask.data()));
            } else if (maskType == "circular")
                xhCheck(xh_halves_circular_mask((int)Z, (int)Y, (int)X, R1, x0c, y0c, z0c, mask.data()));
            else if (maskType == "cylinder")
                xhCheck(xh_halves_cylinder_mask((int)Z, (int)Y, (int)X, R1, H, x0c, y0c, z0c, mask.data()));
            else
                xhCheck(xh_halves_tube_mask((int)Z, (int)Y, (int)X, R1, R2, H, x0c, y0c, z0c, mask.data()));
            // what the helix sees of it (:280-288): the planes of [zFirst, zLast]
            long kept = 0;
            const long nz = std::lround(heightFraction * (double)Z), zFirst = -(nz / 2), zLast = zFirst + nz - 1;
            for (size_t k = 0; k < Z; ++k) {
                const long kl = (long)k - (long)(Z / 2);
                if (hel && (kl < zFirst || kl > zLast)) continue;
                for (size_t e = 0; e < X * Y; ++e) kept += mask[k * X * Y + e] != 0;
            }
            if (kept == 0) REPORT_ERROR(ERR_VALUE_INCORRECT, hel ? "--mask selects no voxel within --heightFraction" : "--mask selects no voxel");
        }
        std::vector<double> trials;
        int64_t ntrials = 0, ydim = 0, xdim = 0;
        if (!local) {
            const char *names = hel ? "--rotHelical and -z" : "--rot and --tilt";
            const double r1[3] = {hel ? z0 : tilt0, hel ? zF : tiltF, hel ? step_z : step_tilt};
            if (xh_fsym_grid(rot0, rotF, step_rot, r1[0], r1[1], r1[2], kMaxTrials, nullptr, &ntrials, &ydim, &xdim) != XH_OK)
                REPORT_ERROR(ERR_ARG_INCORRECT, std::string("the search ranges (") + names + "): " + xh_last_error() + "; at most " + std::to_string(kMaxTrials) +
                                                " trials are enumerated, split the ranges");
            if (ntrials == 0) REPORT_ERROR(ERR_ARG_INCORRECT, std::string("the search ranges (") + names + ") hold no trial: a first value is above its last");
            trials.resize(2 * (size_t)ntrials);
            xhCheck(xh_fsym_grid(rot0, rotF, step_rot, r1[0], r1[1], r1[2], kMaxTrials, trials.data(), &ntrials, &ydim, &xdim));
            if (hel) {
                // a trial the gate lets through must be one the recursion bound admits
                for (int64_t t = 0; t < ntrials; ++t) {
                    int32_t g = 0, depth = 0;
                    xhCheck(xh_fsym_helical_gate((int)Z, trials[2 * t + 1], trials[2 * t], z0, zF, rot0, rotF, &g));
                    if (g) continue;
                    xhCheck(xh_fsym_helical_depth((int)Z, trials[2 * t + 1], heightFraction, helicalDihedral ? 1 : 0, &depth));
                    if (depth < 0) {
                        std::ostringstream o;
                        o << "-z: a rise of " << trials[2 * t + 1] * Ts << " (" << trials[2 * t + 1] << " voxels) is not supported: the rise must be above 0"
                          << (helicalDihedral ? ", and at least 1 voxel for helicalDihedral over an even Z covered entirely" : "");
                        REPORT_ERROR(ERR_ARG_INCORRECT, o.str());
                    }
                }
            }
        }

        // ---- the device
        std::vector<double> V;
        ImageInfo J;
        readDoubles(fn_input, V, J);
        xh_ctx *ctx = nullptr;
        xhCheck(xh_ctx_create_private(device, &ctx));
        XhOwner<xh_ctx> ctxOwner(ctx);
        xh_fsym *h = nullptr;
        xhCheck(xh_fsym_create(ctx, (int)Z, (int)Y, (int)X, local ? 1 : kCapacity, &h));
        XhOwner<xh_fsym> hOwner(h);
        xhCheck(xh_fsym_set_volume(h, V.data(), useMask ? mask.data() : nullptr, useSplines && !hel ? 1 : 0));

        double best_corr = 0, best_rot = 0, best_second = 0;             // the second variable: tilt, or z in voxels
        std::vector<double> corrs;
        if (!local) {
            if (verbose > 0 && !hel) std::cerr << "Searching symmetry axis ...\n";
            init_progress_bar((size_t)ntrials);
            int64_t idx = -1;
            if (ntrials > 0) {
                if (hel) {
                    corrs.resize((size_t)ntrials);
                    const double box[4] = {z0, zF, rot0, rotF};
                    xhCheck(xh_fsym_helical_search(h, trials.data(), ntrials, box, helicalDihedral ? 1 : 0, heightFraction, Cn, &idx, &best_corr, corrs.data()));
                } else
                    xhCheck(xh_fsym_axis_search(h, trials.data(), ntrials, rot_sym, &idx, &best_corr, nullptr));
            }
            if (idx >= 0) {
                best_rot = trials[2 * (size_t)idx];
                best_second = trials[2 * (size_t)idx + 1];
            }
            progress_bar((size_t)ntrials);
        } else {
            std::vector<double> p = {hel ? rotLocal : rot0, hel ? zLocal : tilt0};
            const std::vector<double> steps = {1, 1};
            double fitness = 0;
            int iter = 0;
            LocalCost L{this, h, ""};
            powellOptimizer(p, 1, 2, &localCost, &L, 0.01, fitness, iter, steps);
            if (!L.error.empty()) REPORT_ERROR(ERR_GPU, std::string(hel ? "--localHelical: " : "--localRot: ") + L.error);
            best_rot = p[0];
            best_second = p[1];
            best_corr = -fitness;
        }

        // ---- the report (:255-347)
        if (!hel) {
            double axis[3];
            eulerRow2(best_rot, best_second, axis);
            if (verbose != 0) {
                std::cout << "Symmetry axis (rot,tilt)= " << best_rot << " " << best_second << " --> ";
                for (double v : axis) std::cout << std::setw(10) << v << ' ';
                std::cout << std::endl;
            }
            if (!fn_output.empty()) {
                MetaDataVec MD;
                const size_t id = MD.addObject();
                MD.setValue("angleRot", best_rot, id);
                MD.setValue("angleTilt", best_second, id);
                char b[128];
                snprintf(b, sizeof(b), "[ %.6f %.6f %.6f ]", axis[0], axis[1], axis[2]);
                MD.setValue("direction", std::string(b), id);
                MD.write(fn_output);
            }
        } else {
            if (verbose != 0)
                std::cout << "Symmetry parameters (z,rot)= " << best_second * Ts << " " << best_rot << " correlation=" << best_corr << std::endl;
            if (!fn_output.empty()) {
                MetaDataVec MD;
                const size_t id = MD.addObject();
                MD.setValue("angleRot", best_rot, id);
                MD.setValue("shiftZ", best_second * Ts, id);
                MD.write(fn_output);
                if (!local) writeVolume(FileName(fn_output).removeAllExtensions() + ".xmp", corrs.data(), (size_t)xdim, (size_t)ydim, 1);
            }
        }
    }

    // row 2 of Euler_angles2matrix(rot, tilt, 0): (sin tilt cos rot, sin tilt sin rot, cos tilt)
    static void eulerRow2(double rot, double tilt, double *axis)
    {
        const double a = rot * M_PI / 180.0, b = tilt * M_PI / 180.0;
        axis[0] = std::sin(b) * std::cos(a);
        axis[1] = std::sin(b) * std::sin(a);
        axis[2] = std::cos(b);
    }

    static std::string dims(const ImageInfo &I) { return std::to_string(I.x) + " x " + std::to_string(I.y) + " x " + std::to_string(I.z); }
};

}  // namespace mc
#endif
