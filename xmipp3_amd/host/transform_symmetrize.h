// transform_symmetrize.h -- xmipp_transform_symmetrize: ProgSymmetrize (reconstruction/symmetrize.{h,cpp}) with the symmetrisation on the
// device behind the C ABI (xh_sym_*). The option lines, defaults, show() text and error messages of symmetrize.cpp:63-114, plus --device.
// -i takes an image, a volume, a stack, or a metadata of them; without -o every input is overwritten, which is how
// xmipp_reconstruct_significant calls the program (reconstruct_significant.cpp:611-618, :800-806). Volume or image is decided by Z: an
// image needs a number for --sym, a volume a group (or helical / helicalDihedral). All 2-D inputs of one size go through one launch.
// Another program runs it in-process on a fresh object: read(argc, argv), then tryRun().
// Refused before any device is touched, each with its reason:
//  - --mask_in: it goes through xmippCore's selfArrayByArrayMask, which is not in the reference tree, and as called (op1 = V_in, :164) it
//    overwrites the result instead of accumulating, so there is nothing to be faithful to;
//  - --sym dihedral: symmetry_Dihedral's search over 360 x 0.4 Z resamplings, not built yet;
//  - --spline other than 1 and 3; several devices; input rows with geometry columns (readApplyGeo, :240, is not applied);
//  - helix parameters for which interpolatedElement3DHelical's recursion has no bound (xh_sym_helical_depth), zHelical <= 1 voxel among
//    them, where the reference itself never terminates;
//  - a metadata of volumes with -o (the reference writes a stack of volumes, which the image writer here does not have), and a stack
//    of volumes as input, with or without -o.
#ifndef XMIPP3_AMD_TRANSFORM_SYMMETRIZE_H
#define XMIPP3_AMD_TRANSFORM_SYMMETRIZE_H
#include "programs.h"

namespace mc {

class ProgSymmetrize : public XmippProgram {
public:
    std::string fn_in, fn_out, fn_sym, fn_sym2, fn_Maskin;
    bool doMask = false, helical = false, dihedral = false, helicalDihedral = false, do_not_generate_subgroup = false, wrap = true, sum = false;
    double Ts = 1, zHelical = 0, rotHelical = 0, rotPhaseHelical = 0, heightFraction = 0.95;
    int Cn = 1, splineOrder = 3, symorder = -1, device = 0;
    SymList SL;

    void defineParams() override
    {
        addUsageLine("Symmetrize volumes and images ");
        addParamsLine("    -i <input>           : Input image, volume, stack or metadata of them");
        addParamsLine("   [-o <output=\"\">]      : Output file (a stack for several images); without it the input is overwritten");
        addParamsLine("    --sym <symmetry>     : For 2D images: a number");
        addParamsLine("                         : For 3D volumes: a symmetry file or point-group description");
        addParamsLine("                         : Valid point-group descriptions are:");
        addParamsLine("                         : C1, Ci, Cs, Cn (from here on n must be an integer number with no more than 2 digits)");
        addParamsLine("                         : Cnv, Cnh, Sn, Dn, Dnv, Dnh, T, Td, Th, O, Oh");
        addParamsLine("                         : I, I1, I2, I3, I4, I5, Ih, helical, dihedral, helicalDihedral");
        addParamsLine("                         :+ For a full description of symmetries look at");
        addParamsLine("                         :+ https://i2pc.github.io/docs/Utils/Conventions/index.html#symmetry");
        addParamsLine("   [--sym2 <sym2=C1>]    : Only for helical, or helicalDihedral");
        addParamsLine("                         : You may use any other Cn symmetry");
        addParamsLine("   [--helixParams <z> <rot> <rotPhase=0>]: Helical parameters z(Angstroms), rot(degrees), rotPhase(degrees)");
        addParamsLine("                         :+ V(r,theta,z)=V(r,theta+rotHelix+rotPhase,z+zHelix)");
        addParamsLine("   [--heightFraction <f=0.95>]: Height fraction used for symmetrizing a helix");
        addParamsLine("   [--sampling <T=1>]    : Sampling rate (A/pixel). Used only for helical parameters");
        addParamsLine("   [--no_group]          : For 3D volumes: do not generate symmetry subgroup");
        addParamsLine("   [--dont_wrap]         : by default, the image/volume is wrapped");
        addParamsLine("   [--sum]               : compute the sum of the images/volumes instead of the average. This is useful for symmetrizing pieces");
        addParamsLine("   [--mask_in <fileName>]: symmetrize only in the masked area");
        addParamsLine("   [--spline <order=3>]  : Spline order for the interpolation (valid values are 1 and 3)");
        addParamsLine("   [--device <id=0>]     : HIP device (one device only)");
        addExampleLine("Symmetrize a list of images with 6 fold symmetry", false);
        addExampleLine("   xmipp_transform_symmetrize -i input.sel --sym 6");
        addExampleLine("Symmetrize with i3 symmetry and the volume is not wrapped", false);
        addExampleLine("   xmipp_transform_symmetrize -i input.vol --sym i3 --dont_wrap");
    }

    void readParams() override
    {
        // symmetrize.cpp:32-60
        fn_in = getParam("-i");
        fn_out = getParam("-o");
        fn_sym = getParam("--sym");
        fn_sym2 = getParam("--sym2");
        doMask = false;
        if (checkParam("--mask_in")) {
            fn_Maskin = getParam("--mask_in");
            doMask = true;
        }
        helical = (fn_sym == "helical");
        dihedral = (fn_sym == "dihedral");
        helicalDihedral = (fn_sym == "helicalDihedral");
        if (helical || helicalDihedral) {
            Ts = getDoubleParam("--sampling");
            zHelical = getDoubleParam("--helixParams", 0) / Ts;
            rotHelical = getDoubleParam("--helixParams", 1) * M_PI / 180.0;
            rotPhaseHelical = getDoubleParam("--helixParams", 2) * M_PI / 180.0;
            if (fn_sym2.size() < 2 || (fn_sym2[0] != 'c' && fn_sym2[0] != 'C') || fn_sym2.find_first_not_of("0123456789", 1) != std::string::npos)
                REPORT_ERROR(ERR_ARG_INCORRECT, "--sym2 " + fn_sym2 + ": a Cn symmetry is expected");
            Cn = std::stoi(fn_sym2.substr(1));
        }
        do_not_generate_subgroup = checkParam("--no_group");
        wrap = !checkParam("--dont_wrap");
        sum = checkParam("--sum");
        heightFraction = getDoubleParam("--heightFraction");
        splineOrder = (int)getIntParam("--spline");
        const std::string dev = getParam("--device");
        // refused before any device is touched
        if (dev.find(',') != std::string::npos) REPORT_ERROR(ERR_ARG_INCORRECT, "--device " + dev + ": this program runs on one device");
        device = parseGpuDevice(dev);
        if (doMask)
            REPORT_ERROR(ERR_NOT_IMPLEMENTED, "--mask_in: the masked sum goes through xmippCore's selfArrayByArrayMask, which is not available; as the reference calls it "
                                              "every symmetry copy overwrites the result inside the mask instead of being accumulated");
        if (dihedral)
            REPORT_ERROR(ERR_NOT_IMPLEMENTED, "--sym dihedral: symmetry_Dihedral's search for the dihedral axis is not available yet");
        if (splineOrder != 1 && splineOrder != 3)
            REPORT_ERROR(ERR_ARG_INCORRECT, "--spline " + std::to_string(splineOrder) + ": valid values are 1 and 3");
        if ((helical || helicalDihedral) && !(zHelical > 1))
            REPORT_ERROR(ERR_ARG_INCORRECT, "--helixParams: a rise of " + fmtG(zHelical) + " voxels; the helical interpolation needs more than 1 voxel (at 1 or less the "
                                            "reference's recursion never terminates)");
    }

    static std::string fmtG(double v) { char b[64]; snprintf(b, sizeof(b), "%g", v); return b; }

    void show() const
    {
        // symmetrize.cpp:94-114 after XmippMetadataProgram::show
        if (verbose == 0) return;
        std::cout << "Input File: " << fn_in << std::endl;
        if (!fn_out.empty()) std::cout << "Output File: " << fn_out << std::endl;
        std::cout << "Symmetry: " << fn_sym << std::endl
                  << "No group: " << do_not_generate_subgroup << std::endl
                  << "Wrap:     " << wrap << std::endl
                  << "Sum:      " << sum << std::endl
                  << "Spline:   " << splineOrder << std::endl;
        if (doMask) std::cout << "mask_in    " << fn_Maskin << std::endl;
        if (helical)
            std::cout << "RotHelical: " << rotHelical * 180.0 / M_PI << std::endl
                      << "RotPhaseHelical: " << rotPhaseHelical * 180.0 / M_PI << std::endl
                      << "ZHelical:   " << zHelical * Ts << "Height fraction: " << heightFraction << std::endl;
        if (helical || helicalDihedral) std::cout << "Symmetry2: " << fn_sym2 << std::endl;
    }

    // symmetrize.cpp:217-230
    void preProcess()
    {
        if (!helical && !dihedral && !helicalDihedral) {
            if (!fileExists(fn_sym) && isdigit((unsigned char)fn_sym[0])) symorder = atoi(fn_sym.c_str());
            else {
                const double accuracy = do_not_generate_subgroup ? -1 : 1e-6;
                SL.readSymmetryFile(fn_sym, accuracy);
                symorder = -1;
            }
        }
    }

    struct Item { std::string in, out; ImageInfo info; };

    static bool isMetadataName(const std::string &fn)
    {
        const std::string e = FileName(fn).extension();
        return e == "xmd" || e == "sel" || e == "doc" || e == "star";
    }

    // image `index` (1-based) of an existing stack, in place
    static void writeIntoStack(const std::string &name, const float *data)
    {
        FileName fn(name);
        const ImageInfo I = readInfo(fn.path);
        const size_t idx = fn.number(), per = I.x * I.y;
        if (!I.isStack || I.z != 1 || idx < 1 || idx > I.n || I.mode != 2) REPORT_ERROR(ERR_IO_NOREAD, "Image::write: cannot replace " + name);
        const size_t off = I.mrc ? I.headerBytes + (idx - 1) * per * 4 : I.headerBytes + (idx - 1) * (I.perImageHeader + per * 4) + I.perImageHeader;
        std::fstream f(fn.path, std::ios::binary | std::ios::in | std::ios::out);
        f.seekp((std::streamoff)off);
        f.write((const char *)data, per * 4);
        if (!f.good()) REPORT_ERROR(ERR_IO_NOREAD, "Image::write: short write to " + fn.path);
    }

    void run() override
    {
        show();
        preProcess();
        // ---- what is to be done, from headers alone
        std::vector<Item> items;
        MetaDataVec md;
        const bool isMd = isMetadataName(fn_in);
        if (isMd) {
            readEnabledRows(fn_in, md);
            for (const char *l : {"shiftX", "shiftY", "shiftZ", "angleRot", "angleTilt", "anglePsi", "flip", "scale"})
                if (md.containsLabel(l))
                    REPORT_ERROR(ERR_NOT_IMPLEMENTED, std::string("the input metadata has the geometry column ") + l + ": the reference applies it on reading (readApplyGeo), "
                                                      "which is not available; apply the geometry first");
            if (!md.containsLabel("image")) REPORT_ERROR(ERR_MD_MISSINGLABEL, "the input metadata has no image column");
            for (size_t r = 0; r < md.size(); ++r) {
                Item it;
                md.getValue("image", it.in, r);
                items.push_back(it);
            }
        } else {
            const ImageInfo I = readInfo(fn_in);
            if (I.isStack && !FileName(fn_in).hasNumber())
                for (size_t k = 1; k <= I.n; ++k) { Item it; it.in = std::to_string(k) + "@" + fn_in; items.push_back(it); }
            else { Item it; it.in = fn_in; items.push_back(it); }
        }
        if (items.empty()) REPORT_ERROR(ERR_MD_NOOBJ, "no input images");
        const bool single = items.size() == 1 && !isMd;
        size_t nImages = 0;
        for (size_t k = 0; k < items.size(); ++k) {
            Item &it = items[k];
            it.info = readInfo(it.in);
            const ImageInfo &I = it.info;
            if (I.z == 1) {
                // processImage :250-258
                if (helical) REPORT_ERROR(ERR_ARG_INCORRECT, "Helical symmetrization is not meant for images");
                if (symorder == -1) REPORT_ERROR(ERR_ARG_MISSING, "The symmetry order is not valid for images");
                if (symorder < 1 || symorder > 1024) REPORT_ERROR(ERR_ARG_INCORRECT, "--sym " + fn_sym + ": an order between 1 and 1024 is expected");
                ++nImages;
            } else {
                if (!(SL.symsNo() > 0 || helical || helicalDihedral)) REPORT_ERROR(ERR_ARG_MISSING, "The symmetry description is not valid for volumes");
                if (helical || helicalDihedral) {
                    int32_t depth = -1;
                    xhCheck(xh_sym_helical_depth((int)I.z, zHelical, heightFraction, helicalDihedral ? 1 : 0, &depth));
                    if (depth < 0)
                        REPORT_ERROR(ERR_ARG_INCORRECT, "helix of rise " + fmtG(zHelical) + " voxels and height fraction " + fmtG(heightFraction) + " on " + std::to_string(I.z) +
                                                        " planes: the helical interpolation's recursion is bounded only for 1 < rise <= Z and 0 < heightFraction <= 1");
                    if (Cn < 1 || Cn > 99) REPORT_ERROR(ERR_ARG_INCORRECT, "--sym2 " + fn_sym2 + ": n between 1 and 99 is expected");
                }
                if (!single && !fn_out.empty())
                    REPORT_ERROR(ERR_NOT_IMPLEMENTED, "several volumes with -o: the reference writes a stack of volumes, which is not available; run without -o to overwrite the inputs");
            }
            if (I.isStack && I.z > 1)
                REPORT_ERROR(ERR_NOT_IMPLEMENTED, it.in + " is a stack of volumes, which the image reader and writer here do not have; give the volumes as files of their own");
            if (I.x < 2 || I.y < 2 || I.x > 1024 || I.y > 1024 || I.z > 1024)
                REPORT_ERROR(ERR_MATRIX_DIM, "A box of " + std::to_string(I.x) + " x " + std::to_string(I.y) + " x " + std::to_string(I.z) + " is not supported (2 .. 1024 a side)");
            it.out = single ? (fn_out.empty() ? it.in : fn_out) : (fn_out.empty() ? it.in : std::to_string(k + 1) + "@" + fn_out);
        }
        if (nImages != 0 && nImages != items.size() && !fn_out.empty()) REPORT_ERROR(ERR_NOT_IMPLEMENTED, "images and volumes in one input with -o");

        // ---- the device
        xh_ctx *ctx = nullptr;
        xhCheck(xh_ctx_create_private(device, &ctx));
        XhOwner<xh_ctx> ctxOwner(ctx);
        std::vector<bool> done(items.size(), false);
        std::unique_ptr<StackWriter> stackOut;
        if (!single && !fn_out.empty()) stackOut.reset(new StackWriter(fn_out, items[0].info.x, items[0].info.y, items.size()));
        for (size_t k = 0; k < items.size(); ++k) {
            if (done[k]) continue;
            const ImageInfo I = items[k].info;
            // everything of this shape: the images of one size in one launch, a volume on its own
            std::vector<size_t> group;
            for (size_t m = k; m < items.size(); ++m)
                if (!done[m] && items[m].info.x == I.x && items[m].info.y == I.y && items[m].info.z == I.z && (I.z == 1 || m == k)) group.push_back(m);
            if (stackOut && (I.x != items[0].info.x || I.y != items[0].info.y)) REPORT_ERROR(ERR_MATRIX_DIM, "images of different sizes cannot go to one output stack");
            const size_t per = I.x * I.y * I.z, n = group.size();
            std::vector<double> in(per * n), out(per * n);
            std::vector<float> f;
            ImageInfo J;
            for (size_t g = 0; g < n; ++g) {
                readImage(items[group[g]].in, f, J);
                std::copy(f.begin(), f.end(), in.begin() + g * per);
            }
            xh_sym *h = nullptr;
            xhCheck(xh_sym_create(ctx, (int)I.z, (int)I.y, (int)I.x, &h));
            XhOwner<xh_sym> hOwner(h);
            DeviceBuffer dIn, dOut;
            dIn.upload(ctx, in.data(), sizeof(double) * in.size());
            dOut.reserve(ctx, sizeof(double) * out.size());
            if (I.z == 1)
                xhCheck(xh_sym_symmetrize_images(h, dIn.as<double>(), (int)n, symorder, splineOrder, wrap ? 1 : 0, sum ? 1 : 0, dOut.as<double>()));
            else if (helical || helicalDihedral)
                xhCheck(xh_sym_helical(h, dIn.as<double>(), zHelical, rotHelical, rotPhaseHelical, Cn, helicalDihedral ? 1 : 0, heightFraction, splineOrder, dOut.as<double>()));
            else {
                std::vector<double> R;
                for (int i = 0; i < SL.symsNo(); ++i) R.insert(R.end(), SL.R[i].begin(), SL.R[i].end());
                xhCheck(xh_sym_set_matrices(h, R.data(), SL.symsNo()));
                xhCheck(xh_sym_symmetrize(h, dIn.as<double>(), splineOrder, wrap ? 1 : 0, sum ? 1 : 0, dOut.as<double>()));
            }
            xhCheck(xh_memcpy_d2h(ctx, out.data(), dOut.p, sizeof(double) * out.size()));
            for (size_t g = 0; g < n; ++g) {
                const Item &it = items[group[g]];
                const double *o = out.data() + g * per;
                if (stackOut) {
                    f.assign(o, o + per);
                    stackOut->write(group[g], f.data());
                } else if (FileName(it.out).hasNumber()) {
                    f.assign(o, o + per);
                    writeIntoStack(it.out, f.data());
                } else
                    writeVolume(it.out, o, I.x, I.y, I.z);
                done[group[g]] = true;
            }
            forgetImageReadCache();                            // inputs may have been rewritten: the next read opens them anew
        }
        if (stackOut) {
            stackOut->finish();
            // the output metadata next to the stack, as the other per-image programs write it
            MetaDataVec mo;
            for (size_t k = 0; k < items.size(); ++k) mo.setValue("image", items[k].out, mo.addObject());
            const std::string stem = fn_out.substr(0, fn_out.find_last_of('.'));
            mo.write(stem + ".xmd");
        }
    }
};

}  // namespace mc
#endif
