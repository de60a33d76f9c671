// subtract_projection.h -- xmipp_subtract_projection: ProgSubtractProjection (reconstruction/subtract_projection.{h,cpp}) behind the
// C ABI (xh_sub_*). Options as in defineParams (:116-151) plus --dev. -i / -o as angular_continuous_assign2.h handles them: -o is a stack
// and the metadata is written next to it (.xmd). Every input column is carried over; image is replaced, subtractionR2, subtractionBeta0,
// subtractionBeta1 and subtractionB are added, and enabled = -1 is set for a particle that --nonNegative rejects (writeParticle :161-174).
// Refused with ERR_NOT_IMPLEMENTED: --noise_est (the reference seeds rand with time(0)), ctfModel files, non-square particles, a non-cubic
// volume, particles of another size than the volume, the generic --oroot / --oext, several devices. --save is accepted and ignored: the
// reference reads it only under debug defines. --sigma is accepted and unused, as in the reference.
#ifndef XMIPP3_AMD_SUBTRACT_PROJECTION_H
#define XMIPP3_AMD_SUBTRACT_PROJECTION_H
#include "ctf_programs.h"

namespace mc {

class ProgSubtractProjection : public XmippProgram {
public:
    std::string fn_in, fn_out, fnVolR, fnMaskRoi, fnMaskVol;
    xh_sub_params prm;
    int device = 0, batch = 256;

    void defineParams() override
    {
        addUsageLine("This program computes the subtraction between particles and a reference");
        addUsageLine(" volume, by computing its projections with the same angles that input particles have.");
        addUsageLine(" Then, each particle and the correspondent projection of the reference volume are numerically");
        addUsageLine(" adjusted and subtracted using a mask which denotes the region of interest to keep or subtract.");
        addUsageLine("+Output labels added (xmippCore spellings): subtractionR2, subtractionBeta0, subtractionBeta1, subtractionB.");
        addParamsLine("   -i <metadata>               : Metadata with the particles and their alignment");
        addParamsLine("   -o <stack>                  : Stack of subtracted particles; the metadata is written next to it (.xmd)");
        addParamsLine("   --ref <volume>              : Reference volume to subtract");
        addParamsLine("  [--mask_roi <mask_roi=\"\">] : 3D mask for region of interest to keep or subtract, no mask implies subtraction of whole images");
        addParamsLine("  [--cirmaskrad <c=-1.0>]      : Apply circular mask to proyected particles. Radius = -1 fits a sphere in the reference volume.");
        addParamsLine("  [--mask <mask=\"\">]         : Provide a mask to be applied. Any desity out of the mask is removed from further analysis.");
        addParamsLine("  [--sampling <sampling=1>]    : Sampling rate (A/pixel)");
        addParamsLine("  [--max_resolution <f=-1>]    : Maximum resolution in Angtroms up to which the substraction is calculated. By default (-1) it is set to sampling/sqrt(2).");
        addParamsLine("  [--padding <p=2>]            : Padding factor for Fourier projector");
        addParamsLine("  [--sigma <s=1>]              : Decay of the filter (sigma) to smooth the mask transition");
        addParamsLine("  [--nonNegative]              : Ignore particles with negative beta0 or R2");
        addParamsLine("  [--boost]                    : Perform a boosting of original particles");
        addParamsLine("  [--save <structure=\"\">]    : Path for saving intermediate files (accepted and ignored: read only under debug defines)");
        addParamsLine("  [--subtract]                 : The mask contains the region to SUBTRACT");
        addParamsLine("  [--realSpaceProjection]      : Project volume in real space to avoid Fourier artifacts");
        addParamsLine("  [--ignoreCTF]                : Do not consider CTF in the subtraction. Use if particles have been CTF corrected.");
        addParamsLine("  [--noise_est]                : not implemented (the reference seeds its random sampling with time(0))");
        addParamsLine("  [--oroot <root=\"\">]        : not implemented (the generic output root of XmippMetadataProgram)");
        addParamsLine("  [--oext <ext=\"\">]          : not implemented (the generic output extension of XmippMetadataProgram)");
        addParamsLine("  [--dev <id=0>]               : GPU device to use (one device only: several are refused)");
        addParamsLine("  [--batch <n=256>]            : Particles per device step");
        addExampleLine("A typical use is:", false);
        addExampleLine("xmipp_subtract_projection -i input_particles.xmd --ref input_map.mrc --mask_roi mask_vol.mrc -o output_particles.stk --sampling 1 --max_resolution 4");
    }

    void readParams() override
    {
        if (!checkParam("-i")) REPORT_ERROR(ERR_ARG_MISSING, "-i is mandatory");
        if (!checkParam("-o")) REPORT_ERROR(ERR_ARG_MISSING, "-o is mandatory");
        if (!checkParam("--ref")) REPORT_ERROR(ERR_ARG_MISSING, "--ref is mandatory");
        if (checkParam("--noise_est")) REPORT_ERROR(ERR_NOT_IMPLEMENTED, "--noise_est is not available (its sampling is seeded with time(0) in the reference)");
        if (checkParam("--oroot") || checkParam("--oext"))
            REPORT_ERROR(ERR_NOT_IMPLEMENTED, "--oroot / --oext are not available: -o names the output stack, its metadata is written next to it");
        fn_in = getParam("-i");
        fn_out = getParam("-o");
        fnVolR = getParam("--ref");
        fnMaskRoi = getParam("--mask_roi");
        xh_sub_defaults(&prm);
        prm.sampling = getDoubleParam("--sampling");
        prm.padding = getDoubleParam("--padding");
        prm.max_resolution = getDoubleParam("--max_resolution");
        // readParams :74-83: --cirmaskrad wins over --mask
        if (checkParam("--cirmaskrad")) prm.cirmaskrad = getDoubleParam("--cirmaskrad");
        else if (checkParam("--mask")) fnMaskVol = getParam("--mask");
        prm.non_negative = checkParam("--nonNegative");
        prm.boost = checkParam("--boost");
        prm.subtract = checkParam("--subtract");
        prm.real_space = checkParam("--realSpaceProjection");
        prm.ignore_ctf = checkParam("--ignoreCTF");
        if (checkParam("--save")) std::cerr << "xmipp_subtract_projection: --save is ignored (the reference reads it only under debug defines)" << std::endl;
        if (checkParam("--dev")) device = parseGpuDevice(getParam("--dev"));
        batch = std::max(1, (int)getIntParam("--batch"));
    }

    static std::string slot(size_t i, const std::string &stack) { return std::to_string(i + 1) + "@" + stack; }

    // a volume as doubles about the Xmipp origin; it must have the side D (D = 0: any cube, returned)
    static void readCube(const std::string &fn, std::vector<double> &v, size_t &D, const char *what)
    {
        std::vector<float> f;
        ImageInfo I;
        readImage(fn, f, I);
        if (I.x != I.y || I.x != I.z) REPORT_ERROR(ERR_NOT_IMPLEMENTED, std::string("the ") + what + " must be a cube (a non-cubic volume is not supported)");
        if (D && I.x != D) REPORT_ERROR(ERR_NOT_IMPLEMENTED, std::string("the ") + what + " must have the size of the reference volume");
        D = I.x;
        v.assign(f.begin(), f.end());
    }

    static void checkParticle(const std::string &fn, const ImageInfo &I, size_t D)
    {
        if (I.x != I.y) REPORT_ERROR(ERR_NOT_IMPLEMENTED, fn + ": the particles must be square");
        if (I.x != D || I.z != 1) REPORT_ERROR(ERR_NOT_IMPLEMENTED, fn + ": the particles must have the size of the reference volume");
    }

    void run() override
    {
        MetaDataVec md;
        readEnabledRows(fn_in, md);
        const size_t n = md.size();
        if (n == 0) REPORT_ERROR(ERR_MD_NOOBJ, "no enabled images in " + fn_in);
        if (!md.containsLabel("image")) REPORT_ERROR(ERR_MD_BADLABEL, fn_in + ": does not have the image label");
        if (md.containsLabel("ctfModel") && !prm.ignore_ctf)
            REPORT_ERROR(ERR_NOT_IMPLEMENTED, "CTFs given as ctfModel files are not read; give the CTF columns (ctfDefocusU ...) or --ignoreCTF");
        const bool hasCTF = md.containsLabel("ctfDefocusU") && !prm.ignore_ctf;       // applyCTF :219
        // preProcess (:514-632)
        size_t D = 0;
        std::vector<double> vol, roi, maskvol;
        readCube(fnVolR, vol, D, "reference volume");
        if (!fnMaskRoi.empty()) readCube(fnMaskRoi, roi, D, "--mask_roi volume");
        if (!fnMaskVol.empty()) readCube(fnMaskVol, maskvol, D, "--mask volume");
        const size_t per = D * D;
        std::vector<float> one, fl(per);
        {
            // the first particle's shape is checked before a device is touched; every particle is checked again as it is read
            std::string fn;
            md.getValue("image", fn, 0);
            ImageInfo I;
            readImage(fn, one, I);
            checkParticle(fn, I, D);
        }
        xh_ctx *ctx = nullptr;
        xhCheck(xh_ctx_create_private(device, &ctx));
        XhOwner<xh_ctx> ctxOwner(ctx);
        xh_sub *h = nullptr;
        xhCheck(xh_sub_create(ctx, vol.data(), (int)D, roi.empty() ? nullptr : roi.data(), maskvol.empty() ? nullptr : maskvol.data(), &prm, batch, &h));
        XhOwner<xh_sub> hOwner(h);
        StackWriter stack(fn_out, D, D, n);
        MetaDataVec out;
        out.labels = md.labels;
        const size_t group = 4096;      // particles on the host at a time
        for (size_t g0 = 0; g0 < n; g0 += group) {
            const size_t m = std::min(group, n - g0);
            std::vector<float> imgs(m * per);
            std::vector<xh_sub_row> rows(m);
            for (size_t k = 0; k < m; ++k) {
                const size_t id = g0 + k;
                std::string fn;
                md.getValue("image", fn, id);
                ImageInfo I;
                readImage(fn, one, I);
                checkParticle(fn, I, D);
                std::copy(one.begin(), one.end(), imgs.begin() + k * per);
                // processParticle :246-252
                xh_sub_row &r = rows[k];
                std::memset(&r, 0, sizeof(r));
                r.rot = md.getDouble("angleRot", id, 0); r.tilt = md.getDouble("angleTilt", id, 0); r.psi = md.getDouble("anglePsi", id, 0);
                r.shift_x = md.getDouble("shiftX", id, 0); r.shift_y = md.getDouble("shiftY", id, 0);
                r.has_ctf = hasCTF;
                if (hasCTF) readCtfRow(md, id, r.ctf);
            }
            xhCheck(xh_sub_load(h, imgs.data(), (int)m, (int)D, (int)D, rows.data()));
            std::vector<double> diff(m * per);
            std::vector<xh_sub_result> res(m);
            xhCheck(xh_sub_run(h, diff.data(), res.data()));
            for (size_t k = 0; k < m; ++k) {
                const size_t id = g0 + k;
                for (size_t q = 0; q < per; ++q) fl[q] = (float)diff[k * per + q];
                stack.write(id, fl.data());
                // writeParticle :161-174
                const size_t o = out.addObject();
                for (const std::string &l : md.labels) { std::string v; if (md.getValue(l, v, id)) out.setValue(l, v, o); }
                out.setValue("image", slot(id, fn_out), o);
                out.setValue("subtractionR2", res[k].R2adj, o);
                out.setValue("subtractionBeta0", res[k].beta0, o);
                out.setValue("subtractionBeta1", res[k].beta1, o);
                out.setValue("subtractionB", res[k].b, o);
                if (res[k].enabled == -1) out.setValue("enabled", -1L, o);
            }
        }
        stack.finish();
        FileName fo(fn_out);
        out.write(fo.path.substr(0, fo.path.find_last_of('.')) + ".xmd");
    }
};

}  // namespace mc
#endif
