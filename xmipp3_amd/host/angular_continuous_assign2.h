// angular_continuous_assign2.h -- xmipp_angular_continuous_assign2: ProgAngularContinuousAssign2
// (reconstruction/angular_continuous_assign2.{h,cpp}) with its search and images behind the C ABI (xh_ca2_*). Same flags and defaults
// (defineParams :112-145), same output metadata (processImage :622-661, postProcess :688-728). The Powell searches of all particles of a
// group advance in lockstep on the device, --batch evaluations per step.
#ifndef XMIPP3_AMD_ANGULAR_CONTINUOUS_ASSIGN2_H
#define XMIPP3_AMD_ANGULAR_CONTINUOUS_ASSIGN2_H
#include "ctf_programs.h"

namespace mc {

class ProgAngularContinuousAssign2 : public XmippProgram {
public:
    std::string fn_in, fn_out, fnVol, originalImageLabel, fnResiduals, fnProjections;
    xh_ca2_params prm;
    bool ignoreCTF = false;
    int device = 0, batch = 4096;

    void defineParams() override
    {
        // angular_continuous_assign2.cpp:112-145 over the -i / -o of XmippMetadataProgram (each image produces an output)
        addUsageLine("Make a continuous angular assignment");
        addUsageLine("+Output labels (xmippCore spellings): imageOriginal, image, angleRot, angleTilt, anglePsi, shiftX, shiftY, flip, cost,");
        addUsageLine("+weightContinuous2, continuousX, continuousY, continuousFlip, continuousScaleX, continuousScaleY, continuousScaleAngle,");
        addUsageLine("+continuousA, continuousB, ctfDefocusU, ctfDefocusV, ctfDefocusAngle, ctfDefocusChange, corrIdx, corrMask, corrWeight,");
        addUsageLine("+imedValue, imageResidual, imageRef. corrWeight is not computed and is written as 0.");
        addParamsLine("   -i <metadata>               : Metadata with initial alignment");
        addParamsLine("   -o <stack>                  : Stack of images prepared for 3D reconstruction; the metadata is written next to it (.xmd)");
        addParamsLine("   --ref <volume>              : Reference volume");
        addParamsLine("  [--max_shift <s=-1>]         : Maximum shift allowed in pixels");
        addParamsLine("  [--max_scale <s=0.02>]       : Maximum scale change");
        addParamsLine("  [--max_angular_change <a=5>] : Maximum angular change allowed (in degrees)");
        addParamsLine("  [--max_defocus_change <d=500>] : Maximum defocus change allowed (in Angstroms)");
        addParamsLine("  [--max_resolution <f=4>]     : Maximum resolution (A)");
        addParamsLine("  [--max_gray_scale <a=0.05>]  : Maximum gray scale change");
        addParamsLine("  [--max_gray_shift <b=0.05>]  : Maximum gray shift change as a factor of the image standard deviation");
        addParamsLine("  [--sampling <Ts=1>]          : Sampling rate (A/pixel)");
        addParamsLine("  [--Rmax <R=-1>]              : Maximum radius (px). -1=Half of volume size");
        addParamsLine("  [--padding <p=2>]            : Padding factor");
        addParamsLine("  [--optimizeGray]             : Optimize gray values");
        addParamsLine("  [--optimizeShift]            : Optimize shift");
        addParamsLine("  [--optimizeScale]            : Optimize scale");
        addParamsLine("  [--optimizeAngles]           : Optimize angles");
        addParamsLine("  [--optimizeDefocus]          : Optimize defocus");
        addParamsLine("  [--ignoreCTF]                : Ignore CTF");
        addParamsLine("  [--applyTo <label=image>]    : Which is the source of images to apply the final transformation");
        addParamsLine("  [--phaseFlipped]             : Input images have been phase flipped");
        addParamsLine("  [--sameDefocus]              : Force defocusU = defocusV");
        addParamsLine("  [--oresiduals <stack=\"\">]  : Output stack for the residuals");
        addParamsLine("  [--oprojections <stack=\"\">] : Output stack for the projections");
        addParamsLine("  [--dev <id=0>]               : GPU device to use (one device only: several are refused)");
        addParamsLine("  [--batch <n=4096>]           : Cost evaluations per device step (searches advancing in lockstep)");
        addParamsLine("  [--nThreads <n=1>]           : accepted for the CUDA program's command lines, ignored");
        addParamsLine("  [--skipThreshold <t=0>]      : accepted for the CUDA program's command lines, ignored");
        addExampleLine("A typical use is:", false);
        addExampleLine("xmipp_angular_continuous_assign2 -i anglesFromDiscreteAssignment.xmd --ref reference.vol -o assigned_angles.stk");
    }

    void readParams() override
    {
        if (!checkParam("-i")) REPORT_ERROR(ERR_ARG_MISSING, "-i is mandatory");
        if (!checkParam("-o")) REPORT_ERROR(ERR_ARG_MISSING, "-o is mandatory");
        if (!checkParam("--ref")) REPORT_ERROR(ERR_ARG_MISSING, "--ref is mandatory");
        fn_in = getParam("-i");
        fn_out = getParam("-o");
        fnVol = getParam("--ref");
        xh_ca2_defaults(&prm);
        prm.max_shift = getDoubleParam("--max_shift");
        prm.max_scale = getDoubleParam("--max_scale");
        prm.max_defocus_change = getDoubleParam("--max_defocus_change");
        prm.max_angular_change = getDoubleParam("--max_angular_change");
        prm.max_resolution = getDoubleParam("--max_resolution");
        prm.max_gray_scale = getDoubleParam("--max_gray_scale");
        prm.max_gray_shift = getDoubleParam("--max_gray_shift");
        prm.sampling = getDoubleParam("--sampling");
        prm.Rmax = (double)getIntParam("--Rmax");
        prm.padding = (double)getIntParam("--padding");
        prm.optimize_gray = checkParam("--optimizeGray");
        prm.optimize_shift = checkParam("--optimizeShift");
        prm.optimize_scale = checkParam("--optimizeScale");
        prm.optimize_angles = checkParam("--optimizeAngles");
        prm.optimize_defocus = checkParam("--optimizeDefocus");
        ignoreCTF = checkParam("--ignoreCTF");
        originalImageLabel = getParam("--applyTo");
        prm.phase_flipped = checkParam("--phaseFlipped");
        prm.same_defocus = checkParam("--sameDefocus");
        fnResiduals = checkParam("--oresiduals") ? getParam("--oresiduals") : std::string();
        fnProjections = checkParam("--oprojections") ? getParam("--oprojections") : std::string();
        if (checkParam("--dev")) device = parseGpuDevice(getParam("--dev"));
        batch = std::max(1, (int)getIntParam("--batch"));
        if (!(prm.optimize_gray || prm.optimize_shift || prm.optimize_scale || prm.optimize_angles || prm.optimize_defocus))
            REPORT_ERROR(ERR_ARG_MISSING, "none of --optimizeGray, --optimizeShift, --optimizeScale, --optimizeAngles, --optimizeDefocus is given: nothing to search");
    }

    static std::string slot(size_t i, const std::string &stack) { return std::to_string(i + 1) + "@" + stack; }

    void run() override
    {
        MetaDataVec md;
        readEnabledRows(fn_in, md);
        const size_t n = md.size();
        if (n == 0) REPORT_ERROR(ERR_MD_NOOBJ, "no enabled images in " + fn_in);
        if (!md.containsLabel("image")) REPORT_ERROR(ERR_MD_BADLABEL, fn_in + ": does not have the image label");
        if (!md.containsLabel(originalImageLabel)) REPORT_ERROR(ERR_MD_BADLABEL, fn_in + ": does not have the --applyTo label " + originalImageLabel);
        if (md.containsLabel("ctfModel") && !md.containsLabel("ctfDefocusU") && !ignoreCTF)
            REPORT_ERROR(ERR_NOT_IMPLEMENTED, "CTFs given as ctfModel files are not read; give the CTF columns (ctfDefocusU ...) or --ignoreCTF");
        const bool hasCTF = md.containsLabel("ctfDefocusU") && !ignoreCTF;
        // preProcess (:157-222)
        std::vector<float> vol;
        ImageInfo V;
        readImage(fnVol, vol, V);
        if (V.x != V.y || V.x != V.z) REPORT_ERROR(ERR_MULTIDIM_SIZE, "the reference volume must be a cube");
        const size_t D = V.x, per = D * D;
        xh_ctx *ctx = nullptr;
        xhCheck(xh_ctx_create_private(device, &ctx));
        XhOwner<xh_ctx> ctxOwner(ctx);
        DeviceBuffer dvol;
        dvol.upload(ctx, vol.data(), vol.size() * sizeof(float));
        xh_ca2 *h = nullptr;
        xhCheck(xh_ca2_create(ctx, dvol.as<float>(), (int)D, &prm, batch, &h));
        XhOwner<xh_ca2> hOwner(h);
        dvol.release();
        const bool l1 = prm.optimize_gray != 0;

        StackWriter stack(fn_out, D, D, n);
        std::unique_ptr<StackWriter> sres, sproj;
        if (!fnResiduals.empty()) sres.reset(new StackWriter(fnResiduals, D, D, n));
        if (!fnProjections.empty()) sproj.reset(new StackWriter(fnProjections, D, D, n));
        const std::vector<float> zeros(per, 0.f);
        MetaDataVec out;
        out.labels = md.labels;
        std::vector<double> outCost;
        // a group of particles is on the host at a time; its searches share the device steps
        const size_t group = 4096;
        DeviceBuffer dimg;
        dimg.reserve(ctx, 3 * per * sizeof(double));
        std::vector<double> dbl(3 * per);
        std::vector<float> one, fl(per);
        for (size_t g0 = 0; g0 < n; g0 += group) {
            const size_t m = std::min(group, n - g0);
            std::vector<float> imgs(m * per), orig;
            std::vector<xh_ca2_row> rows(m);
            for (size_t k = 0; k < m; ++k) {
                const size_t id = g0 + k;
                std::string fn;
                md.getValue("image", fn, id);
                ImageInfo I;
                readImage(fn, one, I);
                if (I.x != I.y) REPORT_ERROR(ERR_MULTIDIM_SIZE, fn + ": the images must be square");
                if (I.x != D || I.z != 1) REPORT_ERROR(ERR_MULTIDIM_SIZE, fn + ": the images must have the size of the reference volume");
                std::copy(one.begin(), one.end(), imgs.begin() + k * per);
                // processImage :421-445
                xh_ca2_row &r = rows[k];
                readPoseRow(md, id, hasCTF, r);
                r.gray_a = 1; r.gray_b = 0;
                if (md.containsLabel("continuousScaleX")) {
                    r.scale_x = md.getDouble("continuousScaleX", id, 0); r.scale_y = md.getDouble("continuousScaleY", id, 0);
                    r.scale_angle = md.getDouble("continuousScaleAngle", id, 0);
                    r.shift_x = md.getDouble("continuousX", id, 0); r.shift_y = md.getDouble("continuousY", id, 0);
                    r.flip = md.getDouble("continuousFlip", id, 0) != 0;
                }
                if (l1 && md.containsLabel("continuousA")) { r.gray_a = md.getDouble("continuousA", id, 1); r.gray_b = md.getDouble("continuousB", id, 0); }
            }
            xhCheck(xh_ca2_load(h, imgs.data(), (int)m, (int)D, (int)D, rows.data()));
            std::vector<double> X(13 * m), cost(m);
            std::vector<int32_t> iter(m), enabled(m);
            std::vector<int64_t> evals(m);
            xhCheck(xh_ca2_refine(h, X.data(), cost.data(), iter.data(), evals.data(), enabled.data()));
            // the final transform of the --applyTo images (:571-613)
            if (originalImageLabel == "image") orig.swap(imgs);
            else {
                orig.resize(m * per);
                for (size_t k = 0; k < m; ++k) {
                    std::string fn;
                    md.getValue(originalImageLabel, fn, g0 + k);
                    ImageInfo I;
                    readImage(fn, one, I);
                    if (I.x != D || I.y != D || I.z != 1) REPORT_ERROR(ERR_MULTIDIM_SIZE, fn + ": the images must have the size of the reference volume");
                    std::copy(one.begin(), one.end(), orig.begin() + k * per);
                }
            }
            std::vector<float> applied(m * per);
            xhCheck(xh_ca2_apply(h, orig.data(), X.data(), applied.data()));
            // outputs at the final variables: one more evaluation there precedes them (the reference reads what Powell evaluated last,
            // which is generally not the minimum it returns); the enabled particles are evaluated --batch at a time
            std::vector<char> searched(m), ok(m);
            std::vector<double> measures(3 * m, 0.0);
            std::vector<int32_t> pick;
            for (size_t k = 0; k < m; ++k) {
                searched[k] = !(std::fabs(rows[k].scale_x) > prm.max_scale || std::fabs(rows[k].scale_y) > prm.max_scale);   // :489-491
                ok[k] = searched[k] && !(cost[k] > 1e30 || (cost[k] > 0 && !l1));                                          // :523
                stack.write(g0 + k, searched[k] ? &applied[k * per] : zeros.data());
                if (ok[k]) pick.push_back((int32_t)k);
                else {
                    if (sproj) sproj->write(g0 + k, zeros.data());
                    if (sres) sres->write(g0 + k, zeros.data());
                }
            }
            for (size_t c0 = 0; c0 < pick.size(); c0 += (size_t)batch) {
                const size_t mc_ = std::min((size_t)batch, pick.size() - c0);
                std::vector<double> xs(13 * mc_), cs(mc_);
                for (size_t r = 0; r < mc_; ++r) std::copy(&X[13 * (size_t)pick[c0 + r]], &X[13 * (size_t)pick[c0 + r]] + 13, &xs[13 * r]);
                xhCheck(xh_ca2_cost(h, (int)mc_, &pick[c0], xs.data(), cs.data()));
                // xh_ca2_cost keeps a row that is out of bounds off the device (Powell evaluated p + t xi and returns p += t xi, which can
                // round a hair outside a bound): such a row has no images, and the device rows are counted over the others
                int dev = 0;
                for (size_t i = 0; i < mc_; ++i) {
                    const size_t k = (size_t)pick[c0 + i];
                    if (!(cs[i] < 1e30)) {
                        if (sproj) sproj->write(g0 + k, zeros.data());
                        if (sres) sres->write(g0 + k, zeros.data());
                        continue;
                    }
                    const int r = dev++;
                    xhCheck(xh_ca2_measures(h, (int)r, &measures[3 * k]));
                    if (sres || sproj) {
                        xhCheck(xh_ca2_last_images(h, (int)r, dimg.as<double>(), dimg.as<double>() + per, nullptr));
                        xhCheck(xh_memcpy_d2h(ctx, dbl.data(), dimg.p, 2 * per * sizeof(double)));
                        if (sproj) { for (size_t q = 0; q < per; ++q) fl[q] = (float)dbl[q]; sproj->write(g0 + k, fl.data()); }
                        if (sres) { for (size_t q = 0; q < per; ++q) fl[q] = (float)dbl[per + q]; sres->write(g0 + k, fl.data()); }
                    }
                }
            }
            for (size_t k = 0; k < m; ++k) {
                const size_t id = g0 + k;
                const double *p = &X[13 * k];
                if (enabled[k] != 1) continue;                                // postProcess: removeDisabled
                const size_t o = out.addObject();
                for (const std::string &l : md.labels) { std::string v; if (md.getValue(l, v, id)) out.setValue(l, v, o); }
                std::string fnImg;
                md.getValue("image", fnImg, id);
                if (sres) out.setValue("imageResidual", slot(id, fnResiduals), o);
                if (sproj) out.setValue("imageRef", slot(id, fnProjections), o);
                out.setValue("imageOriginal", fnImg, o);
                out.setValue("image", slot(id, fn_out), o);
                out.setValue("angleRot", rows[k].rot + p[7], o);
                out.setValue("angleTilt", rows[k].tilt + p[8], o);
                out.setValue("anglePsi", rows[k].psi + p[9], o);
                out.setValue("shiftX", 0.0, o);
                out.setValue("shiftY", 0.0, o);
                out.setValue("flip", 0L, o);
                outCost.push_back(l1 ? cost[k] : -cost[k]);
                out.setValue("cost", outCost.back(), o);
                if (l1) { out.setValue("continuousA", p[0], o); out.setValue("continuousB", p[1], o); }
                out.setValue("continuousScaleX", p[4], o);
                out.setValue("continuousScaleY", p[5], o);
                out.setValue("continuousScaleAngle", p[6], o);
                out.setValue("continuousX", p[2] + rows[k].shift_x, o);
                out.setValue("continuousY", p[3] + rows[k].shift_y, o);
                out.setValue("continuousFlip", (long)rows[k].flip, o);
                if (hasCTF) {
                    const double U = rows[k].ctf.DeltafU, Vd = rows[k].ctf.DeltafV;
                    out.setValue("ctfDefocusU", U + p[10], o);
                    out.setValue("ctfDefocusV", prm.same_defocus ? U + p[10] : Vd + p[11], o);
                    out.setValue("ctfDefocusAngle", rows[k].ctf.azimuthal_angle + p[12], o);
                    out.setValue("ctfDefocusChange", prm.same_defocus ? 0.5 * (p[10] + p[10]) : 0.5 * (p[10] + p[11]), o);
                }
                out.setValue("corrIdx", measures[3 * k], o);
                out.setValue("corrMask", measures[3 * k + 1], o);
                out.setValue("corrWeight", 0.0, o);
                out.setValue("imedValue", measures[3 * k + 2], o);
            }
        }
        stack.finish();
        if (sres) sres->finish();
        if (sproj) sproj->finish();
        // postProcess (:688-728): weightContinuous2 = minCost / cost (L1), cost / maxCost (correlation)
        double ext = l1 ? 1e38 : -1e38;
        for (double c : outCost) ext = l1 ? std::min(ext, c) : std::max(ext, c);
        for (size_t o = 0; o < out.size(); ++o) out.setValue("weightContinuous2", l1 ? ext / outCost[o] : outCost[o] / ext, o);
        FileName fo(fn_out);
        out.write(fo.path.substr(0, fo.path.find_last_of('.')) + ".xmd");
    }
};

}  // namespace mc
#endif
