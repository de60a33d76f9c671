// angular_sph_alignment.h -- xmipp_angular_sph_alignment: ProgAngularSphAlignment (reconstruction/angular_sph_alignment.{h,cpp}) with
// its cost and its search behind the C ABI (xh_asa_*). Same flags and defaults (defineParams :96-123), same output rows
// (writeImageParameters :424-449): they accumulate in <odir>/sphDone.xmd, which is renamed to -o at the end (finishProcessing :190-193);
// with --resume the images already listed there are skipped. The Powell searches of all particles of a chunk advance in lockstep on the
// device. --useCPU is accepted and ignored: there is one implementation.
// The row writer is this file's own: xmippCore's is not in the reference tree. The reading used: the labels are
// image, enabled, angleRot, angleTilt, anglePsi, shiftX, shiftY, flip, sphDeformation, sphCoefficients, cost; doubles carry 6 decimals;
// the vector is written unquoted as "[ v0 v1 ... ]", every value followed by a space.
#ifndef XMIPP3_AMD_ANGULAR_SPH_ALIGNMENT_H
#define XMIPP3_AMD_ANGULAR_SPH_ALIGNMENT_H
#include <set>
#include "ctf_programs.h"

namespace mc {

class ProgAngularSphAlignment : public XmippProgram {
public:
    std::string fn_in, fn_out, fnVolR, fnMaskR, fnOutDir;
    xh_asa_params prm;
    bool resume = false;
    int device = 0;
    static constexpr int kCapacity = 64;       // evaluations per device step
    static constexpr size_t kChunk = 4096;     // particles on the device at a time

    void defineParams() override
    {
        addUsageLine("Make a continuous angular assignment with deformations");
        addParamsLine("   -i <metadata>               : Metadata with initial alignment");
        addParamsLine("   -o <metadata>               : Metadata with the angular alignment and deformation parameters");
        addParamsLine("   --ref <volume>              : Reference volume");
        addParamsLine("  [--mask <m=\"\">]            : Reference volume mask");
        addParamsLine("  [--odir <outputDir=\".\">]   : Output directory");
        addParamsLine("  [--max_shift <s=-1>]         : Maximum shift allowed in pixels");
        addParamsLine("  [--max_angular_change <a=5>] : Maximum angular change allowed (in degrees)");
        addParamsLine("  [--max_resolution <f=4>]     : Maximum resolution (A)");
        addParamsLine("  [--sampling <Ts=1>]          : Sampling rate (A/pixel)");
        addParamsLine("  [--Rmax <R=-1>]              : Maximum radius (px). -1=Half of volume size");
        addParamsLine("  [--RDef <r=-1>]              : Maximum radius of the deformation (px). -1=Half of volume size");
        addParamsLine("  [--l1 <l1=3>]                : Degree Zernike Polynomials=1,2,3,...");
        addParamsLine("  [--l2 <l2=2>]                : Harmonical depth of the deformation=1,2,3,...");
        addParamsLine("  [--optimizeAlignment]        : Optimize alignment");
        addParamsLine("  [--optimizeDeformation]      : Optimize deformation");
        addParamsLine("  [--optimizeDefocus]          : Optimize defocus");
        addParamsLine("  [--phaseFlipped]             : Input images have been phase flipped");
        addParamsLine("  [--regularization <l=0.01>]  : Regularization weight");
        addParamsLine("  [--resume]                   : Resume processing");
        addParamsLine("  [--device <id=0>]            : GPU device to use");
        addParamsLine("  [--useCPU]                   : accepted for the CUDA program's command lines, ignored");
        addExampleLine("A typical use is:", false);
        addExampleLine("xmipp_angular_sph_alignment -i anglesFromContinuousAssignment.xmd --ref reference.vol -o assigned_anglesAndDeformations.xmd --optimizeAlignment --optimizeDeformation");
    }

    void readParams() override
    {
        fn_in = getParam("-i");
        fn_out = getParam("-o");
        fnVolR = getParam("--ref");
        fnMaskR = getParam("--mask");
        fnOutDir = getParam("--odir");
        xh_asa_defaults(&prm);
        prm.max_shift = getDoubleParam("--max_shift");
        prm.max_angular_change = getDoubleParam("--max_angular_change");
        prm.max_resolution = getDoubleParam("--max_resolution");
        prm.sampling = getDoubleParam("--sampling");
        prm.Rmax = (double)getIntParam("--Rmax");
        prm.RDef = (double)getIntParam("--RDef");
        prm.optimize_alignment = checkParam("--optimizeAlignment");
        prm.optimize_deformation = checkParam("--optimizeDeformation");
        prm.optimize_defocus = checkParam("--optimizeDefocus");
        prm.phase_flipped = checkParam("--phaseFlipped");
        prm.l1 = (int32_t)getIntParam("--l1");
        prm.l2 = (int32_t)getIntParam("--l2");
        prm.lambda = getDoubleParam("--regularization");
        resume = checkParam("--resume");
        device = (int)getIntParam("--device");
        if (device < 0) REPORT_ERROR(ERR_ARG_INCORRECT, "Invalid GPU device '" + getParam("--device") + "'");
        if (checkParam("--useCPU")) std::cerr << "xmipp_angular_sph_alignment: --useCPU is ignored, the cost runs on the device" << std::endl;
        // the degrees the basis is written out for, and at least one stage h = 1 .. l2
        int32_t idx[3 * 45 + 8], n = 0;
        if (xh_asa_stage_active(prm.l1, prm.l2, 0, 0, idx, &n) != XH_OK) REPORT_ERROR(ERR_ARG_INCORRECT, std::string("--l1 / --l2: ") + xh_last_error());
        if (prm.l2 < 1) REPORT_ERROR(ERR_ARG_INCORRECT, "--l2: " + std::to_string(prm.l2) + " leaves no stage to search (the stages are h = 1 .. l2)");
        if (!(prm.optimize_alignment || prm.optimize_deformation || prm.optimize_defocus))
            REPORT_ERROR(ERR_ARG_MISSING, "none of --optimizeAlignment, --optimizeDeformation, --optimizeDefocus is given: nothing to search");
    }

    static const std::vector<std::string> &outLabels()
    {
        static const std::vector<std::string> l = {"image", "enabled", "angleRot", "angleTilt", "anglePsi", "shiftX", "shiftY", "flip",
                                                   "sphDeformation", "sphCoefficients", "cost"};
        return l;
    }

    static std::string cell(const std::string &w) { return " " + (w.size() < 12 ? std::string(12 - w.size(), ' ') : std::string()) + w; }
    static std::string cell(double v) { char b[64]; snprintf(b, sizeof(b), "%.6f", v); return cell(std::string(b)); }

    // createWorkFiles: the header of a fresh sphDone.xmd
    void startDone(const std::string &fnDone) const
    {
        std::ofstream f(fnDone, std::ios::trunc);
        if (!f.good()) REPORT_ERROR(ERR_IO_NOREAD, "cannot write " + fnDone);
        f << "# XMIPP_STAR_1 * \n# \ndata_noname\nloop_\n";
        for (const std::string &l : outLabels()) f << " _" << l << "\n";
    }

    void run() override
    {
        MetaDataVec md;
        readEnabledRows(fn_in, md);
        if (md.size() == 0) REPORT_ERROR(ERR_MD_NOOBJ, "no enabled images in " + fn_in);
        if (!md.containsLabel("image")) REPORT_ERROR(ERR_MD_BADLABEL, fn_in + ": does not have the image label");
        if (md.containsLabel("ctfModel") && !md.containsLabel("ctfDefocusU"))
            REPORT_ERROR(ERR_NOT_IMPLEMENTED, "CTFs given as ctfModel files are not read; give the CTF columns (ctfDefocusU ...)");
        const bool hasCTF = md.containsLabel("ctfDefocusU");      // processImage :314
        // Rerunable: <odir>/sphDone.xmd; --resume keeps it and skips the images it lists
        const std::string fnDone = fnOutDir + "/sphDone.xmd";
        std::set<std::string> done;
        if (resume && fileExists(fnDone)) {
            MetaDataVec d;
            d.read(fnDone);
            for (size_t i = 0; i < d.size(); ++i) { std::string fn; if (d.getValue("image", fn, i)) done.insert(fn); }
        } else
            startDone(fnDone);
        std::vector<size_t> todo;
        for (size_t id = 0; id < md.size(); ++id) {
            std::string fn;
            md.getValue("image", fn, id);
            if (!done.count(fn)) todo.push_back(id);
        }
        if (!todo.empty()) process(md, todo, hasCTF, fnDone);
        // finishProcessing :190-193
        if (std::rename(fnDone.c_str(), fn_out.c_str()) != 0) REPORT_ERROR(ERR_IO_NOREAD, "cannot rename " + fnDone + " to " + fn_out);
    }

    void process(const MetaDataVec &md, const std::vector<size_t> &todo, bool hasCTF, const std::string &fnDone)
    {
        // preProcess (:125-188)
        std::vector<float> vol, maskf;
        ImageInfo V;
        readImage(fnVolR, vol, V);
        if (V.x != V.y || V.x != V.z) REPORT_ERROR(ERR_MULTIDIM_SIZE, "the reference volume must be a cube (a non-cubic volume is not supported)");
        const size_t D = V.x, per = D * D;
        std::vector<int32_t> mask;
        if (!fnMaskR.empty()) {
            ImageInfo M;
            readImage(fnMaskR, maskf, M);
            if (M.x != D || M.y != D || M.z != D) REPORT_ERROR(ERR_MULTIDIM_SIZE, "the mask must have the shape of the reference volume (another shape is not supported)");
            mask.resize(maskf.size());
            for (size_t e = 0; e < maskf.size(); ++e) mask[e] = (int32_t)maskf[e];      // typeCast(aux(), V_mask)
        }
        xh_ctx *ctx = nullptr;
        xhCheck(xh_ctx_create_private(device, &ctx));
        XhOwner<xh_ctx> ctxOwner(ctx);
        DeviceBuffer dvol;
        dvol.reserve(ctx, vol.size() * sizeof(float));
        xhCheck(xh_memcpy_h2d(ctx, dvol.p, vol.data(), vol.size() * sizeof(float)));
        xh_asa *h = nullptr;
        xhCheck(xh_asa_create(ctx, dvol.as<float>(), (int)D, mask.empty() ? nullptr : mask.data(), &prm, kCapacity, &h));
        XhOwner<xh_asa> hOwner(h);
        dvol.release();
        int32_t nvars = 0;
        xhCheck(xh_asa_info(h, nullptr, nullptr, nullptr, &nvars, nullptr));
        std::vector<float> one;
        for (size_t g0 = 0; g0 < todo.size(); g0 += kChunk) {
            const size_t m = std::min(kChunk, todo.size() - g0);
            std::vector<float> imgs(m * per);
            std::vector<xh_asa_row> rows(m);
            std::vector<std::string> names(m);
            for (size_t k = 0; k < m; ++k) {
                const size_t id = todo[g0 + k];
                md.getValue("image", names[k], id);
                ImageInfo I;
                readImage(names[k], one, I);
                if (I.x != D || I.y != D || I.z != 1) REPORT_ERROR(ERR_MULTIDIM_SIZE, names[k] + ": the images must have the size of the reference volume");
                std::copy(one.begin(), one.end(), imgs.begin() + k * per);
                readPoseRow(md, id, hasCTF, rows[k]);      // processImage :304-325
            }
            xhCheck(xh_asa_load(h, imgs.data(), (int)m, (int)D, (int)D, rows.data()));
            std::vector<double> X((size_t)nvars * m), cost(m), deformation(m);
            std::vector<int32_t> iter(m), enabled(m);
            std::vector<int64_t> evals(m);
            xhCheck(xh_asa_refine(h, X.data(), cost.data(), enabled.data(), deformation.data(), iter.data(), evals.data()));
            // writeImageParameters :424-449, appended to sphDone.xmd
            std::string buf;
            for (size_t k = 0; k < m; ++k) {
                const double *p = &X[(size_t)nvars * k], *t = p + (nvars - 8);
                buf += names[k].find(' ') != std::string::npos ? " '" + names[k] + "'" : cell(names[k]);
                buf += cell(std::to_string(enabled[k] == 1 ? 1 : -1));
                buf += cell(rows[k].rot + t[2]);
                buf += cell(rows[k].tilt + t[3]);
                buf += cell(rows[k].psi + t[4]);
                buf += cell(rows[k].shift_x + t[0]);
                buf += cell(rows[k].shift_y + t[1]);
                buf += cell(std::to_string((int)rows[k].flip));
                buf += cell(deformation[k]);
                buf += " [ ";
                for (int v = 0; v < nvars; ++v) { char b[64]; snprintf(b, sizeof(b), "%.6f ", p[v]); buf += b; }
                buf += "]";
                buf += cell(-cost[k]);      // correlation = -cost (:374-375)
                buf += " \n";
            }
            std::ofstream f(fnDone, std::ios::app);
            f << buf;
            f.flush();
            if (!f.good()) REPORT_ERROR(ERR_IO_NOREAD, "short write to " + fnDone);
        }
    }
};

}  // namespace mc
#endif
