// forward_art_zernike3d.h -- xmipp_forward_art_zernike3d: ProgForwardArtZernike3DGPU (reconstruction_adapt_cuda11/
// forward_art_zernike3d_gpu.{h,cpp}) with its forward model, residual and update behind the C ABI (xh_faz_*). Same flags and defaults
// (defineParams :124-173), the same order of presentation (sortOrthogonal :628-690, or the unseeded shuffle of --sort_random :530-539),
// the same output files: <odir>/<basename of -o>, with --debug_iter a _iter<n>.mrc per iteration, with --save_iter a _partial.mrc on the
// schedule of :587-592. The rows it reads are those xmipp_angular_sph_alignment writes; sphCoefficients must hold the 3 vecSize
// coefficients of the degrees (the trailing pose variables of that program's vector are not part of this program's input). The volume
// stays on the device over the whole run; the particles go up in chunks of the presentation order.
#ifndef XMIPP3_AMD_FORWARD_ART_ZERNIKE3D_H
#define XMIPP3_AMD_FORWARD_ART_ZERNIKE3D_H
#include <numeric>
#include <random>
#include "ctf_programs.h"

namespace mc {

class ProgForwardArtZernike3D : public XmippProgram {
public:
    std::string fn_in, fnVolR, fnMaskRF, fnMaskRB, fnOutDir, fnVolO, fnSym;
    xh_faz_params prm;
    std::vector<double> sigma;
    int niter = 1, save_iter = 0, sort_last_N = 2, mr = 0, dSize = 0, device = 0;
    bool resume = false, removeNegValues = false, debug_iter = false, sort_random = false;
    static constexpr size_t kChunkBytes = (size_t)1 << 30;      // prepared particles (doubles) on the device at a time

    void defineParams() override
    {
        addUsageLine("Template-based canonical volume reconstruction through Zernike3D coefficients");
        addParamsLine("   -i <metadata>               : Metadata with initial alignment");
        addParamsLine("   -o <volume>                 : Refined volume");
        addParamsLine("  [--ref <volume=\"\">]        : Reference volume");
        addParamsLine("  [--maskf <m=\"\">]           : ART forward model reconstruction mask");
        addParamsLine("  [--maskb <m=\"\">]           : ART backward model reconstruction mask");
        addParamsLine("  [--odir <outputDir=\".\">]   : Output directory");
        addParamsLine("  [--sampling <Ts=1>]          : Sampling rate (A/pixel)");
        addParamsLine("  [--RDef <r=-1>]              : Maximum radius of the deformation (px). -1=Half of volume size");
        addParamsLine("  [--l1 <l1=3>]                : Degree Zernike Polynomials=1,2,3,...");
        addParamsLine("  [--l2 <l2=2>]                : Harmonical depth of the deformation=1,2,3,...");
        addParamsLine("  [--blobr <b=4>]              : Blob radius for forward mapping splatting");
        addParamsLine("  [--step <step=1>]            : Voxel index step");
        addParamsLine("  [--sigma <Matrix1D=\"2\">]   : Gaussian sigma");
        addParamsLine("  [--mr <mr=0>]                : Muliresolution levels");
        addParamsLine("  [--dSize <ds=0>]             : Muliresolution size");
        addParamsLine("  [--ltv <ltv=1e-4>]           : Total variation regualrization");
        addParamsLine("  [--ltk <ltv=1e-4>]           : Tikhonov regualrization");
        addParamsLine("  [--ll1 <ll1=1e-4>]           : L1 regualrization");
        addParamsLine("  [--lst <ll1=1e-4>]           : Soft threshold regualrization");
        addParamsLine("  [--sym <sym=c1>]             : Symmetry to be considered during the reconstruction");
        addParamsLine("  [--useZernike]               : Correct heterogeneity with Zernike3D coefficients");
        addParamsLine("  [--useCTF]                   : Correct CTF during ART reconstruction");
        addParamsLine("  [--phaseFlipped]             : Input images have been phase flipped");
        addParamsLine("  [--regularization <l=0.01>]  : ART regularization weight");
        addParamsLine("  [--niter <n=1>]              : Number of ART iterations");
        addParamsLine("  [--debug_iter]               : Save volume after each ART iteration");
        addParamsLine("  [--onlyPositive]             : Remove negative values from generated volumes");
        addParamsLine("  [--save_iter <s=0>]          : Save intermidiate volume after #save_iter iterations");
        addParamsLine("  [--sort_last <N=2>]          : The algorithm sorts projections in the most orthogonally possible way. ");
        addParamsLine("  [--sort_random]              : Random sort of projections");
        addParamsLine("                               : The most orthogonal way is defined as choosing the projection which maximizes the ");
        addParamsLine("                               : dot product with the N previous inserted projections. Use -1 to sort with all  ");
        addParamsLine("                               : previous projections");
        addParamsLine("  [--resume]                   : Resume processing");
        addParamsLine("  [--dev <id=0>]               : GPU device to use (one device only: several are refused)");
        addExampleLine("A typical use is:", false);
        addExampleLine("xmipp_forward_art_zernike3d -i anglesFromContinuousAssignment.xmd --ref reference.vol -o assigned_anglesAndDeformations.xmd --l1 3 --l2 2");
    }

    void readParams() override
    {
        fn_in = getParam("-i");
        fnVolR = getParam("--ref");
        fnMaskRF = getParam("--maskf");
        fnMaskRB = getParam("--maskb");
        fnOutDir = getParam("--odir");
        xh_faz_defaults(&prm);
        prm.RDef = (double)getIntParam("--RDef");
        prm.phase_flipped = checkParam("--phaseFlipped");
        prm.use_ctf = checkParam("--useCTF");
        prm.sampling = getDoubleParam("--sampling");
        prm.l1 = (int32_t)getIntParam("--l1");
        prm.l2 = (int32_t)getIntParam("--l2");
        prm.ltv = getDoubleParam("--ltv");
        prm.ltk = getDoubleParam("--ltk");
        prm.ll1 = getDoubleParam("--ll1");
        prm.lst = getDoubleParam("--lst");
        mr = (int)getIntParam("--mr");            // parsed as in the reference; they reach no arithmetic there either
        dSize = (int)getIntParam("--dSize");
        (void)getIntParam("--blobr");
        prm.step = (int32_t)getIntParam("--step");
        prm.use_zernike = checkParam("--useZernike");
        prm.lambda = getDoubleParam("--regularization");
        resume = checkParam("--resume");
        removeNegValues = checkParam("--onlyPositive");
        niter = (int)getIntParam("--niter");
        debug_iter = checkParam("--debug_iter");
        save_iter = (int)getIntParam("--save_iter");
        sort_last_N = (int)getIntParam("--sort_last");
        sort_random = checkParam("--sort_random");
        fnSym = getParam("--sym");
        const std::string outPath = getParam("-o");
        const size_t slash = outPath.rfind('/');
        fnVolO = fnOutDir + "/" + (slash == std::string::npos ? outPath : outPath.substr(slash + 1));
        std::istringstream ss(getParam("--sigma"));
        std::string tok;
        sigma.clear();
        while (ss >> tok) sigma.push_back(atof(tok.c_str()));
        if (sigma.empty()) REPORT_ERROR(ERR_ARG_INCORRECT, "--sigma: no value");
        if (prm.step < 1) REPORT_ERROR(ERR_ARG_INCORRECT, "--step: " + std::to_string(prm.step) + " must be positive");
        device = parseGpuDevice(getParam("--dev"));
        if (xh_faz_check(prm.l1, prm.l2, -1) != XH_OK) REPORT_ERROR(ERR_ARG_INCORRECT, std::string("--l1 / --l2: ") + xh_last_error());
    }

    void show() const
    {
        if (!verbose) return;
        std::cout << "Input metadata:            " << fn_in << std::endl
                  << "Output directory:          " << fnOutDir << std::endl
                  << "Reference volume:          " << fnVolR << std::endl
                  << "Forward model mask:        " << fnMaskRF << std::endl
                  << "Backward model mask:       " << fnMaskRB << std::endl
                  << "Sampling:                  " << prm.sampling << std::endl
                  << "Max. Radius Deform.        " << prm.RDef << std::endl
                  << "Zernike Degree:            " << prm.l1 << std::endl
                  << "SH Degree:                 " << prm.l2 << std::endl
                  << "Step:                      " << prm.step << std::endl
                  << "Symmetry group:            " << fnSym << std::endl
                  << "Correct CTF:               " << prm.use_ctf << std::endl
                  << "Correct heretogeneity:     " << prm.use_zernike << std::endl
                  << "Remove negative values:    " << removeNegValues << std::endl
                  << "Phase flipped:             " << prm.phase_flipped << std::endl
                  << "Regularization:            " << prm.lambda << std::endl
                  << "Number of iterations:      " << niter << std::endl
                  << "Save every # iterations:   " << save_iter << std::endl;
    }

    // "[ v0 v1 ... ]", or the values alone
    static std::vector<double> parseVector(const std::string &s)
    {
        std::string t = s;
        for (char &ch : t)
            if (ch == '[' || ch == ']' || ch == ',') ch = ' ';
        std::istringstream is(t);
        std::vector<double> v;
        double x;
        while (is >> x) v.push_back(x);
        return v;
    }

    // a mask file as preProcess reads it (:229-233): the values truncated to int
    static void readMask(const std::string &fn, size_t D, std::vector<int32_t> &mask)
    {
        std::vector<float> m;
        ImageInfo M;
        readImage(fn, m, M);
        if (M.x != D || M.y != D || M.z != D) REPORT_ERROR(ERR_MULTIDIM_SIZE, fn + ": the mask must have the shape of the volume");
        mask.resize(m.size());
        for (size_t e = 0; e < m.size(); ++e) mask[e] = (int32_t)m[e];
    }

    void writeOut(xh_faz *h, size_t D, const std::string &fn, std::vector<double> &V) const
    {
        xhCheck(xh_faz_get_volume(h, V.data()));      // recoverVol (:496-518)
        if (removeNegValues)
            for (double &v : V)
                if (v < 0.0) v = 0.0;
        writeVolume(fn, V.data(), D, D, D);
    }

    void run() override
    {
        show();
        MetaDataVec md;
        readEnabledRows(fn_in, md);
        if (md.size() == 0) REPORT_ERROR(ERR_MD_NOOBJ, "no enabled images in " + fn_in);
        // preProcess :178-182
        if (!md.containsLabel("angleRot") || !md.containsLabel("angleTilt") || !md.containsLabel("anglePsi"))
            REPORT_ERROR(ERR_MD_MISSINGLABEL, "Input metadata projection angles are missing. Exiting...");
        if (!md.containsLabel("image")) REPORT_ERROR(ERR_MD_BADLABEL, fn_in + ": does not have the image label");
        if (md.containsLabel("ctfModel") && !md.containsLabel("ctfDefocusU") && prm.use_ctf)
            REPORT_ERROR(ERR_NOT_IMPLEMENTED, "CTFs given as ctfModel files are not read; give the CTF columns (ctfDefocusU ...)");
        const bool hasCTF = md.containsLabel("ctfDefocusU") && prm.use_ctf;      // processImage :418
        const size_t n = md.size();
        // the coefficient vectors, checked before a device is touched
        int32_t vecSize = 0;
        std::vector<double> coef;
        if (prm.use_zernike) {
            if (!md.containsLabel("sphCoefficients")) REPORT_ERROR(ERR_MD_MISSINGLABEL, "--useZernike: the metadata has no sphCoefficients column");
            for (size_t id = 0; id < n; ++id) {
                std::string s;
                md.getValue("sphCoefficients", s, id);
                const std::vector<double> v = parseVector(s);
                if (xh_faz_check(prm.l1, prm.l2, (int32_t)v.size()) != XH_OK)
                    REPORT_ERROR(ERR_ARG_INCORRECT, "row " + std::to_string(id + 1) + " of " + fn_in + ": " + xh_last_error());
                coef.insert(coef.end(), v.begin(), v.end());
            }
            vecSize = (int32_t)(coef.size() / n / 3);
        }
        // the volume (:184-210)
        std::vector<float> tmp;
        std::vector<double> V;
        size_t D = 0;
        if (!fnVolR.empty()) {
            ImageInfo I;
            readImage(fnVolR, tmp, I);
            if (I.x != I.y || I.x != I.z) REPORT_ERROR(ERR_MULTIDIM_SIZE, "the reference volume must be a cube (a non-cubic volume is not supported)");
            D = I.x;
            V.assign(tmp.begin(), tmp.end());
        } else {
            std::string fn0;
            md.getValue("image", fn0, 0);
            D = readInfo(fn0).x;
            V.assign(D * D * D, 0.0);
        }
        if (resume && fileExists(fnVolO)) {
            ImageInfo I;
            readImage(fnVolO, tmp, I);
            if (I.x != D || I.y != D || I.z != D) REPORT_ERROR(ERR_MULTIDIM_SIZE, fnVolO + ": the volume to resume from has another size");
            V.assign(tmp.begin(), tmp.end());
        }
        std::vector<int32_t> maskF, maskB;
        if (!fnMaskRF.empty()) readMask(fnMaskRF, D, maskF);
        if (!fnMaskRB.empty()) readMask(fnMaskRB, D, maskB);
        // the symmetry list (:345-357); the left matrices are the identity
        SymList SL;
        SL.readSymmetryFile(fnSym);
        std::vector<double> sym;
        for (const auto &R : SL.R) sym.insert(sym.end(), R.begin(), R.end());
        // the order of presentation
        std::vector<double> rot(n), tilt(n);
        for (size_t id = 0; id < n; ++id) { rot[id] = md.getDouble("angleRot", id, 0); tilt[id] = md.getDouble("angleTilt", id, 0); }
        std::vector<int32_t> order(n);
        if (sort_random) {
            std::vector<size_t> ids(n);
            std::iota(ids.begin(), ids.end(), 0);
            auto rng = std::default_random_engine{};
            std::shuffle(ids.begin(), ids.end(), rng);
            for (size_t i = 0; i < n; ++i) order[i] = (int32_t)ids[i];
        } else {
            if (verbose) std::cout << "Sorting projections orthogonally...\n" << std::endl;
            xhCheck(xh_faz_sort_orthogonal((int32_t)n, rot.data(), tilt.data(), sort_last_N, order.data()));
        }
        std::vector<int32_t> save(n);
        xhCheck(xh_faz_save_schedule((int32_t)n, save_iter, save.data()));

        xh_ctx *ctx = nullptr;
        xhCheck(xh_ctx_create_private(device, &ctx));
        XhOwner<xh_ctx> ctxOwner(ctx);
        xh_faz *h = nullptr;
        xhCheck(xh_faz_create(ctx, (int32_t)D, V.data(), maskF.empty() ? nullptr : maskF.data(), maskB.empty() ? nullptr : maskB.data(), sigma.data(),
                              (int32_t)sigma.size(), sym.empty() ? nullptr : sym.data(), (int32_t)SL.symsNo(), &prm, &h));
        XhOwner<xh_faz> hOwner(h);
        int32_t per = 1;
        xhCheck(xh_faz_info(h, nullptr, nullptr, nullptr, &per));
        const FileName fo(fnVolO);
        const std::string stem = fo.removeAllExtensions();
        const size_t pix = D * D, chunk = std::max<size_t>(1, std::min(n, kChunkBytes / (pix * sizeof(double))));
        size_t loaded0 = n;      // the first image of the chunk on the device (n: none)
        std::vector<float> imgs, one;
        std::vector<xh_faz_row> rows;
        std::vector<double> cchunk, errors;
        for (int iter = 0; iter < niter; ++iter) {
            std::cout << "Running iteration " << iter + 1 << " with lambda=" << prm.lambda << std::endl;
            for (size_t g0 = 0; g0 < n; g0 += chunk) {
                const size_t m = std::min(chunk, n - g0);
                if (loaded0 != g0) {
                    imgs.resize(m * pix);
                    rows.resize(m);
                    cchunk.resize((size_t)3 * vecSize * m);
                    for (size_t k = 0; k < m; ++k) {
                        const size_t id = (size_t)order[g0 + k];
                        std::string fn;
                        md.getValue("image", fn, id);
                        if (verbose >= 2) std::cout << "Processing " << fn << std::endl;
                        ImageInfo I;
                        readImage(fn, one, I);
                        if (I.x != D || I.y != D || I.z != 1) REPORT_ERROR(ERR_MULTIDIM_SIZE, fn + ": the images must have the size of the volume");
                        std::copy(one.begin(), one.end(), imgs.begin() + k * pix);
                        readPoseRow(md, id, hasCTF, rows[k]);      // processImage :401-424
                        if (prm.use_zernike) std::copy(coef.begin() + id * 3 * vecSize, coef.begin() + (id + 1) * 3 * vecSize, cchunk.begin() + k * 3 * vecSize);
                    }
                    xhCheck(xh_faz_load(h, imgs.data(), (int32_t)m, (int32_t)D, (int32_t)D, rows.data(), prm.use_zernike ? cchunk.data() : nullptr));
                    loaded0 = g0;
                }
                // one sweep per stretch between two saves of the partial volume
                size_t a = 0;
                while (a < m) {
                    size_t b = a;
                    while (b < m && !save[g0 + b]) ++b;
                    const size_t cnt = std::min(m, b + 1) - a;
                    errors.resize(cnt * per);
                    xhCheck(xh_faz_sweep(h, (int32_t)a, (int32_t)cnt, errors.data()));
                    if (verbose >= 2)
                        for (size_t k = 0; k < cnt; ++k)
                            for (int s = 0; s < per; ++s) {
                                const size_t id = (size_t)order[g0 + a + k];
                                std::cout << "Error for image " << (long)md.getDouble("itemId", id, (double)(id + 1)) << " (" << g0 + a + k + 1 << ") in iteration "
                                          << iter + 1 << " : " << errors[k * per + s] << std::endl;
                            }
                    if (b < m) writeOut(h, D, stem + "_partial.mrc", V);
                    a += cnt;
                }
            }
            if (debug_iter) writeOut(h, D, stem + "_iter" + std::to_string(iter + 1) + ".mrc", V);
        }
        writeOut(h, D, fnVolO, V);      // finishProcessing :382-386
    }
};

}  // namespace mc
#endif
