// reconstruct_significant.h -- xmipp_reconstruct_significant: ProgReconstructSignificant (reconstruction/reconstruct_significant.cpp)
// with alignImagesConsideringMirrors for every (image, volume, direction) triple and both weightings on the device (xh_rsig_*). Same
// options, defaults, show() text, messages and output files as the reference program. The gallery and the reconstruction are the
// classes of programs.h run in this process on fresh objects; nothing is spawned. No MPI: the rank logic is dropped.
#ifndef XMIPP3_AMD_RECONSTRUCT_SIGNIFICANT_H
#define XMIPP3_AMD_RECONSTRUCT_SIGNIFICANT_H
#include "programs.h"
#include <filesystem>
#include <set>

namespace mc {

class ProgReconstructSignificant : public XmippProgram {
public:
    struct GalleryImage { std::string fnImg; double rot = 0, tilt = 0; };

    std::string fnIn, fnDir, fnSym, fnInit, fnFirstGallery;
    double alpha0 = 0.05, alphaF = 0.005, angularSampling = 5, maxShift = -1, tilt0 = 0, tiltF = 90, angDistance = 10;
    double currentAlpha = 0, deltaAlpha2 = 0;
    int Niter = 10, Nvolumes = 1, numOrientationsPerParticle = 10, iter = 0, device = 0;
    bool keepIntermediateVolumes = false, useImed = false, strict = false, applyFisher = false, doReconstruct = true, useForValidation = false,
         dontCheckMirrors = false;
    MetaDataVec mdIn;
    size_t Xdim = 0;
    std::vector<std::vector<GalleryImage>> mdGallery;
    std::vector<double> images;                    // [Nimgs][Xdim][Xdim]
    std::vector<double> cc, weight;                // [Nimgs][Nvols][Ndirs] of the iteration, as the reference keeps them

    void defineParams() override
    {
        // reconstruct_significant.cpp:39-67
        addUsageLine("Generate 3D reconstructions from projections using random orientations");
        addUsageLine("+Output labels (xmippCore spellings): enabled, maxCC, cost, angleRot, angleTilt, anglePsi, shiftX, shiftY, flip, imageIndex, ref, ref3d,");
        addUsageLine("+weight, weightSignificant.");
        addParamsLine("   -i <md_file>                : Metadata file with input projections");
        addParamsLine("  [--numberOfVolumes <N=1>]    : Number of volumes to reconstruct");
        addParamsLine("  [--initvolumes <md_file=\"\">] : Set of initial volumes. If none is given, a single volume");
        addParamsLine("                               : is reconstructed with random angles assigned to the images");
        addParamsLine("                               : (that start needs xmipp_transform_symmetrize and is refused here)");
        addParamsLine("  [--initgallery <md_file=\"\">]   : Gallery of projections from a single volume");
        addParamsLine("  [--odir <outputDir=\".\">]   : Output directory");
        addParamsLine("  [--sym <symfile=c1>]         : Enforce symmetry in projections (only c1 is available here)");
        addParamsLine("  [--iter <N=10>]              : Number of iterations");
        addParamsLine("  [--alpha0 <N=0.05>]          : Initial significance");
        addParamsLine("  [--alphaF <N=0.005>]         : Final significance");
        addParamsLine("  [--keepIntermediateVolumes]  : Keep the volume of each iteration");
        addParamsLine("  [--angularSampling <a=5>]    : Angular sampling in degrees for generating the projection gallery");
        addParamsLine("  [--maxShift <s=-1>]          : Maximum shift allowed (+-this amount)");
        addParamsLine("  [--minTilt <t=0>]            : Minimum tilt angle");
        addParamsLine("  [--maxTilt <t=90>]           : Maximum tilt angle");
        addParamsLine("  [--useImed]                  : Use Imed for weighting");
        addParamsLine("  [--strictDirection]          : Images not significant for a direction are also discarded");
        addParamsLine("  [--angDistance <a=10>]       : Angular distance");
        addParamsLine("  [--dontApplyFisher]          : Do not select directions using Fisher");
        addParamsLine("                               : (as in the reference, reconstruct_significant.cpp:88, giving this flag switches the Fisher selection ON)");
        addParamsLine("  [--dontReconstruct]          : Do not reconstruct");
        addParamsLine("  [--useForValidation <numOrientationsPerParticle=10>] : Use the program for validation. This number defines the number of possible orientations per particle");
        addParamsLine("  [--dontCheckMirrors]         : Don't check mirrors in the alignment process");
        addParamsLine("  [--device <id=0>]            : HIP device");
    }

    void readParams() override
    {
        // :70-101
        fnIn = getParam("-i");
        fnDir = getParam("--odir");
        fnSym = getParam("--sym");
        fnInit = getParam("--initvolumes");
        alpha0 = getDoubleParam("--alpha0");
        alphaF = getDoubleParam("--alphaF");
        Niter = (int)getIntParam("--iter");
        keepIntermediateVolumes = checkParam("--keepIntermediateVolumes");
        angularSampling = getDoubleParam("--angularSampling");
        maxShift = getDoubleParam("--maxShift");
        tilt0 = getDoubleParam("--minTilt");
        tiltF = getDoubleParam("--maxTilt");
        useImed = checkParam("--useImed");
        strict = checkParam("--strictDirection");
        angDistance = getDoubleParam("--angDistance");
        Nvolumes = (int)getIntParam("--numberOfVolumes");
        applyFisher = checkParam("--dontApplyFisher");
        fnFirstGallery = getParam("--initgallery");
        doReconstruct = !checkParam("--dontReconstruct");
        useForValidation = checkParam("--useForValidation");
        numOrientationsPerParticle = (int)getIntParam("--useForValidation");
        dontCheckMirrors = checkParam("--dontCheckMirrors");
        device = (int)getIntParam("--device");
        if (!doReconstruct) {
            std::cout << "Setting iterations to 1 because of --dontReconstruct\n";
            Niter = 1;      // Make sure that there is a single iteration
        }
        // refused before any device is touched: both need xmipp_transform_symmetrize, a real-space volume symmetriser this project lacks
        if (fnSym != "c1")
            REPORT_ERROR(ERR_NOT_IMPLEMENTED, "--sym " + fnSym + ": the volumes of every iteration would go through xmipp_transform_symmetrize, which is not available; only c1");
        if (fnInit.empty() && fnFirstGallery.empty())
            REPORT_ERROR(ERR_NOT_IMPLEMENTED, "neither --initvolumes nor --initgallery: the random start symmetrises its volume with xmipp_transform_symmetrize, "
                                              "which is not available; give one of the two");
    }

    void show() const
    {
        // :104-141
        if (verbose <= 0) return;
        std::cout << "Input metadata              : " << fnIn << std::endl;
        std::cout << "Output directory            : " << fnDir << std::endl;
        std::cout << "Initial significance        : " << alpha0 << std::endl;
        std::cout << "Final significance          : " << alphaF << std::endl;
        std::cout << "Number of iterations        : " << Niter << std::endl;
        std::cout << "Keep intermediate volumes   : " << keepIntermediateVolumes << std::endl;
        std::cout << "Angular sampling            : " << angularSampling << std::endl;
        std::cout << "Maximum shift               : " << maxShift << std::endl;
        std::cout << "Minimum tilt                : " << tilt0 << std::endl;
        std::cout << "Maximum tilt                : " << tiltF << std::endl;
        std::cout << "Use Imed                    : " << useImed << std::endl;
        std::cout << "Angular distance            : " << angDistance << std::endl;
        std::cout << "Apply Fisher                : " << applyFisher << std::endl;
        std::cout << "Reconstruct                 : " << doReconstruct << std::endl;
        std::cout << "useForValidation            : " << useForValidation << std::endl;
        std::cout << "dontCheckMirrors            : " << dontCheckMirrors << std::endl;
        if (fnSym != "") std::cout << "Symmetry for projections    : " << fnSym << std::endl;
        if (fnFirstGallery == "") {
            if (fnInit != "") std::cout << "Initial volume              : " << fnInit << std::endl;
            else std::cout << "Number of volumes           : " << Nvolumes << std::endl;
        } else
            std::cout << "Gallery                     : " << fnFirstGallery << std::endl;
        if (useForValidation) std::cout << " numOrientationsPerParticle : " << numOrientationsPerParticle << std::endl;
    }

    // The significance of every iteration as the reference's loop computes it: currentAlpha is set back to alpha0 at the top of every
    // iteration (:416) and the deltaAlpha added at its end (:582) never reaches an alignment, so --alphaF has no effect. Kept as written.
    double alphaOfIteration(int) const { return alpha0; }
    void showSchedule() const
    {
        if (verbose <= 0 || useForValidation) return;      // the validation alpha depends on the gallery (numberOfProjections)
        const double deltaAlpha = Niter > 1 ? (alphaF - alpha0) / (Niter - 1) : 0;
        std::cout << "Significance schedule (deltaAlpha " << deltaAlpha << " is added after every iteration and reset before the next, as in the reference):" << std::endl;
        for (int it = 1; it <= Niter; ++it)
            std::cout << "  iteration " << it << ": alpha " << alphaOfIteration(it) << ", significance " << 1 - alphaOfIteration(it) - deltaAlpha2 << std::endl;
    }

    std::string name(const char *what, int it, int nVolume, const char *ext) const
    {
        char b[64];
        snprintf(b, sizeof(b), "/%s_iter%03d_%02d.%s", what, it, nVolume, ext);
        return fnDir + b;
    }
    static void deleteFile(const std::string &fn) { std::remove(fn.c_str()); }

    // one of the classes of programs.h on a fresh object, with a command line
    template <class P> static void runInProcess(P &program, const std::vector<std::string> &args, const char *who)
    {
        std::vector<const char *> argv{who};
        for (auto &a : args) argv.push_back(a.c_str());
        program.read((int)argv.size(), argv.data());
        const int rc = program.tryRun();
        if (rc != 0) REPORT_ERROR(ERR_LOGIC_ERROR, std::string(who) + " failed with code " + std::to_string(rc));
    }

    static std::string fmt(double v) { char b[64]; snprintf(b, sizeof(b), "%f", v); return b; }

    void produceSideinfo()
    {
        // :741-870
        std::error_code ec;
        if (!std::filesystem::exists(fnDir) && !std::filesystem::create_directories(fnDir, ec)) REPORT_ERROR(ERR_IO_NOREAD, "cannot create " + fnDir);
        readEnabledRows(fnIn, mdIn);
        if (mdIn.size() == 0) REPORT_ERROR(ERR_MD_NOOBJ, "No enabled images in " + fnIn);
        for (size_t i = 0; i < mdIn.size(); ++i) {
            for (const char *l : {"maxCC", "angleRot", "angleTilt", "anglePsi", "shiftX", "shiftY"}) mdIn.setValue(l, std::string("0.0"), i);
            mdIn.setValue("weight", std::string("1.0"), i);
        }
        std::vector<float> img;
        for (size_t i = 0; i < mdIn.size(); ++i) {
            std::string fn;
            if (!mdIn.getValue("image", fn, i)) REPORT_ERROR(ERR_MD_BADLABEL, fnIn + ": does not have MDL_IMAGE label");
            ImageInfo I;
            readImage(fn, img, I);
            if (i == 0) {
                Xdim = I.x;
                if (I.x != I.y || I.z != 1) REPORT_ERROR(ERR_MULTIDIM_SIZE, fnIn + ": the images must be square and 2-D");
                if (Xdim % 2 != 0 || Xdim < 16) REPORT_ERROR(ERR_MULTIDIM_SIZE, fnIn + ": images of " + std::to_string(Xdim) + " pixels; an even size of at least 16 is needed");
                images.resize(mdIn.size() * Xdim * Xdim);
            } else if (I.x != Xdim || I.y != Xdim || I.z != 1)
                REPORT_ERROR(ERR_MULTIDIM_SIZE, fnIn + ": " + fn + " differs in size from the first image");
            for (size_t k = 0; k < Xdim * Xdim; ++k) images[i * Xdim * Xdim + k] = img[k];
        }
        if (fnFirstGallery == "") {
            // :822-840: the input volumes as the iteration 0 volumes
            MetaDataVec mdInit;
            mdInit.read(fnInit);
            std::vector<float> V;
            for (size_t idx = 0; idx < mdInit.size(); ++idx) {
                std::string fnVol;
                if (!mdInit.getValue("image", fnVol, idx)) REPORT_ERROR(ERR_MD_BADLABEL, fnInit + ": does not have MDL_IMAGE label");
                ImageInfo I;
                readImage(fnVol, V, I);
                if (I.x != Xdim || I.y != Xdim || I.z != Xdim) REPORT_ERROR(ERR_MULTIDIM_SIZE, fnVol + ": the volume must be a cube of the images' size");
                std::vector<double> Vd(V.begin(), V.end());
                writeVolume(name("volume", 0, (int)idx, "vol"), Vd.data(), Xdim, Xdim, Xdim);
            }
            Nvolumes = (int)mdInit.size();
            if (Nvolumes == 0) REPORT_ERROR(ERR_MD_NOOBJ, "No volumes in " + fnInit);
        } else
            Nvolumes = 1;
        for (int idx = 0; idx < Nvolumes; ++idx) mdIn.write(name("angles", 0, idx, "xmd"));
        mdGallery.assign(Nvolumes, {});
        iter = 0;
    }

    // :628-702: the galleries of this iteration -> [Nvolumes . Ndirs][Xdim][Xdim] doubles
    void generateProjections(std::vector<double> &gallery)
    {
        const bool generate = iter > 1 || fnFirstGallery == "";
        if (generate)
            for (int n = 0; n < Nvolumes; ++n) {
                ProgAngularProjectLibrary lib;
                runInProcess(lib, {"-i", name("volume", iter - 1, n, "vol"), "-o", name("gallery", iter, n, "stk"), "--sampling_rate", fmt(angularSampling), "--sym", fnSym,
                                   "--compute_neighbors", "--angular_distance", "-1", "--experimental_images", name("angles", iter - 1, n, "xmd"), "--min_tilt_angle", fmt(tilt0),
                                   "--max_tilt_angle", fmt(tiltF), "--device", std::to_string(device), "-v", "0"}, "xmipp_angular_project_library");
            }
        gallery.clear();
        std::vector<float> img;
        for (int n = 0; n < Nvolumes; ++n) {
            // :663-672: the given gallery's stack is the metadata file's name with the extension stk
            const std::string fnMeta = generate ? name("gallery", iter, n, "doc") : fnFirstGallery;
            const size_t dot = fnFirstGallery.rfind('.');
            const std::string fnStack = generate ? name("gallery", iter, n, "stk") : fnFirstGallery.substr(0, dot == std::string::npos || dot < fnFirstGallery.rfind('/') + 1 ? std::string::npos : dot) + ".stk";
            MetaDataVec mdAux;
            mdAux.read(fnMeta);
            mdGallery[n].clear();
            for (size_t k = 0; k < mdAux.size(); ++k) {
                GalleryImage I;
                mdAux.getValue("image", I.fnImg, k);
                mdAux.getValue("angleRot", I.rot, k);
                mdAux.getValue("angleTilt", I.tilt, k);
                mdGallery[n].push_back(I);
                // the pixels come from the stack, image k + 1 for row k, not from the row's image name (:671, :683, :695)
                char num[32];
                snprintf(num, sizeof(num), "%06zu@", k + 1);
                const std::string fnProj = num + fnStack;
                ImageInfo info;
                readImage(fnProj, img, info);
                if (info.x != Xdim || info.y != Xdim) REPORT_ERROR(ERR_MULTIDIM_SIZE, fnProj + ": the gallery must have the images' size");
                if (info.n != mdAux.size())
                    REPORT_ERROR(ERR_MULTIDIM_SIZE, fnStack + " holds " + std::to_string(info.n) + " projections, " + fnMeta + " " + std::to_string(mdAux.size()) + " rows");
                gallery.insert(gallery.end(), img.begin(), img.begin() + Xdim * Xdim);
            }
            if (mdGallery[n].size() != mdGallery[0].size()) REPORT_ERROR(ERR_MULTIDIM_SIZE, "the galleries of the volumes differ in size");
        }
        if (mdGallery[0].empty()) REPORT_ERROR(ERR_MD_NOOBJ, "the gallery is empty");
    }

    void numberOfProjections()
    {
        // :704-739
        const double number_of_projections = (double)mdGallery[0].size();
        alpha0 = numOrientationsPerParticle / number_of_projections;
        alphaF = alpha0;
        deltaAlpha2 = 1 / (2 * number_of_projections);
        std::cout << " Changing angular sampling to " << angularSampling << std::endl;
        std::cout << " Number of projections taking into account angular sampling and symmetry " << number_of_projections << std::endl;
        std::cout << " changing alpha0 to " << alpha0 << std::endl;
    }

    // transformationMatrix2Parameters2D of M.inv() (:216-219)
    static void parametersOf(const double *m, bool &flip, double &shiftX, double &shiftY, double &psi)
    {
        double o[9];
        o[0] = m[8] * m[4] - m[7] * m[5]; o[1] = -(m[8] * m[1] - m[7] * m[2]); o[2] = m[5] * m[1] - m[4] * m[2];
        o[3] = -(m[8] * m[3] - m[6] * m[5]); o[4] = m[8] * m[0] - m[6] * m[2]; o[5] = -(m[5] * m[0] - m[3] * m[2]);
        o[6] = m[7] * m[3] - m[6] * m[4]; o[7] = -(m[7] * m[0] - m[6] * m[1]); o[8] = m[4] * m[0] - m[3] * m[1];
        const double t = 1.0 / (m[0] * o[0] + m[3] * o[1] + m[6] * o[2]);
        for (double &v : o) v *= t;
        flip = (o[0] * o[4] - o[1] * o[3]) < 0;
        const int sgn = flip ? -1 : 1;
        const double cosine = sgn * o[0], sine = sgn * o[1];
        const double invScale = 1 / std::sqrt(cosine * cosine + sine * sine);
        shiftX = o[2] * invScale; shiftY = o[5] * invScale;
        psi = std::atan2(sine, cosine) * 180. / M_PI;
    }

    size_t copyInputRow(MetaDataVec &md, size_t i) const
    {
        for (auto &l : mdIn.labels) md.addLabel(l);
        const size_t id = md.addObject();
        for (size_t c = 0; c < mdIn.labels.size(); ++c) md.rows[id][md.col(mdIn.labels[c])] = mdIn.rows[i][c];
        return id;
    }

    // alignImagesToGallery (:145-382), the reweighting by direction (:434-495) and the metadata of the iteration (:497-572).
    // Returns whether a volume was left without images.
    bool alignAndWrite(const std::vector<double> &gallery)
    {
        const size_t Nimgs = mdIn.size(), Nvols = (size_t)Nvolumes, Ndirs = mdGallery[0].size(), G = Nvols * Ndirs, per = Xdim * Xdim, pairs = Nimgs * G;
        const double one_alpha = 1 - currentAlpha - deltaAlpha2;
        std::cout << "Current significance: " << one_alpha << std::endl;
        std::cerr << "Aligning images ...\n";
        if (G > 65535) REPORT_ERROR(ERR_NOT_IMPLEMENTED, std::to_string(G) + " gallery projections: at most 65535 are supported");

        xh_ctx *ctx = nullptr;
        xhCheck(xh_ctx_create_private(device, &ctx));
        XhOwner<xh_ctx> ctxOwner(ctx);
        // M [N][G][9], cc, imed and weight [N][G] stay on the device from the alignment to the end of the direction stage
        const size_t bytesNG = sizeof(double) * 12 * pairs;
        void *pNG = nullptr;
        if (xh_malloc(ctx, bytesNG, &pNG) != XH_OK)
            REPORT_ERROR(ERR_GPU, "the alignment of " + std::to_string(Nimgs) + " images against " + std::to_string(G) + " projections keeps " + std::to_string(bytesNG) +
                                  " bytes of matrices, correlations, imed and weights on the device, which do not fit: " + xh_last_error());
        DeviceBuffer dNG;
        dNG.ctx = ctx; dNG.p = pNG; dNG.bytes = bytesNG;
        double *dM = dNG.as<double>(), *dCC = dM + 9 * pairs, *dImed = dCC + pairs, *dW = dImed + pairs;

        const int cpp = dontCheckMirrors ? 2 : 4;
        const int batch = (int)std::min<size_t>(pairs * cpp, 8192);
        xh_rsig *h = nullptr;
        xhCheck(xh_rsig_create(ctx, (int)Xdim, (int)G, batch, &h));
        XhOwner<xh_rsig> hOwner(h);
        {
            DeviceBuffer dGal;
            dGal.upload(ctx, gallery.data(), sizeof(double) * per * G);
            xhCheck(xh_rsig_load_gallery(h, dGal.as<double>(), (int)G));
        }
        // the images in chunks of at most 256 MiB
        const size_t chunk = std::max<size_t>(1, std::min(Nimgs, ((size_t)256 << 20) / (per * sizeof(double))));
        DeviceBuffer dImgs;
        dImgs.reserve(ctx, sizeof(double) * per * chunk);
        for (size_t i0 = 0; i0 < Nimgs; i0 += chunk) {
            const size_t n = std::min(chunk, Nimgs - i0);
            xhCheck(xh_memcpy_h2d(ctx, dImgs.p, images.data() + i0 * per, sizeof(double) * per * n));
            xhCheck(xh_rsig_align(h, dImgs.as<double>(), (int)n, dontCheckMirrors ? 0 : 1, dM + 9 * i0 * G, dCC + i0 * G, dImed + i0 * G, nullptr, nullptr, nullptr, nullptr, nullptr));
        }
        dImgs.release();
        std::vector<double> rot(G), tilt(G);
        for (size_t v = 0; v < Nvols; ++v)
            for (size_t d = 0; d < Ndirs; ++d) { rot[v * Ndirs + d] = mdGallery[v][d].rot; tilt[v * Ndirs + d] = mdGallery[v][d].tilt; }
        std::cerr << "Readjusting weights ..." << std::endl;
        xhCheck(xh_rsig_weights(h, dM, dCC, dImed, (int)Nimgs, (int)Nvols, (int)Ndirs, rot.data(), tilt.data(), angDistance, one_alpha, applyFisher, useImed, strict, maxShift, dW));
        std::vector<double> M(9 * pairs), imed(pairs);
        cc.resize(pairs); weight.resize(pairs);
        xhCheck(xh_memcpy_d2h(ctx, M.data(), dM, sizeof(double) * 9 * pairs));
        xhCheck(xh_memcpy_d2h(ctx, cc.data(), dCC, sizeof(double) * pairs));           // with the maxShift penalty, as the reference stores them
        xhCheck(xh_memcpy_d2h(ctx, imed.data(), dImed, sizeof(double) * pairs));
        xhCheck(xh_memcpy_d2h(ctx, weight.data(), dW, sizeof(double) * pairs));

        // the rows: per volume, image after image, direction after direction; a pair has a row when its final weight is positive (the
        // reference adds a row for every selected pair and drops those whose weight ended at 0 or below, :515-518)
        std::vector<MetaDataVec> mdPartial(Nvols), mdPM(Nvols);
        for (size_t nImg = 0; nImg < Nimgs; ++nImg) {
            // :249-286: the best assignment for the projection matching
            double bestCorr = -2;
            size_t best = 0;
            for (size_t g = 0; g < G; ++g)
                if (cc[nImg * G + g] > bestCorr) { bestCorr = cc[nImg * G + g]; best = g; }
            bool flip;
            double shiftX, shiftY, anglePsi;
            parametersOf(&M[9 * (nImg * G + best)], flip, shiftX, shiftY, anglePsi);
            if (useForValidation && dontCheckMirrors) flip = false;
            const size_t bestVolume = best / Ndirs;
            if (maxShift < 0 || (maxShift > 0 && std::fabs(shiftX) < maxShift && std::fabs(shiftY) < maxShift)) {
                MetaDataVec &md = mdPM[bestVolume];
                const size_t id = copyInputRow(md, nImg);
                md.setValue("enabled", 1L, id);
                md.setValue("maxCC", bestCorr, id);
                md.setValue("angleRot", mdGallery[bestVolume][best % Ndirs].rot, id);
                md.setValue("angleTilt", mdGallery[bestVolume][best % Ndirs].tilt, id);
                md.setValue("anglePsi", anglePsi, id);
                md.setValue("shiftX", -shiftX, id);
                md.setValue("shiftY", -shiftY, id);
                md.setValue("flip", flip ? 1L : 0L, id);
            }
            for (size_t g = 0; g < G; ++g) {
                const size_t p = nImg * G + g, nVolume = g / Ndirs, nDir = g % Ndirs;
                if (!(weight[p] > 0)) continue;
                parametersOf(&M[9 * p], flip, shiftX, shiftY, anglePsi);
                if (useForValidation && dontCheckMirrors) flip = false;
                if (flip) shiftX *= -1;
                MetaDataVec &md = mdPartial[nVolume];
                const size_t id = copyInputRow(md, nImg);
                md.setValue("enabled", 1L, id);
                md.setValue("maxCC", cc[p], id);
                md.setValue("cost", imed[p], id);
                md.setValue("angleRot", mdGallery[nVolume][nDir].rot, id);
                md.setValue("angleTilt", mdGallery[nVolume][nDir].tilt, id);
                md.setValue("anglePsi", anglePsi, id);
                md.setValue("shiftX", -shiftX, id);
                md.setValue("shiftY", -shiftY, id);
                md.setValue("flip", flip ? 1L : 0L, id);
                md.setValue("imageIndex", (long)nImg, id);
                md.setValue("ref", (long)nDir, id);
                md.setValue("ref3d", (long)nVolume, id);
                md.setValue("weight", weight[p], id);
                md.setValue("weightSignificant", weight[p], id);
            }
        }
        bool emptyVolumes = false;
        for (size_t nVolume = 0; nVolume < Nvols; ++nVolume) {
            const int nv = (int)nVolume;
            const std::string fnAngles = name("angles", iter, nv, "xmd");
            if (mdPartial[nVolume].size() > 0) mdPartial[nVolume].write(fnAngles);
            else {
                std::cout << fnAngles << " is empty. Not written." << std::endl;
                emptyVolumes = true;
            }
            if (mdPM[nVolume].size() > 0 && fileExists(fnAngles)) {
                mdPM[nVolume].write(name("images", iter, nv, "xmd"));
                // :535-550, the three xmipp_metadata_utilities calls: the rows of images whose image name occurs in angles
                std::set<std::string> names;
                std::string s;
                for (size_t k = 0; k < mdPartial[nVolume].size(); ++k)
                    if (mdPartial[nVolume].getValue("image", s, k)) names.insert(s);
                MetaDataVec sig;
                sig.labels = mdPM[nVolume].labels;
                for (size_t k = 0; k < mdPM[nVolume].size(); ++k)
                    if (mdPM[nVolume].getValue("image", s, k) && names.count(s)) sig.rows.push_back(mdPM[nVolume].rows[k]);
                sig.write(name("images_significant", iter, nv, "xmd"));
            } else
                std::cout << name("images", iter, nv, "xmd") << " empty. Not written." << std::endl;
            deleteFile(fnDir + "/gallery_iter" + iterTag(iter, nv) + "_sampling.xmd");
            deleteFile(name("gallery", iter, nv, "doc"));
            deleteFile(name("gallery", iter, nv, "stk"));
            if (iter >= 1 && !keepIntermediateVolumes) {
                deleteFile(name("volume", iter - 1, nv, "vol"));
                deleteFile(name("images", iter - 1, nv, "xmd"));
                deleteFile(name("angles", iter - 1, nv, "xmd"));
                deleteFile(name("images_significant", iter - 1, nv, "xmd"));
            }
        }
        if (verbose >= 2) {
            char b[64];
            snprintf(b, sizeof(b), "/cc_iter%03d.vol", iter);
            writeVolume(fnDir + b, cc.data(), Ndirs, Nvols, Nimgs);
            snprintf(b, sizeof(b), "/weight_iter%03d.vol", iter);
            writeVolume(fnDir + b, weight.data(), Ndirs, Nvols, Nimgs);
        }
        return emptyVolumes;
    }
    static std::string iterTag(int it, int nVolume) { char b[32]; snprintf(b, sizeof(b), "%03d_%02d", it, nVolume); return b; }

    // :589-626: xmipp_reconstruct_fourier --sym c1 --weight in its double-precision form, then transform_mask --mask circular -Xdim/2
    void reconstructCurrent()
    {
        std::cerr << "Reconstructing volumes ..." << std::endl;
        for (int nVolume = 0; nVolume < Nvolumes; ++nVolume) {
            const std::string fnAngles = name("angles", iter, nVolume, "xmd"), fnVolume = name("volume", iter, nVolume, "vol");
            if (!fileExists(fnAngles)) continue;
            MetaDataVec MD;
            MD.read(fnAngles);
            std::cout << "Volume " << nVolume << ": number of images=" << MD.size() << std::endl;
            std::cout << "xmipp_reconstruct_fourier -i " << fnAngles << " -o " << fnVolume << " --sym " << fnSym << " --weight -v 0" << std::endl;
            {
                ProgRecFourierAccel rec;
                rec.rfArithmetic = true;
                runInProcess(rec, {"-i", fnAngles, "-o", fnVolume, "--sym", fnSym, "--weight", "--device", std::to_string(device), "-v", "0"}, "xmipp_reconstruct_fourier");
            }
            std::cout << "xmipp_transform_mask -i " << fnVolume << " --mask circular -" << Xdim / 2 << " -v 0" << std::endl;
            std::vector<float> V;
            ImageInfo I;
            readImage(fnVolume, V, I);
            std::vector<int32_t> mask(V.size());
            xhCheck(xh_halves_circular_mask((int)I.z, (int)I.y, (int)I.x, -(double)(Xdim / 2), 0, 0, 0, mask.data()));
            std::vector<double> Vd(V.size());
            for (size_t k = 0; k < V.size(); ++k) Vd[k] = mask[k] ? (double)V[k] : 0.0;
            writeVolume(fnVolume, Vd.data(), I.x, I.y, I.z);
        }
    }

    void run() override
    {
        // :386-587
        show();
        showSchedule();
        produceSideinfo();
        std::vector<double> gallery;
        for (iter = 1; iter <= Niter; iter++) {
            std::cout << "\nIteration " << iter << std::endl;
            generateProjections(gallery);
            if (useForValidation) numberOfProjections();
            currentAlpha = alpha0;
            const double deltaAlpha = Niter > 1 ? (alphaF - alpha0) / (Niter - 1) : 0;
            const bool emptyVolumes = alignAndWrite(gallery);
            if (doReconstruct) reconstructCurrent();
            else break;
            currentAlpha += deltaAlpha;
            if (emptyVolumes) break;
        }
    }
};

}  // namespace mc
#endif
