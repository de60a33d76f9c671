// align_significant.h -- xmipp_align_significant: AProgAlignSignificant (reconstruction/aalign_significant.cpp) with the device side of
// ProgAlignSignificantGPU (reconstruction_adapt_cuda/align_significant_gpu.cpp) behind the C ABI (xh_align_sig_*). Same flags, error
// messages, refusals and output metadata as the reference program.
#ifndef XMIPP3_AMD_ALIGN_SIGNIFICANT_H
#define XMIPP3_AMD_ALIGN_SIGNIFICANT_H
#include "programs.h"
#include <filesystem>

namespace mc {

class ProgAlignSignificant : public XmippProgram {
public:
    struct Data {
        std::string fn;
        MetaDataVec md;
        size_t x = 0, y = 0, n = 0;
        std::vector<float> data;                 // [n][y][x], cropped to even sizes
        std::vector<float> rots, tilts;          // references only
        std::vector<long> indexes;               // references only: their `ref` values
    };
    struct Assignment {
        size_t refIndex, imgIndex;
        float weight, merit;
        float pose[9];
    };

    Data refs, imgs;
    std::string fnOut, fnStk, fnXmd;
    double angDistance = 10;
    size_t keepBestN = 1;
    bool allowSwap = false, useWeight = false, doUpdate = false;
    int device = 0;
    std::vector<Assignment> assignments;

    void defineParams() override
    {
        // aalign_significant.cpp:35-44 and align_significant_gpu.cpp:31-34
        addUsageLine("Find alignment of the experimental images in respect to a set of references");
        addUsageLine("+Output labels (xmippCore spellings): enabled, angleRot, angleTilt, weightSignificant, weight, anglePsi, shiftX, shiftY,");
        addUsageLine("+flip, ref, imageIndex, maxCC; the updated references' blocks: classes@ with ref, image, classCount and class%06d_images@.");
        addParamsLine("   -i <md_file>                    : Metadata file with the experimental images");
        addParamsLine("   -r <md_file>                    : Metadata file with the reference images");
        addParamsLine("   -o <md_file>                    : Resulting metadata file with the aligned images");
        addParamsLine("   [--thr <N=-1>]                  : Maximal number of the processing CPU threads");
        addParamsLine("   [--angDistance <a=10>]          : Angular distance");
        addParamsLine("   [--odir <outputDir=\".\">]      : Output directory");
        addParamsLine("   [--keepBestN <N=1>]             : For each image, store N best alignments to references. N must be smaller than no. of references");
        addParamsLine("   [--allowInputSwap]              : Allow swapping reference and experimental images");
        addParamsLine("   [--useWeightInsteadOfCC]        : Select the best reference using weight, instead of CC");
        addParamsLine("   [--oUpdatedRefs <baseName=\"\">]: Update references using assigned experimental images. Store result here");
        addParamsLine("  [--dev <...>]                    : space-separated list of GPU device(s) to use. Single, 0th GPU used by default");
        addParamsLine("                                   : (one device only: several are refused)");
    }

    void readParams() override
    {
        if (!checkParam("-i")) REPORT_ERROR(ERR_ARG_MISSING, "-i is mandatory");
        if (!checkParam("-r")) REPORT_ERROR(ERR_ARG_MISSING, "-r is mandatory");
        if (!checkParam("-o")) REPORT_ERROR(ERR_ARG_MISSING, "-o is mandatory");
        imgs.fn = getParam("-i");
        refs.fn = getParam("-r");
        const std::string outDir = getParam("--odir");
        std::error_code ec;
        if (!std::filesystem::exists(outDir) && !std::filesystem::create_directories(outDir, ec))
            REPORT_ERROR(ERR_IO_NOREAD, "cannot create " + outDir);
        fnOut = outDir + "/" + getParam("-o");
        angDistance = getDoubleParam("--angDistance");
        const long best = getIntParam("--keepBestN");
        if (best < 0) REPORT_ERROR(ERR_ARG_INCORRECT, "--keepBestN must not be negative");
        keepBestN = (size_t)best;
        allowSwap = checkParam("--allowInputSwap");
        useWeight = checkParam("--useWeightInsteadOfCC");
        doUpdate = checkParam("--oUpdatedRefs");
        if (doUpdate) {
            const std::string base = outDir + "/" + getParam("--oUpdatedRefs");
            fnStk = base + ".stk";
            fnXmd = base + ".xmd";
        }
        if (checkParam("--dev")) {
            const std::string a = getParam("--dev");
            char *end = nullptr;
            const long d = strtol(a.c_str(), &end, 10);
            if (a.empty() || *end) REPORT_ERROR(ERR_ARG_INCORRECT, "Invalid GPU device '" + a + "'");
            if (d < 0) REPORT_ERROR(ERR_ARG_INCORRECT, "Invalid GPU device '" + a + "' (must be non-negative number)");
            device = (int)d;
        }
    }

    void show() const
    {
        if (verbose < 1) return;
        std::cout << "Input metadata              : " << imgs.fn << "\n";
        std::cout << "Reference metadata          : " << refs.fn << "\n";
        std::cout << "Output metadata             : " << fnOut << "\n";
        std::cout << "Angular distance            : " << angDistance << "\n";
        std::cout << "Best references kept        : " << keepBestN << "\n";
        if (doUpdate) std::cout << "Updated references          : " << fnXmd << "\n";
        std::cout << "Device(s)                   : " << device << std::endl;
    }

    // load (:94-190) and validate (:192-204): disabled rows dropped, odd sizes cropped to even ones
    void load(Data &h, bool isRef)
    {
        const size_t origN = readEnabledRows(h.fn, h.md);
        h.n = h.md.size();
        if (isRef && origN != h.n) std::cerr << h.fn << " contains disabled images. This is not expected and might lead to wrong result\n";
        if (!h.md.containsLabel("image")) REPORT_ERROR(ERR_MD_BADLABEL, h.fn + ": does not have MDL_IMAGE label");
        if (isRef && !h.md.containsLabel("ref")) REPORT_ERROR(ERR_MD_BADLABEL, h.fn + ": missing MDL_REF label");
        if (h.n == 0) REPORT_ERROR(ERR_MD_NOOBJ, "No enabled images in " + h.fn);
        if (isRef) {
            if (!h.md.containsLabel("angleRot")) std::cerr << "No roration specified for reference images. Using 0 by default\n";
            if (!h.md.containsLabel("angleTilt")) std::cerr << "No tilt specified for reference images. Using 0 by default\n";
            for (size_t i = 0; i < h.n; ++i) {
                h.rots.push_back((float)h.md.getDouble("angleRot", i, 0));
                h.tilts.push_back((float)h.md.getDouble("angleTilt", i, 0));
                long v = 0;
                h.md.getValue("ref", v, i);
                h.indexes.push_back(v);
            }
        }
        std::vector<float> img;
        for (size_t i = 0; i < h.n; ++i) {
            std::string name;
            h.md.getValue("image", name, i);
            ImageInfo I;
            readImage(name, img, I);
            if (i == 0) {
                if (I.x != (I.x / 2) * 2 || I.y != (I.y / 2) * 2) std::cerr << "We need an even input (sizes must be multiple of two). Input will be cropped\n";
                h.x = (I.x / 2) * 2; h.y = (I.y / 2) * 2;
                h.data.assign(h.n * h.x * h.y, 0.f);
            } else if (I.x / 2 * 2 != h.x || I.y / 2 * 2 != h.y || I.z != 1) {
                REPORT_ERROR(ERR_MULTIDIM_SIZE, h.fn + ": " + name + " differs in size from the first image");
            }
            for (size_t yy = 0; yy < h.y; ++yy) memcpy(&h.data[(i * h.y + yy) * h.x], &img[yy * I.x], h.x * sizeof(float));
        }
    }

    // check (:206-218)
    void check() const
    {
        if (refs.x != imgs.x || refs.y != imgs.y) REPORT_ERROR(ERR_LOGIC_ERROR, "Dimensions of the images to align and reference images do not match");
        if (keepBestN > refs.n) REPORT_ERROR(ERR_LOGIC_ERROR, "--keepBestN is higher than number of references");
        if (refs.n <= 1) REPORT_ERROR(ERR_LOGIC_ERROR, "We need at least two references");
        if (refs.x != refs.y) REPORT_ERROR(ERR_NOT_IMPLEMENTED, "xmipp_align_significant: only square images are supported");
    }

    // M3x3_INV of a float matrix: float cofactors, the reciprocal of the determinant in double, stored as floats
    static void inverse(const float *m, float *o)
    {
        o[0] = m[8] * m[4] - m[7] * m[5]; o[1] = -(m[8] * m[1] - m[7] * m[2]); o[2] = m[5] * m[1] - m[4] * m[2];
        o[3] = -(m[8] * m[3] - m[6] * m[5]); o[4] = m[8] * m[0] - m[6] * m[2]; o[5] = -(m[5] * m[0] - m[3] * m[2]);
        o[6] = m[7] * m[3] - m[6] * m[4]; o[7] = -(m[7] * m[0] - m[6] * m[1]); o[8] = m[4] * m[0] - m[3] * m[1];
        const double t = 1.0 / (double)(m[0] * o[0] + m[3] * o[1] + m[6] * o[2]);
        for (int q = 0; q < 9; ++q) o[q] = (float)(o[q] * t);
    }

    // fillRow (:314-357): the inverse pose through transformationMatrix2Parameters2D, shifts stored negated
    void fillRow(MetaDataVec &md, size_t id, const Assignment &a) const
    {
        float A[9];
        inverse(a.pose, A);
        const bool flip = (A[0] * A[4] - A[1] * A[3]) < 0;
        const float sgn = flip ? -1.f : 1.f;
        const float cosine = sgn * A[0], sine = sgn * A[1];
        const float scale = std::sqrt(cosine * cosine + sine * sine);
        const float invScale = 1 / scale;
        const float shiftX = A[2] * invScale, shiftY = A[5] * invScale;
        const float psi = (float)(std::atan2(sine, cosine) * 180. / M_PI);
        md.setValue("enabled", 1L, id);
        md.setValue("angleRot", (double)refs.rots.at(a.refIndex), id);
        md.setValue("angleTilt", (double)refs.tilts.at(a.refIndex), id);
        md.setValue("weightSignificant", (double)a.weight, id);
        md.setValue("weight", (double)a.weight, id);
        md.setValue("anglePsi", (double)psi, id);
        md.setValue("shiftX", (double)-shiftX, id);
        md.setValue("shiftY", (double)-shiftY, id);
        md.setValue("flip", flip ? 1L : 0L, id);
        md.setValue("ref", refs.indexes.at(a.refIndex), id);
        long index = (long)a.imgIndex + 1;
        md.getValue("imageIndex", index, id);
        md.setValue("imageIndex", index, id);
    }

    // a new row of md holding image i's input row
    size_t copyImageRow(MetaDataVec &md, size_t i) const
    {
        for (auto &l : imgs.md.labels) md.addLabel(l);
        const size_t id = md.addObject();
        for (size_t c = 0; c < imgs.md.labels.size(); ++c) md.rows[id][md.col(imgs.md.labels[c])] = imgs.md.rows[i][c];
        return id;
    }

    static void checkLogDelete(const std::string &fn)
    {
        if (fileExists(fn)) {
            std::cerr << fn << " exists. It will be overwritten.\n";
            std::remove(fn.c_str());
        }
    }

    void run() override
    {
        show();
        load(imgs, false);
        load(refs, true);
        const bool swapped = allowSwap && refs.n > imgs.n;
        if (swapped) {
            std::cerr << "We are swapping reference images and experimental images. This will enhance the performance. This might lead to worse "
                         "results if the experimental images are not well centered. Use it with care!\n";
            std::swap(refs, imgs);
        }
        check();
        const int D = (int)refs.x;
        const size_t per = (size_t)D * D, R = refs.n, N = imgs.n;

        xh_ctx *ctx = nullptr;
        xhCheck(xh_ctx_create_private(device, &ctx));
        XhOwner<xh_ctx> ctxOwner(ctx);
        xh_align_sig *h = nullptr;
        const int batch = (int)std::min<size_t>(R * N, 1024);
        // room for the R references the alignment loads (the input's references, or its images when the roles are swapped), never for
        // the N images: the update of the references takes its count and loads none
        xhCheck(xh_align_sig_create(ctx, D, (int)R, batch, D / 4, std::max(2, D / 20), (D - 3) / 2, 3, &h));
        XhOwner<xh_align_sig> hOwner(h);
        DeviceBuffer dRefs, dImgs, dPoses, dMerit, dWeights;
        dRefs.reserve(ctx, sizeof(float) * per * R);
        dImgs.reserve(ctx, sizeof(float) * per * N);
        dPoses.reserve(ctx, sizeof(float) * 9 * R * N);
        dMerit.reserve(ctx, sizeof(float) * R * N);
        dWeights.reserve(ctx, sizeof(float) * R * N);
        xhCheck(xh_memcpy_h2d(ctx, dRefs.p, refs.data.data(), sizeof(float) * per * R));
        xhCheck(xh_memcpy_h2d(ctx, dImgs.p, imgs.data.data(), sizeof(float) * per * N));
        xhCheck(xh_align_sig_load_references(h, dRefs.as<float>(), (int)R));
        xhCheck(xh_align_sig_align(h, dImgs.as<float>(), (int)N, dPoses.as<float>(), dMerit.as<float>()));
        std::vector<float> poses(9 * R * N), merit(R * N);
        xhCheck(xh_memcpy_d2h(ctx, poses.data(), dPoses.p, sizeof(float) * poses.size()));
        xhCheck(xh_memcpy_d2h(ctx, merit.data(), dMerit.p, sizeof(float) * merit.size()));

        // from here on in the roles of the input: R0 references, N0 images; an estimation made with swapped roles is read transposed,
        // its pose inverted (the IS_ESTIMATION_TRANSPOSED branches of computeWeightsAndSave and computeAssignment)
        if (swapped) std::swap(refs, imgs);
        const size_t R0 = refs.n, N0 = imgs.n;
        std::vector<float> merit0(R0 * N0), pose0(9 * R0 * N0);
        for (size_t r = 0; r < R0; ++r)
            for (size_t s = 0; s < N0; ++s) {
                const size_t e = swapped ? s * N + r : r * N + s;
                merit0[r * N0 + s] = merit[e];
                if (swapped) inverse(&poses[9 * e], &pose0[9 * (r * N0 + s)]);
                else memcpy(&pose0[9 * (r * N0 + s)], &poses[9 * e], 9 * sizeof(float));
            }
        if (swapped) xhCheck(xh_memcpy_h2d(ctx, dMerit.p, merit0.data(), sizeof(float) * merit0.size()));
        xhCheck(xh_align_sig_weights(h, refs.rots.data(), refs.tilts.data(), angDistance, dMerit.as<float>(), (int)R0, (int)N0, dWeights.as<float>()));
        std::vector<float> weights(R0 * N0);
        xhCheck(xh_memcpy_d2h(ctx, weights.data(), dWeights.p, sizeof(float) * weights.size()));

        // computeAssignment (:372-412): the best keepBestN per image, first maximum, values <= 0 skipped
        for (size_t i = 0; i < N0; ++i) {
            std::vector<float> votes(R0);
            for (size_t r = 0; r < R0; ++r) votes[r] = useWeight ? weights[r * N0 + i] : merit0[r * N0 + i];
            for (size_t k = 0; k < keepBestN; ++k) {
                const size_t r = (size_t)(std::max_element(votes.begin(), votes.end()) - votes.begin());
                const float val = votes[r];
                votes[r] = std::numeric_limits<float>::lowest();
                if (val <= 0) continue;
                Assignment a{r, i, weights[r * N0 + i], val, {}};
                memcpy(a.pose, &pose0[9 * (r * N0 + i)], sizeof(a.pose));
                assignments.push_back(a);
            }
        }
        storeAlignedImages();
        if (doUpdate) updateRefs(ctx, h);
    }

    // storeAlignedImages (:415-468): rows sorted by image, then by the criterion; maxCC is the image's best value
    void storeAlignedImages()
    {
        if (assignments.empty()) { MetaDataVec().write(fnOut); return; }
        const bool w = useWeight;
        std::sort(assignments.begin(), assignments.end(), [w](const Assignment &l, const Assignment &r) {
            return l.imgIndex != r.imgIndex ? l.imgIndex < r.imgIndex : (w ? l.weight > r.weight : l.merit > r.merit);
        });
        MetaDataVec out;
        float maxVote = 0;
        for (size_t k = 0; k < assignments.size(); ++k) {
            const Assignment &a = assignments[k];
            if (k == 0 || assignments[k - 1].imgIndex != a.imgIndex) maxVote = a.merit;
            const size_t id = copyImageRow(out, a.imgIndex);
            fillRow(out, id, a);
            out.setValue("maxCC", (double)maxVote, id);
        }
        out.write(fnOut);
    }

    // updateRefs (:470-573, align_significant_gpu.cpp:174-287): the references rebuilt from their assigned images, base.stk and base.xmd
    void updateRefs(xh_ctx *ctx, xh_align_sig *h)
    {
        if (1 < keepBestN) std::cout << "Each experimental image will contribute to more than one reference image.\n";
        const size_t R = refs.n, per = refs.x * refs.y;
        // the images in the roles of the input (the alignment may have run with them swapped)
        DeviceBuffer dImgs, dOut;
        dImgs.reserve(ctx, sizeof(float) * per * imgs.n);
        dOut.reserve(ctx, sizeof(float) * per * R);
        xhCheck(xh_memcpy_h2d(ctx, dImgs.p, imgs.data.data(), sizeof(float) * per * imgs.n));
        const size_t n = assignments.size();
        std::vector<int32_t> ri(n), ii(n);
        std::vector<float> wt(n), ps(9 * n);
        for (size_t k = 0; k < n; ++k) {
            ri[k] = (int32_t)assignments[k].refIndex; ii[k] = (int32_t)assignments[k].imgIndex; wt[k] = assignments[k].weight;
            memcpy(&ps[9 * k], assignments[k].pose, 9 * sizeof(float));
        }
        xhCheck(xh_align_sig_update_refs(h, dImgs.as<float>(), (int)imgs.n, (int)R, (int)n, ri.data(), ii.data(), wt.data(), ps.data(), dOut.as<float>()));
        std::vector<float> out(per * R);
        xhCheck(xh_memcpy_d2h(ctx, out.data(), dOut.p, sizeof(float) * out.size()));
        checkLogDelete(fnStk);
        writeStack(fnStk, out.data(), refs.x, refs.y, R);
        // saveRefXmd: classes@ (ref, image, classCount), one class%06d_images@ block per non-empty reference, rows sorted by image
        checkLogDelete(fnXmd);
        MetaDataVec classes;
        std::vector<std::vector<const Assignment *>> per_ref(R);
        for (auto &a : assignments) per_ref[a.refIndex].push_back(&a);
        for (size_t r = 0; r < R; ++r) {
            const size_t id = classes.addObject();
            classes.setValue("ref", refs.indexes[r], id);
            char name[64];
            snprintf(name, sizeof(name), "%06zu@", r + 1);
            classes.setValue("image", std::string(name) + fnStk, id);
            classes.setValue("classCount", (long)per_ref[r].size(), id);
        }
        classes.write("classes@" + fnXmd, true);
        for (size_t r = 0; r < R; ++r) {
            if (per_ref[r].empty()) continue;
            auto &v = per_ref[r];
            std::stable_sort(v.begin(), v.end(), [](const Assignment *l, const Assignment *q) { return l->imgIndex < q->imgIndex; });
            MetaDataVec md;
            for (const Assignment *a : v) fillRow(md, copyImageRow(md, a->imgIndex), *a);
            char block[64];
            snprintf(block, sizeof(block), "class%06ld_images@", refs.indexes[r]);
            md.write(block + fnXmd, true);
        }
    }
};

}  // namespace mc
#endif
