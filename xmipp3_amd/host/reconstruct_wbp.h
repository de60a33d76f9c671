// reconstruct_wbp.h -- xmipp_reconstruct_wbp: ProgRecWbp (reconstruction/reconstruct_wbp.{h,cpp}) with the filter and the back-projection
// on the device behind the C ABI (xh_wbp_*). The option lines and defaults of defineParams (:90-160), show() (:52-87), the --weight removal
// of zero-weight rows (:191-197), getAllMatrices (:308-359), getSampledMatrices (:231-305) with make_even_distribution and
// find_nearest_direction (xh_wbp_even_distribution, xh_wbp_nearest_direction), the threshold times totimgs, the "Fourier pixels" line
// (:175-177), plus --device. The "+" that marks --threshold, --filsam and --use_each_image as expert options is not part of their names. --doc is accepted and ignored, as readParams (:38-49) never reads it.
// Kept as written: mat_g[].count = (int) count_imgs[i] in sampled mode (:276), so --weight's weights are truncated there; the directions
// use -tilt (:279, :327), the filter +tilt with -rot and -psi (:447), the back-projection -tilt (:373).
// Refused before any device is opened, each with its reason:
//  - --sym without --use_each_image: the sampled branch expands symmetric copies through the angles of Euler_apply_transf, that is
//    Euler_matrix2angles, whose branch conventions live in xmippCore; as written (:291) it also expands the LAST image's rot and tilt
//    rather than the representative direction's;
//  - symmetry lists with an improper matrix (mirrors, inversion): the reference routes those through extracted angles as well;
//  - images of another size than the first, images that are not square, D > 1024, several devices.
#ifndef XMIPP3_AMD_RECONSTRUCT_WBP_H
#define XMIPP3_AMD_RECONSTRUCT_WBP_H
#include "programs.h"

namespace mc {

class ProgRecWbp : public XmippProgram {
public:
    std::string fn_sel, fn_out, fn_sym;
    double threshold = 0.005, sampling = 5;
    int diameter = -2, device = 0;
    bool do_all_matrices = false, do_weights = false;
    SymList SL;

    void defineParams() override
    {
        addUsageLine("Generate 3D reconstruction from projections using the Weighted BackProjection algorithm.");
        addUsageLine("+This program allows you to generate 3D reconstructions from projections ");
        addUsageLine("+using the Weighted BackProjection algorithm with arbitrary geometry as ");
        addUsageLine("+described by Radermacher, M. (1992) Weighted back-projection methods. ");
        addUsageLine("+Electron Tomography, ed. by J. Frank, Plenum Press.");
        addParamsLine("   -i <input_selfile>          : selection file with input images and Euler angles");
        addParamsLine(" [ -o <name=\"wbp.vol\"> ]     : filename for output volume ");
        addParamsLine(" [ --doc <docfile=\"\"> ]      : Ignore headers and get angles from this docfile ");
        addParamsLine(" [ --radius <int=-1> ]         : Reconstruction radius. int=-1 means radius=dim/2 ");
        addParamsLine("                               : The volume will be zero outside this radius");
        addParamsLine(" [ --sym <sym=\"\"> ]          : Enforce symmetry ");
        addParamsLine("                               :+A symmetry file or point-group description.");
        addParamsLine("                               :+Valid point-group descriptions are: C1, Ci, Cs, Cn ");
        addParamsLine("                               :+(from here on n must be an integer number with no ");
        addParamsLine("                               :+more than 2 digits) Cnv, Cnh, Sn, Dn, Dnv, Dnh, T, ");
        addParamsLine("                               :+Td, Th, O, Oh I, I1, I2, I3, I4, I5, Ih. For a full ");
        addParamsLine("                               :+description of symmetries look at https://i2pc.github.io/docs/Utils/Conventions/index.html#symmetry");
        addParamsLine(" [ --threshold <float=0.005> ]  : Lower (relative) threshold for filter values ");
        addParamsLine("                               :+This is to avoid divisions by zero and consequent ");
        addParamsLine("                               :+enhancement of noise. The threshold is given as a relative ");
        addParamsLine("                               :+value with respect to the total number of images. The absolute");
        addParamsLine("                               :+threshold will be calculated internally as the relative threshold");
        addParamsLine("                               :+multiplied by the total number of (symmetry generated) projections.");
        addParamsLine(" [ --filsam <float=5>]         : Angular sampling rate for geometry filter ");
        addParamsLine("                               :+Instead of summing over all experimental images to calculate ");
        addParamsLine("                               :+the arbitrary geometry filter, we bin all images in representative ");
        addParamsLine("                               :+projection directions, which are sampled every filsam degrees.");
        addParamsLine(" [ --use_each_image]           : Use each image instead of sampled representatives for filter ");
        addParamsLine("                               :+If this option is given, all experimental images will be used ");
        addParamsLine("                               :+in the summation to calculate the arbitrary geometry filter. For ");
        addParamsLine("                               :+large datasets this may be considerably slower than the default ");
        addParamsLine("                               :+option of using representative projection directions");
        addParamsLine(" [ --weight]                   : Use weights stored in image headers or the input metadata");
        addParamsLine(" [ --device <id=0>]            : HIP device (one device only)");
        addExampleLine("xmipp_reconstruct_wbp -i images.sel -o reconstruction.vol");
    }

    void readParams() override
    {
        // reconstruct_wbp.cpp:38-49
        fn_sel = getParam("-i");
        fn_out = getParam("-o");
        fn_sym = getParam("--sym");
        threshold = getDoubleParam("--threshold");
        diameter = 2 * (int)getIntParam("--radius");
        sampling = getDoubleParam("--filsam");
        do_all_matrices = checkParam("--use_each_image");
        do_weights = checkParam("--weight");
        const std::string dev = getParam("--device");
        // refused before any device is touched
        if (dev.find(',') != std::string::npos) REPORT_ERROR(ERR_ARG_INCORRECT, "--device " + dev + ": this program runs on one device");
        device = parseGpuDevice(dev);
        if (fn_sym != "" && !do_all_matrices)
            REPORT_ERROR(ERR_NOT_IMPLEMENTED, "--sym without --use_each_image: the sampled filter expands the symmetric directions through the angles of Euler_apply_transf "
                                              "(Euler_matrix2angles), which is not available, and as written it expands the last image's angles rather than the "
                                              "representative direction's; add --use_each_image");
        if (!do_all_matrices && !(sampling >= 0.5 && sampling <= 180)) REPORT_ERROR(ERR_ARG_INCORRECT, "--filsam " + getParam("--filsam") + ": a sampling between 0.5 and 180 degrees is expected");
    }

    void show() const
    {
        // reconstruct_wbp.cpp:52-87
        if (verbose == 0) return;
        std::cerr << " =================================================================" << std::endl;
        std::cerr << " Weighted-back projection (arbitrary geometry) " << std::endl;
        std::cerr << " =================================================================" << std::endl;
        std::cerr << " Input selfile             : " << fn_sel << std::endl;
        std::cerr << " Output volume             : " << fn_out << std::endl;
        if (diameter > 0) std::cerr << " Reconstruction radius     : " << diameter / 2 << std::endl;
        std::cerr << " Relative filter threshold : " << threshold << std::endl;
        if (fn_sym != "") std::cerr << " Symmetry file:            : " << fn_sym << std::endl;
        if (do_all_matrices) std::cerr << " --> Use all projection directions in arbitrary geometry filter" << std::endl;
        else std::cerr << " --> Use sampled directions for filter, sampling = " << sampling << std::endl;
        if (do_weights) std::cerr << " --> Use weights stored in the image headers" << std::endl;
        std::cerr << " -----------------------------------------------------------------" << std::endl;
    }

    struct Row { std::string image; double rot = 0, tilt = 0, psi = 0, xoff = 0, yoff = 0, weight = 1; bool flip = false; };

    void run() override
    {
        show();
        // ---- produceSideInfo :187-215
        MetaDataVec SF;
        readEnabledRows(fn_sel, SF);
        if (!SF.containsLabel("image")) REPORT_ERROR(ERR_MD_MISSINGLABEL, "the input metadata has no image column");
        std::vector<Row> rows;
        for (size_t r = 0; r < SF.size(); ++r) {
            Row q;
            SF.getValue("image", q.image, r);
            // getAnglesForImage :217-229
            q.rot = SF.getDouble("angleRot", r, 0);
            q.tilt = SF.getDouble("angleTilt", r, 0);
            q.psi = SF.getDouble("anglePsi", r, 0);
            q.xoff = SF.getDouble("shiftX", r, 0);
            q.yoff = SF.getDouble("shiftY", r, 0);
            q.flip = SF.getDouble("flip", r, 0) != 0;
            q.weight = SF.getDouble("weight", r, 1);
            if (do_weights && SF.containsLabel("weight") && q.weight == 0.0) continue;       // SF.removeObjects(MDValueEQ(MDL_WEIGHT, 0.0))
            rows.push_back(q);
        }
        if (do_weights && rows.empty()) REPORT_ERROR(ERR_MD_NOOBJ, "there is no input file with weight!=0");
        if (rows.empty()) REPORT_ERROR(ERR_MD_NOOBJ, "no input images");
        const ImageInfo I0 = readInfo(rows[0].image);
        if (I0.x != I0.y || I0.z != 1) REPORT_ERROR(ERR_MATRIX_DIM, "images of " + std::to_string(I0.x) + " x " + std::to_string(I0.y) + " x " + std::to_string(I0.z) + ": square images are expected");
        if (I0.x < 2 || I0.x > 1024) REPORT_ERROR(ERR_MATRIX_DIM, "images of " + std::to_string(I0.x) + " pixels a side are not supported (2 .. 1024)");
        const int dim = (int)I0.x;
        for (const Row &q : rows) {
            const ImageInfo I = readInfo(q.image);
            if (I.x != I0.x || I.y != I0.y || I.z != 1)
                REPORT_ERROR(ERR_MATRIX_DIM, q.image + " is " + std::to_string(I.x) + " x " + std::to_string(I.y) + ", the first image " + std::to_string(I0.x) + " x " + std::to_string(I0.y));
        }
        if (fn_sym != "") {
            SL.readSymmetryFile(fn_sym);
            if (SL.hasImproper())
                REPORT_ERROR(ERR_NOT_IMPLEMENTED, "--sym " + fn_sym + ": a group with mirrors or an inversion; the reference forms their directions through extracted angles "
                                                  "(Euler_matrix2angles), which is not available");
        }
        if (diameter <= 0) diameter = dim;
        if (diameter > dim) REPORT_ERROR(ERR_ARG_INCORRECT, "--radius " + std::to_string(diameter / 2) + ": beyond half the image (" + std::to_string(dim) + " pixels) the reference reads past its sinc table");

        // ---- the matrices of every image, the direction list
        const size_t n = rows.size();
        std::vector<double> hrows(22 * n), dirs(3 * n);
        for (size_t r = 0; r < n; ++r) {
            double *q = &hrows[22 * r];
            q[0] = rows[r].xoff; q[1] = rows[r].yoff; q[2] = rows[r].flip ? 1 : 0; q[3] = do_weights ? rows[r].weight : 1.0;
            xhCheck(xh_wbp_image_matrices(rows[r].rot, rows[r].tilt, rows[r].psi, &dirs[3 * r], q + 4, q + 13));
        }
        std::vector<double> mat_g;
        double totimgs = 0.;
        if (do_all_matrices) getAllMatrices(rows, dirs, mat_g, totimgs);
        else getSampledMatrices(rows, mat_g, totimgs);
        if (mat_g.empty()) REPORT_ERROR(ERR_MD_NOOBJ, "no projection direction has a positive count");
        // Adjust relative threshold
        const double absThreshold = threshold * totimgs;

        // ---- the device: apply2DFilterArbitraryGeometry :517-580
        xh_ctx *ctx = nullptr;
        xhCheck(xh_ctx_create_private(device, &ctx));
        XhOwner<xh_ctx> ctxOwner(ctx);
        const int capacity = (int)std::max<size_t>(1, std::min<size_t>({n, (size_t)256, ((size_t)1 << 28) / ((size_t)dim * dim * 8)}));
        xh_wbp *h = nullptr;
        xhCheck(xh_wbp_create(ctx, dim, capacity, &h));
        XhOwner<xh_wbp> hOwner(h);
        xhCheck(xh_wbp_set_directions(h, mat_g.data(), (int)(mat_g.size() / 4), absThreshold, diameter));
        if (verbose > 0) std::cerr << "--> Back-projecting ..." << std::endl;
        const size_t per = (size_t)dim * dim;
        std::vector<float> batch(per * capacity), f;
        ImageInfo J;
        for (size_t i0 = 0; i0 < n; i0 += capacity) {
            const size_t m = std::min<size_t>(capacity, n - i0);
            for (size_t t = 0; t < m; ++t) {
                readImage(rows[i0 + t].image, f, J);
                std::copy(f.begin(), f.begin() + per, batch.begin() + t * per);
            }
            xhCheck(xh_wbp_add(h, batch.data(), &hrows[22 * i0], (int)m, nullptr));
        }
        std::vector<double> R;
        for (int i = 0; i < SL.symsNo(); ++i) R.insert(R.end(), SL.R[i].begin(), SL.R[i].end());
        xhCheck(xh_wbp_finish(h, R.empty() ? nullptr : R.data(), SL.symsNo()));
        std::vector<double> V(per * dim);
        xhCheck(xh_wbp_volume(h, V.data()));
        int64_t count_thr = 0;
        xhCheck(xh_wbp_count_thr(h, &count_thr));
        // finishProcessing :170-179
        if (verbose > 0)
            std::cerr << "Fourier pixels for which the threshold was not reached: " << (float)(count_thr * 100.) / (n * dim * dim) << " %" << std::endl;
        writeVolume(fn_out, V.data(), dim, dim, dim);
    }

    // getAllMatrices :308-359. A symmetric copy's direction is row 2 of L E(rot, -tilt, psi) R taken from the matrix itself (L is the
    // identity for a proper group), where the reference extracts angles from that matrix and forms the matrix of the angles again
    void getAllMatrices(const std::vector<Row> &rows, const std::vector<double> &dirs, std::vector<double> &mat_g, double &totimgs) const
    {
        for (size_t r = 0; r < rows.size(); ++r) {
            const double *e = &dirs[3 * r];
            const double count = do_weights ? rows[r].weight : 1.;
            mat_g.insert(mat_g.end(), {e[0], e[1], e[2], count});
            totimgs += count;
            for (int i = 0; i < SL.symsNo(); ++i) {
                const std::vector<double> &S = SL.R[i];
                double g[3];
                for (int j = 0; j < 3; ++j) {
                    double s = 0;
                    for (int k = 0; k < 3; ++k) s += e[k] * S[3 * k + j];
                    g[j] = s;
                }
                mat_g.insert(mat_g.end(), {g[0], g[1], g[2], count});
                totimgs += count;
            }
        }
    }

    // getSampledMatrices :231-305, without symmetry
    void getSampledMatrices(const std::vector<Row> &rows, std::vector<double> &mat_g, double &totimgs) const
    {
        if (verbose > 0) std::cerr << "--> Sampling the filter ..." << std::endl;
        int32_t NN = 0;
        xhCheck(xh_wbp_even_distribution(sampling, nullptr, nullptr, 0, &NN));
        std::vector<double> rotList(NN), tiltList(NN), count_imgs(NN, 0.);
        xhCheck(xh_wbp_even_distribution(sampling, rotList.data(), tiltList.data(), NN, &NN));
        for (const Row &q : rows) {
            int32_t idx = -1;
            xhCheck(xh_wbp_nearest_direction(q.rot, q.tilt, rotList.data(), tiltList.data(), NN, &idx));
            if (idx < 0) REPORT_ERROR(ERR_ARG_INCORRECT, "no sampled direction within reach of rot " + std::to_string(q.rot) + ", tilt " + std::to_string(q.tilt));
            count_imgs[idx] += do_weights ? q.weight : 1.;
        }
        for (int i = 0; i < NN; ++i) {
            const int count_i = (int)count_imgs[i];
            if (count_i > 0) {
                double e[3], F[9], B[9];
                xhCheck(xh_wbp_image_matrices(rotList[i], tiltList[i], 0.0, e, F, B));      // row 2 of Euler_angles2matrix(rot, -tilt, 0)
                mat_g.insert(mat_g.end(), {e[0], e[1], e[2], (double)count_i});
                totimgs += count_i;
            }
        }
    }
};

}  // namespace mc
#endif
