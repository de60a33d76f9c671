// volume_local_sharpening.h -- xmipp_volume_local_sharpening, LocalDeblur: ProgLocSharpening
// (reconstruction/volume_local_sharpening.{h,cpp}) with the iterations on the device behind the C ABI (xh_ldb_*). The options of
// defineParams (:44-56) plus --dev; -n is accepted and unused: the transforms run on the device. --md receives one row: iterationNumber
// (MDL_ITER, the last iteration) and cost (MDL_COST, lambda), xmippCore's label strings as far as this tree shows (SURVEY.md Appendix B:
// parity unpinned). The output is written whether or not the stop rule fired (:403-405).
// Refused where the reference divides by zero or reads what it never wrote: 2 sampling - 0.2 <= 0, -i below 1, a resolution map
// without a voxel at or above 2 sampling, volumes of different shapes.
#ifndef XMIPP3_AMD_VOLUME_LOCAL_SHARPENING_H
#define XMIPP3_AMD_VOLUME_LOCAL_SHARPENING_H
#include "programs.h"

namespace mc {

class ProgLocSharpening : public XmippProgram {
public:
    std::string fnVol, fnRes, fnOut, fnMD;
    double sampling = 1, lambda = 1, K = 0.025;
    int Niter = 50, Nthread = 1, device = 0;

    void defineParams() override
    {
        addUsageLine("This function performs local sharpening");
        addParamsLine("  --vol <vol_file=\"\">   : Input volume");
        addParamsLine("  --resolution_map <vol_file=\"\">: Resolution map");
        addParamsLine("  --sampling <s=1>: sampling");
        addParamsLine("  -o <output=\"Sharpening.vol\">: sharpening volume");
        addParamsLine("  [--md <output=\"params.xmd\">]: sharpening params");
        addParamsLine("  [-l <lambda=1>]: regularization param");
        addParamsLine("  [-k <K=0.025>]: K param");
        addParamsLine("  [-i <Niter=50>]: iteration");
        addParamsLine("  [-n <Nthread=1>]: threads number (accepted and unused: the transforms run on the device)");
        addParamsLine("  [--dev <id=0>]: GPU device to use (one device only)");
    }

    void readParams() override
    {
        fnVol = getParam("--vol");
        fnRes = getParam("--resolution_map");
        sampling = getDoubleParam("--sampling");
        lambda = getDoubleParam("-l");
        K = getDoubleParam("-k");
        Niter = (int)getIntParam("-i");
        Nthread = (int)getIntParam("-n");
        fnOut = getParam("-o");
        fnMD = getParam("--md");
        if (checkParam("--dev")) device = parseGpuDevice(getParam("--dev"));
        if (!(sampling > 0) || !(2 * sampling - 0.2 > 0))
            REPORT_ERROR(ERR_ARG_INCORRECT, "--sampling " + std::to_string(sampling) + ": the first band's wL = sampling / (2 sampling - 0.2) is undefined");
        if (Niter < 1) REPORT_ERROR(ERR_ARG_INCORRECT, "-i " + std::to_string(Niter) + ": without an iteration the sharpened map is never assigned");
    }

    void show() const
    {
        if (!verbose) return;
        std::cout << "vol: " << fnVol << std::endl
                  << "resolution_map: " << fnRes << std::endl
                  << "sampling: " << sampling << std::endl
                  << "output: " << fnOut << std::endl
                  << "md: " << fnMD << std::endl
                  << "lambda: " << lambda << std::endl
                  << "K: " << K << std::endl
                  << "Niter: " << Niter << std::endl
                  << "Nthread: " << Nthread << std::endl;
    }

    void run() override
    {
        show();
        std::cout << "Starting..." << std::endl;
        std::vector<double> vol, res;
        ImageInfo IV, IR;
        readDoubles(fnVol, vol, IV);
        readDoubles(fnRes, res, IR);
        sameShape(IV, IR, "The resolution map and the input volume");
        const size_t X = IV.x, Y = IV.y, Z = IV.z, N = X * Y * Z;

        xh_ctx *ctx = nullptr;
        xhCheck(xh_ctx_create_private(device, &ctx));
        XhOwner<xh_ctx> ctxOwner(ctx);
        xh_ldb *h = nullptr;
        xhCheck(xh_ldb_create(ctx, (int)Z, (int)Y, (int)X, 8, &h));
        XhOwner<xh_ldb> hOwner(h);
        DeviceBuffer dVol, dRes, dOut;
        const size_t vb = sizeof(double) * N;
        dVol.upload(ctx, vol.data(), vb);
        dRes.upload(ctx, res.data(), vb);
        dOut.reserve(ctx, vb);
        xhCheck(xh_ldb_load(h, dVol.as<double>(), dRes.as<double>(), sampling, K));
        int32_t n = 0, stopped = 0;
        double lambdaOut = lambda;
        std::vector<xh_ldb_iter> it((size_t)Niter);
        xhCheck(xh_ldb_run(h, lambda, Niter, it.data(), Niter, &n, &stopped, &lambdaOut, dOut.as<double>()));
        if (lambda == 1) std::cout << "  lambda  " << lambdaOut << std::endl;
        std::cout << "iterations: " << n << (stopped ? " (stop rule)" : "") << std::endl;

        MetaDataVec mditer;
        const size_t objId = mditer.addObject();
        mditer.setValue("iterationNumber", (long)n, objId);
        mditer.setValue("cost", lambdaOut, objId);
        mditer.write(fnMD);

        std::vector<double> out(N);
        xhCheck(xh_memcpy_d2h(ctx, out.data(), dOut.p, vb));
        writeVolume(fnOut, out.data(), X, Y, Z);
    }
};

}  // namespace mc
#endif
