// xh_volume.h -- what the programs that work on one Z x Y x X fp64 box through XhFft3d share: the handle's common part, the lap timer,
// the grid-stride loop, the half spectrum's index decomposition and the pointer casts of XhBuf. A new whole-volume program starts here
// ("Whole-volume programs"). Header only; each including file keeps its own -ffp-contract choice.
// Used by xh_halves.hip, xh_mono.hip, xh_ldb.hip, xh_fso.hip and xh_vsub.hip. Not here, on purpose: the programs' frequency formulas and
// filters, each pinned to the rounding of a different reference function.
#ifndef XH_VOLUME_H
#define XH_VOLUME_H
#include "xh_fft3d.h"
#include <algorithm>

// element n of N, a workgroup-strided walk of the whole grid
#define XH_GRID_LOOP(n, N) for (size_t n = (size_t)blockIdx.x * blockDim.x + threadIdx.x; n < (N); n += (size_t)gridDim.x * blockDim.x)

namespace {

struct XhDims { int Z, Y, X, xh; };

// raster element e of the half spectrum [Z][Y][xh] -> its indices
__device__ __forceinline__ void xh_kij(size_t e, XhDims d, int &k, int &i, int &j)
{
    j = (int)(e % d.xh);
    const size_t r = e / d.xh;
    i = (int)(r % d.Y);
    k = (int)(r / d.Y);
}

double *dp(XhBuf &b) { return (double *)b.p; }
xh_cd *cp(XhBuf &b) { return (xh_cd *)b.p; }
float *fp(XhBuf &b) { return (float *)b.p; }
int *ip(XhBuf &b) { return (int *)b.p; }

// workgroups of 256 threads for n elements, at most k per compute unit. Each program keeps its own k: the partial sums of its fixed-order
// reductions depend on it
unsigned xh_grid256(size_t n, int cus, int k) { return (unsigned)std::max<size_t>(1, std::min<size_t>((n + 255) / 256, (size_t)cus * k)); }

// The common part of a volume handle, its base. A handle's own destructor is `~xh_x() { finish(); }`: members go before a base's
// destructor runs, so the wait that XhBuf, XhPinned and XhEvent members rely on cannot live in ~XhVolume.
struct XhVolume {
    xh_ctx *ctx = nullptr;
    XhDims d = {};
    size_t N = 0, NF = 0;       // voxels, coefficients of the half spectrum
    XhFft3d fft;

    // after the program's own argument checks: selects the device, makes the plans
    int init(xh_ctx *c, int Z, int Y, int X)
    {
        XH_HIP(hipSetDevice(c->device));
        ctx = c;
        XH_TRY(xh_fft3d_create(c, Z, Y, X, fft));
        d = XhDims{Z, Y, X, X / 2 + 1};
        N = (size_t)Z * Y * X;
        NF = (size_t)Z * Y * d.xh;
        return XH_OK;
    }

    // nothing on the stream uses the handle's memory or events any more
    void finish()
    {
        if (!ctx) return;
        (void)hipSetDevice(ctx->device);
        (void)hipStreamSynchronize(ctx->stream);
    }
};

// Stage times of a run, the benchmark's switch: the time since the last lap goes to `stage`. Off: nothing is recorded. On: one wait per lap.
template <int NT> struct XhLapTimer {
    xh_ctx *ctx = nullptr;
    XhEvent ev[2];
    bool on = false;
    double ms[NT] = {};

    int create(xh_ctx *c)
    {
        ctx = c;
        XH_TRY(xh_event_create(ev[0]));
        return xh_event_create(ev[1]);
    }
    void zero() { for (double &t : ms) t = 0; }
    void set(bool o) { on = o; zero(); }
    void read(double *h_ms) const { for (int i = 0; i < NT; ++i) h_ms[i] = ms[i]; }
    int start()
    {
        if (on) XH_HIP(hipEventRecord(ev[0], ctx->stream));
        return XH_OK;
    }
    int lap(int stage)
    {
        if (!on) return XH_OK;
        XH_HIP(hipEventRecord(ev[1], ctx->stream));
        XH_HIP(hipEventSynchronize(ev[1]));
        float t = 0;
        XH_HIP(hipEventElapsedTime(&t, ev[0], ev[1]));
        ms[stage] += t;
        XH_HIP(hipEventRecord(ev[0], ctx->stream));
        return XH_OK;
    }
};

}  // namespace

#endif
