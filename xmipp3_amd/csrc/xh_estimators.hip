// xh_estimators.hip -- first slice of the batched estimator API: the extrema finder and the shift estimator
// by correlation, the two building blocks xmipp_cuda_align_significant and FlexAlign share.
//
//   ExtremaFinder::SingleExtremaFinder<T>   reconstruction/single_extrema_finder.cpp:146-300 (CUDA twin: reconstruction_cuda/
//                                           cuda_single_extrema_finder.cpp): Max, Lowest, MaxAroundCenter, LowestAroundCenter of
//                                           n signals, positions as element offsets (float) and values
//   Alignment::ShiftCorrEstimator<T>        reconstruction/shift_corr_estimator.cpp:33-300 (CUDA twin: reconstruction_cuda/
//                                           cuda_shift_corr_estimator.cpp), AlignType::OneToN: correlation of n spectra with one
//                                           reference spectrum (optionally centred), shifts of n images against one reference
//                                           = position of the correlation maximum within maxShift of the centre
//   Alignment::PolarRotationEstimator<T>    reconstruction/polar_rotation_estimator.cpp:33-144, AlignType::OneToN: rotation of n images
//                                           against one reference = arg-max of the rotational correlation of their polar Fourier
//                                           transforms over the rings firstRing .. lastRing (data/polar.cpp:99-148,212-231)
//   Alignment::IterativeAlignmentEstimator<T>  reconstruction/iterative_alignment_estimator.cpp:33-176: rotation and shift estimated in turn,
//                                           the images re-interpolated from the originals by the inverse pose after every step
//                                           (BSplineGeoTransformer::interpolate, bspline_geo_transformer.cpp:103-137: applyGeometry
//                                           LINEAR, IS_INV, DONT_WRAP), both orders tried, the better correlationIndex
//                                           (CorrelationComputer, correlation_computer.cpp:30-56) kept per image
#include "xh_estimators.h"

namespace {
// sComputeCorrelations2DOneToN (shift_corr_estimator.cpp:163-199): inOut = ref conj(inOut), times (-1)^(x+y) when centred
__global__ void __launch_bounds__(256) k_es_correlate(es_cf *__restrict__ inOut, const es_cf *__restrict__ ref, size_t per, int xdim, size_t total, int center)
{
    const size_t t = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (t >= total) return;
    const size_t e = t % per;
    const int y = (int)(e / xdim), x = (int)(e - (size_t)y * xdim);
    const es_cf r = ref[e], o = inOut[t];
    es_cf v = es_cf{r.x * o.x + r.y * o.y, r.y * o.x - r.x * o.y};
    if (center && ((x + y) & 1)) { v.x = -v.x; v.y = -v.y; }
    inOut[t] = v;
}

__global__ void __launch_bounds__(256) k_es_correlate64(xh_cd *__restrict__ inOut, const xh_cd *__restrict__ ref, size_t per, int xdim, size_t total)
{
    const size_t t = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (t >= total) return;
    const size_t e = t % per;
    const int y = (int)(e / xdim), x = (int)(e - (size_t)y * xdim);
    inOut[t] = es_correlate64_at(ref[e], inOut[t], x, y);
}

__global__ void __launch_bounds__(256) k_es_to_complex(const float *__restrict__ in, es_cf *__restrict__ out, size_t tot)
{
    const size_t t = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (t < tot) out[t] = es_cf{in[t], 0.f};
}

__global__ void __launch_bounds__(256) k_es_real(const es_cf *__restrict__ in, float *__restrict__ out, size_t tot)
{
    const size_t t = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (t < tot) out[t] = in[t].x;
}

// es_geometry_at of image blockIdx.y through its matrix A9 [n][9]
__global__ void __launch_bounds__(256) k_es_apply_geometry(const float *__restrict__ in, const double *__restrict__ A9, float *__restrict__ out, int ydim, int xdim)
{
    const size_t t = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (t >= (size_t)ydim * xdim) return;
    const int i = (int)(t / xdim), j = (int)(t - (size_t)i * xdim);
    out[(size_t)blockIdx.y * ydim * xdim + t] = es_geometry_at(in + (size_t)blockIdx.y * ydim * xdim, A9 + 9 * (size_t)blockIdx.y, i, j, ydim, xdim);
}

// correlationIndex(ref, others[b]), block per image
__global__ void __launch_bounds__(256) k_es_corr_index(const float *__restrict__ ref, const float *__restrict__ others, size_t N, float *__restrict__ merit)
{
    const float r = es_corr_index_block(ref, others + (size_t)blockIdx.x * N, N);
    if (threadIdx.x == 0) merit[blockIdx.x] = r;
}

__global__ void __launch_bounds__(256) k_es_rot_fsum(const double2 *__restrict__ Fref, const double2 *__restrict__ F, const EsRing *__restrict__ ringTab, int nrings, int ncoefs,
                                                     int nh, double2 *__restrict__ Fsum)
{
    const int k = blockIdx.x * 256 + threadIdx.x;
    if (k >= nh) return;
    Fsum[(size_t)blockIdx.y * nh + k] = es_rot_fsum_at(Fref, F + (size_t)blockIdx.y * ncoefs, ringTab, nrings, k);
}
}  // namespace

// computeRotation2DOneToN: h_rotations [n] in degrees = imax 360 / (2 N - 1), as floats (getRotations2D is a std::vector<float>)
static int es_rotation_run(EsRotation &R, const float *d_others, int n, float *h_rotations)
{
    xh_ctx *ctx = R.ctx;
    XH_TRY(xh_buf_reserve(ctx, R.coefs, sizeof(double2) * (size_t)R.ncoefs * n));
    XH_TRY(xh_buf_reserve(ctx, R.Fsum, sizeof(double2) * (size_t)R.N * n));
    XH_TRY(xh_buf_reserve(ctx, R.corr, sizeof(double) * (size_t)R.len * n));
    XH_TRY(xh_buf_reserve(ctx, R.imax, sizeof(int) * (size_t)n));
    XH_TRY(es_rotation_transform(R, d_others, n, 1, (double2 *)R.coefs.p));
    hipLaunchKernelGGL(k_es_rot_fsum, dim3((unsigned)((R.N + 255) / 256), n), dim3(256), 0, ctx->stream, (const double2 *)R.Fref.p, (const double2 *)R.coefs.p,
                       (const EsRing *)R.ringTab.p, R.nrings, R.ncoefs, R.N, (double2 *)R.Fsum.p);
    XH_LAUNCH_CHECK();
    hipLaunchKernelGGL(k_es_rot_corr, dim3((unsigned)((R.len + 255) / 256), n), dim3(256), sizeof(double2) * (size_t)R.N, ctx->stream, (const double2 *)R.Fsum.p, R.N, R.len,
                       (double *)R.corr.p);
    XH_LAUNCH_CHECK();
    hipLaunchKernelGGL(k_es_first_max, dim3(n), dim3(256), 0, ctx->stream, (const double *)R.corr.p, R.len, (int *)R.imax.p);
    XH_LAUNCH_CHECK();
    std::vector<int> imax(n);
    XH_HIP(hipMemcpyAsync(imax.data(), R.imax.p, sizeof(int) * n, hipMemcpyDeviceToHost, ctx->stream));
    XH_HIP(hipStreamSynchronize(ctx->stream));
    for (int i = 0; i < n; ++i) h_rotations[i] = (float)((double)imax[i] * (360. / R.len));
    return XH_OK;
}
struct xh_shiftcorr {
    xh_ctx *ctx;
    int x, y, maxShift;
    XhFft2d64 fft;                        // line transforms of any length (xh_plan.h), double precision
    XhBuf ref, work, map, pos;
    bool refLoaded;
    ~xh_shiftcorr()
    {
        (void)hipSetDevice(ctx->device);
        (void)hipStreamSynchronize(ctx->stream);
    }
};


extern "C" {

int xh_extrema_find(xh_ctx *ctx, const float *d_data, int32_t n, int32_t zdim, int32_t ydim, int32_t xdim, int32_t search_type, float max_dist, float *h_positions,
                    float *h_values)
{
    XH_CHECK(ctx && d_data && n >= 1 && zdim >= 1 && ydim >= 1 && xdim >= 1 && (h_positions || h_values), XH_ERR_ARG, "xh_extrema_find: bad argument");
    XH_CHECK(search_type >= 0 && search_type <= 3, XH_ERR_ARG, "xh_extrema_find: search type %d (0 Max, 1 Lowest, 2 MaxAroundCenter, 3 LowestAroundCenter)", search_type);
    const int around = search_type >= 2;
    if (around) {
        XH_CHECK(zdim == 1 && ydim > 1, XH_ERR_UNSUPPORTED, "xh_extrema_find: the search around the centre is for 2-D signals (\"Not implemented\", single_extrema_finder.cpp:97-105)");
        XH_CHECK(max_dist > 0, XH_ERR_ARG, "xh_extrema_find: the maximal distance from the centre must be positive");
    }
    XH_HIP(hipSetDevice(ctx->device));
    const int maxDist = (int)max_dist;                      // size_t maxDist of sFindUniversal2DAroundCenter
    // xHalf - maxDist is unsigned in the reference: a distance beyond the centre's coordinate wraps, and nothing is searched
    const int empty = around && (maxDist > xdim / 2 || maxDist > ydim / 2);
    XhBuf bPos, bVal;
    XH_TRY(xh_buf_alloc(ctx, bPos, sizeof(float) * n));
    XH_TRY(xh_buf_alloc(ctx, bVal, sizeof(float) * n));
    const size_t elems = (size_t)zdim * ydim * xdim;
    if (search_type & 1)
        hipLaunchKernelGGL((k_es_extrema<true>), dim3(n), dim3(256), 0, ctx->stream, d_data, elems, ydim, xdim, around, maxDist, empty, (float *)bPos.p, (float *)bVal.p);
    else
        hipLaunchKernelGGL((k_es_extrema<false>), dim3(n), dim3(256), 0, ctx->stream, d_data, elems, ydim, xdim, around, maxDist, empty, (float *)bPos.p, (float *)bVal.p);
    bool ok = hipGetLastError() == hipSuccess;
    ok = ok && (!h_positions || hipMemcpyAsync(h_positions, bPos.p, sizeof(float) * n, hipMemcpyDeviceToHost, ctx->stream) == hipSuccess);
    ok = ok && (!h_values || hipMemcpyAsync(h_values, bVal.p, sizeof(float) * n, hipMemcpyDeviceToHost, ctx->stream) == hipSuccess);
    ok = ok && hipStreamSynchronize(ctx->stream) == hipSuccess;
    XH_CHECK(ok, XH_ERR_HIP, "xh_extrema_find: device error");
    return XH_OK;
}

int xh_shiftcorr_destroy(xh_shiftcorr *h)
{
    delete h;
    return XH_OK;
}

int xh_shiftcorr_create(xh_ctx *ctx, int32_t xdim, int32_t ydim, int32_t max_shift, xh_shiftcorr **out)
{
    XH_CHECK(ctx && out && xdim >= 2 && ydim >= 2, XH_ERR_ARG, "xh_shiftcorr_create: bad argument");
    // the centring of the correlation by (-1)^(x+y) needs even sizes (computeShifts2DOneToN asserts them), the search a maximal
    // shift sharply below half of the size (AShiftCorrEstimator::check)
    XH_CHECK((xdim & 1) == 0 && (ydim & 1) == 0, XH_ERR_ARG, "xh_shiftcorr_create: only even sizes are supported");
    XH_CHECK(max_shift > 0 && max_shift < xdim / 2 && max_shift < ydim / 2, XH_ERR_ARG, "xh_shiftcorr_create: the maximal shift must be positive and sharply less than half of the size");
    XH_HIP(hipSetDevice(ctx->device));
    std::unique_ptr<xh_shiftcorr> h(new xh_shiftcorr);
    h->ctx = ctx; h->x = xdim; h->y = ydim; h->maxShift = max_shift; h->refLoaded = false;
    // The reference's ShiftCorrEstimator<float> transforms with fftwf; its test images (one-pixel lines) give correlation maps full of
    // exact ties, which single-precision rounding breaks at random.  The device transforms in double and compares the map as floats,
    // so that the first maximum in raster order is the one exact arithmetic has.
    XH_TRY(xh_fft2d64_create(ctx, xdim, ydim, h->fft, "xh_shiftcorr_create"));
    XH_TRY(xh_buf_alloc(ctx, h->ref, sizeof(xh_cd) * (size_t)xdim * ydim));
    *out = h.release();
    return XH_OK;
}

// load2DReferenceOneToN(const T *ref) (:52-62): the reference image [y][x]; its full spectrum is kept
int xh_shiftcorr_load_reference(xh_shiftcorr *h, const float *d_ref)
{
    XH_CHECK(h && d_ref, XH_ERR_ARG, "xh_shiftcorr_load_reference: bad argument");
    xh_ctx *ctx = h->ctx;
    XH_HIP(hipSetDevice(ctx->device));
    const size_t tot = (size_t)h->x * h->y;
    hipLaunchKernelGGL(xh_k_to_complex64<float>, dim3((unsigned)((tot + 255) / 256)), dim3(256), 0, ctx->stream, d_ref, (xh_cd *)h->ref.p, tot);
    XH_LAUNCH_CHECK();
    XH_TRY(xh_fft2d64(ctx, h->fft, (xh_cd *)h->ref.p, 1, false));
    h->refLoaded = true;
    return XH_OK;
}

// computeCorrelations2DOneToN(hw, inOut, ref, dims, center) (:143-161), the static form: n spectra [n][fy][fx] complex against one
int xh_shiftcorr_correlate(xh_ctx *ctx, float *d_inout, const float *d_ref, int32_t n, int32_t fy, int32_t fx, int32_t center)
{
    XH_CHECK(ctx && d_inout && d_ref && n >= 1 && fy >= 1 && fx >= 1, XH_ERR_ARG, "xh_shiftcorr_correlate: bad argument");
    XH_CHECK(!center || (fy & 1) == 0, XH_ERR_ARG, "xh_shiftcorr_correlate: centring needs an even number of rows");
    XH_HIP(hipSetDevice(ctx->device));
    const size_t per = (size_t)fy * fx, total = per * n;
    hipLaunchKernelGGL(k_es_correlate, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, ctx->stream, (es_cf *)d_inout, (const es_cf *)d_ref, per, fx, total, center);
    XH_LAUNCH_CHECK();
    return XH_OK;
}

// computeShift2DOneToN (:201-246) + computeShifts2DOneToN (:248-283): n images [n][y][x] -> h_shifts [n][2] = (x, y) of the
// correlation maximum within maxShift of the centre, as the reference returns it (the shift of the image is its negative)
int xh_shiftcorr_compute_shifts(xh_shiftcorr *h, const float *d_others, int32_t n, float *h_shifts)
{
    XH_CHECK(h && d_others && n >= 1 && h_shifts, XH_ERR_ARG, "xh_shiftcorr_compute_shifts: bad argument");
    XH_CHECK(h->refLoaded, XH_ERR_STATE, "xh_shiftcorr_compute_shifts: Not ready to execute. Call init() before (no reference loaded)");
    xh_ctx *ctx = h->ctx;
    XH_HIP(hipSetDevice(ctx->device));
    const size_t tot = (size_t)h->x * h->y;
    XH_TRY(xh_buf_reserve(ctx, h->map, sizeof(float) * tot * (size_t)n));
    XH_TRY(xh_buf_reserve(ctx, h->pos, sizeof(float) * (size_t)n));
    const int chunk = (int)std::max<size_t>(1, std::min<size_t>((size_t)n, ((size_t)1 << 30) / (sizeof(xh_cd) * tot)));      // at most 1 GiB of work space
    XH_TRY(xh_buf_reserve(ctx, h->work, sizeof(xh_cd) * tot * (size_t)chunk));
    for (int i0 = 0; i0 < n; i0 += chunk) {
        const int m = std::min(chunk, n - i0);
        const size_t total = tot * (size_t)m;
        const unsigned grid = (unsigned)((total + 255) / 256);
        xh_cd *w = (xh_cd *)h->work.p;
        hipLaunchKernelGGL(xh_k_to_complex64<float>, dim3(grid), dim3(256), 0, ctx->stream, d_others + (size_t)i0 * tot, w, total);
        XH_TRY(xh_fft2d64(ctx, h->fft, w, m, false));
        hipLaunchKernelGGL(k_es_correlate64, dim3(grid), dim3(256), 0, ctx->stream, w, (const xh_cd *)h->ref.p, tot, h->x, total);
        XH_TRY(xh_fft2d64(ctx, h->fft, w, m, true));
        hipLaunchKernelGGL(xh_k_real64<float>, dim3(grid), dim3(256), 0, ctx->stream, (const xh_cd *)w, (float *)h->map.p + (size_t)i0 * tot, total);
        XH_LAUNCH_CHECK();
    }
    hipLaunchKernelGGL((k_es_extrema<false>), dim3(n), dim3(256), 0, ctx->stream, (const float *)h->map.p, tot, h->y, h->x, 1, h->maxShift, 0, (float *)h->pos.p, (float *)nullptr);
    XH_LAUNCH_CHECK();
    std::vector<float> pos(n);
    XH_HIP(hipMemcpyAsync(pos.data(), h->pos.p, sizeof(float) * n, hipMemcpyDeviceToHost, ctx->stream));
    XH_HIP(hipStreamSynchronize(ctx->stream));
    const int cX = h->x / 2, cY = h->y / 2;
    for (int i = 0; i < n; ++i) {
        h_shifts[2 * i] = (float)(((int)pos[i] % h->x) - cX);
        h_shifts[2 * i + 1] = (float)(((int)pos[i] / h->x) - cY);
    }
    return XH_OK;
}

// PolarRotationEstimator::load2DReferenceOneToN + computeRotation2DOneToN: best_rotation(reference, image) for n square images, the
// reference's arithmetic (kernels above); h_corr (optional, [n][2 N - 1] doubles) receives the correlation rows
int xh_rotation_estimate(xh_ctx *ctx, const float *d_ref, const float *d_others, int32_t n, int32_t D, int32_t first_ring, int32_t last_ring, float *h_rotations)
{
    XH_CHECK(ctx && d_ref && d_others && h_rotations && n >= 1, XH_ERR_ARG, "xh_rotation_estimate: bad argument");
    XH_HIP(hipSetDevice(ctx->device));
    EsRotation R;
    XH_TRY(es_rotation_create(ctx, d_ref, D, first_ring, last_ring, R));
    XH_TRY(es_rotation_run(R, d_others, n, h_rotations));
    (void)hipStreamSynchronize(ctx->stream);
    return XH_OK;
}

// BSplineGeoTransformer<T>::interpolate (bspline_geo_transformer.cpp:103-137): image i of d_src through matrix h_matrices[i] (3 x 3, row
// major, as applyGeometry(LINEAR, out, in, M, IS_INV, DONT_WRAP) takes it: out(p) = in(M p))
int xh_apply_geometry2d(xh_ctx *ctx, const float *d_src, int32_t n, int32_t ydim, int32_t xdim, const float *h_matrices, float *d_dst)
{
    XH_CHECK(ctx && d_src && d_dst && h_matrices && n >= 1 && ydim >= 1 && xdim >= 1 && d_src != d_dst, XH_ERR_ARG, "xh_apply_geometry2d: bad argument");
    XH_HIP(hipSetDevice(ctx->device));
    std::vector<double> A(9 * (size_t)n);
    for (size_t i = 0; i < A.size(); ++i) A[i] = (double)h_matrices[i];
    XhBuf bA;
    XH_TRY(xh_buf_alloc(ctx, bA, sizeof(double) * A.size()));
    bool ok = hipMemcpyAsync(bA.p, A.data(), sizeof(double) * A.size(), hipMemcpyHostToDevice, ctx->stream) == hipSuccess;
    if (ok) {
        const size_t per = (size_t)ydim * xdim;
        hipLaunchKernelGGL(k_es_apply_geometry, dim3((unsigned)((per + 255) / 256), n), dim3(256), 0, ctx->stream, d_src, (const double *)bA.p, d_dst, ydim, xdim);
        ok = hipGetLastError() == hipSuccess && hipStreamSynchronize(ctx->stream) == hipSuccess;
    }
    XH_CHECK(ok, XH_ERR_HIP, "xh_apply_geometry2d: device error");
    return XH_OK;
}

// CorrelationComputer<T>::compute, MeritType::OneToN, normalizeResult (correlation_computer.cpp:30-56): correlationIndex(ref, other)
int xh_correlation_merit(xh_ctx *ctx, const float *d_ref, const float *d_others, int32_t n, int32_t ydim, int32_t xdim, float *h_merit)
{
    XH_CHECK(ctx && d_ref && d_others && h_merit && n >= 1 && ydim >= 1 && xdim >= 1, XH_ERR_ARG, "xh_correlation_merit: bad argument");
    XH_HIP(hipSetDevice(ctx->device));
    XhBuf b;
    XH_TRY(xh_buf_alloc(ctx, b, sizeof(float) * n));
    hipLaunchKernelGGL(k_es_corr_index, dim3(n), dim3(256), 0, ctx->stream, d_ref, d_others, (size_t)ydim * xdim, (float *)b.p);
    bool ok = hipGetLastError() == hipSuccess;
    ok = ok && hipMemcpyAsync(h_merit, b.p, sizeof(float) * n, hipMemcpyDeviceToHost, ctx->stream) == hipSuccess;
    ok = ok && hipStreamSynchronize(ctx->stream) == hipSuccess;
    XH_CHECK(ok, XH_ERR_HIP, "xh_correlation_merit: device error");
    return XH_OK;
}

// IterativeAlignmentEstimator<T>::compute(others, iters) (iterative_alignment_estimator.cpp:96-176) for n square images of D pixels (even)
// against one reference: h_poses [n][9] (3 x 3 float, row major) and h_merit [n]. The estimators underneath are the three above.
int xh_iterative_alignment(xh_ctx *ctx, const float *d_ref, const float *d_others, int32_t n, int32_t D, int32_t max_shift, int32_t first_ring, int32_t last_ring,
                           int32_t iters, float *h_poses, float *h_merit)
{
    XH_CHECK(ctx && d_ref && d_others && h_poses && h_merit && n >= 1 && iters >= 1, XH_ERR_ARG, "xh_iterative_alignment: bad argument");
    XH_HIP(hipSetDevice(ctx->device));
    xh_shiftcorr *sc = nullptr;
    XH_TRY(xh_shiftcorr_create(ctx, D, D, max_shift, &sc));
    std::unique_ptr<xh_shiftcorr> scOwner(sc);         // destroyed last: its destructor waits for the stream
    EsRotation rotEst;                   // the rotation estimator: the reference's polar transform once for all rounds
    XH_TRY(es_rotation_create(ctx, d_ref, D, first_ring, last_ring, rotEst));
    const size_t per = (size_t)D * D;
    XhBuf bDest;
    XH_TRY(xh_buf_alloc(ctx, bDest, sizeof(float) * per * (size_t)n));
    XH_TRY(xh_shiftcorr_load_reference(sc, d_ref));
    float *dest = (float *)bDest.p;
    std::vector<float> rot(n), sh(2 * (size_t)n), inv(9 * (size_t)n);
    auto applyTransform = [&](const std::vector<float> &poses) {
        // M3x3_INV of every pose (float), then the transformer interpolates the ORIGINAL images with it
        for (int j = 0; j < n; ++j) {
            const float *m = &poses[9 * (size_t)j];
            float *o = &inv[9 * (size_t)j];
            o[0] = m[8] * m[4] - m[7] * m[5]; o[1] = -(m[8] * m[1] - m[7] * m[2]); o[2] = m[5] * m[1] - m[4] * m[2];
            o[3] = -(m[8] * m[3] - m[6] * m[5]); o[4] = m[8] * m[0] - m[6] * m[2]; o[5] = -(m[5] * m[0] - m[3] * m[2]);
            o[6] = m[7] * m[3] - m[6] * m[4]; o[7] = -(m[7] * m[0] - m[6] * m[1]); o[8] = m[4] * m[0] - m[3] * m[1];
            // M3x3_INV: "spduptmp0 = 1.0 / (...)" is a double (SPEED_UP_temps0), the matrix is scaled by it and stored as floats
            const double t = 1.0 / (double)(m[0] * o[0] + m[3] * o[1] + m[6] * o[2]);
            for (int q = 0; q < 9; ++q) o[q] = (float)(o[q] * t);
        }
        return xh_apply_geometry2d(ctx, d_others, n, D, D, inv.data(), dest);
    };
    auto pass = [&](bool rotationFirst, std::vector<float> &poses, std::vector<float> &merit) {
        poses.assign(9 * (size_t)n, 0.f);
        for (int j = 0; j < n; ++j) poses[9 * (size_t)j] = poses[9 * (size_t)j + 4] = poses[9 * (size_t)j + 8] = 1.f;
        int r2 = hipMemcpyAsync(dest, d_others, sizeof(float) * per * (size_t)n, hipMemcpyDeviceToDevice, ctx->stream) == hipSuccess ? XH_OK : XH_ERR_HIP;   // copySrcToDest
        auto stepRotation = [&]() {
            int r3 = es_rotation_run(rotEst, dest, n, rot.data());
            if (r3 != XH_OK) return r3;
            for (int j = 0; j < n; ++j) {
                // rotation2DMatrix(angle, r); lhs = r * lhs
                const double a = (double)rot[j] * 3.14159265358979323846 / 180.0;
                const float c = (float)std::cos(a), s = (float)std::sin(a);
                float *m = &poses[9 * (size_t)j];
                const float r[9] = {c, s, 0.f, -s, c, 0.f, 0.f, 0.f, 1.f};
                float o[9];
                for (int p = 0; p < 3; ++p)
                    for (int q = 0; q < 3; ++q) o[3 * p + q] = r[3 * p] * m[q] + r[3 * p + 1] * m[3 + q] + r[3 * p + 2] * m[6 + q];
                for (int q = 0; q < 9; ++q) m[q] = o[q];
            }
            return applyTransform(poses);
        };
        auto stepShift = [&]() {
            int r3 = xh_shiftcorr_compute_shifts(sc, dest, n, sh.data());
            if (r3 != XH_OK) return r3;
            for (int j = 0; j < n; ++j) { poses[9 * (size_t)j + 2] += sh[2 * j]; poses[9 * (size_t)j + 5] += sh[2 * j + 1]; }
            return applyTransform(poses);
        };
        for (int i = 0; i < iters && r2 == XH_OK; ++i) {
            if (rotationFirst) { r2 = stepRotation(); if (r2 == XH_OK) r2 = stepShift(); }
            else { r2 = stepShift(); if (r2 == XH_OK) r2 = stepRotation(); }
        }
        merit.assign(n, 0.f);
        if (r2 == XH_OK) r2 = xh_correlation_merit(ctx, d_ref, dest, n, D, D, merit.data());
        return r2;
    };
    std::vector<float> pRS, mRS, pSR, mSR;
    XH_TRY(pass(true, pRS, mRS));
    XH_TRY(pass(false, pSR, mSR));
    for (int j = 0; j < n; ++j) {
        const bool sr = mRS[j] < mSR[j];
        h_merit[j] = sr ? mSR[j] : mRS[j];
        std::memcpy(h_poses + 9 * (size_t)j, (sr ? pSR : pRS).data() + 9 * (size_t)j, 9 * sizeof(float));
    }
    return XH_OK;
}

}  // extern "C"
