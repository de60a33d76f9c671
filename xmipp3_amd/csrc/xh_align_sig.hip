// xh_align_sig.hip -- the device side of xmipp_align_significant (reconstruction/aalign_significant.cpp, reconstruction_adapt_cuda/
// align_significant_gpu.cpp): every (reference, image) pair aligned with the chain of xh_iterative_alignment
// (IterativeAlignmentEstimator::compute), the significance weights (computeWeightsAndSave) and the weighted reference update (updateRefs).
//
// The one-reference entry point is called once per reference and moves every pose to the host after every step. Here the unit of
// work is a batch of (reference, image) pairs, pair g = r N + i, so that few images against many references and many images against
// few references fill the device alike. Each reference's polar transform, shift spectrum and pixels are prepared once at load.
// Every step's pose algebra runs in a kernel and never leaves the device. The arithmetic is the one of xh_estimators.h, so this path
// and xh_iterative_alignment agree pair for pair.
#include "xh_estimators.h"

namespace {
// pair b of a batch that starts at the global pair g0 of the [R][n] sweep
__device__ __forceinline__ int as_ref(long long g0, int b, int n) { return (int)((g0 + b) / n); }
__device__ __forceinline__ int as_img(long long g0, int b, int n) { return (int)((g0 + b) % n); }

// M3x3_INV of a float pose as xh_iterative_alignment computes it: float cofactors, the reciprocal of the determinant in double
// (SPEED_UP_temps0), the product stored as floats; the interpolation reads those floats as doubles
__device__ __forceinline__ void as_inverse(const float *m, double *A)
{
#pragma clang fp contract(off)
    float o[9];
    o[0] = m[8] * m[4] - m[7] * m[5]; o[1] = -(m[8] * m[1] - m[7] * m[2]); o[2] = m[5] * m[1] - m[4] * m[2];
    o[3] = -(m[8] * m[3] - m[6] * m[5]); o[4] = m[8] * m[0] - m[6] * m[2]; o[5] = -(m[5] * m[0] - m[3] * m[2]);
    o[6] = m[7] * m[3] - m[6] * m[4]; o[7] = -(m[7] * m[0] - m[6] * m[1]); o[8] = m[4] * m[0] - m[3] * m[1];
    const double t = 1.0 / (double)(m[0] * o[0] + m[3] * o[1] + m[6] * o[2]);
    for (int q = 0; q < 9; ++q) A[q] = (double)(float)(o[q] * t);
}

// copySrcToDest: identity poses (the interpolation through the identity reproduces the image exactly)
__global__ void __launch_bounds__(256) k_as_pose_init(float *__restrict__ pose, double *__restrict__ A, int m)
{
    const int b = blockIdx.x * 256 + threadIdx.x;
    if (b >= m) return;
    for (int q = 0; q < 9; ++q) { pose[9 * (size_t)b + q] = (q % 4 == 0) ? 1.f : 0.f; A[9 * (size_t)b + q] = (q % 4 == 0) ? 1.0 : 0.0; }
}

// the rotation step: angle = imax 360 / (2 N - 1) as the float getRotations2D holds, rotation2DMatrix(angle) times the pose, then its
// inverse
__global__ void __launch_bounds__(256) k_as_pose_rotate(const int *__restrict__ imax, int len, float *__restrict__ pose, double *__restrict__ A, int m)
{
#pragma clang fp contract(off)
    const int b = blockIdx.x * 256 + threadIdx.x;
    if (b >= m) return;
    const float rot = (float)((double)imax[b] * (360. / len));
    const double a = (double)rot * 3.14159265358979323846 / 180.0;
    const float c = (float)cos(a), s = (float)sin(a);
    float *p = pose + 9 * (size_t)b;
    const float r[9] = {c, s, 0.f, -s, c, 0.f, 0.f, 0.f, 1.f};
    float mm[9], o[9];
    for (int q = 0; q < 9; ++q) mm[q] = p[q];
    for (int i = 0; i < 3; ++i)
        for (int q = 0; q < 3; ++q) o[3 * i + q] = r[3 * i] * mm[q] + r[3 * i + 1] * mm[3 + q] + r[3 * i + 2] * mm[6 + q];
    for (int q = 0; q < 9; ++q) p[q] = o[q];
    as_inverse(o, A + 9 * (size_t)b);
}

// the shift step: the position of the correlation maximum relative to the centre added to the pose's translation, then its inverse
__global__ void __launch_bounds__(256) k_as_pose_shift(const float *__restrict__ pos, int D, float *__restrict__ pose, double *__restrict__ A, int m)
{
#pragma clang fp contract(off)
    const int b = blockIdx.x * 256 + threadIdx.x;
    if (b >= m) return;
    const int at = (int)pos[b];
    float *p = pose + 9 * (size_t)b;
    p[2] += (float)((at % D) - D / 2);
    p[5] += (float)((at / D) - D / 2);
    float mm[9];
    for (int q = 0; q < 9; ++q) mm[q] = p[q];
    as_inverse(mm, A + 9 * (size_t)b);
}

// the original image of every pair through the inverse of its current pose
__global__ void __launch_bounds__(256) k_as_apply(const float *__restrict__ images, int n, long long g0, const double *__restrict__ A, float *__restrict__ dest, int D)
{
    const size_t per = (size_t)D * D;
    const size_t t = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (t >= per) return;
    const int b = blockIdx.y;
    const int i = (int)(t / D), j = (int)(t - (size_t)i * D);
    dest[(size_t)b * per + t] = es_geometry_at(images + (size_t)as_img(g0, b, n) * per, A + 9 * (size_t)b, i, j, D, D);
}

// the rotational correlation of pair b against its reference's polar transform
__global__ void __launch_bounds__(256) k_as_rot_fsum(const double2 *__restrict__ Fref, const double2 *__restrict__ F, const EsRing *__restrict__ ringTab, int nrings,
                                                     int ncoefs, int nh, long long g0, int n, double2 *__restrict__ Fsum)
{
    const int k = blockIdx.x * 256 + threadIdx.x;
    if (k >= nh) return;
    const int b = blockIdx.y;
    Fsum[(size_t)b * nh + k] = es_rot_fsum_at(Fref + (size_t)as_ref(g0, b, n) * ncoefs, F + (size_t)b * ncoefs, ringTab, nrings, k);
}

// the centred shift correlation of pair b against its reference's spectrum
__global__ void __launch_bounds__(256) k_as_correlate64(xh_cd *__restrict__ inOut, const xh_cd *__restrict__ refs, int D, long long g0, int n)
{
    const size_t per = (size_t)D * D;
    const size_t e = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (e >= per) return;
    const int b = blockIdx.y;
    const int y = (int)(e / D), x = (int)(e - (size_t)y * D);
    const size_t t = (size_t)b * per + e;
    inOut[t] = es_correlate64_at(refs[(size_t)as_ref(g0, b, n) * per + e], inOut[t], x, y);
}

// correlationIndex(reference of pair b, dest[b]), block per pair
__global__ void __launch_bounds__(256) k_as_corr_index(const float *__restrict__ refs, const float *__restrict__ dest, int D, long long g0, int n, float *__restrict__ merit)
{
    const size_t per = (size_t)D * D;
    const float r = es_corr_index_block(refs + (size_t)as_ref(g0, blockIdx.x, n) * per, dest + (size_t)blockIdx.x * per, per);
    if (threadIdx.x == 0) merit[blockIdx.x] = r;
}

// compute(): per pair the shift -> rotation result replaces the rotation -> shift one where its merit is strictly higher
__global__ void __launch_bounds__(256) k_as_keep_better(const float *__restrict__ poseSR, const float *__restrict__ meritSR, float *__restrict__ pose, float *__restrict__ merit, int m)
{
    const int b = blockIdx.x * 256 + threadIdx.x;
    if (b >= m) return;
    if (merit[b] < meritSR[b]) {
        merit[b] = meritSR[b];
        for (int q = 0; q < 9; ++q) pose[9 * (size_t)b + q] = poseSR[9 * (size_t)b + q];
    }
}

// the highest merit of the references that mask row r selects (figsOfMerit.back() after the ascending sort), block per reference
__global__ void __launch_bounds__(256) k_as_masked_max(const float *__restrict__ merit, const unsigned char *__restrict__ mask, int R, int n, float *__restrict__ maxMerit)
{
    __shared__ float sv[256];
    const int r = blockIdx.x;
    float best = -3.402823466e+38f;
    for (int q = 0; q < R; ++q) {
        if (!mask[(size_t)r * R + q]) continue;
        for (int t = threadIdx.x; t < n; t += 256) best = fmaxf(best, merit[(size_t)q * n + t]);
    }
    sv[threadIdx.x] = best;
    __syncthreads();
    for (int o = 128; o > 0; o >>= 1) {
        if ((int)threadIdx.x < o) sv[threadIdx.x] = fmaxf(sv[threadIdx.x], sv[threadIdx.x + o]);
        __syncthreads();
    }
    if (threadIdx.x == 0) maxMerit[r] = sv[0];
}

// computeWeightsAndSave: the weight of (r, s) = merit / maxMerit . c / (count n - 1), c the rank of the merit in ascending order among
// the count n merits of the references mask row r selects, ties ranked by (reference, image) index. Thread per image s of reference
// r; the merits of every selected reference pass through LDS in tiles of 256.
__global__ void __launch_bounds__(256) k_as_weights(const float *__restrict__ merit, const unsigned char *__restrict__ mask, const float *__restrict__ maxMerit, int R, int n,
                                                    float *__restrict__ weights)
{
#pragma clang fp contract(off)
    __shared__ float tile[256];
    const int r = blockIdx.y;
    const int s = blockIdx.x * 256 + threadIdx.x;
    const float v = s < n ? merit[(size_t)r * n + s] : 0.f;
    unsigned long long c = 0, count = 0;
    for (int q = 0; q < R; ++q) {
        if (!mask[(size_t)r * R + q]) continue;
        ++count;
        for (int t0 = 0; t0 < n; t0 += 256) {
            const int w = min(256, n - t0);
            __syncthreads();
            if ((int)threadIdx.x < w) tile[threadIdx.x] = merit[(size_t)q * n + t0 + threadIdx.x];
            __syncthreads();
            if (q == r) {
                // equal merits of the same reference count when their image comes first
                for (int k = 0; k < w; ++k) c += (tile[k] < v || (tile[k] == v && t0 + k < s)) ? 1 : 0;
            } else {
                const bool before = q < r;
                for (int k = 0; k < w; ++k) c += (tile[k] < v || (before && tile[k] == v)) ? 1 : 0;
            }
        }
    }
    if (s >= n) return;
    const float invMaxMerit = 1.f / maxMerit[r];
    // one merit alone (one image, a reference that selects only itself): the reference divides 0 by 0 here and writes NaN; its rank
    // is 0, and so is its weight
    const unsigned long long total = count * (unsigned long long)n;
    const float cdf = total > 1 ? (float)c / (float)(total - 1) : 0.f;
    weights[(size_t)r * n + s] = v > 0.f ? v * invMaxMerit * cdf : 0.f;
}

// updateRefs: pixel t of reference r = sum over its assignments k (off[r] .. off[r + 1]) of weight[k] . image img[k] through the inverse
// of its pose (A [k][9]), divided by norm[r]; zeros where norm[r] is 0
__global__ void __launch_bounds__(256) k_as_update_refs(const float *__restrict__ images, const int *__restrict__ off, const int *__restrict__ img, const float *__restrict__ weight,
                                                        const double *__restrict__ A, const float *__restrict__ norm, int D, float *__restrict__ out)
{
    const size_t per = (size_t)D * D;
    const size_t t = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (t >= per) return;
    const int r = blockIdx.y;
    const int i = (int)(t / D), j = (int)(t - (size_t)i * D);
    float acc = 0.f;
    for (int k = off[r]; k < off[r + 1]; ++k) acc += weight[k] * es_geometry_at(images + (size_t)img[k] * per, A + 9 * (size_t)k, i, j, D, D);
    const float nr = norm[r];
    out[(size_t)r * per + t] = nr == 0.f ? 0.f : acc / nr;
}
}  // namespace

struct xh_align_sig {
    xh_ctx *ctx = nullptr;
    int D = 0, maxRefs = 0, batch = 0, maxShift = 0, iters = 0, R = 0;
    EsRotation rot;                   // ring table and the per-batch buffers of the rotation estimator
    XhFft2d64 fft;
    XhBuf Fref, refSpec, refs;        // per reference: polar ring DFT, shift spectrum, pixels (for the merit)
    XhBuf dest, work, map, pos, pose, A, meritSR;
    ~xh_align_sig()
    {
        (void)hipSetDevice(ctx->device);
        (void)hipStreamSynchronize(ctx->stream);
    }
};

static unsigned as_blocks(size_t n) { return (unsigned)((n + 255) / 256); }

// the rotation step of a batch of m pairs: polar transform of dest, correlation with each pair's reference, first maximum, pose
static int as_step_rotation(xh_align_sig *h, long long g0, int n, int m, const float *d_images)
{
    xh_ctx *ctx = h->ctx;
    EsRotation &R = h->rot;
    XH_TRY(es_rotation_transform(R, (const float *)h->dest.p, m, 1, (double2 *)R.coefs.p));
    hipLaunchKernelGGL(k_as_rot_fsum, dim3(as_blocks(R.N), m), dim3(256), 0, ctx->stream, (const double2 *)h->Fref.p, (const double2 *)R.coefs.p, (const EsRing *)R.ringTab.p,
                       R.nrings, R.ncoefs, R.N, g0, n, (double2 *)R.Fsum.p);
    XH_LAUNCH_CHECK();
    hipLaunchKernelGGL(k_es_rot_corr, dim3(as_blocks(R.len), m), dim3(256), sizeof(double2) * (size_t)R.N, ctx->stream, (const double2 *)R.Fsum.p, R.N, R.len, (double *)R.corr.p);
    XH_LAUNCH_CHECK();
    hipLaunchKernelGGL(k_es_first_max, dim3(m), dim3(256), 0, ctx->stream, (const double *)R.corr.p, R.len, (int *)R.imax.p);
    XH_LAUNCH_CHECK();
    hipLaunchKernelGGL(k_as_pose_rotate, dim3(as_blocks(m)), dim3(256), 0, ctx->stream, (const int *)R.imax.p, R.len, (float *)h->pose.p, (double *)h->A.p, m);
    XH_LAUNCH_CHECK();
    hipLaunchKernelGGL(k_as_apply, dim3(as_blocks((size_t)h->D * h->D), m), dim3(256), 0, ctx->stream, d_images, n, g0, (const double *)h->A.p, (float *)h->dest.p, h->D);
    XH_LAUNCH_CHECK();
    return XH_OK;
}

// the shift step of a batch of m pairs: centred correlation with each pair's reference spectrum, maximum within maxShift, pose
static int as_step_shift(xh_align_sig *h, long long g0, int n, int m, const float *d_images)
{
    xh_ctx *ctx = h->ctx;
    const int D = h->D;
    const size_t per = (size_t)D * D, total = per * m;
    xh_cd *w = (xh_cd *)h->work.p;
    hipLaunchKernelGGL(xh_k_to_complex64<float>, dim3(as_blocks(total)), dim3(256), 0, ctx->stream, (const float *)h->dest.p, w, total);
    XH_TRY(xh_fft2d64(ctx, h->fft, w, m, false));
    hipLaunchKernelGGL(k_as_correlate64, dim3(as_blocks(per), m), dim3(256), 0, ctx->stream, w, (const xh_cd *)h->refSpec.p, D, g0, n);
    XH_TRY(xh_fft2d64(ctx, h->fft, w, m, true));
    hipLaunchKernelGGL(xh_k_real64<float>, dim3(as_blocks(total)), dim3(256), 0, ctx->stream, (const xh_cd *)w, (float *)h->map.p, total);
    XH_LAUNCH_CHECK();
    hipLaunchKernelGGL((k_es_extrema<false>), dim3(m), dim3(256), 0, ctx->stream, (const float *)h->map.p, per, D, D, 1, h->maxShift, 0, (float *)h->pos.p, (float *)nullptr);
    XH_LAUNCH_CHECK();
    hipLaunchKernelGGL(k_as_pose_shift, dim3(as_blocks(m)), dim3(256), 0, ctx->stream, (const float *)h->pos.p, D, (float *)h->pose.p, (double *)h->A.p, m);
    XH_LAUNCH_CHECK();
    hipLaunchKernelGGL(k_as_apply, dim3(as_blocks(per), m), dim3(256), 0, ctx->stream, d_images, n, g0, (const double *)h->A.p, (float *)h->dest.p, D);
    XH_LAUNCH_CHECK();
    return XH_OK;
}

// one order of compute() for a batch: identity poses, `iters` rounds of the two steps, the merit of the final images
static int as_pass(xh_align_sig *h, bool rotationFirst, long long g0, int n, int m, const float *d_images, float *d_merit)
{
    xh_ctx *ctx = h->ctx;
    hipLaunchKernelGGL(k_as_pose_init, dim3(as_blocks(m)), dim3(256), 0, ctx->stream, (float *)h->pose.p, (double *)h->A.p, m);
    hipLaunchKernelGGL(k_as_apply, dim3(as_blocks((size_t)h->D * h->D), m), dim3(256), 0, ctx->stream, d_images, n, g0, (const double *)h->A.p, (float *)h->dest.p, h->D);
    XH_LAUNCH_CHECK();
    for (int i = 0; i < h->iters; ++i) {
        if (rotationFirst) { XH_TRY(as_step_rotation(h, g0, n, m, d_images)); XH_TRY(as_step_shift(h, g0, n, m, d_images)); }
        else { XH_TRY(as_step_shift(h, g0, n, m, d_images)); XH_TRY(as_step_rotation(h, g0, n, m, d_images)); }
    }
    hipLaunchKernelGGL(k_as_corr_index, dim3(m), dim3(256), 0, ctx->stream, (const float *)h->refs.p, (const float *)h->dest.p, h->D, g0, n, d_merit);
    XH_LAUNCH_CHECK();
    return XH_OK;
}

// M3x3_INV of a float pose on the host, as xh_iterative_alignment's host code and align_significant_gpu.cpp:interpolate compute it
static void as_inverse_host(const float *m, double *A)
{
    float o[9];
    o[0] = m[8] * m[4] - m[7] * m[5]; o[1] = -(m[8] * m[1] - m[7] * m[2]); o[2] = m[5] * m[1] - m[4] * m[2];
    o[3] = -(m[8] * m[3] - m[6] * m[5]); o[4] = m[8] * m[0] - m[6] * m[2]; o[5] = -(m[5] * m[0] - m[3] * m[2]);
    o[6] = m[7] * m[3] - m[6] * m[4]; o[7] = -(m[7] * m[0] - m[6] * m[1]); o[8] = m[4] * m[0] - m[3] * m[1];
    const double t = 1.0 / (double)(m[0] * o[0] + m[3] * o[1] + m[6] * o[2]);
    for (int q = 0; q < 9; ++q) A[q] = (double)(float)(o[q] * t);
}

extern "C" {

int xh_align_sig_destroy(xh_align_sig *h)
{
    delete h;
    return XH_OK;
}

int xh_align_sig_create(xh_ctx *ctx, int32_t D, int32_t max_refs, int32_t batch_pairs, int32_t max_shift, int32_t first_ring, int32_t last_ring, int32_t iters,
                        xh_align_sig **out)
{
    XH_CHECK(ctx && out && iters >= 1, XH_ERR_ARG, "xh_align_sig_create: bad argument");
    XH_CHECK(max_refs >= 1 && max_refs <= 65535, XH_ERR_ARG, "xh_align_sig_create: %d references (1 .. 65535)", max_refs);
    XH_CHECK(batch_pairs >= 1 && batch_pairs <= 65535, XH_ERR_ARG, "xh_align_sig_create: %d pairs per batch (1 .. 65535)", batch_pairs);
    XH_CHECK(D >= 2 && (D & 1) == 0, XH_ERR_ARG, "xh_align_sig_create: only even sizes are supported");
    XH_CHECK(max_shift > 0 && max_shift < D / 2, XH_ERR_ARG, "xh_align_sig_create: the maximal shift must be positive and sharply less than half of the size");
    XH_HIP(hipSetDevice(ctx->device));
    std::unique_ptr<xh_align_sig> h(new xh_align_sig);
    h->ctx = ctx; h->D = D; h->maxRefs = max_refs; h->batch = batch_pairs; h->maxShift = max_shift; h->iters = iters;
    const size_t per = (size_t)D * D, B = (size_t)batch_pairs;
    XH_TRY(es_rotation_plan(ctx, D, first_ring, last_ring, h->rot));
    XH_TRY(xh_fft2d64_create(ctx, D, D, h->fft, "xh_align_sig_create"));
    EsRotation &R = h->rot;
    XH_TRY(xh_buf_alloc(ctx, h->Fref, sizeof(double2) * (size_t)R.ncoefs * max_refs));
    XH_TRY(xh_buf_alloc(ctx, h->refSpec, sizeof(xh_cd) * per * max_refs));
    XH_TRY(xh_buf_alloc(ctx, h->refs, sizeof(float) * per * max_refs));
    XH_TRY(xh_buf_reserve(ctx, R.rings, sizeof(double) * (size_t)R.nsamples * std::max<size_t>(B, max_refs)));
    XH_TRY(xh_buf_reserve(ctx, R.coefs, sizeof(double2) * (size_t)R.ncoefs * B));
    XH_TRY(xh_buf_reserve(ctx, R.Fsum, sizeof(double2) * (size_t)R.N * B));
    XH_TRY(xh_buf_reserve(ctx, R.corr, sizeof(double) * (size_t)R.len * B));
    XH_TRY(xh_buf_reserve(ctx, R.imax, sizeof(int) * B));
    XH_TRY(xh_buf_alloc(ctx, h->dest, sizeof(float) * per * B));
    XH_TRY(xh_buf_alloc(ctx, h->work, sizeof(xh_cd) * per * B));
    XH_TRY(xh_buf_alloc(ctx, h->map, sizeof(float) * per * B));
    XH_TRY(xh_buf_alloc(ctx, h->pos, sizeof(float) * B));
    XH_TRY(xh_buf_alloc(ctx, h->pose, sizeof(float) * 9 * B));
    XH_TRY(xh_buf_alloc(ctx, h->A, sizeof(double) * 9 * B));
    XH_TRY(xh_buf_alloc(ctx, h->meritSR, sizeof(float) * B));
    *out = h.release();
    return XH_OK;
}

// per reference, once: the polar ring DFT, the shift spectrum and a copy of the pixels
int xh_align_sig_load_references(xh_align_sig *h, const float *d_refs, int32_t R)
{
    XH_CHECK(h && d_refs && R >= 1 && R <= h->maxRefs, XH_ERR_ARG, "xh_align_sig_load_references: %d references (1 .. %d)", R, h ? h->maxRefs : 0);
    xh_ctx *ctx = h->ctx;
    XH_HIP(hipSetDevice(ctx->device));
    const size_t per = (size_t)h->D * h->D, total = per * R;
    XH_TRY(es_rotation_transform(h->rot, d_refs, R, 0, (double2 *)h->Fref.p));
    XH_HIP(hipMemcpyAsync(h->refs.p, d_refs, sizeof(float) * total, hipMemcpyDeviceToDevice, ctx->stream));
    hipLaunchKernelGGL(xh_k_to_complex64<float>, dim3(as_blocks(total)), dim3(256), 0, ctx->stream, d_refs, (xh_cd *)h->refSpec.p, total);
    XH_LAUNCH_CHECK();
    XH_TRY(xh_fft2d64(ctx, h->fft, (xh_cd *)h->refSpec.p, R, false));
    XH_HIP(hipStreamSynchronize(ctx->stream));
    h->R = R;
    return XH_OK;
}

int xh_align_sig_align(xh_align_sig *h, const float *d_images, int32_t N, float *d_poses, float *d_merit)
{
    XH_CHECK(h && d_images && N >= 1 && d_poses && d_merit, XH_ERR_ARG, "xh_align_sig_align: bad argument");
    XH_CHECK(h->R >= 1, XH_ERR_STATE, "xh_align_sig_align: no references loaded");
    xh_ctx *ctx = h->ctx;
    XH_HIP(hipSetDevice(ctx->device));
    const long long pairs = (long long)h->R * N;
    for (long long g0 = 0; g0 < pairs; g0 += h->batch) {
        const int m = (int)std::min<long long>(h->batch, pairs - g0);
        float *poses = d_poses + 9 * g0, *merit = d_merit + g0;
        XH_TRY(as_pass(h, true, g0, N, m, d_images, merit));
        XH_HIP(hipMemcpyAsync(poses, h->pose.p, sizeof(float) * 9 * m, hipMemcpyDeviceToDevice, ctx->stream));
        XH_TRY(as_pass(h, false, g0, N, m, d_images, (float *)h->meritSR.p));
        hipLaunchKernelGGL(k_as_keep_better, dim3(as_blocks(m)), dim3(256), 0, ctx->stream, (const float *)h->pose.p, (const float *)h->meritSR.p, poses, merit, m);
        XH_LAUNCH_CHECK();
    }
    XH_HIP(hipStreamSynchronize(ctx->stream));
    return XH_OK;
}

int xh_align_sig_weights(xh_align_sig *h, const float *h_rot, const float *h_tilt, double ang_distance, const float *d_merit, int32_t R, int32_t N, float *d_weights)
{
    XH_CHECK(h && h_rot && h_tilt && d_merit && d_weights && R >= 1 && R <= 65535 && N >= 1, XH_ERR_ARG, "xh_align_sig_weights: bad argument");
    xh_ctx *ctx = h->ctx;
    XH_HIP(hipSetDevice(ctx->device));
    // Euler_distanceBetweenAngleSets(rot_r, tilt_r, 0, rot_q, tilt_q, 0, true): the angle between the projection directions (the third
    // rows of the Euler matrices) in degrees
    std::vector<double> dir(3 * (size_t)R);
    for (int r = 0; r < R; ++r) {
        const double a = (double)h_rot[r] * M_PI / 180., b = (double)h_tilt[r] * M_PI / 180.;
        dir[3 * r] = std::sin(b) * std::cos(a); dir[3 * r + 1] = std::sin(b) * std::sin(a); dir[3 * r + 2] = std::cos(b);
    }
    std::vector<unsigned char> mask((size_t)R * R);
    for (int r = 0; r < R; ++r)
        for (int q = 0; q < R; ++q) {
            const double d = dir[3 * r] * dir[3 * q] + dir[3 * r + 1] * dir[3 * q + 1] + dir[3 * r + 2] * dir[3 * q + 2];
            const double ang = std::acos(std::min(1.0, std::max(-1.0, d))) * 180. / M_PI;
            mask[(size_t)r * R + q] = (r == q || ang <= ang_distance) ? 1 : 0;
        }
    XhBuf bMask, bMax;
    XH_TRY(xh_buf_alloc(ctx, bMask, mask.size()));
    XH_TRY(xh_buf_alloc(ctx, bMax, sizeof(float) * R));
    bool ok = hipMemcpyAsync(bMask.p, mask.data(), mask.size(), hipMemcpyHostToDevice, ctx->stream) == hipSuccess;
    if (ok) {
        hipLaunchKernelGGL(k_as_masked_max, dim3(R), dim3(256), 0, ctx->stream, d_merit, (const unsigned char *)bMask.p, R, N, (float *)bMax.p);
        hipLaunchKernelGGL(k_as_weights, dim3(as_blocks(N), R), dim3(256), 0, ctx->stream, d_merit, (const unsigned char *)bMask.p, (const float *)bMax.p, R, N, d_weights);
        ok = hipGetLastError() == hipSuccess && hipStreamSynchronize(ctx->stream) == hipSuccess;
    }
    XH_CHECK(ok, XH_ERR_HIP, "xh_align_sig_weights: device error");
    return XH_OK;
}

int xh_align_sig_update_refs(xh_align_sig *h, const float *d_images, int32_t N, int32_t R, int32_t n_assign, const int32_t *h_ref_idx, const int32_t *h_img_idx,
                             const float *h_weight, const float *h_pose, float *d_out_refs)
{
    XH_CHECK(h && d_images && N >= 1 && n_assign >= 0 && d_out_refs && (n_assign == 0 || (h_ref_idx && h_img_idx && h_weight && h_pose)), XH_ERR_ARG,
             "xh_align_sig_update_refs: bad argument");
    XH_CHECK(R >= 1 && R <= 65535, XH_ERR_ARG, "xh_align_sig_update_refs: %d references (1 .. 65535)", R);
    for (int k = 0; k < n_assign; ++k)
        XH_CHECK(h_ref_idx[k] >= 0 && h_ref_idx[k] < R && h_img_idx[k] >= 0 && h_img_idx[k] < N, XH_ERR_ARG,
                 "xh_align_sig_update_refs: assignment %d names reference %d / image %d (of %d / %d)", k, h_ref_idx[k], h_img_idx[k], R, N);
    xh_ctx *ctx = h->ctx;
    XH_HIP(hipSetDevice(ctx->device));
    // the assignments grouped by reference, in their given order within a reference; the normaliser is the running sum of the weights
    // of references 0 .. r (norm is declared before the loop over references in align_significant_gpu.cpp:updateRefs)
    std::vector<int> off(R + 1, 0), img(std::max(n_assign, 1)), fill(R, 0);
    std::vector<float> w(std::max(n_assign, 1)), norm(R);
    std::vector<double> A(9 * (size_t)std::max(n_assign, 1));
    for (int k = 0; k < n_assign; ++k) ++off[h_ref_idx[k] + 1];
    for (int r = 0; r < R; ++r) off[r + 1] += off[r];
    for (int k = 0; k < n_assign; ++k) {
        const int r = h_ref_idx[k], at = off[r] + fill[r]++;
        img[at] = h_img_idx[k]; w[at] = h_weight[k];
        as_inverse_host(h_pose + 9 * (size_t)k, &A[9 * (size_t)at]);
    }
    float running = 0.f;
    for (int r = 0; r < R; ++r) {
        float s = 0.f;
        for (int k = off[r]; k < off[r + 1]; ++k) s += w[k];
        running += s;
        norm[r] = running;
    }
    XhBuf bOff, bImg, bW, bA, bNorm;
    XH_TRY(xh_buf_alloc(ctx, bOff, sizeof(int) * off.size()));
    XH_TRY(xh_buf_alloc(ctx, bImg, sizeof(int) * img.size()));
    XH_TRY(xh_buf_alloc(ctx, bW, sizeof(float) * w.size()));
    XH_TRY(xh_buf_alloc(ctx, bA, sizeof(double) * A.size()));
    XH_TRY(xh_buf_alloc(ctx, bNorm, sizeof(float) * norm.size()));
    bool ok = hipMemcpyAsync(bOff.p, off.data(), sizeof(int) * off.size(), hipMemcpyHostToDevice, ctx->stream) == hipSuccess &&
              hipMemcpyAsync(bImg.p, img.data(), sizeof(int) * img.size(), hipMemcpyHostToDevice, ctx->stream) == hipSuccess &&
              hipMemcpyAsync(bW.p, w.data(), sizeof(float) * w.size(), hipMemcpyHostToDevice, ctx->stream) == hipSuccess &&
              hipMemcpyAsync(bA.p, A.data(), sizeof(double) * A.size(), hipMemcpyHostToDevice, ctx->stream) == hipSuccess &&
              hipMemcpyAsync(bNorm.p, norm.data(), sizeof(float) * norm.size(), hipMemcpyHostToDevice, ctx->stream) == hipSuccess;
    if (ok) {
        hipLaunchKernelGGL(k_as_update_refs, dim3(as_blocks((size_t)h->D * h->D), R), dim3(256), 0, ctx->stream, d_images, (const int *)bOff.p, (const int *)bImg.p,
                           (const float *)bW.p, (const double *)bA.p, (const float *)bNorm.p, h->D, d_out_refs);
        ok = hipGetLastError() == hipSuccess && hipStreamSynchronize(ctx->stream) == hipSuccess;
    }
    XH_CHECK(ok, XH_ERR_HIP, "xh_align_sig_update_refs: device error");
    return XH_OK;
}

}  // extern "C"
