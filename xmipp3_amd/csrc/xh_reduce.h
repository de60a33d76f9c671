// xh_reduce.h -- fp64 sums in a fixed order: the one place where the 256-thread tree is written. Equal inputs give equal bits, on
// every call and whatever else runs: no floating-point atomics, and the order of the additions depends on the launch geometry alone.
//  - workgroup: thread t adds the value of thread t + s for s = 128, 64, .. 1;
//  - grid: every workgroup writes its totals to partials [NC][gridDim.x]; one workgroup (xh_k_reduce_final) then sums each row: thread t
//    adds elements t, t + 256, .. in increasing order, the same tree adds the 256 sums, one row after the other.
// The code only adds, so there is nothing to contract: a file built with -ffp-contract=off and one built without it get the same bits
// from it.
#ifndef XH_REDUCE_H
#define XH_REDUCE_H
#include "xh_common.h"

namespace {

// NC sums over the 256 threads of the workgroup, side by side: thread t brings v[c], row c's total is in red[c][0] on return
template <int NC> __device__ __forceinline__ void xh_tree256(double (&red)[NC][256], const double (&v)[NC])
{
    for (int c = 0; c < NC; ++c) red[c][threadIdx.x] = v[c];
    __syncthreads();
    for (int s = 128; s > 0; s >>= 1) {
        if ((int)threadIdx.x < s)
            for (int c = 0; c < NC; ++c) {
                double *r = red[c] + threadIdx.x;
                r[0] += r[s];
            }
        __syncthreads();
    }
}

// one sum; every thread returns the total. red may still be read from the call before: the barrier comes first
__device__ __forceinline__ double xh_block_sum(double v, double (&red)[1][256])
{
    const double a[1] = {v};
    __syncthreads();
    xh_tree256(red, a);
    return red[0][0];
}

// the workgroup's NC totals -> partials [NC][gridDim.x]
template <int NC> __device__ __forceinline__ void xh_block_partials(const double (&v)[NC], double *__restrict__ partials)
{
    __shared__ double red[NC][256];
    xh_tree256(red, v);
    if (threadIdx.x == 0)
        for (int c = 0; c < NC; ++c) partials[(size_t)c * gridDim.x + blockIdx.x] = red[c][0];
}

// partials [NC][G] -> out [NC], one workgroup
__global__ void __launch_bounds__(256) xh_k_reduce_final(const double *__restrict__ partials, int G, int NC, double *__restrict__ out)
{
    __shared__ double red[1][256];
    for (int c = 0; c < NC; ++c) {
        double v[1] = {0.0};
        for (int i = threadIdx.x; i < G; i += 256) v[0] += partials[(size_t)c * G + i];
        xh_tree256(red, v);
        if (threadIdx.x == 0) out[c] = red[0][0];
        __syncthreads();
    }
}

// partials [NC][G] -> d_result [NC] -> NC doubles at h_out (pageable or page-locked), synchronous
int xh_reduce_finish(xh_ctx *ctx, const double *d_partials, int G, int NC, double *d_result, double *h_out)
{
    XH_LAUNCH256(ctx, xh_k_reduce_final, 1, d_partials, G, NC, d_result);
    XH_HIP(hipMemcpyAsync(h_out, d_result, sizeof(double) * NC, hipMemcpyDeviceToHost, ctx->stream));
    XH_HIP(hipStreamSynchronize(ctx->stream));
    return XH_OK;
}

}  // namespace

#endif
