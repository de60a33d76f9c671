// xh_lockstep.h -- the row plumbing of the programs whose unit of device work is one evaluation for each of many (particle, variables)
// rows (xh_ca2.hip, xh_asa.hip): the rows go up through one pinned buffer, the program's own launches evaluate all of them, the results
// come back in one copy behind one stream wait. What the launches are, and what a row and a result hold, is the program's business.
#ifndef XH_LOCKSTEP_H
#define XH_LOCKSTEP_H
#include "xh_common.h"
#include <chrono>
#include <vector>

namespace {
const double kBarrier = 1e38;   // the cost of a vector out of bounds, which never reaches the device

struct XhRowEval {
    xh_ctx *ctx = nullptr;
    int capacity = 0, rowStride = 0, resStride = 0;      // rows per evaluation, doubles per row and per result
    XhBuf d_rows, d_res;
    XhPinned h_rows, h_res;
    int last_rows = 0;                                   // the rows of the last evaluation, whose images are still on the device
    // what xh_*_stats reports; when they are reset and counted is each program's documented contract
    double t_device = 0, t_total = 0;
    int64_t steps = 0, rows = 0;

    int create(xh_ctx *c, int cap, int rowDoubles, int resDoubles)
    {
        ctx = c; capacity = cap; rowStride = rowDoubles; resStride = resDoubles;
        XH_TRY(xh_buf_alloc(ctx, d_rows, sizeof(double) * rowStride * capacity));
        XH_TRY(xh_buf_alloc(ctx, d_res, sizeof(double) * resStride * capacity));
        XH_TRY(xh_pinned_alloc(ctx, h_rows, sizeof(double) * rowStride * capacity));
        return xh_pinned_alloc(ctx, h_res, sizeof(double) * resStride * capacity);
    }
    double *row(int k) const { return h_rows.f64() + (size_t)rowStride * k; }
    const double *res(int k) const { return h_res.f64() + (size_t)resStride * k; }
    const double *dev_rows() const { return (const double *)d_rows.p; }

    int upload(int m) { XH_HIP(hipMemcpyAsync(d_rows.p, h_rows.p, sizeof(double) * rowStride * m, hipMemcpyHostToDevice, ctx->stream)); return XH_OK; }
    // the results of m rows, behind the one stream wait of an evaluation
    int download(int m)
    {
        XH_HIP(hipMemcpyAsync(h_res.p, d_res.p, sizeof(double) * resStride * m, hipMemcpyDeviceToHost, ctx->stream));
        XH_HIP(hipStreamSynchronize(ctx->stream));
        last_rows = m;
        return XH_OK;
    }

    typedef std::chrono::steady_clock::time_point Time;
    static Time now() { return std::chrono::steady_clock::now(); }
    static double since(Time t) { return std::chrono::duration<double>(now() - t).count(); }
    void reset() { t_device = 0; steps = 0; rows = 0; }
    void count(int m, Time t1) { t_device += since(t1); ++steps; rows += m; }      // one device step of m rows that began at t1
    void stats(double *out) const { out[0] = (double)steps; out[1] = (double)rows; out[2] = t_device; out[3] = t_total; }

    // m rows (any m), at most `capacity` per evaluation. Row r is skipped with result(r, nullptr) when oob(r) (it costs the barrier and
    // takes no place in an evaluation); else fill(r, row) writes it and, after eval(k) has run the k rows gathered, result(r, res) reads
    // its result.
    template <class Oob, class Fill, class Eval, class Result> int cost_rows(int m, Oob oob, Fill fill, Eval eval, Result result)
    {
        std::vector<int> dest((size_t)capacity);
        int r = 0;
        while (r < m) {
            int k = 0;
            for (; r < m && k < capacity; ++r) {
                if (oob(r)) { result(r, (const double *)nullptr); continue; }
                XH_TRY(fill(r, row(k)));
                dest[k++] = r;
            }
            if (k == 0) continue;
            XH_TRY(eval(k));
            for (int j = 0; j < k; ++j) result(dest[j], res(j));
        }
        return XH_OK;
    }
};

// the compact vector xc of a search over the variables `active` -> all the variables x; the frozen ones keep base's values
inline void xh_lockstep_expand(const std::vector<int> &active, const double *base, int nvars, const double *xc, double *x)
{
    for (int k = 0; k < nvars; ++k) x[k] = base[k];
    for (size_t k = 0; k < active.size(); ++k) x[active[k]] = xc[k];
}
}  // namespace

#endif
