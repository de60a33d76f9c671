// xh_powell.hip -- the library's one compiled powellOptimizer (host/powell.h) and its lockstep scheduler (host/powell_batch.h): host
// code only. Every search of the library (the sigma search of xh_halves_deconvolve, xh_vds_refine_stage, xh_ca2_refine) and the two
// exported entry points run this translation unit's code, so a problem gets the same bits whichever way it is reached.
#include "xh_common.h"
#include "../host/powell.h"
#include "../host/powell_batch.h"

namespace {
struct PowellUser { xh_cost_fn f; void *user; };
double powell_tramp(double *x, void *prm)
{
    PowellUser *u = (PowellUser *)prm;
    return u->f(x, u->user);
}
}  // namespace

extern "C" {

int xh_powell_minimize(int32_t n, double *p, const double *steps, double ftol, xh_cost_fn f, void *user, double *fret, int32_t *iter)
{
    XH_CHECK(n >= 1 && p && steps && f && fret && iter, XH_ERR_ARG, "xh_powell_minimize: bad argument");
    std::vector<double> pv(p, p + n), sv(steps, steps + n);
    PowellUser u{f, user};
    int it = 0;
    powellOptimizer(pv, 1, n, powell_tramp, &u, ftol, *fret, it, sv);
    for (int j = 0; j < n; ++j) p[j] = pv[j];
    *iter = it;
    return XH_OK;
}

int xh_powell_minimize_batch(int32_t nprob, const int32_t *n, int32_t nmax, double *p, const double *steps, double ftol, int32_t capacity,
                             xh_batch_cost_fn f, void *user, double *fret, int32_t *iter, int64_t *evals)
{
    XH_CHECK(nprob >= 0 && n && nmax >= 1 && p && steps && capacity >= 1 && f && fret && iter, XH_ERR_ARG, "xh_powell_minimize_batch: bad argument");
    return xh_powell_lockstep(nprob, n, nmax, p, steps, ftol, capacity, f, nullptr, user, fret, iter, evals);
}

}  // extern "C"

// the scheduler behind xh_powell_minimize_batch and xh_ca2_refine
int xh_powell_lockstep(int32_t nprob, const int32_t *n, int32_t nmax, double *p, const double *steps, double ftol, int32_t capacity,
                       xh_batch_cost_fn f, xh_lockstep_pre_fn pre, void *user, double *fret, int32_t *iter, int64_t *evals)
{
    for (int q = 0; q < nprob; ++q)
        XH_CHECK(n[q] >= 1 && n[q] <= nmax, XH_ERR_ARG, "xh_powell_minimize_batch: problem %d has %d variables, outside 1..%d", q, n[q], nmax);
    if (nprob == 0) return XH_OK;
    xh_powell::Lockstep L;
    const int rc = L.run(nprob, n, nmax, p, steps, ftol, capacity, f, pre, user, fret, iter, evals);
    XH_CHECK(rc != xh_powell::Lockstep::kNoStacks, XH_ERR_NOMEM, "xh_powell_minimize_batch: out of host memory for %d coroutine stacks", capacity);
    if (rc > 0 || rc < XH_ERR_UNSUPPORTED) xh_set_error("xh_powell_minimize_batch: the cost callback returned %d", rc);
    return rc;
}
