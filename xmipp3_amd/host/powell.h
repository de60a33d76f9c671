// powell.h -- Powell's direction-set minimiser with the calling convention of xmippCore's powellOptimizer:
//     powellOptimizer(p, i0, n, f, prm, ftol, fret, iter, steps)
// minimises f over the n variables p[i0 .. i0+n-1]; f(x, prm) reads them as x[i0] .. x[i0+n-1] (xmippCore passes a 1-based array, so a
// cost written for it reads x[1], x[2] with i0 = 1). The initial directions are the axes scaled by steps; iteration stops when one sweep
// lowers f by less than ftol relative (2 |f_old - f_new| <= ftol (|f_old| + |f_new|)), or after 200 sweeps.
//
// Written from the textbook algorithm (direction set with the discarding rule for the largest decrease, golden-section bracketing,
// Brent's line search with tolerance 2e-4). It is not xmippCore's code: the minima it finds agree with xmippCore's within the stopping
// tolerance, not bit for bit, and so may the sigmas of xmipp_volume_halves_restoration's deconvolution.
// Host only; no device code.
#ifndef XH_POWELL_H
#define XH_POWELL_H
#include <algorithm>
#include <cmath>
#include <vector>

namespace xh_powell {

typedef double (*CostFn)(double *x, void *prm);

struct LineFn {
    CostFn f;
    void *prm;
    int i0, n;
    const double *p, *xi;
    std::vector<double> buf;     // i0 + n entries, the variables at [i0, i0 + n)
    double operator()(double t)
    {
        for (int j = 0; j < n; ++j) buf[i0 + j] = p[j] + t * xi[j];
        return f(buf.data(), prm);
    }
};

// golden-section bracketing of a minimum starting from [a, b]
inline void bracket(LineFn &F, double &a, double &b, double &c, double &fa, double &fb, double &fc)
{
    const double GOLD = 1.618034, GLIMIT = 100.0, TINY = 1e-20;
    fa = F(a); fb = F(b);
    if (fb > fa) { std::swap(a, b); std::swap(fa, fb); }
    c = b + GOLD * (b - a);
    fc = F(c);
    while (fb > fc) {
        const double r = (b - a) * (fb - fc), q = (b - c) * (fb - fa);
        double d = std::max(std::fabs(q - r), TINY);
        if (q - r < 0) d = -d;
        double u = b - ((b - c) * q - (b - a) * r) / (2.0 * d), fu;
        const double ulim = b + GLIMIT * (c - b);
        if ((b - u) * (u - c) > 0.0) {
            fu = F(u);
            if (fu < fc) { a = b; b = u; fa = fb; fb = fu; return; }
            if (fu > fb) { c = u; fc = fu; return; }
            u = c + GOLD * (c - b);
            fu = F(u);
        } else if ((c - u) * (u - ulim) > 0.0) {
            fu = F(u);
            if (fu < fc) { b = c; c = u; u = c + GOLD * (c - b); fb = fc; fc = fu; fu = F(u); }
        } else if ((u - ulim) * (ulim - c) >= 0.0) {
            u = ulim;
            fu = F(u);
        } else {
            u = c + GOLD * (c - b);
            fu = F(u);
        }
        a = b; b = c; c = u;
        fa = fb; fb = fc; fc = fu;
    }
}

// Brent's parabolic / golden-section search in the bracket (a, b, c); returns the minimum, *xmin its abscissa
inline double brent(LineFn &F, double ax, double bx, double cx, double fbx, double tol, double *xmin)
{
    const int ITMAX = 100;
    const double CGOLD = 0.3819660, ZEPS = 1e-10;
    double a = std::min(ax, cx), b = std::max(ax, cx);
    double x = bx, w = bx, v = bx, fx = fbx, fw = fbx, fv = fbx, d = 0.0, e = 0.0;
    for (int it = 0; it < ITMAX; ++it) {
        const double xm = 0.5 * (a + b), tol1 = tol * std::fabs(x) + ZEPS, tol2 = 2.0 * tol1;
        if (std::fabs(x - xm) <= tol2 - 0.5 * (b - a)) break;
        if (std::fabs(e) > tol1) {
            const double r = (x - w) * (fx - fv);
            double q = (x - v) * (fx - fw), p = (x - v) * q - (x - w) * r;
            q = 2.0 * (q - r);
            if (q > 0.0) p = -p;
            q = std::fabs(q);
            const double etemp = e;
            e = d;
            if (std::fabs(p) >= std::fabs(0.5 * q * etemp) || p <= q * (a - x) || p >= q * (b - x)) {
                e = x >= xm ? a - x : b - x;
                d = CGOLD * e;
            } else {
                d = p / q;
                const double u = x + d;
                if (u - a < tol2 || b - u < tol2) d = xm - x >= 0 ? tol1 : -tol1;
            }
        } else {
            e = x >= xm ? a - x : b - x;
            d = CGOLD * e;
        }
        const double u = std::fabs(d) >= tol1 ? x + d : x + (d >= 0 ? tol1 : -tol1);
        const double fu = F(u);
        if (fu <= fx) {
            if (u >= x) a = x; else b = x;
            v = w; w = x; x = u;
            fv = fw; fw = fx; fx = fu;
        } else {
            if (u < x) a = u; else b = u;
            if (fu <= fw || w == x) { v = w; w = u; fv = fw; fw = fu; }
            else if (fu <= fv || v == x || v == w) { v = u; fv = fu; }
        }
    }
    *xmin = x;
    return fx;
}

// minimum of f along p + t xi: p moves there, xi becomes the step taken; returns f at the new p
inline double linmin(CostFn f, void *prm, int i0, int n, std::vector<double> &p, std::vector<double> &xi)
{
    LineFn F{f, prm, i0, n, p.data(), xi.data(), std::vector<double>((size_t)(i0 + n), 0.0)};
    double a = 0.0, b = 1.0, c, fa, fb, fc, xmin;
    bracket(F, a, b, c, fa, fb, fc);
    const double fret = brent(F, a, b, c, fb, 2.0e-4, &xmin);
    for (int j = 0; j < n; ++j) { xi[j] *= xmin; p[j] += xi[j]; }
    return fret;
}

}  // namespace xh_powell

// p: the variables (p.size() >= n; entry j is variable i0 + j), steps: the initial step along each axis
inline void powellOptimizer(std::vector<double> &p, int i0, int n, xh_powell::CostFn f, void *prm, double ftol, double &fret, int &iter,
                            const std::vector<double> &steps)
{
    using namespace xh_powell;
    const int ITMAX = 200;
    const double TINY = 1e-25;
    std::vector<std::vector<double>> xi((size_t)n, std::vector<double>((size_t)n, 0.0));   // xi[d] = direction d
    for (int d = 0; d < n; ++d) xi[d][d] = steps[d];
    std::vector<double> x((size_t)n), pt((size_t)n), ptt((size_t)n), xit((size_t)n), buf((size_t)(i0 + n), 0.0);
    for (int j = 0; j < n; ++j) x[j] = p[j];
    auto eval = [&](const std::vector<double> &q) {
        for (int j = 0; j < n; ++j) buf[i0 + j] = q[j];
        return f(buf.data(), prm);
    };
    fret = eval(x);
    pt = x;
    for (iter = 1;; ++iter) {
        const double fp = fret;
        int ibig = 0;
        double del = 0.0;
        for (int d = 0; d < n; ++d) {
            xit = xi[d];
            const double fptt = fret;
            fret = linmin(f, prm, i0, n, x, xit);
            if (fptt - fret > del) { del = fptt - fret; ibig = d; }
        }
        if (2.0 * (fp - fret) <= ftol * (std::fabs(fp) + std::fabs(fret)) + TINY || iter >= ITMAX) break;
        for (int j = 0; j < n; ++j) { ptt[j] = 2.0 * x[j] - pt[j]; xit[j] = x[j] - pt[j]; pt[j] = x[j]; }
        const double fptt = eval(ptt);
        if (fptt < fp) {
            const double t = 2.0 * (fp - 2.0 * fret + fptt) * (fp - fret - del) * (fp - fret - del) - del * (fp - fptt) * (fp - fptt);
            if (t < 0.0) {
                fret = linmin(f, prm, i0, n, x, xit);
                xi[ibig] = xi[n - 1];
                xi[n - 1] = xit;
            }
        }
    }
    for (int j = 0; j < n; ++j) p[j] = x[j];
}

#endif
