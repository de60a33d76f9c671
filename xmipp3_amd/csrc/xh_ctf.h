// xh_ctf.h -- the CTF model, written once for the device and the host: produceSideInfo, then getValuePureAt /
// getValuePureWithoutDampingAt / the damping envelope at a continuous frequency, in double precision with the reference's formulas
// (data/ctf.h:424-502, 1002-1029; data/ctf.cpp:645-679, 1392-1402). Plain C++ apart from the qualifier macro: the host programs
// compile it with g++.
//
// Callers and the unit of phase_shift that each hands to side_info:
//   xh_ctfops.hip, xh_ca2.hip, xh_asa.hip (through xh_image2d.h)   degrees, as the metadata holds it: side_info converts, like
//                                                                  ctf_phase_flip.cpp:99 and wiener2d.cpp:149 before produceSideInfo
//   xh_rf.hip (the gridder's CTF planes, xh_rf2's scatter),        as it is: readFromMdRow passes the column on and so do these
//   host/ctf_model.h (the matcher's --ctf gallery filter),
//   xh_faz.hip (the ART's CTFINV filter)
#ifndef XH_CTF_H
#define XH_CTF_H
#include <cmath>
#include "../../include/xmipp_hip.h"

#ifdef __HIPCC__
#define XH_CTF_FN __host__ __device__ __forceinline__
#else
#define XH_CTF_FN inline
#endif

namespace {
constexpr double kCtfPI = 3.14159265358979323846;

struct CtfSide {
    double K1, K2, K3, K5, K6, K7, Ksin, Kcos, rad_azimuth, defocus_average, defocus_deviation;
    double DeltaR, K, envR0, envR1, envR2, phase_shift, VPP_radius;
};

// produceSideInfo, data/ctf.cpp:645-679,1392-1402
static inline CtfSide side_info(const xh_ctf_params &c, bool phaseShiftInDegrees)
{
    CtfSide d;
    const double local_Cs = c.Cs * 1e7, local_Ca = c.Ca * 1e7, local_kV = c.kV * 1e3, local_ispr = c.ispr * 1e6;
    const double lambda = 12.2643247 / std::sqrt(local_kV * (1. + 0.978466e-6 * local_kV));
    d.K1 = kCtfPI * lambda;
    d.K2 = kCtfPI / 2 * local_Cs * lambda * lambda * lambda;
    d.K3 = std::pow(0.25 * kCtfPI * local_Ca * lambda * (c.espr / c.kV + 2 * local_ispr), 2) / std::log(2.0);
    d.K5 = kCtfPI * c.DeltaF * lambda;
    d.K6 = kCtfPI * kCtfPI * c.alpha * c.alpha;
    d.K7 = local_Cs * lambda * lambda;
    d.Ksin = std::sqrt(1 - c.Q0 * c.Q0);
    d.Kcos = c.Q0;
    d.rad_azimuth = c.azimuthal_angle * kCtfPI / 180.;
    d.defocus_average = -(c.DeltafU + c.DeltafV) * 0.5;
    d.defocus_deviation = -(c.DeltafU - c.DeltafV) * 0.5;
    d.DeltaR = c.DeltaR; d.K = c.K; d.envR0 = c.envR0; d.envR1 = c.envR1; d.envR2 = c.envR2;
    d.phase_shift = phaseShiftInDegrees ? (c.phase_shift * kCtfPI) / 180 : c.phase_shift;
    d.VPP_radius = c.VPP_radius;
    return d;
}

// A CtfSide rides in an evaluation row as 18 doubles (the host memcpy's it there); q points at the first. A macro, not a function: the
// copy loop has to stay in the kernel's own body. In a callee it is unrolled before it is inlined, d_ctf_at then sees the fields as
// values from the first pass on, and the compiler contracts its sums of two products the other way round (last-bit changes of the CTF).
static_assert(sizeof(CtfSide) == 18 * sizeof(double), "CtfSide rides in an evaluation row as 18 doubles");
#define D_CTF_SIDE_FROM_ROW(s, q)                              \
    CtfSide s;                                                 \
    {                                                          \
        double *sp_ = reinterpret_cast<double *>(&s);          \
        for (int k_ = 0; k_ < 18; ++k_) sp_[k_] = (q)[k_];     \
    }

// J0(0) as d_bessj0 gives it: the quotient of the two leading coefficients, not 1
constexpr double kCtfJ0At0 = 57568490574.0 / 57568490411.0;

XH_CTF_FN double d_bessj0(double x)
{
    const double ax = fabs(x);
    if (ax < 8.0) {
        const double y = x * x;
        const double a1 = 57568490574.0 + y * (-13362590354.0 + y * (651619640.7 + y * (-11214424.18 + y * (77392.33017 + y * (-184.9052456)))));
        const double a2 = 57568490411.0 + y * (1029532985.0 + y * (9494680.718 + y * (59272.64853 + y * (267.8532712 + y * 1.0))));
        return a1 / a2;
    }
    const double z = 8.0 / ax, y = z * z, xx = ax - 0.785398164;
    const double a1 = 1.0 + y * (-0.1098628627e-2 + y * (0.2734510407e-4 + y * (-0.2073370639e-5 + y * 0.2093887211e-6)));
    const double a2 = -0.1562499995e-1 + y * (0.1430488765e-3 + y * (-0.6911147651e-5 + y * (0.7621095161e-6 - y * 0.934935152e-7)));
    return sqrt(0.636619772 / ax) * (cos(xx) * a1 - z * sin(xx) * a2);
}

// getValuePureAt (damping) / getValuePureWithoutDampingAt after precomputeValues(X, Y).
// SHORTCUTS (the gridder's, whose CTF is uniform over a block) skips terms that a zero coefficient leaves without effect, each bit for
// bit the general formula: x + 0 * cos(.) == x, so defocus_deviation == 0 needs no atan2 / cos; exp(-0 * finite) == 1, so K3 == 0 and
// K6 == 0 need no exp; K5 == 0 gives J0(0).
template <bool SHORTCUTS = false>
XH_CTF_FN double d_ctf_at(const CtfSide &s, double X, double Y, bool damping)
{
    const double u2 = X * X + Y * Y, u = sqrt(u2), u4 = u2 * u2;
    double deltaf;
    if (fabs(X) < 1e-6 && fabs(Y) < 1e-6) deltaf = 0;
    else if (SHORTCUTS && s.defocus_deviation == 0) deltaf = s.defocus_average;
    else deltaf = s.defocus_average + s.defocus_deviation * cos(2 * (atan2(Y, X) - s.rad_azimuth));
    double VPP = 0;
    if (round(s.VPP_radius * 1000) != 0) VPP = -s.phase_shift * (1 - exp(-u2 / (2 * s.VPP_radius * s.VPP_radius)));
    const double argument = VPP + s.K1 * deltaf * u2 + s.K2 * u4;
    double sine_part, cosine_part;
    sincos(argument, &sine_part, &cosine_part);
    if (!damping) return -(s.Ksin * sine_part - s.Kcos * cosine_part);
    const double Eespr = (SHORTCUTS && s.K3 == 0) ? 1.0 : exp(-s.K3 * u4);
    const double EdeltaF = (SHORTCUTS && s.K5 == 0) ? kCtfJ0At0 : d_bessj0(s.K5 * u2);
    const double xs = u * s.DeltaR;
    const double EdeltaR = (xs == 0) ? 1.0 : sin(kCtfPI * xs) / (kCtfPI * xs);
    const double aux = s.K7 * u2 * u + deltaf * u;
    const double Ealpha = (SHORTCUTS && s.K6 == 0) ? 1.0 : exp(-s.K6 * aux * aux);
    double E = Eespr * EdeltaF * EdeltaR * Ealpha + s.envR0 + s.envR1 * u + s.envR2 * u2;
    if (E < 0) E = 0;
    return -s.K * (s.Ksin * sine_part - s.Kcos * cosine_part) * E;
}

// the damping envelope alone, E of getValueDampingAt (ctf.h:424-449) clamped at 0: generateEnvelope's -getValueDampingAt() for K = 1
XH_CTF_FN double d_ctf_envelope(const CtfSide &s, double X, double Y)
{
    const double u2 = X * X + Y * Y, u = sqrt(u2), u4 = u2 * u2;
    double deltaf;
    if (fabs(X) < 1e-6 && fabs(Y) < 1e-6) deltaf = 0;
    else deltaf = s.defocus_average + s.defocus_deviation * cos(2 * (atan2(Y, X) - s.rad_azimuth));
    const double Eespr = exp(-s.K3 * u4);
    const double EdeltaF = d_bessj0(s.K5 * u2);
    const double xs = u * s.DeltaR;
    const double EdeltaR = (xs == 0) ? 1.0 : sin(kCtfPI * xs) / (kCtfPI * xs);
    const double aux = s.K7 * u2 * u + deltaf * u;
    const double Ealpha = exp(-s.K6 * aux * aux);
    const double E = Eespr * EdeltaF * EdeltaR * Ealpha + s.envR0 + s.envR1 * u + s.envR2 * u2;
    return E < 0 ? 0.0 : E;
}
}  // namespace
#endif
