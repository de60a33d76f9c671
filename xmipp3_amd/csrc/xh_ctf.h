// xh_ctf.h -- the CTF value on the device, shared by the CTF pre-steps (xh_ctfops.hip), the continuous assignment (xh_ca2.hip) and the
// Zernike3D alignment (xh_asa.hip): produceSideInfo on the host, its 18 doubles read back out of an evaluation row on the device, then
// getValuePureAt / getValuePureWithoutDampingAt / the damping envelope at a continuous frequency, in double precision with the
// reference's formulas (data/ctf.h:424-500, 1002-1029; data/ctf.cpp:645-679, 1392-1402).
#ifndef XH_CTF_H
#define XH_CTF_H
#include <cmath>
#include "xh_common.h"

namespace {
constexpr double kPI = 3.14159265358979323846;

struct CtfSide {
    double K1, K2, K3, K5, K6, K7, Ksin, Kcos, rad_azimuth, defocus_average, defocus_deviation;
    double DeltaR, K, envR0, envR1, envR2, phase_shift, VPP_radius;
};

// produceSideInfo, data/ctf.cpp:645-679,1392-1402; phase_shift arrives in degrees (ctf_phase_flip.cpp:99, wiener2d.cpp:149)
static inline CtfSide side_info(const xh_ctf_params &c)
{
    CtfSide d;
    const double local_Cs = c.Cs * 1e7, local_Ca = c.Ca * 1e7, local_kV = c.kV * 1e3, local_ispr = c.ispr * 1e6;
    const double lambda = 12.2643247 / std::sqrt(local_kV * (1. + 0.978466e-6 * local_kV));
    d.K1 = kPI * lambda;
    d.K2 = kPI / 2 * local_Cs * lambda * lambda * lambda;
    d.K3 = std::pow(0.25 * kPI * local_Ca * lambda * (c.espr / c.kV + 2 * local_ispr), 2) / std::log(2.0);
    d.K5 = kPI * c.DeltaF * lambda;
    d.K6 = kPI * kPI * c.alpha * c.alpha;
    d.K7 = local_Cs * lambda * lambda;
    d.Ksin = std::sqrt(1 - c.Q0 * c.Q0);
    d.Kcos = c.Q0;
    d.rad_azimuth = c.azimuthal_angle * kPI / 180.;
    d.defocus_average = -(c.DeltafU + c.DeltafV) * 0.5;
    d.defocus_deviation = -(c.DeltafU - c.DeltafV) * 0.5;
    d.DeltaR = c.DeltaR; d.K = c.K; d.envR0 = c.envR0; d.envR1 = c.envR1; d.envR2 = c.envR2;
    d.phase_shift = (c.phase_shift * kPI) / 180;
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

__device__ __forceinline__ double d_bessj0(double x)
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

// getValuePureAt (damping) / getValuePureWithoutDampingAt after precomputeValues(X, Y)
__device__ __forceinline__ double d_ctf_at(const CtfSide &s, double X, double Y, bool damping)
{
    const double u2 = X * X + Y * Y, u = sqrt(u2), u4 = u2 * u2;
    double deltaf;
    if (fabs(X) < 1e-6 && fabs(Y) < 1e-6) deltaf = 0;
    else deltaf = s.defocus_average + s.defocus_deviation * cos(2 * (atan2(Y, X) - s.rad_azimuth));
    double VPP = 0;
    if (round(s.VPP_radius * 1000) != 0) VPP = -s.phase_shift * (1 - exp(-u2 / (2 * s.VPP_radius * s.VPP_radius)));
    const double argument = VPP + s.K1 * deltaf * u2 + s.K2 * u4;
    double sine_part, cosine_part;
    sincos(argument, &sine_part, &cosine_part);
    if (!damping) return -(s.Ksin * sine_part - s.Kcos * cosine_part);
    const double Eespr = exp(-s.K3 * u4);
    const double EdeltaF = d_bessj0(s.K5 * u2);
    const double xs = u * s.DeltaR;
    const double EdeltaR = (xs == 0) ? 1.0 : sin(kPI * xs) / (kPI * xs);
    const double aux = s.K7 * u2 * u + deltaf * u;
    const double Ealpha = exp(-s.K6 * aux * aux);
    double E = Eespr * EdeltaF * EdeltaR * Ealpha + s.envR0 + s.envR1 * u + s.envR2 * u2;
    if (E < 0) E = 0;
    return -s.K * (s.Ksin * sine_part - s.Kcos * cosine_part) * E;
}

// the damping envelope alone, E of getValueDampingAt (ctf.h:424-449) clamped at 0: generateEnvelope's -getValueDampingAt() for K = 1
__device__ __forceinline__ double d_ctf_envelope(const CtfSide &s, double X, double Y)
{
    const double u2 = X * X + Y * Y, u = sqrt(u2), u4 = u2 * u2;
    double deltaf;
    if (fabs(X) < 1e-6 && fabs(Y) < 1e-6) deltaf = 0;
    else deltaf = s.defocus_average + s.defocus_deviation * cos(2 * (atan2(Y, X) - s.rad_azimuth));
    const double Eespr = exp(-s.K3 * u4);
    const double EdeltaF = d_bessj0(s.K5 * u2);
    const double xs = u * s.DeltaR;
    const double EdeltaR = (xs == 0) ? 1.0 : sin(kPI * xs) / (kPI * xs);
    const double aux = s.K7 * u2 * u + deltaf * u;
    const double Ealpha = exp(-s.K6 * aux * aux);
    const double E = Eespr * EdeltaF * EdeltaR * Ealpha + s.envR0 + s.envR1 * u + s.envR2 * u2;
    return E < 0 ? 0.0 : E;
}
}  // namespace
#endif
