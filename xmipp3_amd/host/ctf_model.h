// ctf_model.h -- what the host programs do with a CTF description themselves: read its columns out of a metadata table, and evaluate
// it on a grid for the matcher's --ctf gallery filter. The model itself is csrc/xh_ctf.h, the one the device code uses.
#ifndef XMIPP3_AMD_CTF_MODEL_H
#define XMIPP3_AMD_CTF_MODEL_H
#include "minicore.h"
#include "../csrc/xh_ctf.h"

namespace mc {

// CTFDescription::readFromMdRow (data/ctf.cpp:365-388, 1160-1186): the columns a ctfparam file / a particle row carries, resolved once
// per table (MetaDataVec or FastTable), then read row by row with index lookups only
struct CtfColumns {
    int col[19];
    template <class Table> explicit CtfColumns(const Table &t)
    {
        static const char *const labels[19] = {"ctfSamplingRate", "ctfVoltage", "ctfDefocusU", "ctfDefocusV", "ctfDefocusAngle", "ctfSphericalAberration",
                                               "ctfChromaticAberration", "ctfEnergyLoss", "ctfLensStability", "ctfConvergenceCone",
                                               "ctfLongitudinalDisplacement", "ctfTransversalDisplacement", "ctfQ0", "ctfK", "ctfEnvR0", "ctfEnvR1", "ctfEnvR2",
                                               "ctfPhaseShift", "ctfVPPRadius"};
        for (int i = 0; i < 19; ++i) col[i] = t.col(labels[i]);
    }
    template <class Table> void read(const Table &t, size_t id, xh_ctf_params &c) const
    {
        xh_ctf_defaults(&c);
        c.Tm = t.getDouble(col[0], id, 1); c.kV = t.getDouble(col[1], id, 100);
        c.DeltafU = t.getDouble(col[2], id, 0); c.DeltafV = t.getDouble(col[3], id, c.DeltafU);
        c.azimuthal_angle = t.getDouble(col[4], id, 0); c.Cs = t.getDouble(col[5], id, 0);
        c.Ca = t.getDouble(col[6], id, 0); c.espr = t.getDouble(col[7], id, 0);
        c.ispr = t.getDouble(col[8], id, 0); c.alpha = t.getDouble(col[9], id, 0);
        c.DeltaF = t.getDouble(col[10], id, 0); c.DeltaR = t.getDouble(col[11], id, 0);
        c.Q0 = t.getDouble(col[12], id, 0); c.K = t.getDouble(col[13], id, 1);
        c.envR0 = t.getDouble(col[14], id, 0); c.envR1 = t.getDouble(col[15], id, 0); c.envR2 = t.getDouble(col[16], id, 0);
        c.phase_shift = t.getDouble(col[17], id, 0); c.VPP_radius = t.getDouble(col[18], id, 0);
    }
};
inline void readCtfRow(const MetaDataVec &md, size_t id, xh_ctf_params &c) { CtfColumns(md).read(md, id, c); }

// generateCTF (data/ctf.h:1219-1240) for the gallery filter of --ctf (APM:366-402): the pure CTF with its envelope on the paddim x paddim
// grid of FFTW-order digital frequencies / Tm, |.| of it for phase-flipped data. phase_shift goes in as the file holds it.
inline std::vector<double> ctfFilterTable(const xh_ctf_params &c, int paddim, bool phase_flipped)
{
    std::vector<double> M((size_t)paddim * paddim);
    const CtfSide s = side_info(c, false);
    const double iTs = 1.0 / c.Tm;
    for (int i = 0; i < paddim; ++i) {
        const double fy = (double)(i <= paddim / 2 ? i : i - paddim) / paddim * iTs;
        for (int j = 0; j < paddim; ++j) {
            const double fx = (double)(j <= paddim / 2 ? j : j - paddim) / paddim * iTs;
            const double v = d_ctf_at(s, fx, fy, true);
            M[(size_t)i * paddim + j] = phase_flipped ? std::fabs(v) : v;
        }
    }
    return M;
}

}  // namespace mc
#endif
