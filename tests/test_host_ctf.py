"""The CTF model the host programs share with the device code (xmipp3_amd/csrc/xh_ctf.h, compiled here with plain g++ through
tests/host/ctf_probe.cpp) against the oracle's independent restatement, xo_ctf_value_pure_nok / K. No device needed."""
import math
import os
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FIELDS = ("Tm", "kV", "DeltafU", "DeltafV", "azimuthal_angle", "Cs", "Ca", "espr", "ispr", "alpha", "DeltaF", "DeltaR", "Q0", "K",
          "envR0", "envR1", "envR2", "phase_shift", "VPP_radius")
BASE = dict(Tm=1.4, kV=300.0, Cs=2.7, Q0=0.07, K=1.0)
# chosen so that each factor of the envelope lies between 0.2 and 0.95 over the frequencies below (with Ca in mm, espr / kV + 2e6 ispr of 1e-5)
ENVELOPE = dict(Ca=2.0, espr=0.003, ispr=2e-12, alpha=3e-5, DeltaF=80.0, DeltaR=1.5)
# every term of the formula is non-zero in at least one case
CASES = {
    "astigmatic": dict(BASE, DeltafU=18000.0, DeltafV=15500.0, azimuthal_angle=37.0),
    "round": dict(BASE, kV=200.0, DeltafU=21000.0, DeltafV=21000.0, K=0.75),
    "envelope_envR": dict(BASE, DeltafU=18000.0, DeltafV=15500.0, azimuthal_angle=37.0, envR0=0.02, envR1=-0.05, envR2=0.1, **ENVELOPE),
    "phase_plate": dict(BASE, DeltafU=6000.0, DeltafV=5500.0, azimuthal_angle=12.0, phase_shift=1.3, VPP_radius=0.02, **ENVELOPE),
    # K5 u^2 = pi DeltaF lambda u^2 passes 8 at u^2 = 0.043: both branches of J0 run
    "large_focal_spread": dict(BASE, DeltafU=18000.0, DeltafV=18000.0, DeltaF=3000.0),
}
FREQS = [(0.0, 0.0), (1e-7, 0.0), (0.01, 0.02), (0.1, -0.05), (0.2, 0.25), (-0.3, 0.1), (0.357, 0.357)]
# both sides evaluate one formula in double on one libm, arguments below 1e3 rad: the project's fp64 parity bound, on values of magnitude <= K <= 1
BOUND = 1e-12


@pytest.fixture(scope="module")
def probe(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("probe") / "ctf_probe")
    subprocess.check_call(["g++", "-O1", "-std=c++17", "-Wall", "-Wno-unused-function", os.path.join(ROOT, "tests", "host", "ctf_probe.cpp"), "-o", exe])
    return exe


def _fields(kw):
    return [repr(float(kw.get(f, 0.0))) for f in FIELDS]


def _expected(oracle, kw, freqs, degrees=False):
    kw = dict(kw)
    if degrees:
        kw["phase_shift"] = kw.get("phase_shift", 0.0) * math.pi / 180
    p = oracle.ctf_params(**kw)
    exp = np.array([oracle.lib().xo_ctf_value_pure_nok(p, x, y) for x, y in freqs]) / kw["K"]
    assert np.isfinite(exp).all()
    return exp


@pytest.mark.parametrize("case,degrees", [(c, False) for c in CASES] + [("phase_plate", True)])
def test_value_against_the_oracle(probe, oracle, case, degrees):
    """side_info + d_ctf_at with damping at a handful of frequencies, (0, 0) and (1e-7, 0) among them. phase_shift goes to the oracle
    as the radians that side_info makes of it under either setting of the unit flag. Measured maximum over all cases: 1.1e-16."""
    out = subprocess.check_output([probe, "value", str(int(degrees))] + _fields(CASES[case]) + [repr(v) for f in FREQS for v in f], text=True)
    got = np.array([float(x) for x in out.split()])
    exp = _expected(oracle, CASES[case], FREQS, degrees)
    err = np.abs(got - exp).max()
    print(f"{case} degrees={degrees}: max |diff| {err:.3g}, max |value| {np.abs(exp).max():.3g}")
    assert got.shape == exp.shape and np.abs(exp[2:]).max() > 0.05          # away from the origin, where only Q0 is left
    assert err <= BOUND


@pytest.mark.parametrize("flipped", [False, True])
def test_gallery_filter_table_against_the_oracle(probe, oracle, flipped):
    """ctfFilterTable, the matcher's --ctf table: 8 x 8, FFTW-order digital frequencies / Tm, |.| for phase-flipped data."""
    kw, P = CASES["envelope_envR"], 8
    out = subprocess.check_output([probe, "table"] + _fields(kw) + [str(P), str(int(flipped))], text=True)
    got = np.array([[float(x) for x in line.split()] for line in out.splitlines()])
    f = [(i if i <= P // 2 else i - P) / P * (1.0 / kw["Tm"]) for i in range(P)]
    exp = _expected(oracle, kw, [(fx, fy) for fy in f for fx in f]).reshape(P, P)
    if flipped:
        exp = np.abs(exp)
    assert got.shape == (P, P)
    assert np.abs(got - exp).max() <= BOUND
