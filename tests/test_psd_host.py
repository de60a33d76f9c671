"""CPU checks of xmipp_ctf_estimate_from_micrograph and xmipp_psd_estimate: their usage lines and option parsing, every refusal arriving
before a device is opened with its own message and without an output file, the piece and patch lists through the library's host-only calls
(xh_psd_pieces, xh_psd_patches) against the restatement, and the host normalisation of psd_programs.h through a probe. None needs a device:
a refusal that came after opening one would fail here with the library's error instead."""
import os
import subprocess

import numpy as np
import pytest

import xmipp3_amd as xa
from tests import psd_ref as R
from tests import xmipp_io

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CTF = os.path.join(ROOT, "xmipp3_amd", "bin", "xmipp_ctf_estimate_from_micrograph")
PSD = os.path.join(ROOT, "xmipp3_amd", "bin", "xmipp_psd_estimate")
ERR_ARG_INCORRECT, ERR_ARG_MISSING, ERR_MATRIX_DIM, ERR_GPU, ERR_NOT_IMPLEMENTED = 2, 3, 41, 60, 61
MODES = {R.MICROGRAPH: "micrograph", R.REGIONS: "regions", R.PARTICLES: "particles"}


def run(prog, *args):
    return subprocess.run([prog] + [str(a) for a in args], capture_output=True, text=True)


@pytest.fixture(scope="module")
def files(tmp_path_factory):
    d = tmp_path_factory.mktemp("psd")
    rng = np.random.default_rng(0)
    xmipp_io.write_stack(str(d / "mic.stk"), rng.standard_normal((1, 83, 61)))
    xmipp_io.write_stack(str(d / "two.stk"), rng.standard_normal((2, 83, 61)))
    xmipp_io.write_xmd(str(d / "near.pos"), [("particles", ["xcoor", "ycoor"], [[30, 40], [7, 40]])])
    xmipp_io.write_xmd(str(d / "top.pos"), [("particles", ["xcoor", "ycoor"], [[30, 7]])])
    xmipp_io.write_xmd(str(d / "good.pos"), [("particles", ["xcoor", "ycoor"], [[30, 40]])])
    return d


def test_usage_lines():
    r = run(CTF, "--help")
    assert r.returncode == 0
    for line in ("Estimate the CTF from a micrograph.", "--micrograph <arg> : File with the micrograph", "[--oroot <=>] : Rootname for output",
                 "[--psd_estimator <=periodogram>]", "[--pieceDim <=512>] : Size of the piece", "[--overlap <=0.5>]", "[--skipBorders <=2>]", "[--Nsubpiece <=1>]",
                 "[--mode <=micrograph> <=>]", "[--dont_estimate_ctf] : Do not fit a CTF to PSDs", "[--acceleration1D]", "[--N_AR <=24>]", "[--min_freq <=0.03>]",
                 "[--fastDefocus <=2> <=10>]", "[--bootstrapFit <=-1>]", "[--sampling_rate <=1>]", "[--defocusU <=0>]", "[--VPP_radius <=0>]",
                 "[--device <=0>] : HIP device (one device only)"):
        assert line in r.stdout + r.stderr, line
    r = run(PSD, "--help")
    assert r.returncode == 0
    for line in ("-i <arg> : Micrograph to be analyzed", "-o <arg> : PSD to be stored", "[--overlap <=0.4>] : overlap of the patches",
                 "[--patches <=384> <=384>] : size of the patches", "[--threads <=4>]", "[--skipNormalization]", "[--device <=0>]"):
        assert line in r.stdout + r.stderr, line


DONT = "--dont_estimate_ctf"


@pytest.mark.parametrize("mic,args,code,words", [
    ("mic.stk", (), ERR_NOT_IMPLEMENTED, "the CTF fit is not built yet"),
    ("mic.stk", ("--sampling_rate", 1.4, "--voltage", 200, "--spherical_aberration", 2.5, "--defocusU", -15000), ERR_NOT_IMPLEMENTED, "the CTF fit is not built yet"),
    ("mic.stk", (DONT, "--psd_estimator", "ARMA"), ERR_NOT_IMPLEMENTED, "--psd_estimator ARMA: only the periodogram is built"),
    ("mic.stk", (DONT, "--bootstrapFit", 5), ERR_NOT_IMPLEMENTED, "--bootstrapFit belongs to the CTF fit"),
    ("mic.stk", (DONT, "--Nsubpiece", 2), ERR_NOT_IMPLEMENTED, "--Nsubpiece 2: only 1 is built"),
    ("mic.stk", (DONT, "--pieceDim", 64), ERR_MATRIX_DIM, "the micrograph of 83 x 61 is smaller than a piece of 64"),
    ("mic.stk", (DONT, "--pieceDim", 1025), ERR_ARG_INCORRECT, "--pieceDim 1025: piece sides of 2 .. 1024 are supported"),
    ("mic.stk", (DONT, "--pieceDim", 1), ERR_ARG_INCORRECT, "--pieceDim 1: piece sides of 2 .. 1024 are supported"),
    ("mic.stk", (DONT, "--pieceDim", 16, "--overlap", 1.0), ERR_ARG_INCORRECT, "0 <= overlap < 1"),
    ("mic.stk", (DONT, "--pieceDim", 16, "--skipBorders", 4), ERR_GPU, "no piece is left (7 x 10 divisions, skipBorders 4), where the reference divides by zero"),
    ("mic.stk", (DONT, "--pieceDim", 16, "--mode", "regions"), ERR_GPU, "The micrograph is not big enough to skip 2 pieces on each side"),
    ("mic.stk", (DONT, "--pieceDim", 16, "--mode", "particles", "near.pos"), ERR_GPU, "particle 2 at (x 7, y 40) is nearer than pieceDim / 2 = 8 to the left or top edge"),
    ("mic.stk", (DONT, "--pieceDim", 16, "--mode", "particles", "top.pos"), ERR_GPU, "particle 1 at (x 30, y 7) is nearer than pieceDim / 2 = 8"),
    ("mic.stk", (DONT, "--pieceDim", 16, "--mode", "particles"), ERR_ARG_MISSING, "--mode particles needs the file with the positions"),
    ("mic.stk", (DONT, "--pieceDim", 16, "--mode", "tiles"), ERR_ARG_INCORRECT, "--mode tiles: micrograph, regions or particles"),
    ("mic.stk", (DONT, "--pieceDim", 16, "--device", "0,1"), ERR_ARG_INCORRECT, "--device 0,1: this program runs on one device"),
    ("two.stk", (DONT, "--pieceDim", 16, "--skipBorders", 1, "--mode", "regions"), ERR_ARG_INCORRECT, "a stack of 2 micrographs is taken in --mode micrograph only"),
    ("two.stk", (DONT, "--pieceDim", 16, "--mode", "particles", "good.pos"), ERR_ARG_INCORRECT, "a stack of 2 micrographs is taken in --mode micrograph only"),
])
def test_ctf_program_refusals_come_before_any_device(files, mic, args, code, words):
    args = [files / a if isinstance(a, str) and a.endswith(".pos") else a for a in args]
    r = run(CTF, "--micrograph", files / mic, "--oroot", files / "refused", *args)
    assert r.returncode == code, r.stderr
    assert words in r.stderr, r.stderr
    assert not os.path.exists(files / "refused.psd") and not os.path.exists(files / "refused.psdstk")


@pytest.mark.parametrize("args,code,words", [
    (("--patches", 62, 16), ERR_MATRIX_DIM, "the patch of 16 x 62 is larger than the micrograph of 83 x 61"),
    (("--patches", 16, 84), ERR_MATRIX_DIM, "the patch of 84 x 16 is larger than the micrograph of 83 x 61"),
    (("--patches", 16, 16, "--overlap", 1.0), ERR_ARG_INCORRECT, "--overlap 1.0: 0 <= overlap < 1 is expected"),
    (("--patches", 16, 16, "--overlap", -0.1), ERR_ARG_INCORRECT, "0 <= overlap < 1 is expected"),
    (("--patches", 16, 1025), ERR_ARG_INCORRECT, "patch sides of 2 .. 1024 are supported"),
    (("--patches", 16, 16, "--device", "0,1"), ERR_ARG_INCORRECT, "this program runs on one device"),
])
def test_psd_program_refusals_come_before_any_device(files, args, code, words):
    out = files / "refused.psd"
    r = run(PSD, "-i", files / "mic.stk", "-o", out, "--threads", 7, *args)
    assert r.returncode == code, r.stderr
    assert words in r.stderr, r.stderr
    assert not os.path.exists(out)


def test_mandatory_options():
    assert run(CTF, "--dont_estimate_ctf").returncode == ERR_ARG_MISSING
    assert run(PSD, "-i", "x.stk").returncode == ERR_ARG_MISSING


@pytest.mark.parametrize("case", [c for c in R.cases() if c["dtype"] == np.float64], ids=lambda c: c["name"])
def test_piece_lists_against_the_restatement(case):
    _, Y, X = case["mic"].shape
    corners, slots, div = xa.psd_pieces(Y, X, case["py"], case["overlap"], case["skipBorders"], MODES[case["mode"]], case["pos"])
    assert corners.tolist() == [list(c) for c in case["corners"][0]] and slots.tolist() == case["slots"] and div == case["div"]


def test_piece_list_refusals():
    for kw, words in ((dict(mode="regions", skipBorders=2), "not big enough to skip 2 pieces"), (dict(mode="particles", pos=[(7, 30)]), "unsigned subtraction wraps"),
                      (dict(skipBorders=4), "no piece is left"), (dict(pieceDim=62), "smaller than a piece"), (dict(pieceDim=1025), "2 .. 1024"),
                      (dict(overlap=1.0), "overlap")):
        with pytest.raises(xa.XhError, match=words):
            xa.psd_pieces(83, 61, **{"pieceDim": 16, **kw})


def test_patch_lists_against_the_restatement():
    for Y, X, py, px, bx, by, ov in ((83, 61, 16, 24, 0, 0, 0.5), (83, 61, 24, 16, 0, 0, 0.4), (513, 512, 367, 64, 5, 5, 0.9), (32, 32, 5, 5, 0, 5, 0.2),
                                     (83, 61, 83, 61, 0, 0, 0.0), (512, 256, 64, 5, 5, 0, 0.9)):
        assert xa.psd_patches(Y, X, py, px, bx, by, ov).tolist() == [list(c) for c in R.patches(Y, X, py, px, bx, by, ov)]
    for args, words in (((83, 61, 84, 16), "larger than the micrograph"), ((83, 61, 16, 16, 30, 0), "borders"), ((83, 61, 16, 16, 0, 0, 1.0), "overlap")):
        with pytest.raises(xa.XhError, match=words):
            xa.psd_patches(*args)


def test_strip():
    assert xa.psd_strip() == R.STRIP


@pytest.fixture(scope="module")
def probe(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("probe") / "psd_probe")
    subprocess.check_call(["g++", "-O1", "-std=c++17", "-pthread", "-Wall", "-Wno-unused-function", os.path.join(ROOT, "tests", "host", "psd_probe.cpp"), "-o", exe])
    return exe


def test_host_normalisation_against_the_restatement(probe, tmp_path):
    rng = np.random.default_rng(7)
    for k, shape in enumerate(((24, 16), (17, 17), (96, 96))):
        v = (100 * np.abs(rng.standard_normal(shape))).astype(np.float32)
        v[0, 0], v[1, 1], v[2, 2] = 0.0, 1e-3, 1e7
        path = str(tmp_path / f"v{k}.bin")
        v.tofile(path)
        r = subprocess.run([probe, path], capture_output=True)
        assert r.returncode == 0
        got = np.frombuffer(r.stdout, np.float32).reshape(shape)
        assert np.array_equal(got, R.normalize_psd(v))
