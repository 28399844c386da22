"""The calibration references and the host arithmetic of the calibration entries, on the CPU (no device):

  * calibref.direct64 against its 50-digit repeat on every input family the GPU tests use: the errors that calibref.BARS are
    8 x of, recomputed here; the share of points whose worst output is undecided stays inside the GPU tests' 5 % cap
  * the r x r identity in float64 on gpemu_calib_project's tables against the same 50-digit numbers: inside the
    bars before a device runs
  * gpemu_calib_project through ctypes against 50 digits, and its error codes
"""
import ctypes as C
import functools
import os

import numpy as np
import pytest

import calibref as R
from madaiemulator_amd import abi

EPS = np.finfo(float).eps


@functools.lru_cache(maxsize=None)
def family(i):
    c = R.all_cases()[i]
    pts = R.mp_points(c)
    ref, wref = R.direct_mp(c, pts)
    s64, w64 = R.direct64(c)
    return c, pts, ref, wref, s64, w64


NAMES = [a[0] for a in R.CASES] + ["special_" + k for k in R.SPECIALS]


@pytest.mark.parametrize("i", range(len(NAMES)), ids=NAMES)
def test_float64_reference_against_50_digits(i):
    c, pts, ref, wref, s64, w64 = family(i)
    if c["name"] == "special_v_huge":
        # float64 cannot factor S + A D A^T at v = 1e30 (what the r x r form is for): the GPU test of this family takes the
        # 50-digit numbers alone; the per-output rows do not need the factorisation and still agree
        assert np.all(R.err(s64[2:, pts], ref[2:]) <= R.MEASURED[2:, None])
        return
    e = R.err(s64[:, pts], ref).max(axis=1)
    print(c["name"], e)
    assert np.all(e <= R.MEASURED), (c["name"], e)
    comp = R.worst_comparable(s64)
    if c["name"] != "special_ties":                      # (its top two are one output twice: the tie test asserts the index)
        assert 1.0 - comp.mean() <= 0.05
    assert np.array_equal(w64[pts][comp[pts]], wref[comp[pts]])


def test_bars_are_eight_times_the_measured_errors():
    assert np.array_equal(R.BARS, 8.0 * R.MEASURED)


@pytest.mark.parametrize("i", range(len(NAMES)), ids=NAMES)
def test_r_form_on_projected_tables_is_inside_the_bars(i):
    c, pts, ref, _, s64, _ = family(i)
    pj = abi.calib_project(c["ybar"], c["A"], c["z"], S=c["S"], sd=c["sd"])
    assert pj["status"] == abi.OK and pj["info"] == 0
    rf = R.rform64(c, pj)
    assert np.all(R.err(rf[:, pts], ref[:2]) <= R.BARS[:2, None])
    if c["name"] != "special_v_huge":
        assert np.all(R.err(rf, s64[:2]) <= R.BARS[:2, None])


@pytest.mark.parametrize("i", range(len(NAMES)), ids=NAMES)
def test_project_against_50_digits(i):
    """Bound: every step is a Cholesky factorisation or a triangular solve in float64, backward stable, so the forward error
    of m_hat and Sigma_z is c eps (cond(S) + cond(G)) relative to their largest element, with c = 256 covering the
    dimension factors at nt <= 130; the scalars likewise against max(1, |value|)."""
    c = R.all_cases()[i]
    pj = abi.calib_project(c["ybar"], c["A"], c["z"], S=c["S"], sd=c["sd"])
    assert pj["status"] == abi.OK
    ref = R.project_mp(c)
    S = R._smat(c)
    G = c["A"].T @ np.linalg.solve(S, c["A"])
    tol = 256 * EPS * (np.linalg.cond(S) + np.linalg.cond(G))
    assert np.abs(pj["mhat"] - ref["mhat"]).max() <= tol * np.abs(ref["mhat"]).max()
    assert np.abs(pj["sigz"] - ref["sigz"]).max() <= tol * np.abs(ref["sigz"]).max()
    for k in ("c_perp", "logdet_S", "logdet_G"):
        assert abs(pj[k] - ref[k]) <= tol * max(1.0, abs(ref[k])), k
    assert pj["c_perp"] >= 0.0
    assert np.array_equal(pj["sigz"], pj["sigz"].T)      # symmetric bit for bit


def test_project_r_equals_nt_has_no_misfit_left():
    c = R.make_case(*R.CASES[10])                        # nr = nt = 16
    pj = abi.calib_project(c["ybar"], c["A"], c["z"], sd=c["sd"])
    assert pj["status"] == abi.OK and 0.0 <= pj["c_perp"] <= 1e-20


def test_project_error_codes():
    L = abi.load()
    c = R.make_case(*R.CASES[3])                         # nr 4, nt 7, full S
    nt, nr = c["nt"], c["nr"]
    dp = lambda a: None if a is None else a.ctypes.data_as(C.POINTER(C.c_double))
    mhat, sigz, consts, info = np.empty(16), np.empty(256), np.empty(3), C.c_int(-5)

    def rc(nt=nt, nr=nr, ybar=c["ybar"], A=c["A"], z=c["z"], S=c["S"], sd=None, mhat=mhat, sigz=sigz, consts=consts, info=C.byref(info)):
        return L.gpemu_calib_project(nt, nr, dp(ybar), dp(A), dp(z), dp(S), dp(sd), dp(mhat), dp(sigz), dp(consts), info)

    assert rc() == abi.OK and info.value == 0
    sd = np.full(nt, 0.2)
    for kw in (dict(ybar=None), dict(A=None), dict(z=None), dict(mhat=None), dict(sigz=None), dict(consts=None), dict(info=None),
               dict(S=None), dict(sd=sd), dict(nt=0), dict(nr=0), dict(nr=nt + 1), dict(nr=17, nt=18), dict(nt=1025)):
        assert rc(**kw) == abi.ERR_ARG, kw
    for key in ("ybar", "A", "z", "S"):
        for v in (np.nan, np.inf):
            bad = c[key].copy()
            bad.flat[1] = v
            assert rc(**{key: bad}) == abi.ERR_ARG, (key, v)
    for v in (0.0, -0.1, np.nan):
        bad = sd.copy(); bad[2] = v
        assert rc(S=None, sd=bad) == abi.ERR_ARG
    assert rc(S=None, sd=sd) == abi.OK
    Sb = c["S"].copy(); Sb[1, 1] = -1.0
    assert rc(S=Sb) == abi.ERR_NOT_PD and info.value == 2 and np.isnan(consts).all()
    Ab = c["A"].copy(); Ab[:, 2] = 0.0
    assert rc(A=Ab) == abi.ERR_NOT_PD and info.value == 3
    Ab = c["A"].copy(); Ab[:, 3] = 2.0 * Ab[:, 0]         # no full column rank, to working precision
    assert rc(A=Ab) == abi.ERR_NOT_PD and info.value == 4


# ------------------------------------------------------------------ the CLI's observation file (parsed before any device is touched)
def _cli(tmp_path, text, extra=()):
    import os
    import subprocess
    from madaiemulator_amd import build
    build.build_all()
    snap = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "g6_multi_snapshot.txt")     # six outputs
    f = tmp_path / "obs.dat"
    f.write_text(text)
    return subprocess.run([build.CLI_BIN, "implausibility", snap, f"--observations={f}"] + list(extra), input="", capture_output=True,
                          text=True, timeout=120)


GOOD = "6\n" + "".join(f"{1.0 + t} 0.1{' 0.02' if t % 2 else ''}\n" for t in range(6))
COV = "covariance\n" + "".join(" ".join("0.01" if i == j else "0.001" for j in range(6)) + "\n" for i in range(6))


@pytest.mark.parametrize("text", [GOOD, GOOD + "\n", GOOD + COV], ids=["sd", "trailing_blank", "covariance"])
def test_cli_accepts_good_observation_files(tmp_path, text):
    """no points on stdin: where a device exists the run ends well; where none does it fails later, never in the parser"""
    out = _cli(tmp_path, text)
    assert "observation file" not in out.stderr, out.stderr
    assert out.returncode == 0 or "HIP device" in out.stderr or "gpemu error" in out.stderr, out.stderr


@pytest.mark.parametrize("text,why", [
    ("", "the number of outputs is missing"),
    ("5\n" + "1 0.1\n" * 5, "has 5 outputs, the model 6"),
    ("6\n" + "1 0.1\n" * 5, "ends before every output"),
    ("6\n" + "1 0.1\n" * 5 + "1\n", "two or three numbers"),
    ("6\n" + "1 0.1\n" * 5 + "1 0.1 0.0 7\n", "two or three numbers"),
    ("6\n" + "1 0.1\n" * 5 + "1 0\n", "sd > 0"),
    ("6\n" + "1 0.1\n" * 5 + "1 0.1 -0.5\n", "rel >= 0"),
    ("6\n" + "1 0.1\n" * 5 + "nan 0.1\n", "finite"),
    (GOOD + "variance\n", "is expected here"),
    (GOOD + COV[:-20], "covariance matrix"),
    (GOOD + COV.replace("0.001\n", "0.001 3\n", 1), "too many entries"),
    (GOOD + COV + COV, "is expected here"),
], ids=lambda v: None)
def test_cli_refuses_malformed_observation_files(tmp_path, text, why):
    out = _cli(tmp_path, text)
    assert out.returncode == 1 and why in out.stderr, (out.returncode, out.stderr)
    assert out.stdout == ""


def test_cli_refuses_pca_output_with_observations(tmp_path):
    out = _cli(tmp_path, GOOD, ["--pca_output"])
    assert out.returncode == 1 and "exclude each other" in out.stderr
    out = _cli(tmp_path, GOOD, ["--level=4"])
    assert out.returncode == 1 and "--level" in out.stderr


# ------------------------------------------------------------------ the interactive loop with extra values per point (no device)
@pytest.fixture(scope="module")
def loop_drivers(tmp_path_factory):
    import os
    import subprocess
    from madaiemulator_amd import build
    build.build_all()
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    tmp = tmp_path_factory.mktemp("ioextra")
    exes = []
    for src in ("io_loop_extra_driver.c", "io_loop_driver.c"):
        exe = str(tmp / src[:-2])
        subprocess.check_call(["gcc", "-std=gnu99", "-O1", "-I", os.path.join(root, "include"), "-I", build.HOST_SRC, "-o", exe,
                               os.path.join(root, "tests", "c", src), "-L", build.LIBDIR, "-lEmuMI", "-lgpemu_hip",
                               f"-Wl,-rpath,{build.LIBDIR}", "-lm", "-lpthread"])
        exes.append(exe)
    return exes


def _loop_expected(X, nout, nprint, nextra, binary):
    s = X.sum(axis=1)
    rows = np.zeros((len(X), 2 * nprint + nextra))
    for i in range(nout):
        rows[:, 2 * i] = (i + 1) * s
        rows[:, 2 * i + 1] = X[:, 0] * X[:, 0] + i
    for e in range(nextra):
        rows[:, 2 * nprint + e] = (e + 1) * X[:, 0] - s
    return rows.tobytes() if binary else "".join("%.17f\n" % v for v in rows.ravel()).encode()


@pytest.mark.parametrize("binary", [0, 1])
@pytest.mark.parametrize("nextra", [0, 3])
def test_extra_loop_burst_and_lone_point(loop_drivers, binary, nextra):
    """a burst of 20 000 waiting points (more than one 16 384-point batch) and then a lone point on the open pipe: every
    answer in input order, the extras behind the point's pairs; with nextra = 0 the bytes of gpemu_host_interactive_loop"""
    import subprocess
    extra_drv, plain_drv = loop_drivers
    rng = np.random.default_rng(9)
    X = rng.normal(size=(20000, 3))
    payload = X.tobytes() if binary else ("\n".join(" ".join(repr(float(v)) for v in r) for r in X) + "\n").encode()
    args = ["3", "2", "3", str(binary)]
    p = subprocess.run([extra_drv] + args + [str(nextra)], input=payload, capture_output=True, timeout=120)
    assert p.returncode == 0, p.stderr[-500:]
    assert p.stdout == _loop_expected(X, 2, 3, nextra, binary)
    assert int(p.stderr.split()[1]) == 20000
    if nextra == 0:
        q = subprocess.run([plain_drv] + args, input=payload, capture_output=True, timeout=120)
        assert q.returncode == 0 and q.stdout == p.stdout
    # a lone point is answered at once, while stdin stays open
    proc = subprocess.Popen([extra_drv] + args + [str(nextra)], stdin=subprocess.PIPE, stdout=subprocess.PIPE, stderr=subprocess.PIPE)
    try:
        one = X[:1]
        want = _loop_expected(one, 2, 3, nextra, binary)
        proc.stdin.write(one.tobytes() if binary else b"0.25 1.5 -2\n")
        proc.stdin.flush()
        if not binary:
            want = _loop_expected(np.array([[0.25, 1.5, -2.0]]), 2, 3, nextra, 0)
        got = b""
        import select
        while len(got) < len(want):
            ready, _, _ = select.select([proc.stdout], [], [], 10.0)
            assert ready, "no answer to a lone point: the loop is waiting for more input"
            got += os.read(proc.stdout.fileno(), len(want) - len(got))
        assert got == want
        proc.stdin.close()
        assert proc.wait(timeout=10) == 0
    finally:
        if proc.poll() is None:
            proc.kill()
        proc.stdout.close(); proc.stderr.close()


def test_extra_loop_argument_check(loop_drivers):
    """values without a function or a negative count: refused before anything is read"""
    import subprocess
    p = subprocess.run([loop_drivers[0], "3", "2", "3", "0", "-1"], input=b"1 2 3\n", capture_output=True, timeout=30)
    assert p.returncode == 3 and p.stdout == b""
