"""Implausibility and calibration likelihood through the C host layer (libEmuMI.so: alloc_observations,
emulate_points_multi_implausibility, emulate_points_multi_nonimplausible) on the committed multi-output snapshot (N = 100,
three components, six outputs).  The kernels are judged in tests/test_gpu_calib.py; here the layer above them:

  * the statistics against calibref's direct nt x nt form evaluated at the library's OWN PCA-space means and variances
    (emulate_points_multi(..., pca_space = 1, ...)), under calibref.BARS -- this family's float64 reference is checked against
    50 digits here, under the same calibref.MEASURED the bars are eight times of
  * the per-output denominators against emulate_points_multi's observable-space means and variances, to the layer's parity
    bar 1e-8
  * the selection entry against the selection computed in numpy on the full entry's statistics, and its rows bit for bit
  * chi2 against sum_t I_t^2: with a full S and A D A^T they must differ, and chi2 must still be the direct form's
"""
import ctypes
import subprocess

import numpy as np
import pytest

import calibref as R
from madaiemulator_amd import abi, build
from test_host_api import parse_snapshot  # noqa: F401
from test_host_mean import G6SNAP, compile_driver, multi_queries  # noqa: F401  (multi_queries: a fixture)

RTOL = 1e-8


@pytest.fixture(scope="module")
def calib_driver(tmp_path_factory):
    return compile_driver(tmp_path_factory.mktemp("drv"), "host_calib_driver.c", False)


def observation_set(sd, full, hasrel):
    rng = np.random.default_rng(5 + 2 * full + hasrel)
    nt = sd["nt"]
    sig = 0.1 * sd["Y"].std(axis=0)
    z = sd["Y"][7] + sig * rng.standard_normal(nt)
    S = None
    if full:
        corr = 0.5 * np.ones((nt, nt)) + 0.5 * np.eye(nt)
        S = np.outer(sig, sig) * corr
    rel = np.full(nt, 0.02) if hasrel else None
    return z, sig, S, rel


def rows(out, tag):
    return np.array([line.split()[1:] for line in out.splitlines() if line.startswith(tag + " ")], float)


@pytest.fixture(scope="module", params=[(0, 0), (1, 1)], ids=["diag", "full_rel"])
def run(request, calib_driver, multi_queries, tmp_path_factory):
    full, hasrel = request.param
    sd, qfile, nq = multi_queries
    z, sig, S, rel = observation_set(sd, full, hasrel)
    path = tmp_path_factory.mktemp("obs") / "obs.dat"
    with open(path, "w") as f:
        f.write(f"{full} {hasrel}\n")
        for a in (z, S if full else sig) + ((rel,) if hasrel else ()):
            f.write(" ".join(repr(float(x)) for x in np.ravel(a)) + "\n")
    stat_all = None
    outs = {}
    for cuts in (("inf", "1", "inf"), None):
        if cuts is None:                                  # cuts at this run's own medians: about a quarter survives
            cuts = (repr(float(np.median(stat_all[:, 0]))), "2", repr(float(np.median(stat_all[:, 3]))))
        out = subprocess.run([calib_driver, G6SNAP, qfile, str(path)] + list(cuts), capture_output=True, text=True, timeout=300)
        assert out.returncode == 0, out.stderr[-3000:]
        outs[cuts] = out.stdout
        stat_all = rows(out.stdout, "stat")
    case = dict(name="g6", nt=sd["nt"], nr=sd["nr"], M=nq, ybar=sd["Y"].mean(axis=0), A=sd["evecs"] * np.sqrt(sd["evals"]), z=z,
                S=S, sd=None if full else sig, rel=rel)
    case["obs_file"], case["qfile"] = str(path), qfile
    return sd, nq, case, outs


@pytest.mark.gpu
def test_statistics_against_the_direct_form(run):
    sd, nq, c, outs = run
    for cuts, out in outs.items():
        st = rows(out, "stat")
        assert st.shape == (nq, 6) and rows(out, "same")[0, 0] == 0
        c["mean"], c["var"] = np.ascontiguousarray(rows(out, "pca_m").T), np.ascontiguousarray(rows(out, "pca_v").T)
        # ybar and A bit for bit as the library's back-projection holds them (they agree with the snapshot's to rounding)
        ybar, A = rows(out, "ybar")[0], np.ascontiguousarray(rows(out, "acol").T)
        assert np.allclose(ybar, c["ybar"], rtol=1e-12, atol=1e-12) and np.allclose(A, c["A"], rtol=1e-12, atol=1e-12)
        c["ybar"], c["A"] = ybar, A
        sref, wref = R.direct64(c)
        pts = list(range(0, nq, 9))
        e64 = R.err(sref[:, pts], R.direct_mp(c, pts)[0]).max(axis=1)
        assert np.all(e64 <= R.MEASURED), e64            # this family's reference is as good as the bars assume
        e = R.err(st[:, :5].T, sref).max(axis=1)
        print("host statistics against the direct form:", e, "bars", R.BARS)
        assert np.all(e <= R.BARS), e
        comp = R.worst_comparable(sref)
        assert 1.0 - comp.mean() <= 0.05 and np.array_equal(st[comp, 5].astype(int), wref[comp])
        pj = abi.calib_project(c["ybar"], c["A"], c["z"], S=c["S"], sd=c["sd"])
        mis = rows(out, "misfit")[0]
        assert mis[0] == pj["c_perp"] and mis[1] == c["nt"] - c["nr"]


@pytest.mark.gpu
def test_denominators_against_observable_space_variances(run):
    sd, nq, c, outs = run
    out = next(iter(outs.values()))
    st, mo, vo = rows(out, "stat"), rows(out, "obs_m"), rows(out, "obs_v")
    rel = c["rel"] if c["rel"] is not None else np.zeros(c["nt"])
    S = R._smat(c)
    I = np.abs(c["z"] - mo) / np.sqrt(np.maximum(vo, 0.0) + np.diag(S) + (rel * mo) ** 2)
    top = -np.sort(-I, axis=1)[:, :3]
    e = np.abs(st[:, 2:5] - top) / np.maximum(1.0, np.abs(top))
    print("largest three implausibilities against emulate_points_multi's outputs:", e.max())
    assert e.max() <= RTOL
    gap = (top[:, 0] - top[:, 1]) / np.maximum(1.0, top[:, 0]) > RTOL
    assert np.array_equal(st[gap, 5].astype(int), np.argmax(I, axis=1)[gap])


@pytest.mark.gpu
def test_selection_against_numpy(run):
    sd, nq, c, outs = run
    for cuts, out in outs.items():
        st, keep = rows(out, "stat"), rows(out, "keep")
        c2, level, cI = float(cuts[0]), int(cuts[1]), float(cuts[2])
        want = np.flatnonzero((st[:, 0] <= c2) & (st[:, 1 + level] <= cI))
        assert int(rows(out, "nkeep")[0, 0]) == want.size
        if cuts[0] == "inf":
            assert want.size == nq
        else:
            assert 0 < want.size < nq
        assert np.array_equal(keep[:, 0].astype(int), want)
        assert np.array_equal(keep[:, 1:], st[want, :5])   # the survivors' rows are the full entry's, bit for bit


@pytest.mark.gpu
def test_chi2_keeps_the_correlation_between_outputs(run):
    """nt - nr = 3 directions of the outputs cannot be moved by any parameter value and A D A^T is far from diagonal: the
    joint chi2 is not sum_t I_t^2, which is what a diagonal-only rule would return"""
    sd, nq, c, outs = run
    out = next(iter(outs.values()))
    st, mo, vo = rows(out, "stat"), rows(out, "obs_m"), rows(out, "obs_v")
    rel = c["rel"] if c["rel"] is not None else np.zeros(c["nt"])
    diag_rule = np.sum((c["z"] - mo) ** 2 / (np.maximum(vo, 0.0) + np.diag(R._smat(c)) + (rel * mo) ** 2), axis=1)
    assert np.median(np.abs(st[:, 0] - diag_rule) / np.maximum(st[:, 0], diag_rule)) > 1e-2


def write_cli_observation_file(path, z, sig, S, rel):
    """the CLI's format: nt, then "value sd [rel]" per output, then optionally "covariance" and the matrix"""
    with open(path, "w") as f:
        f.write(f"{len(z)}\n")
        for t in range(len(z)):
            f.write(f"{float(z[t])!r} {float(sig[t])!r}" + (f" {float(rel[t])!r}" if rel is not None else "") + "\n")
        if S is not None:
            f.write("covariance\n")
            for row in S:
                f.write(" ".join(repr(float(x)) for x in row) + "\n")


@pytest.mark.gpu
def test_cli_implausibility_mode(run, tmp_path):
    """interactive_emulator implausibility: the kept points' lines carry the C entries' bits, the parameters as given, and
    the worst output of the full entry; stderr reports the fraction kept and c_perp with its degrees of freedom"""
    sd, nq, c, outs = run
    obsf = tmp_path / "obs_cli.dat"
    write_cli_observation_file(obsf, c["z"], np.sqrt(np.diag(R._smat(c))) if c["S"] is not None else c["sd"], c["S"], c["rel"])
    Q = np.loadtxt(c["qfile"], ndmin=2)
    for cuts, want in outs.items():
        args = [build.CLI_BIN, "implausibility", G6SNAP, f"--observations={obsf}", f"--chi2={cuts[0]}", f"--level={cuts[1]}", f"--cut={cuts[2]}"]
        out = subprocess.run(args, stdin=open(c["qfile"]), capture_output=True, text=True, timeout=300)
        assert out.returncode == 0, out.stderr[-3000:]
        lines = out.stdout.splitlines()
        assert lines[0].startswith("# index param_0") and lines[0].endswith("worst_output")
        got = np.array([ln.split() for ln in lines[1:]], float).reshape(-1, 1 + sd["d"] + 6)
        keep, st = rows(want, "keep"), rows(want, "stat")
        assert np.array_equal(got[:, 0], keep[:, 0]) and np.array_equal(got[:, 1 + sd["d"]:6 + sd["d"]], keep[:, 1:])
        idx = got[:, 0].astype(int)
        assert np.array_equal(got[:, 1:1 + sd["d"]], Q[idx]) and np.array_equal(got[:, -1], st[idx, 5])
        mis = rows(want, "misfit")[0]
        assert f"kept {len(idx)} of {nq} points" in out.stderr and f"c_perp {mis[0]:.17g} with {int(mis[1])} degrees of freedom" in out.stderr
        quiet = subprocess.run(args + ["--quiet"], stdin=open(c["qfile"]), capture_output=True, text=True, timeout=300)
        assert quiet.returncode == 0 and quiet.stdout.splitlines() == lines[1:]


@pytest.mark.gpu
@pytest.mark.parametrize("binary", [False, True])
def test_cli_interactive_mode_with_observations(run, tmp_path, binary):
    """interactive_mode --observations: the header counts 2 nt + 3 returns and names the three; every point's pairs are the
    bytes the mode writes without the flag, followed by chi2, log likelihood and maximum implausibility of the C entry"""
    sd, nq, c, outs = run
    nt, d = sd["nt"], sd["d"]
    obsf = tmp_path / "obs_cli.dat"
    write_cli_observation_file(obsf, c["z"], np.sqrt(np.diag(R._smat(c))) if c["S"] is not None else c["sd"], c["S"], c["rel"])
    Q = np.loadtxt(c["qfile"], ndmin=2)
    payload = Q.tobytes() if binary else open(c["qfile"], "rb").read()
    base = [build.CLI_BIN, "interactive_mode", G6SNAP] + (["--binary"] if binary else [])
    plain = subprocess.run(base, input=payload, capture_output=True, timeout=300)
    flag = subprocess.run(base + [f"--observations={obsf}"], input=payload, capture_output=True, timeout=300)
    assert plain.returncode == 0 and flag.returncode == 0, flag.stderr[-3000:]
    nhead = 1 + d + 1 + 2 * nt                            # the header is text in either mode
    hp, hf = plain.stdout.split(b"\n", nhead)[:nhead], flag.stdout.split(b"\n", nhead + 3)[:nhead + 3]
    assert hp[:1 + d] == hf[:1 + d] and hp[1 + d] == str(2 * nt).encode() and hf[1 + d] == str(2 * nt + 3).encode()
    assert hf[2 + d:2 + d + 2 * nt] == hp[2 + d:] and hf[-3:] == [b"joint_implausibility", b"log_likelihood", b"max_implausibility"]
    bp, bf = plain.stdout.split(b"\n", nhead)[nhead], flag.stdout.split(b"\n", nhead + 3)[nhead + 3]
    st = rows(next(iter(outs.values())), "stat")
    if binary:
        vp, vf = np.frombuffer(bp).reshape(nq, 2 * nt), np.frombuffer(bf).reshape(nq, 2 * nt + 3)
        assert vf[:, :2 * nt].tobytes() == vp.tobytes() and np.array_equal(vf[:, 2 * nt:], st[:, :3])
    else:
        lp, lf = bp.split(b"\n")[:-1], bf.split(b"\n")[:-1]
        assert len(lp) == nq * 2 * nt and len(lf) == nq * (2 * nt + 3)
        for q in range(nq):
            rowf = lf[q * (2 * nt + 3):(q + 1) * (2 * nt + 3)]
            assert rowf[:2 * nt] == lp[q * 2 * nt:(q + 1) * 2 * nt]
            assert rowf[2 * nt:] == [("%.17f" % v).encode() for v in st[q, :3]]
    bad = subprocess.run(base + [f"--observations={obsf}", "--pca_output"], input=payload, capture_output=True, timeout=60)
    assert bad.returncode == 1 and b"exclude each other" in bad.stderr and bad.stdout == b""


@pytest.fixture(scope="module")
def emupp_driver(tmp_path_factory):
    return compile_driver(tmp_path_factory.mktemp("drvpp"), "emupp_calib_driver.cpp", True)


@pytest.mark.gpu
def test_cpp_class_hands_on_the_c_entries(run, emupp_driver):
    """emulator::SetObservations / QueryEmulatorImplausibility / QueryEmulatorNonImplausible: the C entries' bits"""
    sd, nq, c, outs = run
    for cuts, want in outs.items():
        out = subprocess.run([emupp_driver, G6SNAP, c["qfile"], c["obs_file"]] + list(cuts), capture_output=True, text=True, timeout=300)
        assert out.returncode == 0, out.stderr[-3000:]
        for tag in ("stat", "nkeep", "keep"):
            assert np.array_equal(rows(out.stdout, tag), rows(want, tag)), tag


def test_symbols_are_exported():
    build.build_all()
    dev, host = ctypes.CDLL(build.HIP_LIB), ctypes.CDLL(build.HOST_LIB)
    for name in ("gpemu_calib_project", "gpemu_calib_setup", "gpemu_calib_release", "gpemu_calib_eval", "gpemu_calib_eval_dev",
                 "gpemu_calib_select", "gpemu_calib_select_dev", "gpemu_calib_gather_dev", "gpemu_ctx_device"):
        assert hasattr(dev, name) and name in abi.SYMBOLS
    for name in ("alloc_observations", "free_observations", "gpemu_host_observations_misfit", "gpemu_host_confidence_to_rel",
                 "emulate_points_multi_implausibility", "emulate_points_multi_nonimplausible"):
        assert hasattr(host, name)
    epp = open(build.EPP_LIB, "rb").read()
    for name in (b"SetObservations", b"QueryEmulatorImplausibility", b"QueryEmulatorNonImplausible"):
        assert name in epp                                # (mangled: the name is part of the symbol)
    assert abi.PROF_CALIB == 16


def test_confidence_rule_against_erfinv():
    """sig / qnorm(1 - sig / 2) with qnorm(1 - sig / 2) = sqrt 2 erfinv(1 - sig) at 50 digits.  Bound: x solves
    erfc(x / sqrt 2) = sig, whose float64 evaluation is good to a few eps relative, so x moves by eps sig / (|f'(x)| x)
    relative, f' = sqrt(2 / pi) exp(-x^2 / 2); 8 eps (1 + that factor) covers it"""
    import mpmath as mp
    mp.mp.dps = 50
    build.build_all()
    host = ctypes.CDLL(build.HOST_LIB)
    fn = host.gpemu_host_confidence_to_rel
    fn.restype, fn.argtypes = ctypes.c_double, [ctypes.c_double]
    for sig in (1e-12, 1e-6, 0.001, 0.01, 0.05, 0.1, 0.3173, 0.5, 0.9, 0.99):
        x = mp.sqrt(2) * mp.erfinv(1 - mp.mpf(sig))
        want = float(mp.mpf(sig) / x)
        cond = float(mp.mpf(sig) / (mp.sqrt(2 / mp.pi) * mp.exp(-x * x / 2) * x))
        got = fn(sig)
        assert abs(got - want) <= 8 * np.finfo(float).eps * (1 + cond) * abs(want), (sig, got, want)
    for bad in (0.0, 1.0, -0.1, 1.5, np.nan):
        assert np.isnan(fn(bad))
