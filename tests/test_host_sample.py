"""Posterior samples of the parameters through the C host layer (libEmuMI.so: emulate_sample_posterior_multi), the C++ class
(emulator::SamplePosterior) and the command-line tool (interactive_emulator sample) on the committed multi-output snapshot.
The kernels and the run are judged in tests/test_gpu_sample.py; here the layers above them:

  * with given starts the host entry returns, bit for bit, what the library's run returns through the bridge, and what a
    second call returns
  * the default starts lie in the prior's support and are the replica's draws (tests/sampleref.prior_draws) to 1e-12
  * the summary's mean, standard deviation and quantiles against numpy on the returned trace, to rounding; tau against the
    replica's estimator on the ensemble-mean series
  * the C++ method hands on the C entry's bits
  * the CLI: nrec x W lines of d + 1 numbers in %.17g, two runs print the same bytes, every refusal has its message
"""
import ctypes
import subprocess

import numpy as np
import pytest

import sampleref as R
from madaiemulator_amd import abi, build
from test_host_api import parse_snapshot  # noqa: F401
from test_host_calib import write_cli_observation_file
from test_host_mean import G6SNAP, compile_driver

W, NSTEPS, BURN, THIN, SEED, STRETCH = 16, 30, 6, 2, 20101, 2.0
NREC = sum(1 for g in range(NSTEPS) if g >= BURN and (g + 1) % THIN == 0)


def rows(out, tag):
    return np.array([line.split()[1:] for line in out.splitlines() if line.startswith(tag + " ")], float)


@pytest.fixture(scope="module")
def case(tmp_path_factory):
    """the snapshot, an observation set around one training run, and a prior: uniform on the design's range but for parameter
    1, Gaussian around the range's centre"""
    sd = parse_snapshot(open(G6SNAP).read().split())
    d, nt = sd["d"], sd["nt"]
    assert W // 2 >= d + 1
    X = sd["models"][0]["X"]
    lo, hi, kind = X.min(axis=0).copy(), X.max(axis=0).copy(), np.zeros(d, dtype=int)
    if d > 1:
        kind[1], lo[1], hi[1] = 1, 0.5 * (X[:, 1].min() + X[:, 1].max()), 0.25 * (X[:, 1].max() - X[:, 1].min())
    sig = 0.3 * sd["Y"].std(axis=0)
    z = sd["Y"][7] + sig * np.cos(np.arange(nt))
    tmp = tmp_path_factory.mktemp("sample")
    obsf, priorf, x0f, cliobs, cliprior = (str(tmp / n) for n in ("obs.dat", "prior.dat", "x0.dat", "obs_cli.dat", "prior_cli.dat"))
    with open(obsf, "w") as f:
        f.write(" ".join(repr(float(v)) for v in z) + "\n" + " ".join(repr(float(v)) for v in sig) + "\n")
    with open(priorf, "w") as f:
        f.writelines(f"{int(k)} {float(a)!r} {float(b)!r}\n" for k, a, b in zip(kind, lo, hi))
    with open(cliprior, "w") as f:
        f.writelines(f"{'gaussian' if k else 'uniform'} {float(a)!r} {float(b)!r}\n" for k, a, b in zip(kind, lo, hi))
    write_cli_observation_file(cliobs, z, sig, None, None)
    x0 = X[7] + 0.05 * (X.max(axis=0) - X.min(axis=0)) * (R.prior_draws(5, W, np.zeros(d), np.ones(d), np.zeros(d, dtype=int)) - 0.5)
    x0 = np.clip(x0, np.where(kind == 1, -np.inf, lo), np.where(kind == 1, np.inf, hi))
    np.savetxt(x0f, x0, fmt="%.17g")
    return dict(sd=sd, d=d, lo=lo, hi=hi, kind=kind, obsf=obsf, priorf=priorf, x0f=x0f, x0=np.loadtxt(x0f, ndmin=2), cliobs=cliobs,
                cliprior=cliprior)


def run_args(c, x0f):
    return [G6SNAP, c["obsf"], c["priorf"], x0f, str(W), str(NSTEPS), str(BURN), str(THIN), str(SEED), repr(STRETCH)]


@pytest.fixture(scope="module")
def given(case, tmp_path_factory):
    drv = compile_driver(tmp_path_factory.mktemp("drv"), "host_sample_driver.c", False)
    out = subprocess.run([drv] + run_args(case, case["x0f"]), capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stderr[-3000:]
    dflt = subprocess.run([drv] + run_args(case, "-"), capture_output=True, text=True, timeout=300)
    assert dflt.returncode == 0, dflt.stderr[-3000:]
    return out.stdout, dflt.stdout


@pytest.mark.gpu
def test_host_entry_returns_the_library_runs_bits(case, given):
    out, _ = given
    d = case["d"]
    assert int(rows(out, "nrec")[0, 0]) == NREC and rows(out, "same")[0, 0] == 0
    tr = rows(out, "trace")
    assert tr.shape == (NREC * W, d + 1) and np.all(np.isfinite(tr))
    assert np.array_equal(rows(out, "start"), case["x0"])
    assert np.array_equal(tr[-W:, :d], rows(out, "end")) or THIN > 1 and (NSTEPS % THIN) != 0
    acc = rows(out, "accept")[0, 0]
    assert 0.0 < acc < 1.0
    uni = case["kind"] == 0
    assert np.all((tr[:, :d][:, uni] >= case["lo"][uni]) & (tr[:, :d][:, uni] <= case["hi"][uni]))


@pytest.mark.gpu
def test_default_starts_are_the_replicas_prior_draws(case, given):
    _, out = given
    d, lo, hi, kind = case["d"], case["lo"], case["hi"], case["kind"]
    st = rows(out, "start")
    want = R.prior_draws(SEED, W, lo, hi, kind)
    assert st.shape == (W, d) and rows(out, "same")[0, 0] == 0
    uni = kind == 0
    assert np.all((st[:, uni] >= lo[uni]) & (st[:, uni] <= hi[uni])) and np.all(np.isfinite(st))
    assert np.all(np.abs(st - want) <= 1e-12 * np.maximum(np.abs(want), np.abs(hi)))
    assert np.unique(st[:, 0]).size == W
    assert rows(out, "trace").shape == (NREC * W, d + 1)


@pytest.mark.gpu
def test_summary_against_numpy(case, given):
    for out in given:
        d = case["d"]
        x = rows(out, "trace")[:, :d]
        sm = rows(out, "summary")
        assert sm.shape == (6, d)
        tol = lambda v: 64 * np.finfo(float).eps * np.maximum(np.abs(v), np.abs(x).max(axis=0))
        for got, want in ((sm[0], x.mean(axis=0)), (sm[1], x.std(axis=0)), (sm[2], np.quantile(x, 0.025, axis=0)),
                          (sm[3], np.quantile(x, 0.5, axis=0)), (sm[4], np.quantile(x, 0.975, axis=0))):
            assert np.all(np.abs(got - want) <= tol(want)), (got, want)
        em = x.reshape(NREC, W, d).mean(axis=1)
        tau = np.array([R.autocorr_time(em[:, j]) for j in range(d)])
        assert np.all(np.abs(sm[5] - tau) <= 1e-9 * np.abs(tau)), (sm[5], tau)


@pytest.mark.gpu
def test_cpp_class_hands_on_the_c_entry(case, given, tmp_path_factory):
    drv = compile_driver(tmp_path_factory.mktemp("drvpp"), "emupp_sample_driver.cpp", True)
    for x0f, want in ((case["x0f"], given[0]), ("-", given[1])):
        out = subprocess.run([drv] + run_args(case, x0f), capture_output=True, text=True, timeout=300)
        assert out.returncode == 0, out.stderr[-3000:]
        for tag in ("nrec", "accept", "trace", "summary"):
            assert np.array_equal(rows(out.stdout, tag), rows(want, tag)), tag


@pytest.mark.gpu
def test_cli_sample_mode(case, given):
    d = case["d"]
    args = [build.CLI_BIN, "sample", G6SNAP, f"--observations={case['cliobs']}", f"--prior={case['cliprior']}", f"--walkers={W}",
            f"--steps={NSTEPS}", f"--burn={BURN}", f"--thin={THIN}", f"--seed={SEED}", f"--stretch={STRETCH!r}"]
    a = subprocess.run(args, capture_output=True, timeout=300)
    b = subprocess.run(args, capture_output=True, timeout=300)
    assert a.returncode == 0 and b.returncode == 0, a.stderr[-3000:]
    assert a.stdout == b.stdout                               # two runs print the same bytes
    lines = a.stdout.decode().splitlines()
    assert lines[0] == "# " + " ".join(f"param_{j}" for j in range(d)) + " log_posterior"
    assert len(lines) == 1 + NREC * W
    got = np.array([ln.split() for ln in lines[1:]], float)
    assert got.shape == (NREC * W, d + 1)
    # the default starts of the C entry under the same prior, seed and run: the same chain
    assert np.array_equal(got, rows(given[1], "trace"))
    assert all(tok == "%.17g" % float(tok) for ln in lines[1:4] for tok in ln.split())
    err = a.stderr.decode()
    sm = rows(given[1], "summary")
    assert f"{W} walkers, {NSTEPS} steps, {NREC} recorded (burn {BURN}, thin {THIN}), seed {SEED}" in err
    for j in range(d):
        assert f"# param_{j} mean {sm[0, j]:.17g} sd {sm[1, j]:.17g} q2.5 {sm[2, j]:.17g} q50 {sm[3, j]:.17g} q97.5 {sm[4, j]:.17g}" in err
    assert "fewer than 50 autocorrelation times" in err       # 12 recorded steps cannot be 50 tau
    quiet = subprocess.run(args + ["--quiet"], capture_output=True, timeout=300)
    assert quiet.returncode == 0 and quiet.stdout.decode().splitlines() == lines[1:]
    # without --prior / --box: uniform on the design's range
    plain = subprocess.run(args[:4] + args[5:], capture_output=True, timeout=300)
    assert plain.returncode == 0, plain.stderr[-3000:]
    X = case["sd"]["models"][0]["X"]
    p = np.array([ln.split() for ln in plain.stdout.decode().splitlines()[1:]], float)
    assert p.shape == (NREC * W, d + 1) and np.all((p[:, :d] >= X.min(axis=0)) & (p[:, :d] <= X.max(axis=0)))


@pytest.mark.gpu
def test_cli_refusals(case, tmp_path):
    base = [build.CLI_BIN, "sample", G6SNAP]
    obs = f"--observations={case['cliobs']}"
    box = tmp_path / "box.dat"
    with open(box, "w") as f:
        f.writelines("0 1\n" for _ in range(case["d"]))
    for extra, msg in (([], "sample needs --observations=FILE"),
                       ([obs, "--walkers=15"], "--walkers=W needs an even W"),
                       ([obs, "--walkers=2"], "each half of the walkers needs at least d + 1"),
                       ([obs, f"--box={box}", f"--prior={case['cliprior']}"], "--box=FILE and --prior=FILE exclude each other"),
                       ([obs, "--stretch=1"], "--stretch=a needs a finite a > 1"),
                       ([obs, "--steps=0"], "--steps=T needs T >= 1"),
                       ([obs, "--pca_output"], "exclude each other")):
        out = subprocess.run(base + extra, capture_output=True, text=True, timeout=60)
        assert out.returncode == 1 and msg in out.stderr and out.stdout == "", (extra, out.returncode, out.stderr[-500:])


def test_symbols_are_exported():
    build.build_all()
    dev, host = ctypes.CDLL(build.HIP_LIB), ctypes.CDLL(build.HOST_LIB)
    for name in ("gpemu_philox4x32", "gpemu_sample_uniforms", "gpemu_sample_set_prior", "gpemu_sample_release", "gpemu_sample_propose_dev",
                 "gpemu_sample_accept_dev", "gpemu_sample_logpost_dev", "gpemu_calib_sample", "gpemu_test_sample_chunk"):
        assert hasattr(dev, name) and name in abi.SYMBOLS
    for name in ("emulate_sample_posterior_multi", "gpemu_host_sample_starts", "gpemu_host_sample_nrec", "gpemu_host_autocorr_time",
                 "gpemu_host_calib_sample"):
        assert hasattr(host, name)
    assert b"SamplePosterior" in open(build.EPP_LIB, "rb").read()


def test_default_starts_need_no_device():
    """gpemu_host_sample_starts is host arithmetic on the library's generator: the replica's draws to 1e-12"""
    build.build_all()
    host = ctypes.CDLL(build.HOST_LIB)
    dp, ip = ctypes.POINTER(ctypes.c_double), ctypes.POINTER(ctypes.c_int)
    host.gpemu_host_sample_starts.argtypes = [ctypes.c_ulonglong, ctypes.c_int, ctypes.c_int, ip, dp, dp, dp]
    host.gpemu_host_sample_starts.restype = None
    lo, hi, kind = np.array([-1.0, 3.0, 0.5]), np.array([2.0, 0.25, 0.75]), np.array([0, 1, 0], dtype=np.int32)
    for seed in (0, 7, 2 ** 63 + 5):
        x0 = np.empty((40, 3))
        host.gpemu_host_sample_starts(seed, 40, 3, kind.ctypes.data_as(ip), lo.ctypes.data_as(dp), hi.ctypes.data_as(dp), x0.ctypes.data_as(dp))
        want = R.prior_draws(seed, 40, lo, hi, kind)
        assert np.all(np.abs(x0 - want) <= 1e-12 * np.maximum(np.abs(want), np.abs(hi)))
        assert x0[:, [0, 2]].tobytes() == want[:, [0, 2]].tobytes()       # the uniform coordinates: +, * alone, the same bits
