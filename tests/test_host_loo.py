"""Leave-one-out validation through the C host layer (libEmuMI.so: emulate_loo, emulate_loo_multi) and the CLI's
`validate` run mode, against the device library's own entry and against brute-force refits through the oracle."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

import looref
from madaiemulator_amd import abi, build, synth
from oracle import oracle as O
from test_host_api import parse_snapshot

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
UNI = os.path.join(ROOT, "tests", "golden", "ref_inputs", "uni-simple.input_model_file.dat")
G6SNAP = os.path.join(ROOT, "tests", "golden", "g6_multi_snapshot.txt")


@pytest.fixture(scope="module")
def cli():
    build.build_all()
    return build.CLI_BIN


@pytest.fixture(scope="module")
def loo_driver(tmp_path_factory):
    build.build_all()
    exe = str(tmp_path_factory.mktemp("drv") / "host_loo_driver")
    subprocess.check_call(["gcc", "-std=gnu99", "-O1", "-I", os.path.join(ROOT, "include"), "-I", build.HOST_SRC,
                           "-o", exe, os.path.join(ROOT, "tests", "c", "host_loo_driver.c"),
                           "-L", build.LIBDIR, "-lEmuMI", "-lgpemu_hip", f"-Wl,-rpath,{build.LIBDIR}", "-lm"])
    return exe


# ------------------------------------------------------------------ 8. emulate_loo == gpemu_loo
@pytest.mark.gpu
@pytest.mark.parametrize("cov,order", [(1, 1), (3, 0)])
def test_emulate_loo_equals_the_device_entry(loo_driver, gpu_ctx, cov, order):
    X, Y = synth.read_input_model_file(UNI)
    y = Y[:, 0]
    th = np.array([0.3, -3.0, -0.4]) if cov == 1 else np.array([1.3, 0.02, np.log(0.8)])
    out = subprocess.run([loo_driver, "loo", UNI, str(cov), str(order)] + [repr(float(t)) for t in th], capture_output=True,
                         text=True, timeout=300)
    assert out.returncode == 0, out.stderr[-3000:]
    got = np.array([line.split()[1:] for line in out.stdout.splitlines() if line.startswith("loo ")], float)
    assert got.shape == (len(y), 2)
    gpu_ctx.set_model(cov, order, X, y)
    _, rc = gpu_ctx.predict_setup(th)
    assert rc == abi.OK
    m, v = gpu_ctx.loo()
    assert np.array_equal(got[:, 0], m) and np.array_equal(got[:, 1], v)      # the same launches on the same state
    assert looref.min_offdiag(O.cov_matrix(cov, X, th)) >= looref.CLAMP
    mo, vo = looref.oracle_refits(cov, order, X, y, th, range(len(y)))
    em, ev = looref.errors(m, v, mo, vo, O.cov(cov, X[0], X[0], th))
    print(f"uni-simple cov {cov} order {order}: {em:.3e} {ev:.3e}")
    assert em < 1e-8 and ev < 1e-8


# ------------------------------------------------------------------ 9. the CLI's validate mode
def g6_reference():
    """per component: leave-one-out at every training point by refits through the oracle; then the back-projection"""
    sd = parse_snapshot(open(G6SNAP).read().split())
    N, nt, nr = sd["N"], sd["nt"], sd["nr"]
    mr, vr = np.empty((N, nr)), np.empty((N, nr))
    for c, mod in enumerate(sd["models"]):
        assert looref.min_offdiag(O.cov_matrix(mod["cov"], mod["X"], mod["thetas"])) >= looref.CLAMP
        mr[:, c], vr[:, c] = looref.oracle_refits(mod["cov"], mod["order"], mod["X"], mod["z"], mod["thetas"], range(N))
    ybar = sd["Y"].mean(axis=0)
    mean, var = np.empty((N, nt)), np.empty((N, nt))
    for i in range(N):
        mean[i], var[i] = O.pca_backproject(ybar, sd["evals"], sd["evecs"], mr[i], vr[i])
    return sd, mr, vr, mean, var


@pytest.mark.gpu
def test_validate_mode_on_the_g6_snapshot(cli, tmp_path):
    sd, mr, vr, mean, var = g6_reference()
    N, nt, nr, d = sd["N"], sd["nt"], sd["nr"], sd["d"]
    out = subprocess.run([cli, "validate", G6SNAP], capture_output=True, text=True, timeout=300, cwd=tmp_path)
    assert out.returncode == 0, out.stderr[-3000:]
    lines = out.stdout.splitlines()
    # the header interactive_mode prints: d, the parameter names, 2 nt, the output names
    header = [str(d)] + [f"param_{i}" for i in range(d)] + [str(2 * nt)]
    for i in range(nt):
        header += [f"mean_{i}", f"variance_{i}"]
    assert lines[:len(header)] == header
    vals = np.array([ln.split() for ln in lines[len(header):]], float).reshape(N, nt, 2)
    # the G6 test's tolerances (test_host_api.py::test_multi_output_golden_g6_through_the_c_layer)
    assert np.max(np.abs(vals[:, :, 0] - mean)) < 1e-8 * max(1.0, np.abs(mean).max())
    assert np.max(np.abs(vals[:, :, 1] - var)) < 1e-8 * max(1e-3, np.abs(var).max())
    # the summary on stderr, recomputed from stdout and the training matrix as given in the input
    summ = [ln.split() for ln in out.stderr.splitlines() if ln.startswith("# loo output ")]
    assert [s[3] for s in summ] == [f"{j}:" for j in range(nt)]
    for j, s in enumerate(summ):
        assert s[4] == "rmse" and s[6] == "mean_standardised_sq"
        r = sd["Y"][:, j] - vals[:, j, 0]
        assert float(s[5]) == pytest.approx(np.sqrt(np.mean(r * r)), rel=1e-12)
        assert float(s[7]) == pytest.approx(np.mean(r * r / vals[:, j, 1]), rel=1e-12)
    # --quiet: the N lines alone, nothing on stderr about the outputs
    q = subprocess.run([cli, "validate", G6SNAP, "--quiet"], capture_output=True, text=True, timeout=300, cwd=tmp_path)
    assert q.returncode == 0 and q.stdout.splitlines() == lines[len(header):] and "# loo output" not in q.stderr
    # --pca_output (which, as in the reference's option parser, implies --quiet): nr pairs per line, the components' own values
    z = subprocess.run([cli, "validate", G6SNAP, "--pca_output"], capture_output=True, text=True, timeout=300, cwd=tmp_path)
    assert z.returncode == 0, z.stderr[-3000:]
    pv = np.array([ln.split() for ln in z.stdout.splitlines()], float).reshape(N, nr, 2)
    assert np.max(np.abs(pv[:, :, 0] - mr)) < 1e-8 * max(1.0, np.abs(mr).max())
    assert np.max(np.abs(pv[:, :, 1] - vr)) < 1e-8 * max(1e-3, np.abs(vr).max())


# ------------------------------------------------------------------ 10. without a device
def test_usage_names_validate_and_a_missing_snapshot_fails(cli, tmp_path):
    def go(*args):
        return subprocess.run([cli] + list(args), capture_output=True, text=True, timeout=60, cwd=tmp_path)

    r = go("no_such_mode", "x")
    assert r.returncode != 0 and r.stderr.startswith("useage:")
    assert "validate MODEL_SNAPSHOT_FILE" in r.stderr and "print_thetas MODEL_SNAPSHOT_FILE" in r.stderr
    a, b = go("validate", "no_such_snapshot"), go("print_thetas", "no_such_snapshot")
    assert a.returncode != 0 and b.returncode != 0 and a.stderr == b.stderr and a.stdout == b.stdout == ""


def test_symbols_are_exported():
    build.build_all()
    dev, host = ctypes.CDLL(build.HIP_LIB), ctypes.CDLL(build.HOST_LIB)
    for name in ("gpemu_loo", "gpemu_loo_dev"):
        assert hasattr(dev, name) and name in abi.SYMBOLS
    for name in ("emulate_loo", "emulate_loo_multi"):
        assert hasattr(host, name)
    assert abi.PROF_LOO == 7 and hasattr(abi.Context, "loo")
