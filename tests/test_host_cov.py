"""The joint posterior covariance through the C host layer (libEmuMI.so: emulate_points_cov and its halves,
emulate_points_multi_cov) and the C++ class (emulator::QueryEmulatorCovariance) on the reference's example inputs and the
committed multi-output snapshot.  The device entry itself is judged against an independent reference in
tests/test_gpu_predict_cov.py; here the layers above it are checked: they hand on the device entry's bits, the
observable-space matrices are the numpy back-projection of the per-component ones,
cov_Y[t] = sum_c evecs[t][c]^2 evals[c] Sigma_c, to 1e-12 of the matrix's largest entry (nr terms: nr 2^-53 is what a
summation order can move), and the C++ class's diagonal is QueryEmulator's Errors squared to rounding."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

from madaiemulator_amd import abi, build, synth
from test_host_api import parse_snapshot  # noqa: F401  (used by the multi_queries fixture's module)
from test_host_mean import G6SNAP, UNI, UNI_Q, compile_driver, multi_queries  # noqa: F401  (multi_queries: a fixture)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def cov_driver(tmp_path_factory):
    return compile_driver(tmp_path_factory.mktemp("drv"), "host_cov_driver.c", False)


@pytest.fixture(scope="module")
def multi_out(cov_driver, multi_queries):
    sd, qfile, nq = multi_queries
    out = subprocess.run([cov_driver, "multi", G6SNAP, qfile], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stderr[-3000:]
    return out.stdout


def rows(out, tag):
    n = len(tag.split())
    return np.array([line.split()[n:] for line in out.splitlines() if line.startswith(tag + " ")], float)


@pytest.mark.gpu
@pytest.mark.parametrize("cov,order", [(1, 1), (3, 0), (2, 3)])
def test_emulate_points_cov_hands_on_the_device_entry(cov_driver, cov, order):
    """emulate_points_cov carries the bits of gpemu_predict_cov on a context of the test's own; a NULL mean, the pair and a
    second call change no bit; emulate_points after it returns what it returns alone"""
    th = np.array([0.3, -3.0, -0.4]) if cov == 1 else np.array([1.3, 0.02, np.log(0.8)])
    out = subprocess.run([cov_driver, "uni", UNI, UNI_Q, str(cov), str(order)] + [repr(float(t)) for t in th],
                         capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stderr[-3000:]
    X, Y = synth.read_input_model_file(UNI)
    d = X.shape[1]
    Xq = np.array(open(UNI_Q).read().split(), float).reshape(-1, d)
    M = Xq.shape[0]
    mean, S = rows(out.stdout, "mean")[0], rows(out.stdout, "cov")
    assert mean.shape == (M,) and S.shape == (M, M)
    assert rows(out.stdout, "same")[0, 0] == 0
    c = abi.Context(0)
    try:
        c.set_model(cov, order, X, Y[:, 0])
        _, rc = c.predict_setup(th)
        assert rc == abi.OK
        pm, pv = c.predict(Xq)
        m, Sd = c.predict_cov(Xq)
    finally:
        c.close()
    assert np.array_equal(mean, m) and np.array_equal(S, Sd)
    b = rows(out.stdout, "batch")
    assert np.array_equal(b[:, 0], pm) and np.array_equal(b[:, 1], pv)


@pytest.mark.gpu
def test_emulate_points_multi_cov(multi_out, multi_queries):
    sd, qfile, nq = multi_queries
    nr, nt = sd["nr"], sd["nt"]
    pca_m, obs_m = rows(multi_out, "pca_m"), rows(multi_out, "obs_m")
    assert pca_m.shape == (nq, nr) and obs_m.shape == (nq, nt)
    # PCA space: the per-component calls, bit for bit
    comp = []
    for c in range(nr):
        Sc = rows(multi_out, f"pca_c {c}")
        assert Sc.shape == (nq, nq)
        assert np.array_equal(Sc, rows(multi_out, f"comp_c {c}")) and np.array_equal(pca_m[:, c], rows(multi_out, f"comp_m {c}")[0])
        comp.append(Sc)
    # observable space: the reference's variance rule on every element, its mean rule on the means
    f = sd["evecs"] * np.sqrt(sd["evals"])
    f2 = sd["evecs"] ** 2 * sd["evals"]
    multi_v = rows(multi_out, "multi_v")
    for t in range(nt):
        St = rows(multi_out, f"obs_c {t}")
        want = sum(f2[t, c] * comp[c] for c in range(nr))
        err = float(np.max(np.abs(St - want)) / np.max(np.abs(want)))
        ed = float(np.max(np.abs(np.diag(St) - multi_v[:, t])) / np.max(np.abs(multi_v[:, t])))
        print(f"output {t}: against the back-projection {err:.3e} (bar 1e-12), diagonal against emulate_points_multi's variance {ed:.3e} (bar 1e-8)")
        assert St.shape == (nq, nq) and np.all(np.isfinite(St)) and np.array_equal(St, St.T)
        assert err <= 1e-12 and ed <= 1e-8
    want_m = sd["Y"].mean(axis=0) + pca_m @ f.T
    assert np.max(np.abs(obs_m - want_m) / np.maximum(1.0, np.abs(want_m))) <= 1e-12
    multi_m = rows(multi_out, "multi_m")
    assert np.max(np.abs(obs_m - multi_m) / np.maximum(1.0, np.abs(multi_m))) <= 1e-8


@pytest.mark.gpu
@pytest.mark.parametrize("pca", [False, True])
def test_query_emulator_covariance(tmp_path, multi_out, multi_queries, pca):
    """the C++ class returns the numbers of emulate_points_multi_cov, and a diagonal that is QueryEmulator's Errors squared to
    rounding"""
    sd, qfile, nq = multi_queries
    exe = compile_driver(tmp_path, "emupp_cov_driver.cpp", True)
    out = subprocess.run([exe, G6SNAP, qfile] + (["pca"] if pca else []), capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stderr[-3000:]
    no = sd["nr"] if pca else sd["nt"]
    tag = "pca" if pca else "obs"
    m, e = rows(out.stdout, "m"), rows(out.stdout, "e")
    assert np.array_equal(m, rows(multi_out, tag + "_m")) and e.shape == (nq, no)
    for o in range(no):
        S = rows(out.stdout, f"c {o}")
        assert np.array_equal(S, rows(multi_out, f"{tag}_c {o}"))
        v = np.diag(S)
        # (at a training point the variance rounds to about -1e-18 and QueryEmulator's error bar is NaN there)
        scale = np.abs(v).max()
        pos = v > 1e-8 * scale
        assert pos.sum() > pos.size // 2 and np.max(np.abs(e[pos, o] ** 2 - v[pos])) <= 1e-8 * scale
        assert np.all(np.abs(v[~pos]) <= 1e-8 * scale)


def test_symbols_are_exported():
    build.build_all()
    dev, host, epp = ctypes.CDLL(build.HIP_LIB), ctypes.CDLL(build.HOST_LIB), open(build.EPP_LIB, "rb").read()
    for name in ("gpemu_predict_cov", "gpemu_predict_cov_dev"):
        assert hasattr(dev, name) and name in abi.SYMBOLS
    for name in ("emulate_points_cov", "emulate_points_cov_enqueue", "emulate_points_cov_collect", "emulate_points_multi_cov"):
        assert hasattr(host, name)
    assert b"QueryEmulatorCovariance" in epp             # (mangled: the name is part of the symbol)
    assert abi.PROF_COV == 11
    for name in ("predict_cov", "predict_cov_dev"):
        assert hasattr(abi.Context, name)
    hdr = open(os.path.join(ROOT, "include", "gpemu.h")).read()
    assert "#define GPEMU_PROF_COV     11" in hdr
