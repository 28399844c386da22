"""The mean gradient through the C host layer (libEmuMI.so: emulate_points_mean_grad, emulate_points_multi_mean_grad) and
the C++ class (emulator::QueryEmulatorMeanGradients) on the reference's example inputs.  The device entry itself is judged
against an independent reference in tests/test_gpu_mean_grad.py; here the layers above it are checked: against central
differences (h = 1e-5) of the mean-only entries beside them -- a sanity yardstick only, bar 1e-6 max(1, |grad|_inf) -- and
the observable-space gradients against the numpy back-projection of the per-component ones,
grad_Y[t][j] = sum_c evecs[t][c] sqrt(evals[c]) grad_c[j], to 1e-12."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

from madaiemulator_amd import abi, build
from test_host_api import parse_snapshot
from test_host_mean import G6SNAP, UNI, UNI_Q, compile_driver, multi_queries  # noqa: F401  (multi_queries: a fixture)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CD_TOL = 1e-6


@pytest.fixture(scope="module")
def grad_driver(tmp_path_factory):
    return compile_driver(tmp_path_factory.mktemp("drv"), "host_mean_grad_driver.c", False)


def rows(out, tag):
    return np.array([line.split()[1:] for line in out.splitlines() if line.startswith(tag + " ")], float)


def near(what, g, c, tol):
    """g, c: (queries, outputs, d)"""
    scale = np.maximum(1.0, np.max(np.abs(g), axis=-1))
    err = float(np.max(np.max(np.abs(g - c), axis=-1) / scale))
    print(f"{what}: max_j |grad - other| / max(1, |grad|_inf) = {err:.3e}  (bar {tol:.1e})")
    assert np.all(np.isfinite(g)) and err <= tol, (what, err)


@pytest.mark.gpu
@pytest.mark.parametrize("cov,order", [(1, 1), (3, 0), (2, 3)])
def test_emulate_points_mean_grad(grad_driver, cov, order):
    th = np.array([0.3, -3.0, -0.4]) if cov == 1 else np.array([1.3, 0.02, np.log(0.8)])
    out = subprocess.run([grad_driver, "uni", UNI, UNI_Q, str(cov), str(order)] + [repr(float(t)) for t in th],
                         capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stderr[-3000:]
    v = rows(out.stdout, "uni")
    nq = len(open(UNI_Q).read().split())
    d = (v.shape[1] - 2) // 2
    assert v.shape[0] == nq // d and v.shape[1] == 2 + 2 * d
    assert np.max(np.abs(v[:, 1] - v[:, 0]) / np.maximum(1.0, np.abs(v[:, 0]))) <= 1e-8      # the returned mean
    near(f"uni cov {cov} order {order}", v[:, None, 2:2 + d], v[:, None, 2 + d:], CD_TOL)


@pytest.mark.gpu
def test_emulate_points_multi_mean_grad(grad_driver, multi_queries):
    sd, qfile, nq = multi_queries
    d = sd["d"]
    out = subprocess.run([grad_driver, "multi", G6SNAP, qfile], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stderr[-3000:]
    got = {}
    for tag, no in (("pca", sd["nr"]), ("obs", sd["nt"])):
        m, g, c = rows(out.stdout, tag + "_m"), rows(out.stdout, tag + "_g"), rows(out.stdout, tag + "_c")
        assert m.shape == (nq, no) and g.shape == (nq, no * d) and c.shape == (nq, no * d)
        got[tag] = (m, g.reshape(nq, no, d))
        near(tag + " space against central differences", g.reshape(nq, no, d), c.reshape(nq, no, d), CD_TOL)
    # observable space is the linear part of the reference's rule applied to the PCA-space results
    want_g = np.einsum("tc,qcj->qtj", sd["evecs"] * np.sqrt(sd["evals"]), got["pca"][1])
    near("observable space against the back-projection", got["obs"][1], want_g, 1e-12)
    want_m = sd["Y"].mean(axis=0) + (got["pca"][0] * np.sqrt(sd["evals"])) @ sd["evecs"].T
    assert np.max(np.abs(got["obs"][0] - want_m)) <= 1e-12 * max(1.0, np.abs(want_m).max())


@pytest.mark.gpu
@pytest.mark.parametrize("pca", [False, True])
def test_query_emulator_mean_gradients(tmp_path, multi_queries, pca):
    sd, qfile, nq = multi_queries
    d = sd["d"]
    exe = compile_driver(tmp_path, "emupp_mean_grad_driver.cpp", True)
    out = subprocess.run([exe, G6SNAP, qfile] + (["pca"] if pca else []), capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stderr[-3000:]
    no = sd["nr"] if pca else sd["nt"]
    m, g, c = rows(out.stdout, "m"), rows(out.stdout, "g"), rows(out.stdout, "c")
    assert m.shape == (nq, 2 * no) and g.shape == (nq, no * d) and c.shape == (nq, no * d)
    assert np.max(np.abs(m[:, :no] - m[:, no:]) / np.maximum(1.0, np.abs(m[:, no:]))) <= 1e-8
    near("QueryEmulatorMeanGradients against central differences", g.reshape(nq, no, d), c.reshape(nq, no, d), CD_TOL)


def test_symbols_are_exported():
    build.build_all()
    dev, host, epp = ctypes.CDLL(build.HIP_LIB), ctypes.CDLL(build.HOST_LIB), open(build.EPP_LIB, "rb").read()
    for name in ("gpemu_predict_mean_grad", "gpemu_predict_mean_grad_dev", "gpemu_predict_mean_grad_enqueue",
                 "gpemu_predict_mean_grad_collect"):
        assert hasattr(dev, name) and name in abi.SYMBOLS
    for name in ("emulate_points_mean_grad", "emulate_points_mean_grad_enqueue", "emulate_points_mean_grad_collect",
                 "emulate_points_multi_mean_grad"):
        assert hasattr(host, name)
    assert b"QueryEmulatorMeanGradients" in epp          # (mangled: the name is part of the symbol)
    assert abi.PROF_MEAN_GRAD == 9
    for name in ("predict_mean_grad", "predict_mean_grad_dev", "predict_mean_grad_enqueue", "predict_mean_grad_collect"):
        assert hasattr(abi.Context, name)
    hdr = open(os.path.join(ROOT, "include", "gpemu.h")).read()
    assert "#define GPEMU_PROF_MEAN_GRAD 9" in hdr
