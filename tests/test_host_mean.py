"""The mean-only prediction through the C host layer (libEmuMI.so: emulate_points_mean, emulate_points_multi_mean) and the
C++ class (emulator::QueryEmulatorMeans) against the means of the mean+variance entries beside them, on the reference's
example inputs.  Bar: |mean_only - mean| <= 1e-8 * max(1, |mean|) per value (the project's prediction bar); the device
entry itself is judged against an independent reference in tests/test_gpu_predict_mean.py."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

from madaiemulator_amd import abi, build, synth
from test_host_api import parse_snapshot

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REF = os.path.join(ROOT, "tests", "golden", "ref_inputs")
UNI = os.path.join(REF, "uni-simple.input_model_file.dat")
UNI_Q = os.path.join(REF, "uni-simple.sample_locations.dat")
G6SNAP = os.path.join(ROOT, "tests", "golden", "g6_multi_snapshot.txt")
RTOL = 1e-8


def compile_driver(tmp, src, cxx):
    build.build_all()
    exe = str(tmp / os.path.splitext(src)[0])
    cmd = (["g++", "-std=c++11"] if cxx else ["gcc", "-std=gnu99"]) + ["-O1", "-I", os.path.join(ROOT, "include"), "-I", build.HOST_SRC,
           "-o", exe, os.path.join(ROOT, "tests", "c", src), "-L", build.LIBDIR]
    cmd += (["-lEmuPlusPlusMI"] if cxx else []) + ["-lEmuMI", "-lgpemu_hip", f"-Wl,-rpath,{build.LIBDIR}", "-lm"]
    subprocess.check_call(cmd)
    return exe


@pytest.fixture(scope="module")
def mean_driver(tmp_path_factory):
    return compile_driver(tmp_path_factory.mktemp("drv"), "host_mean_driver.c", False)


@pytest.fixture(scope="module")
def multi_queries(tmp_path_factory):
    """training points of the snapshot (the nugget rule) and points inside its box"""
    sd = parse_snapshot(open(G6SNAP).read().split())
    X = sd["models"][0]["X"]
    lo, hi = X.min(axis=0), X.max(axis=0)
    Q = np.vstack([X[:5], lo + (hi - lo) * synth.queries(70, sd["d"], 4)])
    path = tmp_path_factory.mktemp("q") / "queries.dat"
    np.savetxt(path, Q, fmt="%.17g")
    return sd, str(path), len(Q)


def agree(a, b):
    err = float(np.max(np.abs(a - b) / np.maximum(1.0, np.abs(b))))
    print(f"max |mean_only - mean| / max(1,|mean|) = {err:.3e}")
    assert np.all(np.isfinite(a)) and err <= RTOL, err


@pytest.mark.gpu
@pytest.mark.parametrize("cov,order", [(1, 1), (3, 0)])
def test_emulate_points_mean(mean_driver, cov, order):
    th = np.array([0.3, -3.0, -0.4]) if cov == 1 else np.array([1.3, 0.02, np.log(0.8)])
    out = subprocess.run([mean_driver, "uni", UNI, UNI_Q, str(cov), str(order)] + [repr(float(t)) for t in th],
                         capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stderr[-3000:]
    got = np.array([line.split()[1:] for line in out.stdout.splitlines() if line.startswith("uni ")], float)
    nq = len(open(UNI_Q).read().split())
    assert got.shape == (nq, 3)
    agree(got[:, 2], got[:, 0])


@pytest.mark.gpu
def test_emulate_points_multi_mean(mean_driver, multi_queries):
    sd, qfile, nq = multi_queries
    out = subprocess.run([mean_driver, "multi", G6SNAP, qfile], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stderr[-3000:]
    for tag, no in (("pca", sd["nr"]), ("obs", sd["nt"])):
        v = np.array([line.split()[1:] for line in out.stdout.splitlines() if line.startswith(tag + " ")], float)
        assert v.shape == (nq, 2 * no)
        v = v.reshape(nq, no, 2)
        agree(v[:, :, 1], v[:, :, 0])
    # observable space is the reference's rule applied to the PCA-space means: training_mean + evecs diag(sqrt(evals)) m
    pca = np.array([line.split()[1:] for line in out.stdout.splitlines() if line.startswith("pca ")], float).reshape(nq, -1, 2)
    obs = np.array([line.split()[1:] for line in out.stdout.splitlines() if line.startswith("obs ")], float).reshape(nq, -1, 2)
    want = sd["Y"].mean(axis=0) + (pca[:, :, 1] * np.sqrt(sd["evals"])) @ sd["evecs"].T
    assert np.max(np.abs(obs[:, :, 1] - want)) <= 1e-12 * max(1.0, np.abs(want).max())


@pytest.mark.gpu
@pytest.mark.parametrize("pca", [False, True])
def test_query_emulator_means(tmp_path, multi_queries, pca):
    sd, qfile, nq = multi_queries
    exe = compile_driver(tmp_path, "emupp_mean_driver.cpp", True)
    out = subprocess.run([exe, G6SNAP, qfile] + (["pca"] if pca else []), capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stderr[-3000:]
    v = np.array([line.split()[1:] for line in out.stdout.splitlines() if line.startswith("q ")], float)
    no = sd["nr"] if pca else sd["nt"]
    assert v.shape == (nq, 2 * no)
    v = v.reshape(nq, no, 2)
    agree(v[:, :, 1], v[:, :, 0])


def test_symbols_are_exported():
    build.build_all()
    dev, host = ctypes.CDLL(build.HIP_LIB), ctypes.CDLL(build.HOST_LIB)
    for name in ("gpemu_predict_mean", "gpemu_predict_mean_dev", "gpemu_predict_mean_enqueue", "gpemu_predict_mean_collect"):
        assert hasattr(dev, name) and name in abi.SYMBOLS
    for name in ("emulate_points_mean", "emulate_points_mean_enqueue", "emulate_points_mean_collect", "emulate_points_multi_mean"):
        assert hasattr(host, name)
    assert abi.PROF_MEAN == 8
    for name in ("predict_mean", "predict_mean_dev", "predict_mean_enqueue", "predict_mean_collect"):
        assert hasattr(abi.Context, name)
    hdr = open(os.path.join(ROOT, "include", "gpemu.h")).read()
    assert "#define GPEMU_PROF_MEAN    8" in hdr and "emulator.c:672-704" in hdr
