"""K-fold / leave-group-out validation through the C host layer (libEmuMI.so: emulate_lgo, emulate_lgo_multi) and the CLI's
`validate --folds=K` / `--groups=FILE` modes, against the device library's own entry and against LAPACK refits per PCA
component (tests/lgoref.py, which checks itself first)."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

import lgoref
from madaiemulator_amd import abi, build, synth
from oracle import oracle as O
from test_host_api import parse_snapshot

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
UNI = os.path.join(ROOT, "tests", "golden", "ref_inputs", "uni-simple.input_model_file.dat")
G6SNAP = os.path.join(ROOT, "tests", "golden", "g6_multi_snapshot.txt")
RTOL = lgoref.RTOL
K = 3


@pytest.fixture(scope="module")
def cli():
    build.build_all()
    return build.CLI_BIN


@pytest.fixture(scope="module")
def lgo_driver(tmp_path_factory):
    build.build_all()
    exe = str(tmp_path_factory.mktemp("drv") / "host_lgo_driver")
    subprocess.check_call(["gcc", "-std=gnu99", "-O1", "-I", os.path.join(ROOT, "include"), "-I", build.HOST_SRC,
                           "-o", exe, os.path.join(ROOT, "tests", "c", "host_lgo_driver.c"),
                           "-L", build.LIBDIR, "-lEmuMI", "-lgpemu_hip", f"-Wl,-rpath,{build.LIBDIR}", "-lm"])
    return exe


@pytest.fixture(scope="module")
def g6():
    """the G6 snapshot and, per PCA component, the reference of three interleaved folds; then the back-projection"""
    sd = parse_snapshot(open(G6SNAP).read().split())
    N, nt, nr = sd["N"], sd["nt"], sd["nr"]
    group = lgoref.folds(N, K)
    refs = [lgoref.reference(m["cov"], m["order"], m["X"], m["z"], m["thetas"], group) for m in sd["models"]]
    mr = np.column_stack([r["mean"] for r in refs])
    vr = np.column_stack([r["var"] for r in refs])
    ybar = sd["Y"].mean(axis=0)
    mean, var = np.empty((N, nt)), np.empty((N, nt))
    for i in range(N):
        mean[i], var[i] = O.pca_backproject(ybar, sd["evals"], sd["evecs"], mr[i], vr[i])
    return dict(sd=sd, group=group, refs=refs, mr=mr, vr=vr, mean=mean, var=var)


def close(got, want, floor=1.0):
    return np.max(np.abs(got - want)) < RTOL * max(floor, float(np.abs(want).max()))


def check_stats(maha, logpdf, refs):
    for c, r in enumerate(refs):
        assert np.max(np.abs(maha[c] - r["maha"]) / np.maximum(1.0, r["maha"])) < RTOL
        assert np.max(np.abs(logpdf[c] - r["logpdf"]) / np.maximum(1.0, np.abs(r["logpdf"]))) < RTOL


# ------------------------------------------------------------------ emulate_lgo == gpemu_lgo
@pytest.mark.gpu
@pytest.mark.parametrize("cov,order", [(1, 1), (3, 0)])
def test_emulate_lgo_equals_the_device_entry(lgo_driver, gpu_ctx, cov, order):
    X, Y = synth.read_input_model_file(UNI)
    y = Y[:, 0]
    N = len(y)
    th = np.array([0.3, -3.0, -0.4]) if cov == 1 else np.array([1.3, 0.02, np.log(0.8)])
    out = subprocess.run([lgo_driver, "lgo", UNI, str(cov), str(order), str(K)] + [repr(float(t)) for t in th], capture_output=True,
                         text=True, timeout=300)
    assert out.returncode == 0, out.stderr[-3000:]
    pts = np.array([ln.split()[1:] for ln in out.stdout.splitlines() if ln.startswith("lgo ")], float)
    grp = np.array([ln.split()[1:] for ln in out.stdout.splitlines() if ln.startswith("grp ")], float)
    assert pts.shape == (N, 3) and grp.shape == (K, 2)
    gpu_ctx.set_model(cov, order, X, y)
    _, rc = gpu_ctx.predict_setup(th)
    assert rc == abi.OK
    group = lgoref.folds(N, K)
    res = gpu_ctx.lgo(group)
    assert res["status"] == abi.OK
    for j, k in enumerate(("mean", "var", "werr")):                        # the same launches on the same state
        assert np.array_equal(pts[:, j], res[k]), k
    assert np.array_equal(grp[:, 0], res["maha"]) and np.array_equal(grp[:, 1], res["logpdf"])
    ref = lgoref.reference(cov, order, X, y, th, group)
    e = lgoref.worst([lgoref.errors(g, r, ref["kappa"]) for g, r in zip(lgoref.split(res, ref["groups"]), ref["per_group"])])
    print(f"uni-simple cov {cov} order {order}: {e}")
    assert all(v < RTOL for v in e.values()), e


# ------------------------------------------------------------------ emulate_lgo_multi
@pytest.mark.gpu
@pytest.mark.parametrize("pca", [1, 0])
def test_emulate_lgo_multi_on_the_g6_snapshot(lgo_driver, g6, pca):
    sd = g6["sd"]
    N, nr, nout = sd["N"], sd["nr"], sd["nr"] if pca else sd["nt"]
    out = subprocess.run([lgo_driver, "multi", G6SNAP, str(K), str(pca)], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stderr[-3000:]
    pts = np.array([ln.split()[1:] for ln in out.stdout.splitlines() if ln.startswith("pt")], float).reshape(N, nout, 2)
    st = np.array([ln.split()[1:] for ln in out.stdout.splitlines() if ln.startswith("stat ")], float)
    assert st.shape == (nr * K, 4) and np.array_equal(st[:, 0], np.repeat(np.arange(nr), K)) and np.array_equal(st[:, 1], np.tile(np.arange(K), nr))
    mean, var = (g6["mr"], g6["vr"]) if pca else (g6["mean"], g6["var"])
    assert close(pts[:, :, 0], mean) and close(pts[:, :, 1], var, 1e-3)
    check_stats(st[:, 2].reshape(nr, K), st[:, 3].reshape(nr, K), g6["refs"])      # in PCA space whatever the outputs' space


# ------------------------------------------------------------------ the CLI
@pytest.mark.gpu
def test_validate_folds_on_the_g6_snapshot(cli, g6, tmp_path):
    sd = g6["sd"]
    N, nt, nr, d = sd["N"], sd["nt"], sd["nr"], sd["d"]

    def go(*args):
        return subprocess.run([cli, "validate", G6SNAP] + list(args), capture_output=True, text=True, timeout=300, cwd=tmp_path)

    out = go(f"--folds={K}")
    assert out.returncode == 0, out.stderr[-3000:]
    lines = out.stdout.splitlines()
    header = [str(d)] + [f"param_{i}" for i in range(d)] + [str(2 * nt)]
    for i in range(nt):
        header += [f"mean_{i}", f"variance_{i}"]
    assert lines[:len(header)] == header                                   # the leave-one-out mode's header
    vals = np.array([ln.split() for ln in lines[len(header):]], float).reshape(N, nt, 2)
    assert close(vals[:, :, 0], g6["mean"]) and close(vals[:, :, 1], g6["var"], 1e-3)
    summ = [ln.split() for ln in out.stderr.splitlines() if ln.startswith("# lgo output ")]
    assert [s[3] for s in summ] == [f"{j}:" for j in range(nt)]
    for j, s in enumerate(summ):
        assert s[4] == "rmse" and s[6] == "mean_standardised_sq"
        r = sd["Y"][:, j] - vals[:, j, 0]
        assert float(s[5]) == pytest.approx(np.sqrt(np.mean(r * r)), rel=1e-12)
        assert float(s[7]) == pytest.approx(np.mean(r * r / vals[:, j, 1]), rel=1e-12)
    comp = [ln.split() for ln in out.stderr.splitlines() if ln.startswith("# lgo component ")]
    assert [s[3] for s in comp] == [f"{c}:" for c in range(nr)]
    for c, s in enumerate(comp):
        assert s[4] == "maha" and s[6] == "dof" and s[8] == "logpdf" and int(s[7]) == N
        ms, ls = float(np.sum(g6["refs"][c]["maha"])), float(np.sum(g6["refs"][c]["logpdf"]))
        assert abs(float(s[5]) - ms) < RTOL * max(1.0, ms) * K and abs(float(s[9]) - ls) < RTOL * max(1.0, abs(ls)) * K
    # --quiet: the N lines alone
    q = go(f"--folds={K}", "--quiet")
    assert q.returncode == 0 and q.stdout.splitlines() == lines[len(header):] and "# lgo" not in q.stderr
    # --pca_output (implies --quiet, as in the reference's option parser): the components' own values
    z = go(f"--folds={K}", "--pca_output")
    assert z.returncode == 0, z.stderr[-3000:]
    pv = np.array([ln.split() for ln in z.stdout.splitlines()], float).reshape(N, nr, 2)
    assert close(pv[:, :, 0], g6["mr"]) and close(pv[:, :, 1], g6["vr"], 1e-3)
    # --groups=FILE with the folds' labels: the same lines; with a point never left out: NaN on its line
    gf = tmp_path / "groups.txt"
    gf.write_text("\n".join(str(int(g)) for g in g6["group"]) + "\n")
    f = go(f"--groups={gf}", "--quiet")
    assert f.returncode == 0 and f.stdout.splitlines() == lines[len(header):]
    lab = g6["group"].copy()
    lab[4] = -1
    gf.write_text(" ".join(str(int(g)) for g in lab) + "\n")
    f = go(f"--groups={gf}", "--quiet")
    assert f.returncode == 0, f.stderr[-3000:]
    rows = np.array([ln.split() for ln in f.stdout.splitlines()], float)
    assert rows.shape == (N, 2 * nt) and np.all(np.isnan(rows[4])) and not np.isnan(np.delete(rows, 4, axis=0)).any()


# ------------------------------------------------------------------ without a device
def test_usage_names_the_options_and_they_exclude_each_other(cli, tmp_path):
    def go(*args):
        return subprocess.run([cli] + list(args), capture_output=True, text=True, timeout=60, cwd=tmp_path)

    r = go("no_such_mode", "x")
    assert r.returncode != 0 and r.stderr.startswith("useage:")
    assert "--folds=K" in r.stderr and "--groups=FILE" in r.stderr
    for args in (("--folds=3", "--holdout=h.dat"), ("--groups=g.txt", "--holdout=h.dat"), ("--folds=3", "--groups=g.txt")):
        x = go("validate", G6SNAP, *args)
        assert x.returncode == 1 and x.stderr.startswith("useage:") and x.stdout == ""


def test_symbols_are_exported():
    build.build_all()
    dev, host = ctypes.CDLL(build.HIP_LIB), ctypes.CDLL(build.HOST_LIB)
    for name in ("gpemu_lgo", "gpemu_lgo_dev", "gpemu_lgo_release"):
        assert hasattr(dev, name) and name in abi.SYMBOLS
    for name in ("emulate_lgo", "emulate_lgo_enqueue", "emulate_lgo_collect", "emulate_lgo_multi"):
        assert hasattr(host, name)
    assert abi.PROF_LGO == 13
    assert all(hasattr(abi.Context, n) for n in ("lgo", "lgo_dev", "lgo_release"))
