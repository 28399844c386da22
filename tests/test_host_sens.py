"""Sensitivity analysis through the C host layer (libEmuMI.so: emulate_sensitivity, emulate_main_effects, the enqueue /
collect pair, emulate_sensitivity_multi, emulate_main_effects_multi), the C++ class and the CLI's `sensitivity` mode, against
the device library's own entries (same launches on the same state: same bits) and against tests/sensref.py.

The multi-output test is the one that fails if the observable-space variances are formed by the squared rule of the
posterior variance (sum_c B_tc^2 var_c): its reference is the back-projected function y_t(x) = ybar_t + sum_c B_tc m_c(x)
itself -- by quadrature, with no closed form and no decomposition into components, and by sensref's closed form over all pairs
of components."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

import sensref as R
from madaiemulator_amd import abi, build, synth
from test_gpu_sens import TOL, model_of
from test_host_api import parse_snapshot
from test_host_mean import compile_driver

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TWOD = os.path.join(ROOT, "tests", "golden", "ref_inputs", "uni-2d-param.input_model_file.dat")
G = 5
QUAD_BAR = 1e-11          # quadrature with 48 nodes against the closed form, relative to the scale (test_sensref.py: below 1e-13)


@pytest.fixture(scope="module")
def cli():
    build.build_all()
    return build.CLI_BIN


@pytest.fixture(scope="module")
def sens_driver(tmp_path_factory):
    return compile_driver(tmp_path_factory.mktemp("drv"), "host_sens_driver.c", False)


def rows(text, tag):
    """the numbers of every line that starts with `tag `, one row per line"""
    return np.array([ln[len(tag) + 1:].split() for ln in text.splitlines() if ln.startswith(tag + " ")], float)


def write_box(path, lo, hi):
    path.write_text("".join(f"{a!r} {b!r}\n" for a, b in zip(map(float, lo), map(float, hi))))
    return str(path)


def grid_of(lo, hi, g=G):
    return np.stack([lo + k * (hi - lo) / (g - 1) for k in range(g)], axis=1)


def twod():
    X, Y = synth.read_input_model_file(TWOD)
    return X, Y[:, 0], np.array([0.2, -3.0, np.log(0.5 * np.ptp(X[:, 0])), np.log(0.5 * np.ptp(X[:, 1]))])


def state_of(ctx, order, X, y, th):
    ctx.set_model(1, order, X, y)
    _, rc = ctx.predict_setup(th)
    assert rc == abi.OK
    return model_of(th, *ctx.pred_state())


@pytest.fixture(scope="module")
def two_components(tmp_path_factory):
    """a snapshot with three outputs on two PCA components (d = 2), different lengths per component"""
    X, y = synth.design(60, 2, 5)
    Y = synth.multi_outputs(X, y, 3)
    Z, evals, evecs, ybar = synth.pca_zmatrix(Y, 1.0)
    assert Z.shape[1] == 2
    ths = [np.array([0.0, -4.0, np.log(0.6), np.log(0.7)]), np.array([0.1, -3.5, np.log(0.5), np.log(0.9)])]
    path = tmp_path_factory.mktemp("snap") / "two_components.txt"
    text = synth.snapshot_text(X, Y, evals, evecs, Z, 1, 1, ths)
    path.write_text(text)
    sd = parse_snapshot(text.split())                    # the numbers as the snapshot's decimals give them back
    return dict(path=str(path), X=sd["X"], Z=np.column_stack([m["z"] for m in sd["models"]]), evals=sd["evals"], evecs=sd["evecs"],
                ybar=sd["Y"].mean(axis=0), ths=[m["thetas"] for m in sd["models"]], order=1)


# ------------------------------------------------------------------ emulate_sensitivity == gpemu_sens_cov
@pytest.mark.gpu
@pytest.mark.parametrize("order", [0, 2])
def test_single_output_entries_equal_the_device_entries(sens_driver, gpu_ctx, tmp_path, order):
    X, y, th = twod()
    lo, hi = X.min(axis=0) + 0.1 * np.ptp(X, axis=0), X.max(axis=0)
    box = write_box(tmp_path / "box.txt", lo, hi)
    out = subprocess.run([sens_driver, "single", TWOD, "1", str(order), box, str(G)] + [repr(float(t)) for t in th],
                         capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stderr[-3000:]
    m = state_of(gpu_ctx, order, X, y, th)
    dev = gpu_ctx.sens_cov(lo, hi)
    e0, var = rows(out.stdout, "sens")[0]
    assert e0 == dev["e0"][0] and var == dev["cov_all"]
    assert np.array_equal(rows(out.stdout, "first")[0], dev["cov_first"])
    assert np.array_equal(rows(out.stdout, "total")[0], dev["cov_all"] - dev["cov_rest"])
    pair = rows(out.stdout, "pair")[0]
    assert np.array_equal(pair, [dev["e0"][0], dev["e0"][1], dev["cov_all"]])
    assert np.array_equal(rows(out.stdout, "pfirst")[0], dev["cov_first"]) and np.array_equal(rows(out.stdout, "prest")[0], dev["cov_rest"])
    e0m, main = gpu_ctx.sens_main(lo, hi, grid_of(lo, hi))
    assert np.array_equal(rows(out.stdout, "main"), np.column_stack([np.arange(2), main]))
    assert rows(out.stdout, "e0main")[0, 0] == e0m
    ref, scale = R.covariances(R.NP, X, m, m, lo, hi)
    assert R.scaled_errors(dev, ref, scale) < TOL


# ------------------------------------------------------------------ the multi-output contraction
def reference_outputs(tc, lo, hi, pca, ctxs):
    """per output: e0, var, first, total (closed form over all pairs of components) with their scales, and the same four by
    quadrature of the back-projected function itself"""
    X, nr = tc["X"], 2
    ms = [state_of(ctxs[c], tc["order"], X, tc["Z"][:, c], tc["ths"][c]) for c in range(nr)]
    B = np.eye(nr) if pca else tc["evecs"] * np.sqrt(tc["evals"])
    shift = np.zeros(nr) if pca else tc["ybar"]
    pairs = {(c, k): R.covariances(R.NP, X, ms[c], ms[k], lo, hi) for c in range(nr) for k in range(nr)}
    comp = lambda q: np.column_stack([R.mean_function(X, m, q) for m in ms])
    out = []
    for t in range(B.shape[0]):
        acc = {k: 0.0 for k in ("cov_all", "cov_first", "cov_rest")}
        scl = {k: 0.0 for k in acc}
        for (c, k), (v, s) in pairs.items():
            for key in acc:
                acc[key] = acc[key] + B[t, c] * B[t, k] * v[key]
                scl[key] = scl[key] + abs(B[t, c] * B[t, k]) * s[key]
        e0 = shift[t] + sum(B[t, c] * pairs[(c, c)][0]["e0"][0] for c in range(nr))
        f = lambda q, t=t: shift[t] + comp(q) @ B[t]
        quad = R.quadrature_fn(f, f, lo, hi)
        out.append(dict(e0=e0, var=acc["cov_all"], first=acc["cov_first"], total=acc["cov_all"] - acc["cov_rest"],
                        s_var=scl["cov_all"], s_first=scl["cov_first"], s_total=scl["cov_all"] + scl["cov_rest"],
                        q_e0=quad["e0"][0], q_var=quad["cov_all"], q_first=quad["cov_first"], q_total=quad["cov_all"] - quad["cov_rest"],
                        squared=sum(B[t, c] ** 2 * pairs[(c, c)][0]["cov_all"] for c in range(nr)), ms=ms, B=B, shift=shift))
    return out


@pytest.mark.gpu
@pytest.mark.parametrize("pca", [0, 1])
def test_multi_output_contraction(sens_driver, two_components, gpu_ctx, tmp_path, pca):
    tc = two_components
    X = tc["X"]
    lo, hi = X.min(axis=0), X.max(axis=0) - 0.2
    box = write_box(tmp_path / "box.txt", lo, hi)
    out = subprocess.run([sens_driver, "multi", tc["path"], box, str(G), str(pca)], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stderr[-3000:]
    other = abi.Context(0)
    try:
        ref = reference_outputs(tc, lo, hi, pca, [gpu_ctx, other])
    finally:
        other.close()
    nout = 2 if pca else 3
    head, first, total = rows(out.stdout, "out"), rows(out.stdout, "first"), rows(out.stdout, "total")
    assert head.shape == (nout, 3) and first.shape == (nout, 3) and total.shape == (nout, 3)
    bar = 4 * TOL                                       # four pairs of components, each to TOL of its scale
    grid = grid_of(lo, hi)
    for t, r in enumerate(ref):
        e0, var = head[t, 1:]
        print(f"output {t}: var {var:.6g} (squared rule would give {r['squared']:.6g}), first {first[t, 1:]}, total {total[t, 1:]}")
        # the closed form over all pairs, and quadrature of the back-projected function itself
        assert abs(var - r["var"]) < bar * r["s_var"] and abs(var - r["q_var"]) < QUAD_BAR * r["s_var"]
        assert np.all(np.abs(first[t, 1:] - r["first"]) < bar * r["s_first"]) and np.all(np.abs(first[t, 1:] - r["q_first"]) < QUAD_BAR * r["s_first"])
        assert np.all(np.abs(total[t, 1:] - r["total"]) < bar * r["s_total"]) and np.all(np.abs(total[t, 1:] - r["q_total"]) < QUAD_BAR * r["s_total"])
        assert abs(e0 - r["q_e0"]) < QUAD_BAR * max(1.0, abs(e0))
        if not pca:
            # the squared rule is a different number, by far more than any bar here
            assert abs(r["squared"] - r["var"]) > 1e5 * bar * r["s_var"]
        # main effects: the mean half of the rule on the components' curves
        curves = [R.main_effects(R.NP, X, m, lo, hi, grid)[0]["main"] for m in r["ms"]]
        want = r["shift"][t] + sum(r["B"][t, c] * curves[c] for c in range(2))
        got = rows(out.stdout, f"main {t}")[:, 1:]
        assert np.max(np.abs(got - want)) < 1e-12 * max(1.0, np.abs(want).max())
        assert abs(rows(out.stdout, f"e0main {t}")[0, 0] - e0) < 1e-12 * max(1.0, abs(e0))


@pytest.mark.gpu
@pytest.mark.parametrize("pca", [0, 1])
def test_cpp_methods(sens_driver, two_components, tmp_path, pca):
    """the C++ class returns the numbers of the C entries, the two index vectors divided by the variance"""
    tc = two_components
    lo, hi = tc["X"].min(axis=0), tc["X"].max(axis=0) - 0.2
    box = write_box(tmp_path / "box.txt", lo, hi)
    exe = compile_driver(tmp_path, "emupp_sens_driver.cpp", True)
    cpp = subprocess.run([exe, tc["path"], box, str(G)] + (["pca"] if pca else []), capture_output=True, text=True, timeout=300)
    c = subprocess.run([sens_driver, "multi", tc["path"], box, str(G), str(pca)], capture_output=True, text=True, timeout=300)
    assert cpp.returncode == 0 and c.returncode == 0, cpp.stderr[-3000:] + c.stderr[-3000:]
    head = rows(c.stdout, "out")
    assert np.array_equal(rows(cpp.stdout, "out"), head)
    for tag in ("first", "total"):
        want = rows(c.stdout, tag)
        want[:, 1:] /= head[:, 2:3]
        assert np.array_equal(rows(cpp.stdout, tag), want)
    assert np.array_equal(rows(cpp.stdout, "main"), rows(c.stdout, "main")) and np.array_equal(rows(cpp.stdout, "e0main"), rows(c.stdout, "e0main"))


# ------------------------------------------------------------------ the CLI
@pytest.mark.gpu
def test_cli_sensitivity_on_a_reference_input(cli, gpu_ctx, tmp_path):
    X, y, th = twod()
    d, order = 2, 1
    snap = tmp_path / "snap.txt"
    text = synth.single_output_snapshot(X, y, 1, order, th)
    snap.write_text(text)
    sd = parse_snapshot(text.split())                    # the numbers as the snapshot's decimals give them back
    X, z, lam, th = sd["X"], sd["models"][0]["z"], float(sd["evals"][0]), sd["models"][0]["thetas"]

    def go(*args):
        return subprocess.run([cli, "sensitivity", str(snap)] + list(args), capture_output=True, text=True, timeout=300, cwd=tmp_path)

    # the component the snapshot holds: the centred, scaled training column
    m = state_of(gpu_ctx, order, X, z, th)
    lo, hi = X.min(axis=0), X.max(axis=0)

    def expect(lo, hi):
        ref, scale = R.covariances(R.NP, X, m, m, lo, hi)
        V = lam * ref["cov_all"]
        return V, lam * ref["cov_first"] / V, lam * (ref["cov_all"] - ref["cov_rest"]) / V, y.mean() + np.sqrt(lam) * ref["e0"][0]

    out = go()
    assert out.returncode == 0, out.stderr[-3000:]
    lines = out.stdout.splitlines()
    header = [str(d)] + [f"param_{j} {lo[j]!r} {hi[j]!r}" for j in range(d)] + ["1"]        # the default box: the design's range
    assert [ln.split()[0] for ln in lines[:len(header)]] == [h.split()[0] for h in header]
    assert np.array_equal(np.array([ln.split()[1:] for ln in lines[1:1 + d]], float), np.column_stack([lo, hi]))
    assert len(lines) == len(header) + 1
    vals = np.array(lines[-1].split(), float)
    assert vals.shape == (1 + 2 * d,)                                                            # variance, d first, d total
    V, S, T, E0 = expect(lo, hi)
    assert abs(vals[0] - V) < 1e-9 * V and np.allclose(vals[1:1 + d], S, rtol=0, atol=1e-9) and np.allclose(vals[1 + d:], T, rtol=0, atol=1e-9)
    assert np.all(vals[1:1 + d] <= vals[1 + d:] + 1e-12) and np.all(vals[1 + d:] <= 1 + 1e-12)
    # --quiet: the line alone; --pca_output (implies --quiet): the component's own variance, the same indices
    q = go("--quiet")
    assert q.returncode == 0 and q.stdout.splitlines() == lines[-1:]
    zz = go("--pca_output")
    pv = np.array(zz.stdout.split(), float)
    assert zz.returncode == 0 and pv.shape == vals.shape and abs(pv[0] - V / lam) < 1e-9 * V / lam and np.allclose(pv[1:], vals[1:], rtol=0, atol=1e-9)
    # --box=FILE and --grid=G: d curves of G values, then E0
    lo2, hi2 = lo + 0.25 * (hi - lo), hi - 0.1 * (hi - lo)
    box = write_box(tmp_path / "box.txt", lo2, hi2)
    b = go(f"--box={box}", f"--grid={G}", "--quiet")
    assert b.returncode == 0, b.stderr[-3000:]
    bl = b.stdout.splitlines()
    assert len(bl) == 1 + d + 1
    V2, S2, T2, E02 = expect(lo2, hi2)
    v2 = np.array(bl[0].split(), float)
    assert abs(v2[0] - V2) < 1e-9 * V2 and np.allclose(v2[1:1 + d], S2, rtol=0, atol=1e-9) and np.allclose(v2[1 + d:], T2, rtol=0, atol=1e-9)
    assert abs(v2[0] - V) > 1e-3 * V                                                             # the box matters
    curves = np.array([ln.split() for ln in bl[1:1 + d]], float)
    mref = R.main_effects(R.NP, X, m, lo2, hi2, grid_of(lo2, hi2))[0]["main"]
    assert curves.shape == (d, G) and np.allclose(curves, y.mean() + np.sqrt(lam) * mref, rtol=0, atol=1e-9 * max(1.0, np.abs(y).max()))
    assert abs(float(bl[-1]) - E02) < 1e-9 * max(1.0, abs(E02))
    # a bad box file, a bad grid
    (tmp_path / "bad.txt").write_text("0.1 0.9\n0.5 0.5\n")
    assert go(f"--box={tmp_path / 'bad.txt'}").returncode != 0
    assert go("--grid=0").returncode != 0


def test_cli_refuses_a_matern_snapshot_and_names_the_mode(cli, tmp_path):
    """no device is needed to refuse: the covariance function is read from the snapshot"""
    X, y, _ = twod()
    snap = tmp_path / "matern.txt"
    snap.write_text(synth.single_output_snapshot(X, y, 3, 1, np.array([1.0, 0.01, np.log(0.6)])))
    r = subprocess.run([cli, "sensitivity", str(snap)], capture_output=True, text=True, timeout=60, cwd=tmp_path)
    assert r.returncode != 0 and "power-exponential covariance only" in r.stderr and r.stdout == ""
    u = subprocess.run([cli, "no_such_mode", "x"], capture_output=True, text=True, timeout=60, cwd=tmp_path)
    assert u.returncode != 0 and "sensitivity MODEL_SNAPSHOT_FILE [--box=FILE] [--grid=G]" in u.stderr


def test_symbols_are_exported():
    build.build_all()
    dev, host = ctypes.CDLL(build.HIP_LIB), ctypes.CDLL(build.HOST_LIB)
    for name in ("gpemu_sens_cov", "gpemu_sens_cov_dev", "gpemu_sens_main", "gpemu_sens_release", "gpemu_test_pred_state"):
        assert hasattr(dev, name) and name in abi.SYMBOLS
    for name in ("emulate_sensitivity", "emulate_main_effects", "emulate_sensitivity_enqueue", "emulate_sensitivity_collect",
                 "emulate_sensitivity_multi", "emulate_main_effects_multi"):
        assert hasattr(host, name)
    assert abi.PROF_SENS == 14
    assert all(hasattr(abi.Context, n) for n in ("sens_cov", "sens_cov_dev", "sens_main", "sens_release", "pred_state"))
