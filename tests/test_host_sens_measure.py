"""The input measure of the sensitivity analysis through the C host layer (libEmuMI.so: emulate_sensitivity_measure,
emulate_sensitivity_measure_multi), the C++ class (emulator::SetSensitivityMeasure) and the CLI's `sensitivity --prior=FILE`,
against the device library's own entries (same launches on the same state: same bits) and against tests/sensmeasureref.py.

The multi-output test takes the rule of tests/test_host_sens.py: its reference is the back-projected function
y_t(x) = ybar_t + sum_c B_tc m_c(x) itself, integrated by tensor quadrature against the mixed measure (Gauss-Legendre on the
uniform parameter, Gauss-Hermite on the Gaussian one) -- no closed form, no decomposition into components -- beside the closed
form of the reference over all pairs of components.

QUAD_BAR.  Gauss-Legendre with n nodes integrates the smooth mean function as in test_host_sens.py (1e-11 of the scale).  Gauss-
Hermite converges more slowly: the integrand in the standardised variable z is a sum of exp(-s sd^2 (z - z_i)^2 / 2), entire
but of growth order 2, and n = 64 nodes at s sd^2 <= 0.4 (sd 0.3 at lengths >= 0.5 of a unit range) leave a remainder below
1e-12; the test measures it as the difference between 64 and 48 nodes, asserts that it is below 1e-11, and takes 1e-11."""
import os
import subprocess

import numpy as np
import pytest

import sensref as R
import sensmeasureref as M
from madaiemulator_amd import abi, build, synth
from test_gpu_sens_measure import TOL, TOL_S
from test_host_api import parse_snapshot
from test_host_mean import compile_driver
from test_host_sens import TWOD, rows, state_of, twod, two_components  # noqa: F401  (two_components is a fixture)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
G = 5
QUAD_BAR = 1e-11
KIND = np.array([0, 1], dtype=np.int32)                   # parameter 0 uniform, parameter 1 Gaussian


@pytest.fixture(scope="module")
def cli():
    build.build_all()
    return build.CLI_BIN


@pytest.fixture(scope="module")
def measure_driver(tmp_path_factory):
    return compile_driver(tmp_path_factory.mktemp("drv"), "host_sens_measure_driver.c", False)


def write_measure(path, kind, lo, hi):
    path.write_text("".join(f"{int(k)} {float(a)!r} {float(b)!r}\n" for k, a, b in zip(kind, lo, hi)))
    return str(path)


def write_prior(path, kind, lo, hi):
    path.write_text("".join(f"{'gaussian' if k else 'uniform'} {float(a)!r} {float(b)!r}\n" for k, a, b in zip(kind, lo, hi)))
    return str(path)


def write_grid(path, grid):
    path.write_text("".join(" ".join(repr(float(v)) for v in r) + "\n" for r in grid))
    return str(path)


def span_grid(kind, lo, hi, g=G):
    """g equally spaced values per parameter over the box, or over mean -+ 2 sd of a Gaussian parameter (the CLI's rule)"""
    glo, ghi = np.where(kind == 1, lo - 2.0 * hi, lo), np.where(kind == 1, lo + 2.0 * hi, hi)
    return np.stack([glo + k * (ghi - glo) / (g - 1) for k in range(g)], axis=1)


# ------------------------------------------------------------------ emulate_sensitivity under a measure == the device entries
@pytest.mark.gpu
@pytest.mark.parametrize("order", [0, 2])
def test_single_output_entries_equal_the_device_entries(measure_driver, gpu_ctx, tmp_path, order):
    X, y, th = twod()
    lo, hi = np.array([X[:, 0].min() + 0.1, 0.3]), np.array([X[:, 0].max(), 0.35])     # (0.3, 0.35): mean and sd, and a box too
    grid = span_grid(KIND, lo, hi)
    out = subprocess.run([measure_driver, "single", TWOD, "1", str(order), write_measure(tmp_path / "m.txt", KIND, lo, hi),
                          write_grid(tmp_path / "g.txt", grid), str(G)] + [repr(float(t)) for t in th], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stderr[-3000:]
    m = state_of(gpu_ctx, order, X, y, th)
    uniform = gpu_ctx.sens_cov(lo, hi)
    gpu_ctx.sens_set_measure(KIND)
    dev = gpu_ctx.sens_cov(lo, hi)
    e0, var = rows(out.stdout, "sens")[0]
    assert e0 == dev["e0"][0] and var == dev["cov_all"] and var != uniform["cov_all"]
    assert np.array_equal(rows(out.stdout, "first")[0], dev["cov_first"])
    assert np.array_equal(rows(out.stdout, "total")[0], dev["cov_all"] - dev["cov_rest"])
    e0m, main = gpu_ctx.sens_main(lo, hi, grid)
    assert np.array_equal(rows(out.stdout, "main"), np.column_stack([np.arange(2), main])) and rows(out.stdout, "e0main")[0, 0] == e0m
    post = gpu_ctx.sens_post(lo, hi)
    assert np.array_equal(rows(out.stdout, "post")[0], np.concatenate([[post["s_none"], post["s_all"]], post["s_first"], post["s_rest"]]))
    assert np.array_equal(rows(out.stdout, "vpair")[0], gpu_ctx.sens_pairs(lo, hi))
    # the measure set back to all uniform: the same bounds are a box again
    assert np.array_equal(rows(out.stdout, "usens")[0], [uniform["e0"][0], uniform["cov_all"]])
    ref, scale = M.covariances(KIND, R.NP, X, m, m, lo, hi)
    assert R.scaled_errors(dev, ref, scale) < TOL


# ------------------------------------------------------------------ the multi-output contraction under a mixed measure
def reference_outputs(tc, lo, hi, pca, ctxs):
    """per output: e0, var, first, total (closed form over all pairs of components) with their scales, the same four by
    quadrature of the back-projected function itself, and the quadrature's own remainder"""
    X, nr = tc["X"], 2
    ms = [state_of(ctxs[c], tc["order"], X, tc["Z"][:, c], tc["ths"][c]) for c in range(nr)]
    B = np.eye(nr) if pca else tc["evecs"] * np.sqrt(tc["evals"])
    shift = np.zeros(nr) if pca else tc["ybar"]
    pairs = {(c, k): M.covariances(KIND, R.NP, X, ms[c], ms[k], lo, hi) for c in range(nr) for k in range(nr)}
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
        quad, coarse = M.quadrature_fn(KIND, f, f, lo, hi, n=64), M.quadrature_fn(KIND, f, f, lo, hi, n=48)
        rem = max(float(np.max(np.abs(np.asarray(quad[k]) - np.asarray(coarse[k])) / scl[k])) for k in acc)
        out.append(dict(e0=e0, var=acc["cov_all"], first=acc["cov_first"], total=acc["cov_all"] - acc["cov_rest"],
                        s_var=scl["cov_all"], s_first=scl["cov_first"], s_total=scl["cov_all"] + scl["cov_rest"],
                        q_e0=quad["e0"][0], q_var=quad["cov_all"], q_first=quad["cov_first"], q_total=quad["cov_all"] - quad["cov_rest"],
                        q_rem=rem, squared=sum(B[t, c] ** 2 * pairs[(c, c)][0]["cov_all"] for c in range(nr)), ms=ms, B=B, shift=shift))
    return out


@pytest.mark.gpu
@pytest.mark.parametrize("pca", [0, 1])
def test_multi_output_contraction_under_a_mixed_measure(measure_driver, two_components, gpu_ctx, tmp_path, pca):
    tc = two_components
    X = tc["X"]
    w = np.ptp(X, axis=0)
    lo, hi = np.array([X[:, 0].min(), X[:, 1].min() + 0.45 * w[1]]), np.array([X[:, 0].max() - 0.2, 0.3 * w[1]])
    grid = span_grid(KIND, lo, hi)
    out = subprocess.run([measure_driver, "multi", tc["path"], write_measure(tmp_path / "m.txt", KIND, lo, hi),
                          write_grid(tmp_path / "g.txt", grid), str(G), str(pca)], capture_output=True, text=True, timeout=300)
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
    for t, r in enumerate(ref):
        e0, var = head[t, 1:]
        print(f"output {t}: var {var:.6g} (squared rule would give {r['squared']:.6g}), first {first[t, 1:]}, total {total[t, 1:]}, "
              f"quadrature 64 against 48 nodes {r['q_rem']:.2e}")
        assert r["q_rem"] < QUAD_BAR
        assert abs(var - r["var"]) < bar * r["s_var"] and abs(var - r["q_var"]) < QUAD_BAR * r["s_var"]
        assert np.all(np.abs(first[t, 1:] - r["first"]) < bar * r["s_first"]) and np.all(np.abs(first[t, 1:] - r["q_first"]) < QUAD_BAR * r["s_first"])
        assert np.all(np.abs(total[t, 1:] - r["total"]) < bar * r["s_total"]) and np.all(np.abs(total[t, 1:] - r["q_total"]) < QUAD_BAR * r["s_total"])
        assert abs(e0 - r["q_e0"]) < QUAD_BAR * max(1.0, abs(e0))
        if not pca:
            assert abs(r["squared"] - r["var"]) > 1e5 * bar * r["s_var"]
        curves = [M.main_effects(KIND, R.NP, X, m, lo, hi, grid)[0]["main"] for m in r["ms"]]
        want = r["shift"][t] + sum(r["B"][t, c] * curves[c] for c in range(2))
        got = rows(out.stdout, f"main {t}")[:, 1:]
        assert np.max(np.abs(got - want)) < 1e-12 * max(1.0, np.abs(want).max())
        assert abs(rows(out.stdout, f"e0main {t}")[0, 0] - e0) < 1e-12 * max(1.0, abs(e0))
        # the uncertainty terms ran under the same measure: Var*[E0] >= 0, IMSE >= Var*[E0], E*[V] = V + IMSE - Var*[E0]
        ve0, imse, evar = rows(out.stdout, f"unc {t}")[0]
        assert ve0 >= 0 and imse >= ve0 and abs(evar - (var + imse - ve0)) <= 8 * TOL_S * (abs(var) + imse + ve0) + bar * r["s_var"]


@pytest.mark.gpu
@pytest.mark.parametrize("pca", [0, 1])
def test_cpp_method(measure_driver, two_components, tmp_path, pca):
    """emulator::SetSensitivityMeasure: the C++ class returns the numbers of the C entries under the same measure"""
    tc = two_components
    X = tc["X"]
    lo, hi = np.array([X[:, 0].min(), 0.45]), np.array([X[:, 0].max() - 0.2, 0.3])
    mf = write_measure(tmp_path / "m.txt", KIND, lo, hi)
    gf = write_grid(tmp_path / "g.txt", span_grid(KIND, lo, hi))
    exe = compile_driver(tmp_path, "emupp_sens_measure_driver.cpp", True)
    cpp = subprocess.run([exe, tc["path"], mf] + (["pca"] if pca else []), capture_output=True, text=True, timeout=300)
    c = subprocess.run([measure_driver, "multi", tc["path"], mf, gf, str(G), str(pca)], capture_output=True, text=True, timeout=300)
    assert cpp.returncode == 0 and c.returncode == 0, cpp.stderr[-3000:] + c.stderr[-3000:]
    head = rows(c.stdout, "out")
    assert np.array_equal(rows(cpp.stdout, "out"), head)
    for tag in ("first", "total"):
        want = rows(c.stdout, tag)
        want[:, 1:] /= head[:, 2:3]
        assert np.array_equal(rows(cpp.stdout, tag), want)


# ------------------------------------------------------------------ the CLI
@pytest.mark.gpu
def test_cli_prior_file(cli, gpu_ctx, tmp_path):
    X, y, th = twod()
    d, order = 2, 1
    snap = tmp_path / "snap.txt"
    text = synth.single_output_snapshot(X, y, 1, order, th)
    snap.write_text(text)
    sd = parse_snapshot(text.split())                    # the numbers as the snapshot's decimals give them back
    X, z, lam, th = sd["X"], sd["models"][0]["z"], float(sd["evals"][0]), sd["models"][0]["thetas"]

    def go(*args):
        return subprocess.run([cli, "sensitivity", str(snap)] + list(args), capture_output=True, text=True, timeout=300, cwd=tmp_path)

    m = state_of(gpu_ctx, order, X, z, th)
    lo, hi = np.array([0.1, 0.4]), np.array([0.9, 0.25])
    prior = write_prior(tmp_path / "prior.txt", KIND, lo, hi)
    out = go(f"--prior={prior}", f"--grid={G}")
    assert out.returncode == 0, out.stderr[-3000:]
    lines = out.stdout.splitlines()
    # the header: d, one line per parameter with its kind and its two numbers, the number of outputs
    assert lines[0] == "2" and lines[3] == "1"
    assert lines[1].split()[:2] == ["param_0", "uniform"] and lines[2].split()[:2] == ["param_1", "gaussian"]
    assert np.array_equal(np.array([ln.split()[2:] for ln in lines[1:3]], float), np.column_stack([lo, hi]))
    assert len(lines) == 4 + 1 + d + 1
    ref, _ = M.covariances(KIND, R.NP, X, m, m, lo, hi)
    V = lam * ref["cov_all"]
    vals = np.array(lines[4].split(), float)
    assert abs(vals[0] - V) < 1e-9 * V
    assert np.allclose(vals[1:1 + d], ref["cov_first"] / ref["cov_all"], rtol=0, atol=1e-9)
    assert np.allclose(vals[1 + d:], (ref["cov_all"] - ref["cov_rest"]) / ref["cov_all"], rtol=0, atol=1e-9)
    # the curves: the uniform parameter over its box, the Gaussian one over mean -+ 2 sd
    grid = span_grid(KIND, lo, hi)
    assert grid[1, 0] == 0.4 - 0.5 and grid[1, -1] == 0.4 + 0.5
    curves = np.array([ln.split() for ln in lines[5:5 + d]], float)
    mref = M.main_effects(KIND, R.NP, X, m, lo, hi, grid)[0]["main"]
    assert curves.shape == (d, G) and np.allclose(curves, y.mean() + np.sqrt(lam) * mref, rtol=0, atol=1e-9 * max(1.0, np.abs(y).max()))
    assert abs(float(lines[-1]) - (y.mean() + np.sqrt(lam) * ref["e0"][0])) < 1e-9 * max(1.0, abs(y.mean()))
    # --quiet: no header
    q = go(f"--prior={prior}", f"--grid={G}", "--quiet")
    assert q.returncode == 0 and q.stdout.splitlines() == lines[4:]
    # all-uniform priors: the numbers of the same box given with --box, under the header with the kinds
    box = tmp_path / "box.txt"
    box.write_text("0.1 0.9\n0.2 0.8\n")
    (tmp_path / "uprior.txt").write_text("uniform 0.1 0.9\nuniform 0.2 0.8\n")
    b, u = go(f"--box={box}", f"--grid={G}", "--pairs", f"--surface=0,1"), go(f"--prior={tmp_path / 'uprior.txt'}", f"--grid={G}", "--pairs", "--surface=0,1")
    assert b.returncode == 0 and u.returncode == 0
    assert u.stdout.splitlines()[4:] == b.stdout.splitlines()[4:] and u.stdout.splitlines()[1] == "param_0 uniform 0.10000000000000001 0.90000000000000002"
    # bad files: status 1 and a message that names the format; --box and --prior together
    for bad in ("uniform 0.1 0.9\n", "uniform 0.1 0.9\ngaussian 0.4 0\n", "uniform 0.1 0.9\ngaussian 0.4 -1\n", "uniform 0.9 0.1\ngaussian 0.4 0.2\n",
                "uniform 0.1 0.9\nnormal 0.4 0.2\n", "uniform 0.1 0.9\ngaussian nan 0.2\n", "0.1 0.9\n0.2 0.8\n"):
        (tmp_path / "bad.txt").write_text(bad)
        r = go(f"--prior={tmp_path / 'bad.txt'}")
        assert r.returncode == 1 and "gaussian MEAN SD" in r.stderr and r.stdout == "", bad
    assert go(f"--prior={tmp_path / 'missing.txt'}").returncode != 0
    both = go(f"--prior={prior}", f"--box={box}")
    assert both.returncode != 0 and "exclude each other" in both.stderr


@pytest.mark.gpu
def test_cli_output_without_the_flag_is_what_it_was(cli, tmp_path):
    """every byte of a run without --prior, against the text the same command printed before the flag existed
    (tests/golden/sens_cli_without_prior.txt, recorded from the build before the measure switch on this snapshot and box).  The
    numbers are the device's: every sum of these entries has one order and an all-uniform context takes the kernels it took
    before, so the same bits come back and the whole text is compared, header, indices, curves, bands, pairs and surface."""
    X, y, th = twod()
    snap = tmp_path / "snap.txt"
    snap.write_text(synth.single_output_snapshot(X, y, 1, 1, th))
    box = tmp_path / "box.txt"
    box.write_text("0.1 0.9\n0.2 0.8\n")
    out = subprocess.run([cli, "sensitivity", str(snap), f"--box={box}", "--grid=4", "--uncertainty", "--pairs", "--surface=0,1"],
                         capture_output=True, text=True, timeout=300, cwd=tmp_path)
    assert out.returncode == 0, out.stderr[-3000:]
    want = open(os.path.join(ROOT, "tests", "golden", "sens_cli_without_prior.txt")).read()
    assert out.stdout == want


def test_symbols_are_exported():
    import ctypes
    build.build_all()
    dev, host = ctypes.CDLL(build.HIP_LIB), ctypes.CDLL(build.HOST_LIB)
    for name in ("gpemu_sens_set_measure", "gpemu_sens_get_measure"):
        assert hasattr(dev, name) and name in abi.SYMBOLS
    for name in ("emulate_sensitivity_measure", "emulate_sensitivity_measure_multi"):
        assert hasattr(host, name)
    assert (abi.MEASURE_UNIFORM, abi.MEASURE_GAUSS) == (0, 1)
    assert all(hasattr(abi.Context, n) for n in ("sens_set_measure", "sens_get_measure"))
