"""The expected IMSE reduction of candidate runs through the C host layer (libEmuMI.so: emulate_design_gain,
emulate_design_gain_multi), the C++ class (emulator::QueryEmulatorDesignGain) and the CLI's `design` mode, against the device
library's own entry (same launches on the same state: same bits), against the composition rule computed in numpy from the
per-component numbers, and against quadrature of the posterior covariance itself.

One run observes every PCA component, and the components are independent a posteriori: the IMSE of output t is
sum_c B_tc^2 s_all^c, so its drop is gain(y_t) = sum_c B_tc^2 gain_c -- the squared rule of gpemu_host_backproject, no cross
terms.  The quadrature test is the one that fails if the gains are contracted like means (sum_c B_tc gain_c).

The quadrature bar.  c*_c(x, x*) is formed in fp64 from the device's P (entries of size 1 / nugget = 55) and is some 1e-3 where
it matters, so each value is good to about 1e-11 of itself and the 24 x 24 Gauss-Legendre sum of its squares to a few 1e-11;
QUAD_RTOL = 1e-9 leaves two digits for the quadrature's own convergence on these smooth integrands.

The other modes of the CLI are covered by the tests they came with, which run unchanged: their output is byte for byte what it
was (the measure-file parsing they share with `design` moved into one function, its messages and exit paths as they were)."""
import subprocess

import numpy as np
import pytest

import sensref as R
import senspostref as SP
from madaiemulator_amd import abi, build, synth
from test_host_mean import compile_driver
from test_host_sens import cli, rows, two_components, twod, write_box          # noqa: F401  (fixtures)

EPS = 2.0 ** -52
QUAD_RTOL = 1e-9


@pytest.fixture(scope="module")
def design_driver(tmp_path_factory):
    return compile_driver(tmp_path_factory.mktemp("drv"), "host_design_driver.c", False)


def setting(tc, tmp_path):
    X = tc["X"]
    lo, hi = X.min(axis=0), X.max(axis=0) - 0.2
    r = np.random.default_rng(31)
    Xq = (lo - 0.2) + (hi - lo + 0.4) * r.random((7, 2))                 # inside and outside the box
    Xq = np.vstack([Xq, Xq[:1]])                                         # a repeated candidate: a tie
    pts = tmp_path / "points.txt"
    pts.write_text("".join(" ".join(repr(float(v)) for v in x) + "\n" for x in Xq))
    return lo, hi, Xq, write_box(tmp_path / "box.txt", lo, hi), str(pts)


def loadings(tc, pca):
    return np.eye(2) if pca else tc["evecs"] * np.sqrt(tc["evals"])


def component_state(ctx, tc, c):
    ctx.set_model(1, tc["order"], tc["X"], tc["Z"][:, c])
    _, rc = ctx.predict_setup(tc["ths"][c])
    assert rc == abi.OK


@pytest.mark.gpu
@pytest.mark.parametrize("pca", [0, 1])
def test_composition_rule(design_driver, two_components, gpu_ctx, tmp_path, pca):
    tc = two_components
    lo, hi, Xq, box, pts = setting(tc, tmp_path)
    out = subprocess.run([design_driver, tc["path"], box, pts, str(pca)], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stderr[-3000:]
    comp, cnum, cvar = (rows(out.stdout, t)[:, 1:] for t in ("comp", "cnum", "cvar"))
    # the components' entries return the bits of the device entry on the same state
    quad = []
    for c in range(2):
        component_state(gpu_ctx, tc, c)
        dev = gpu_ctx.design_gain(lo, hi, Xq)
        assert np.array_equal(comp[c], dev["gain"]) and np.array_equal(cnum[c], dev["num"]) and np.array_equal(cvar[c], dev["var"])
        assert np.array_equal(comp[c][0], comp[c][-1])                                   # the repeated candidate
        # ... and the gain is the average of c*(x, x*)^2 over the box, by quadrature of the posterior covariance itself
        gpu_ctx.sens_post(lo, hi)
        P, G, Q = gpu_ctx.sens_post_state()
        th = tc["ths"][c]
        m = dict(A=float(np.exp(th[0])), s=np.exp(-2.0 * th[2:]))
        nodes = [SP.gauss_nodes(lo[l], hi[l]) for l in range(2)]
        mesh = np.stack([g.ravel() for g in np.meshgrid(nodes[0][0], nodes[1][0], indexing="ij")], axis=1)
        wt = np.multiply.outer(nodes[0][1], nodes[1][1]).ravel()
        cs = SP.cstar(tc["X"], m, P, G, Q, mesh, Xq)
        quad.append((wt @ (cs * cs)) / cvar[c])
        assert np.allclose(comp[c], quad[c], rtol=QUAD_RTOL, atol=0)
    # outputs: the squared rule, no cross terms; the total is the sum over the outputs
    B = loadings(tc, pca)
    gain, total = rows(out.stdout, "gain")[:, 1:], rows(out.stdout, "total")[:, 1]
    want = comp.T @ (B ** 2).T                                                            # npoints x nout
    assert gain.shape == want.shape == (len(Xq), B.shape[0])
    assert np.all(np.abs(gain - want) <= 8 * EPS * want)
    assert np.all(np.abs(total - gain.sum(axis=1)) <= 8 * EPS * total)
    assert np.allclose(gain, np.array(quad).T @ (B ** 2).T, rtol=QUAD_RTOL, atol=0)
    if not pca:
        assert np.all(np.abs(gain - comp.T @ B.T) > 1e6 * EPS * want)                     # the mean rule is a different number


@pytest.mark.gpu
@pytest.mark.parametrize("pca", [0, 1])
def test_cpp_method(design_driver, two_components, tmp_path, pca):
    tc = two_components
    lo, hi, Xq, box, pts = setting(tc, tmp_path)
    exe = compile_driver(tmp_path, "emupp_design_driver.cpp", True)
    cpp = subprocess.run([exe, tc["path"], box, pts] + (["pca"] if pca else []), capture_output=True, text=True, timeout=300)
    c = subprocess.run([design_driver, tc["path"], box, pts, str(pca)], capture_output=True, text=True, timeout=300)
    assert cpp.returncode == 0 and c.returncode == 0, cpp.stderr[-3000:] + c.stderr[-3000:]
    for tag in ("gain", "total"):
        assert np.array_equal(rows(cpp.stdout, tag), rows(c.stdout, tag)) and len(rows(c.stdout, tag)) == len(Xq)


@pytest.mark.gpu
def test_cli_design(cli, design_driver, two_components, gpu_ctx, tmp_path):
    tc = two_components
    lo, hi, Xq, box, pts = setting(tc, tmp_path)
    text = open(pts).read()

    def go(*args):
        return subprocess.run([cli, "design", tc["path"], f"--box={box}"] + list(args), input=text, capture_output=True, text=True, timeout=300,
                              cwd=tmp_path)

    drv = subprocess.run([design_driver, tc["path"], box, pts, "0"], capture_output=True, text=True, timeout=300)
    assert drv.returncode == 0, drv.stderr[-3000:]
    total = rows(drv.stdout, "total")[:, 1]
    s_all = []
    for c in range(2):
        component_state(gpu_ctx, tc, c)
        s_all.append(gpu_ctx.sens_post(lo, hi)["s_all"])
    imse = float(((loadings(tc, 0) ** 2) @ np.array(s_all)).sum())
    out = go()
    assert out.returncode == 0, out.stderr[-3000:]
    lines = out.stdout.splitlines()
    assert lines[0] == "# index param_0 param_1 expected_imse_reduction imse" and len(lines) == 1 + len(Xq)
    vals = np.array([ln.split() for ln in lines[1:]], float)
    assert np.array_equal(vals[:, 0], np.arange(len(Xq))) and np.array_equal(vals[:, 1:3], Xq)
    assert np.array_equal(vals[:, 3], total)
    assert np.all(vals[:, 4] == vals[0, 4]) and abs(vals[0, 4] - imse) <= 1e-12 * imse
    assert np.all(vals[:, 3] >= 0) and np.all(vals[:, 3] <= vals[:, 4])
    # --quiet: no header; --best=K: the K largest, largest first, the tie (candidates 0 and 7) in input order
    q = go("--quiet")
    assert q.returncode == 0 and q.stdout.splitlines() == lines[1:]
    order = sorted(range(len(Xq)), key=lambda i: (-total[i], i))
    for K in (3, len(Xq), 100):
        b = go(f"--best={K}", "--quiet")
        assert b.returncode == 0, b.stderr[-3000:]
        assert b.stdout.splitlines() == [lines[1 + i] for i in order[:K]]
    assert order.index(0) + 1 == order.index(7)
    assert go("--best=0").returncode != 0
    # a box file that cannot be used, points that are not whole
    (tmp_path / "bad.txt").write_text("0.1 0.9\n0.5 0.5\n")
    assert subprocess.run([cli, "design", tc["path"], f"--box={tmp_path / 'bad.txt'}"], input=text, capture_output=True, text=True, timeout=300,
                          cwd=tmp_path).returncode != 0
    odd = subprocess.run([cli, "design", tc["path"]], input="0.1 0.2 0.3\n", capture_output=True, text=True, timeout=300, cwd=tmp_path)
    assert odd.returncode != 0 and "whole points" in odd.stderr and odd.stdout == ""


def test_cli_refuses_a_matern_snapshot_and_usage_names_the_mode(cli, tmp_path):
    """no device is needed to refuse: the covariance function is read from the snapshot"""
    X, y, _ = twod()
    snap = tmp_path / "matern.txt"
    snap.write_text(synth.single_output_snapshot(X, y, 3, 1, np.array([1.0, 0.01, np.log(0.6)])))
    r = subprocess.run([cli, "design", str(snap)], input="0.5 0.5\n", capture_output=True, text=True, timeout=60, cwd=tmp_path)
    assert r.returncode != 0 and "power-exponential covariance only" in r.stderr and r.stdout == ""
    u = subprocess.run([cli, "no_such_mode", "x"], capture_output=True, text=True, timeout=60, cwd=tmp_path)
    assert u.returncode != 0 and "design MODEL_SNAPSHOT_FILE [--box=FILE | --prior=FILE] [--best=K]" in u.stderr


def test_symbols_are_exported():
    import ctypes
    build.build_all()
    dev, host = ctypes.CDLL(build.HIP_LIB), ctypes.CDLL(build.HOST_LIB)
    for name in ("gpemu_design_gain", "gpemu_design_gain_dev", "gpemu_test_design_state"):
        assert hasattr(dev, name), name
    for name in ("emulate_design_gain", "emulate_design_gain_multi"):
        assert hasattr(host, name), name
