"""Second-order sensitivity analysis through the C host layer (libEmuMI.so: emulate_sensitivity_pairs, its enqueue / collect
pair, emulate_sensitivity_pairs_post, emulate_sensitivity_pairs_uncertainty, emulate_interaction_surface, their _multi forms),
the C++ class and the CLI's `sensitivity --pairs / --surface`, against the device library's own entries (same launches on
the same state: same bits), against tests/senspairref.py and against the composition rules computed in numpy.

The multi-output test fails if the two halves swap their rules: in observable space V_jk(y_t) = sum_{c,c'} B_tc B_tc'
cov_pair(c, c') keeps the cross terms between components, S_jk(y_t) = sum_c B_tc^2 S_jk^c has none."""
import ctypes
import subprocess

import numpy as np
import pytest

import sensref as R
import senspairref as SPR
from madaiemulator_amd import abi, build, synth
from test_gpu_sens_pairs import TOL
from test_host_api import parse_snapshot
from test_host_mean import compile_driver
from test_host_sens import G, cli, rows, state_of, two_components, twod, write_box          # noqa: F401  (fixtures)

EPS = 2.0 ** -52


@pytest.fixture(scope="module")
def pairs_driver(tmp_path_factory):
    return compile_driver(tmp_path_factory.mktemp("drv"), "host_sens_pairs_driver.c", False)


def box_of(tc):
    return tc["X"].min(axis=0), tc["X"].max(axis=0) - 0.2


def run(exe, *args):
    out = subprocess.run([exe] + [str(a) for a in args], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stderr[-3000:]
    return out.stdout


@pytest.mark.gpu
@pytest.mark.parametrize("pca", [0, 1])
def test_entries_and_composition_rules(pairs_driver, two_components, gpu_ctx, tmp_path, pca):
    tc = two_components
    X, d, nr, npairs = tc["X"], 2, 2, 1
    lo, hi = box_of(tc)
    txt = run(pairs_driver, tc["path"], write_box(tmp_path / "box.txt", lo, hi), G, pca, 0, 1)
    gj, gk = (lo[l] + np.arange(G) * (hi[l] - lo[l]) / (G - 1) for l in (0, 1))
    xj, xk = np.repeat(gj, G), np.tile(gk, G)
    other = abi.Context(0)
    try:
        ctxs = [gpu_ctx, other]
        ms = [state_of(ctxs[c], tc["order"], X, tc["Z"][:, c], tc["ths"][c]) for c in range(nr)]
        cpair, cspair, cjoint, cfx, ce0, cs = [], [], [], [], [], []
        for c in range(nr):
            # the components' entries return the bits of the device entries on the same state
            dev, cov = ctxs[c].sens_pairs(lo, hi), ctxs[c].sens_cov(lo, hi)
            cpair.append(rows(txt, f"cpair {c}")[0])
            assert np.array_equal(cpair[c], dev)
            assert np.array_equal(rows(txt, f"cinter {c}")[0], [dev[0] - cov["cov_first"][0] - cov["cov_first"][1]])
            cspair.append(rows(txt, f"cspair {c}")[0])
            assert np.array_equal(cspair[c], ctxs[c].sens_pairs_post(lo, hi))
            e0, joint, inter = ctxs[c].sens_joint(lo, hi, 0, 1, xj, xk)
            cjoint.append(rows(txt, f"cjoint {c}")[:, 1:])
            cfx.append(rows(txt, f"cfx {c}")[:, 1:])
            ce0.append(rows(txt, f"ce0 {c}")[0, 0])
            assert np.array_equal(cjoint[c].ravel(), joint) and np.array_equal(cfx[c].ravel(), inter) and ce0[c] == e0
            # the posterior expectations through emulate_sensitivity_pairs_uncertainty
            s = ctxs[c].sens_post(lo, hi)
            cs.append(s)
            tol = 8 * EPS * (abs(dev[0]) + s["s_all"])
            assert abs(rows(txt, f"cevpair {c}")[0, 0] - (dev[0] + cspair[c][0] - s["s_none"])) <= tol
            want = dev[0] - cov["cov_first"].sum() + cspair[c][0] - s["s_first"].sum() + s["s_none"]
            assert abs(rows(txt, f"ceinter {c}")[0, 0] - want) <= tol
            # the two halves of a pair of components are the device's cross entry
            for c2 in range(c, nr):
                assert np.array_equal(rows(txt, f"xpair {c} {c2}")[0], ctxs[c].sens_pairs(lo, hi, ctxs[c2]))
        B = np.eye(nr) if pca else tc["evecs"] * np.sqrt(tc["evals"])
        shift = np.zeros(nr) if pca else tc["ybar"]
        nout = B.shape[0]
        ref = {(c, k): SPR.pair_covariances(R.NP, X, ms[c], ms[k], lo, hi) for c in range(nr) for k in range(nr)}
        cross = {(c, k): ctxs[c].sens_pairs(lo, hi, ctxs[k]) for c in range(nr) for k in range(nr)}
        first = {(c, k): ctxs[c].sens_cov(lo, hi, ctxs[k])["cov_first"] for c in range(nr) for k in range(nr)}
        vpair, inter, evpair, einter = (rows(txt, t)[:, 1:] for t in ("vpair", "inter", "evpair", "einter"))
        assert vpair.shape == inter.shape == evpair.shape == einter.shape == (nout, npairs)
        for t in range(nout):
            # the plug-in half: the full quadratic form, against the reference (four pairs of components, each to TOL of its scale)
            # and against the device's own cross terms to rounding
            want = sum(B[t, c] * B[t, k] * ref[(c, k)][0]["cov_pair"] for c in range(nr) for k in range(nr))
            scale = sum(abs(B[t, c] * B[t, k]) * ref[(c, k)][1]["cov_pair"] for c in range(nr) for k in range(nr))
            # (the host layer calls the device for c <= c' and counts c < c' twice; the device's (c', c) differs from (c, c') in rounding)
            devq = sum((1 + (c < k)) * B[t, c] * B[t, k] * cross[(c, k)] for c in range(nr) for k in range(c, nr))
            devf = sum((1 + (c < k)) * B[t, c] * B[t, k] * first[(c, k)] for c in range(nr) for k in range(c, nr))
            assert np.all(np.abs(vpair[t] - want) < 4 * TOL * scale)
            assert np.all(np.abs(vpair[t] - devq) <= 8 * EPS * scale)
            assert np.all(np.abs(inter[t] - (devq - devf.sum())) <= 16 * EPS * scale)
            squared = sum(B[t, c] ** 2 * cpair[c] for c in range(nr))
            if not pca:
                assert np.all(np.abs(squared - vpair[t]) > 1e5 * 4 * TOL * scale)          # the squared rule is another number
            # the S half: the squared rule
            sp = sum(B[t, c] ** 2 * cspair[c] for c in range(nr))
            sn = sum(B[t, c] ** 2 * cs[c]["s_none"] for c in range(nr))
            sf = sum(B[t, c] ** 2 * cs[c]["s_first"] for c in range(nr))
            tol = 16 * EPS * (scale + sum(B[t, c] ** 2 * cs[c]["s_all"] for c in range(nr)))
            assert np.all(np.abs(evpair[t] - (vpair[t] + sp - sn)) <= tol)
            assert np.all(np.abs(einter[t] - (inter[t] + sp - sf.sum() + sn)) <= tol)
            # the surface: linear in the components, the training mean on the surface and E0 alone
            jw = shift[t] + sum(B[t, c] * cjoint[c] for c in range(nr))
            fw = sum(B[t, c] * cfx[c] for c in range(nr))
            big = max(1.0, np.abs(jw).max())
            assert np.max(np.abs(rows(txt, f"joint {t}")[:, 1:] - jw)) <= 1e-12 * big
            assert np.max(np.abs(rows(txt, f"fx {t}")[:, 1:] - fw)) <= 1e-12 * max(np.abs(B[t]) @ [np.abs(f).max() for f in cfx], 1e-300)
            assert abs(rows(txt, f"e0 {t}")[0, 0] - (shift[t] + sum(B[t, c] * ce0[c] for c in range(nr)))) <= 1e-12 * big
    finally:
        other.close()


@pytest.mark.gpu
@pytest.mark.parametrize("pca", [0, 1])
def test_cpp_methods(pairs_driver, two_components, tmp_path, pca):
    """the C++ class returns the numbers of the C entries, the interaction variances divided by the variance"""
    tc = two_components
    lo, hi = box_of(tc)
    box = write_box(tmp_path / "box.txt", lo, hi)
    exe = compile_driver(tmp_path, "emupp_sens_pairs_driver.cpp", True)
    cpp = run(exe, tc["path"], box, G, 0, 1, *(["pca"] if pca else []))
    c = run(pairs_driver, tc["path"], box, G, pca, 0, 1)
    for tag in ("vpair", "evpair", "einter", "e0", "joint", "fx"):
        got = rows(cpp, tag)
        assert got.size and np.array_equal(got, rows(c, tag)), tag
    # second-order indices: inter / V, V = V_01 for two parameters
    assert np.array_equal(rows(cpp, "second")[:, 1:], rows(c, "inter")[:, 1:] / _variances(tc, lo, hi, pca, tmp_path)[:, None])


def _variances(tc, lo, hi, pca, tmp_path):
    drv = compile_driver(tmp_path, "host_sens_driver.c", False)
    out = run(drv, "multi", tc["path"], write_box(tmp_path / "box2.txt", lo, hi), G, pca)
    return rows(out, "out")[:, 2]


@pytest.mark.gpu
def test_cli_pairs_and_surface_on_a_reference_input(cli, gpu_ctx, tmp_path):
    """uni-2d-param: the appended lines against the reference; everything before them is the output without the new flags"""
    X, y, th = twod()
    d, order = 2, 1
    snap = tmp_path / "snap.txt"
    text = synth.single_output_snapshot(X, y, 1, order, th)
    snap.write_text(text)
    sd = parse_snapshot(text.split())
    X, z, lam, th = sd["X"], sd["models"][0]["z"], float(sd["evals"][0]), sd["models"][0]["thetas"]
    m = state_of(gpu_ctx, order, X, z, th)
    lo, hi = X.min(axis=0), X.max(axis=0)

    def go(*args):
        r = subprocess.run([cli, "sensitivity", str(snap), "--quiet"] + list(args), capture_output=True, text=True, timeout=300, cwd=tmp_path)
        assert r.returncode == 0, r.stderr[-3000:]
        return r.stdout, r.stderr

    cov, _ = R.covariances(R.NP, X, m, m, lo, hi)
    pair, _ = SPR.pair_covariances(R.NP, X, m, m, lo, hi)
    second = (pair["cov_pair"][0] - cov["cov_first"].sum()) / cov["cov_all"]
    for base in ([], [f"--grid={G}", "--uncertainty"]):
        plain, plain_err = go(*base)
        with_pairs, err = go(*base, "--pairs")
        assert with_pairs.startswith(plain) and err == plain_err
        extra = with_pairs[len(plain):].splitlines()
        assert len(extra) == (2 if "--uncertainty" in base else 1)
        assert all(len(ln.split()) == 1 for ln in extra)
        assert abs(float(extra[0]) - second) < 1e-9
        if "--uncertainty" in base:
            v = gpu_ctx.sens_pairs(lo, hi)[0] - gpu_ctx.sens_cov(lo, hi)["cov_first"].sum()
            s, sp = gpu_ctx.sens_post(lo, hi), gpu_ctx.sens_pairs_post(lo, hi)[0]
            cv = gpu_ctx.sens_cov(lo, hi)["cov_all"]
            want = (v + sp - s["s_first"].sum() + s["s_none"]) / (cv + s["s_all"] - s["s_none"])
            assert abs(float(extra[1]) - want) < 1e-9
    # two parameters: nothing but the two main effects and their interaction
    assert abs(second - (1.0 - cov["cov_first"].sum() / cov["cov_all"])) < 1e-9
    # --surface=j,k with --grid=G: G lines of G interaction effects, in the output's units
    plain, _ = go(f"--grid={G}")
    surf, _ = go(f"--grid={G}", "--surface=0,1")
    assert surf.startswith(plain)
    fx = np.array([ln.split() for ln in surf[len(plain):].splitlines()], float)
    gj, gk = (lo[l] + np.arange(G) * (hi[l] - lo[l]) / (G - 1) for l in (0, 1))
    ref, scale = SPR.joint_surface(R.NP, X, m, lo, hi, 0, 1, np.repeat(gj, G), np.tile(gk, G))
    assert fx.shape == (G, G) and np.allclose(fx.ravel(), np.sqrt(lam) * ref["inter"], rtol=0, atol=1e-9 * np.sqrt(lam) * scale["inter"].max())
    both, _ = go(f"--grid={G}", "--pairs", "--surface=0,1")
    assert both.startswith(plain) and len(both[len(plain):].splitlines()) == 1 + G
    # a surface needs a grid and two different parameters
    for bad in (["--surface=0,1"], [f"--grid={G}", "--surface=0,0"], [f"--grid={G}", "--surface=0,2"], [f"--grid={G}", "--surface=1"]):
        r = subprocess.run([cli, "sensitivity", str(snap)] + bad, capture_output=True, text=True, timeout=300, cwd=tmp_path)
        assert r.returncode != 0 and "--surface=j,k" in r.stderr


def test_usage_names_the_new_flags(cli, tmp_path):
    u = subprocess.run([cli, "no_such_mode", "x"], capture_output=True, text=True, timeout=60, cwd=tmp_path)
    assert u.returncode != 0 and "[--pairs] [--surface=j,k]" in u.stderr


def test_symbols_are_exported():
    build.build_all()
    dev, host = ctypes.CDLL(build.HIP_LIB), ctypes.CDLL(build.HOST_LIB)
    for name in ("gpemu_sens_pairs", "gpemu_sens_pairs_dev", "gpemu_sens_pairs_post", "gpemu_sens_pairs_post_dev", "gpemu_sens_joint"):
        assert hasattr(dev, name) and name in abi.SYMBOLS
    for name in ("emulate_sensitivity_pairs", "emulate_sensitivity_pairs_enqueue", "emulate_sensitivity_pairs_collect",
                 "emulate_sensitivity_pairs_post", "emulate_sensitivity_pairs_uncertainty", "emulate_interaction_surface",
                 "emulate_sensitivity_pairs_multi", "emulate_sensitivity_pairs_uncertainty_multi", "emulate_interaction_surface_multi"):
        assert hasattr(host, name)
    assert all(hasattr(abi.Context, n) for n in ("sens_pairs", "sens_pairs_dev", "sens_pairs_post", "sens_pairs_post_dev", "sens_joint"))
