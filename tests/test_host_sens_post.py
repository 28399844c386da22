"""The emulator-uncertainty terms of the sensitivity analysis through the C host layer (libEmuMI.so: emulate_sensitivity_post,
emulate_sensitivity_uncertainty, emulate_main_effects_var / _band, their _multi forms) and the CLI's `sensitivity --uncertainty`,
against the device library's own entries (same launches on the same state: same bits) and against the composition rules
computed in numpy from the per-component numbers.

The multi-output test is the one that fails if the S terms are contracted over pairs of components like the plug-in part, or
the plug-in part by the squared rule: in observable space S_u(y_t) = sum_c B_tc^2 S_u^c (the components are independent a
posteriori) while V, V_j, VT_j keep their cross terms."""
import subprocess

import numpy as np
import pytest

from madaiemulator_amd import abi, build
from test_host_mean import compile_driver
from test_host_sens import G, cli, rows, two_components, write_box          # noqa: F401  (fixtures)

EPS = 2.0 ** -52


@pytest.fixture(scope="module")
def post_driver(tmp_path_factory):
    return compile_driver(tmp_path_factory.mktemp("drv"), "host_sens_post_driver.c", False)


def box_of(tc):
    return tc["X"].min(axis=0), tc["X"].max(axis=0) - 0.2


@pytest.mark.gpu
@pytest.mark.parametrize("pca", [0, 1])
def test_composition_rules(post_driver, two_components, gpu_ctx, tmp_path, pca):
    tc = two_components
    X, d, nr = tc["X"], 2, 2
    lo, hi = box_of(tc)
    box = write_box(tmp_path / "box.txt", lo, hi)
    out = subprocess.run([post_driver, tc["path"], box, str(G), str(pca)], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stderr[-3000:]
    txt = out.stdout
    grid = np.stack([lo + k * (hi - lo) / (G - 1) for k in range(G)], axis=1)
    # the components' entries return the bits of the device entries on the same state
    comp, cvar = rows(txt, "comp")[:, 1:], []
    for c in range(nr):
        gpu_ctx.set_model(1, tc["order"], X, tc["Z"][:, c])
        _, rc = gpu_ctx.predict_setup(tc["ths"][c])
        assert rc == abi.OK
        dev = gpu_ctx.sens_post(lo, hi)
        assert np.array_equal(comp[c], np.concatenate([[dev["s_none"], dev["s_all"]], dev["s_first"], dev["s_rest"]]))
        _, var, ve0 = gpu_ctx.sens_main_var(lo, hi, grid)
        cvar.append(rows(txt, f"cvar {c}")[:, 1:])
        assert np.array_equal(cvar[c], var) and rows(txt, f"cvare0 {c}")[0, 0] == ve0
        # E*[V_j] = V_j + S_j - S_none and its companions through emulate_sensitivity_uncertainty
        (e0, V), first, total = rows(txt, f"cplug {c}")[0], rows(txt, f"cfirst {c}")[0], rows(txt, f"ctotal {c}")[0]
        s_none, s_all, s_first, s_rest = comp[c][0], comp[c][1], comp[c][2:2 + d], comp[c][2 + d:]
        unc = rows(txt, f"cunc {c}")[0]
        assert unc[0] == s_none and unc[1] == s_all
        tol = 4 * EPS * (abs(V) + s_all)
        assert abs(unc[2] - (V + s_all - s_none)) <= tol
        assert np.all(np.abs(rows(txt, f"cefirst {c}")[0] - (first + s_first - s_none)) <= tol)
        assert np.all(np.abs(rows(txt, f"cetotal {c}")[0] - (total + s_all - s_rest)) <= tol)
        assert s_none <= s_first.min() and s_first.max() <= s_all and s_none <= s_rest.min() and s_rest.max() <= s_all
    # outputs: the S terms by the squared rule, the plug-in part as emulate_sensitivity_multi returns it (cross terms and all)
    B = np.eye(nr) if pca else tc["evecs"] * np.sqrt(tc["evals"])
    nout = B.shape[0]
    S = (B ** 2) @ comp                                  # nout x (2 + 2 d)
    plug, pfirst, ptotal = rows(txt, "plug")[:, 1:], rows(txt, "pfirst")[:, 1:], rows(txt, "ptotal")[:, 1:]
    unc, efirst, etotal = rows(txt, "unc")[:, 1:], rows(txt, "efirst")[:, 1:], rows(txt, "etotal")[:, 1:]
    assert unc.shape == (nout, 3) and efirst.shape == (nout, d) and etotal.shape == (nout, d)
    for t in range(nout):
        tol = 8 * EPS * (abs(plug[t, 1]) + S[t, 1])
        assert abs(unc[t, 0] - S[t, 0]) <= tol and abs(unc[t, 1] - S[t, 1]) <= tol
        assert abs(unc[t, 2] - (plug[t, 1] + S[t, 1] - S[t, 0])) <= tol
        assert np.all(np.abs(efirst[t] - (pfirst[t] + S[t, 2:2 + d] - S[t, 0])) <= tol)
        assert np.all(np.abs(etotal[t] - (ptotal[t] + S[t, 1] - S[t, 2 + d:])) <= tol)
        if not pca:
            # contracting the S terms over pairs like the plug-in part would need cross terms that do not exist; the full
            # quadratic form with the components' S as "diagonal" and nothing else IS the squared rule -- and the plain sum
            # sum_c B_tc S^c (the mean rule) is a different number
            assert abs((B[t] @ comp)[1] - S[t, 1]) > 1e6 * tol
        sd_want = np.sqrt(sum(B[t, c] ** 2 * cvar[c] for c in range(nr)))
        sd = rows(txt, f"sd {t}")[:, 1:]
        assert sd.shape == (d, G) and np.all(np.abs(sd - sd_want) <= 8 * EPS * sd_want + 1e-300)
        assert abs(rows(txt, f"e0main {t}")[0, 0] - plug[t, 0]) <= 1e-12 * max(1.0, abs(plug[t, 0]))


@pytest.mark.gpu
@pytest.mark.parametrize("pca", [0, 1])
def test_cpp_methods(post_driver, two_components, tmp_path, pca):
    """the C++ class returns the numbers of the C entries"""
    tc = two_components
    lo, hi = box_of(tc)
    box = write_box(tmp_path / "box.txt", lo, hi)
    exe = compile_driver(tmp_path, "emupp_sens_post_driver.cpp", True)
    cpp = subprocess.run([exe, tc["path"], box, str(G)] + (["pca"] if pca else []), capture_output=True, text=True, timeout=300)
    c = subprocess.run([post_driver, tc["path"], box, str(G), str(pca)], capture_output=True, text=True, timeout=300)
    assert cpp.returncode == 0 and c.returncode == 0, cpp.stderr[-3000:] + c.stderr[-3000:]
    for tag in ("unc", "efirst", "etotal", "main", "sd", "e0main"):
        got = rows(cpp.stdout, tag)
        assert got.size and np.array_equal(got, rows(c.stdout, tag)), tag


@pytest.mark.gpu
def test_cli_uncertainty(cli, post_driver, two_components, tmp_path):
    """without --uncertainty the output is byte for byte what the old entries give; with it, the extra lines in their places"""
    tc = two_components
    d, nout = 2, 3
    lo, hi = box_of(tc)
    box = write_box(tmp_path / "box.txt", lo, hi)

    def go(*args):
        r = subprocess.run([cli, "sensitivity", tc["path"], f"--box={box}", f"--grid={G}", "--quiet"] + list(args), capture_output=True,
                           text=True, timeout=300, cwd=tmp_path)
        assert r.returncode == 0, r.stderr[-3000:]
        return r.stdout

    drv = subprocess.run([post_driver, tc["path"], box, str(G), "0"], capture_output=True, text=True, timeout=300)
    assert drv.returncode == 0, drv.stderr[-3000:]
    txt = drv.stdout
    fmt = lambda v: " ".join("%.17g" % x for x in v)
    plug, pfirst, ptotal = rows(txt, "plug")[:, 1:], rows(txt, "pfirst")[:, 1:], rows(txt, "ptotal")[:, 1:]
    old = [fmt(np.concatenate([[plug[t, 1]], pfirst[t] / plug[t, 1], ptotal[t] / plug[t, 1]])) for t in range(nout)]
    for t in range(nout):
        old += [fmt(c) for c in rows(txt, f"main {t}")[:, 1:]] + ["%.17g" % rows(txt, f"e0main {t}")[0, 0]]
    plain = go()
    assert plain == "\n".join(old) + "\n"
    unc, efirst, etotal = rows(txt, "unc")[:, 1:], rows(txt, "efirst")[:, 1:], rows(txt, "etotal")[:, 1:]
    new = old[:nout] + [fmt(np.concatenate([[np.sqrt(unc[t, 0]), unc[t, 1], unc[t, 2]], efirst[t] / unc[t, 2], etotal[t] / unc[t, 2]]))
                        for t in range(nout)]
    for t in range(nout):
        for j in range(d):
            new += [fmt(rows(txt, f"main {t} {j}")[0]), fmt(rows(txt, f"sd {t} {j}")[0])]
        new.append("%.17g" % rows(txt, f"e0main {t}")[0, 0])
    with_unc = go("--uncertainty")
    assert with_unc == "\n".join(new) + "\n"
    # without --grid: the index lines, then the uncertainty lines
    r = subprocess.run([cli, "sensitivity", tc["path"], f"--box={box}", "--quiet", "--uncertainty"], capture_output=True, text=True,
                       timeout=300, cwd=tmp_path)
    assert r.returncode == 0 and r.stdout == "\n".join(new[:2 * nout]) + "\n"


def test_symbols_are_exported():
    import ctypes
    build.build_all()
    dev, host = ctypes.CDLL(build.HIP_LIB), ctypes.CDLL(build.HOST_LIB)
    for name in ("gpemu_sens_post", "gpemu_sens_post_dev", "gpemu_sens_main_var", "gpemu_test_sens_post_state"):
        assert hasattr(dev, name) and name in abi.SYMBOLS
    for name in ("emulate_sensitivity_post", "emulate_sensitivity_uncertainty", "emulate_main_effects_var", "emulate_main_effects_band",
                 "emulate_sensitivity_uncertainty_multi", "emulate_main_effects_band_multi"):
        assert hasattr(host, name)
    assert abi.PROF_SENS_POST == 15
    assert all(hasattr(abi.Context, n) for n in ("sens_post", "sens_post_dev", "sens_main_var", "sens_post_state"))
