"""The gain over a weighted set of target points through the C host layer (libEmuMI.so: emulate_design_target_set,
emulate_design_target_gain, emulate_design_target_gain_multi), the C++ class (emulator::QueryEmulatorTargetedDesignGain) and the
CLI's `design --targets=FILE`, against the device library's own entries (same launches on the same state: same bits) and against
the composition rule computed in numpy from the per-component numbers.

One run observes every PCA component, and the components are independent a posteriori: the weighted variance of output t over the
targets is sum_c B_tc^2 target_var_c and its drop is gain(y_t) = sum_c B_tc^2 gain_c -- the squared rule of
gpemu_host_backproject, no cross terms, as for emulate_design_gain_multi."""
import subprocess

import numpy as np
import pytest

from madaiemulator_amd import abi, build, synth
from test_host_calib import write_cli_observation_file
from test_host_design import component_state, loadings
from test_host_mean import compile_driver
from test_host_sens import cli, rows, two_components, twod                     # noqa: F401  (fixtures)

EPS = 2.0 ** -52


@pytest.fixture(scope="module")
def target_driver(tmp_path_factory):
    return compile_driver(tmp_path_factory.mktemp("drv"), "host_design_target_driver.c", False)


def lines_of(A):
    return "".join(" ".join(repr(float(v)) for v in x) + "\n" for x in A)


def setting(tc, tmp_path):
    """70 targets with uneven weights (one of them 0) around a corner of the design, 8 candidates of which the last repeats the first"""
    X = tc["X"]
    lo, hi = X.min(axis=0), X.max(axis=0)
    r = np.random.default_rng(47)
    Xt = lo + 0.4 * (hi - lo) * r.random((70, 2))
    w = 0.5 + r.random(70)
    w[3] = 0.0
    Xq = (lo - 0.1) + (hi - lo + 0.2) * r.random((7, 2))
    Xq = np.vstack([Xq, Xq[:1]])
    tg, pts = tmp_path / "targets_w.txt", tmp_path / "points.txt"
    tg.write_text(lines_of(np.column_stack([Xt, w])))
    pts.write_text(lines_of(Xq))
    return Xt, w, Xq, str(tg), str(pts)


@pytest.mark.gpu
@pytest.mark.parametrize("pca", [0, 1])
def test_composition_rule(target_driver, two_components, gpu_ctx, tmp_path, pca):
    tc = two_components
    Xt, w, Xq, tg, pts = setting(tc, tmp_path)
    out = subprocess.run([target_driver, tc["path"], tg, pts, str(pca)], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stderr[-3000:]
    comp, cnum, cvar, cvt = (rows(out.stdout, t)[:, 1:] for t in ("comp", "cnum", "cvar", "cvt"))
    ctv = rows(out.stdout, "ctv")[:, 1]
    for c in range(2):                           # the components' entries return the bits of the device entries on the same state
        component_state(gpu_ctx, tc, c)
        st = gpu_ctx.design_target_set(Xt, w)
        dev = gpu_ctx.design_target_gain(Xq)
        assert np.array_equal(comp[c], dev["gain"]) and np.array_equal(cnum[c], dev["num"]) and np.array_equal(cvar[c], dev["var"])
        assert ctv[c] == st["target_var"] and np.array_equal(cvt[c], st["var_t"])
        assert np.array_equal(comp[c][0], comp[c][-1])                                   # the repeated candidate
        assert np.all(comp[c] >= 0) and np.all(comp[c] <= ctv[c])
    assert np.array_equal(rows(out.stdout, "again")[0, 1:], comp[0])                      # set, gain, release behind the multi call
    B = loadings(tc, pca)                        # outputs: the squared rule, no cross terms; the total is the sum over the outputs
    gain, total, tv = rows(out.stdout, "gain")[:, 1:], rows(out.stdout, "total")[:, 1], rows(out.stdout, "tv")[0, 1:]
    want, want_tv = comp.T @ (B ** 2).T, (B ** 2) @ ctv
    assert gain.shape == want.shape == (len(Xq), B.shape[0]) and tv.shape == want_tv.shape
    assert np.all(np.abs(gain - want) <= 8 * EPS * want) and np.all(np.abs(tv - want_tv) <= 8 * EPS * want_tv)
    assert np.all(np.abs(total - gain.sum(axis=1)) <= 8 * EPS * total)
    if not pca:
        assert np.all(np.abs(gain - comp.T @ B.T) > 1e6 * EPS * want)                     # the mean rule is a different number


@pytest.mark.gpu
@pytest.mark.parametrize("pca", [0, 1])
def test_cpp_method(target_driver, two_components, tmp_path, pca):
    tc = two_components
    Xt, w, Xq, tg, pts = setting(tc, tmp_path)
    exe = compile_driver(tmp_path, "emupp_design_target_driver.cpp", True)
    cpp = subprocess.run([exe, tc["path"], tg, pts] + (["pca"] if pca else []), capture_output=True, text=True, timeout=300)
    c = subprocess.run([target_driver, tc["path"], tg, pts, str(pca)], capture_output=True, text=True, timeout=300)
    assert cpp.returncode == 0 and c.returncode == 0, cpp.stderr[-3000:] + c.stderr[-3000:]
    for tag, n in (("gain", len(Xq)), ("total", len(Xq)), ("tv", 1)):
        assert np.array_equal(rows(cpp.stdout, tag), rows(c.stdout, tag)) and len(rows(c.stdout, tag)) == n


@pytest.mark.gpu
def test_cli_design_targets(cli, target_driver, two_components, tmp_path):
    tc = two_components
    Xt, w, Xq, tg, pts = setting(tc, tmp_path)
    text = open(pts).read()
    plain = tmp_path / "targets.txt"             # equal weights: what the CLI gives every target
    plain.write_text("# a comment line\n" + lines_of(Xt[:5]) + "\n   # another, after an empty line\n" + lines_of(Xt[5:]))
    eq = tmp_path / "targets_eq.txt"
    eq.write_text(lines_of(np.column_stack([Xt, np.full(len(Xt), 1.0 / len(Xt))])))

    def go(*args, targets=plain):
        return subprocess.run([cli, "design", tc["path"], f"--targets={targets}"] + list(args), input=text, capture_output=True, text=True,
                              timeout=300, cwd=tmp_path)

    drv = subprocess.run([target_driver, tc["path"], str(eq), pts, "0"], capture_output=True, text=True, timeout=300)
    assert drv.returncode == 0, drv.stderr[-3000:]
    total, tv = rows(drv.stdout, "total")[:, 1], rows(drv.stdout, "tv")[0, 1:]
    out = go()
    assert out.returncode == 0, out.stderr[-3000:]
    lines = out.stdout.splitlines()
    assert lines[0] == "# index param_0 param_1 expected_target_variance_reduction target_variance" and len(lines) == 1 + len(Xq)
    vals = np.array([ln.split() for ln in lines[1:]], float)
    assert np.array_equal(vals[:, 0], np.arange(len(Xq))) and np.array_equal(vals[:, 1:3], Xq)
    assert np.array_equal(vals[:, 3], total)
    assert np.all(vals[:, 4] == vals[0, 4]) and abs(vals[0, 4] - tv.sum()) <= 8 * EPS * tv.sum()
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
    # further columns are ignored; the parameters may start at a later column
    wide = tmp_path / "targets_wide.txt"
    wide.write_text("# index param_0 param_1 chi2\n" + "".join(f"{i} {float(x[0])!r} {float(x[1])!r} {3.5 + i}\n" for i, x in enumerate(Xt)))
    assert go("--targets-column=1", targets=wide).stdout == out.stdout
    assert go(targets=eq).stdout == out.stdout                                           # (the weight column is a further column)
    short = go("--targets-column=2", targets=wide)
    assert short.returncode == 0 and short.stdout != out.stdout                          # (param_1, chi2): other targets
    r = go("--targets-column=3", targets=wide)
    assert r.returncode != 0 and "fewer than 5 columns" in r.stderr and r.stdout == ""
    r = go(targets=tmp_path / "no_such_file.txt")
    assert r.returncode != 0 and r.stdout == ""


@pytest.mark.gpu
def test_cli_takes_the_output_of_sample_and_of_implausibility(cli, two_components, tmp_path):
    tc = two_components
    Xt, w, Xq, tg, pts = setting(tc, tmp_path)
    text = open(pts).read()
    obs = tmp_path / "obs.txt"
    Yhat = tc["ybar"] + 0.1
    write_cli_observation_file(obs, Yhat, np.full(len(Yhat), 0.3), None, None)
    smp = subprocess.run([cli, "sample", tc["path"], f"--observations={obs}", "--walkers=8", "--steps=6", "--burn=2", "--seed=3"],
                         capture_output=True, text=True, timeout=300, cwd=tmp_path)
    assert smp.returncode == 0, smp.stderr[-3000:]
    chain = tmp_path / "chain.txt"
    chain.write_text(smp.stdout)
    S = np.array([ln.split() for ln in smp.stdout.splitlines() if not ln.startswith("#")], float)
    assert S.shape == (32, 3)
    out = subprocess.run([cli, "design", tc["path"], f"--targets={chain}"], input=text, capture_output=True, text=True, timeout=300, cwd=tmp_path)
    assert out.returncode == 0, out.stderr[-3000:]
    bare = tmp_path / "chain_bare.txt"
    bare.write_text(lines_of(S[:, :2]))
    ref = subprocess.run([cli, "design", tc["path"], f"--targets={bare}"], input=text, capture_output=True, text=True, timeout=300, cwd=tmp_path)
    assert ref.returncode == 0 and out.stdout == ref.stdout and len(out.stdout.splitlines()) == 1 + len(Xq)
    # implausibility's lines start with the index: the parameters from column 1 on
    imp = subprocess.run([cli, "implausibility", tc["path"], f"--observations={obs}", "--cut=inf"], input=lines_of(S[:, :2]),
                         capture_output=True, text=True, timeout=300, cwd=tmp_path)
    assert imp.returncode == 0, imp.stderr[-3000:]
    kept = tmp_path / "kept.txt"
    kept.write_text(imp.stdout)
    assert len([ln for ln in imp.stdout.splitlines() if not ln.startswith("#")]) == 32
    out2 = subprocess.run([cli, "design", tc["path"], f"--targets={kept}", "--targets-column=1"], input=text, capture_output=True, text=True,
                          timeout=300, cwd=tmp_path)
    assert out2.returncode == 0 and out2.stdout == ref.stdout, out2.stderr[-3000:]


def matern_snapshot(tmp_path):
    X, y, _ = twod()
    snap = tmp_path / "matern.txt"
    snap.write_text(synth.single_output_snapshot(X, y, 3, 1, np.array([1.0, 0.01, np.log(0.6)])))
    tg = tmp_path / "t.txt"
    tg.write_text(lines_of(X[:9] + 0.01))
    return X, y, str(snap), str(tg)


def test_cli_exclusions_need_no_device(cli, tmp_path):
    """--targets excludes --box, --prior and --batch; without it a Matern snapshot is refused as before; the usage names it"""
    X, y, snap, tg = matern_snapshot(tmp_path)
    (tmp_path / "box.txt").write_text("0 1\n0 1\n")
    for extra in (["--box=box.txt"], ["--prior=box.txt"], ["--batch=2"]):
        r = subprocess.run([cli, "design", snap, f"--targets={tg}"] + extra, input="0.5 0.5\n", capture_output=True, text=True, timeout=60,
                           cwd=tmp_path)
        assert r.returncode != 0 and "--targets=FILE excludes --box, --prior and --batch" in r.stderr and r.stdout == "", extra
    r = subprocess.run([cli, "design", snap, "--targets-column=1"], input="0.5 0.5\n", capture_output=True, text=True, timeout=60, cwd=tmp_path)
    assert r.returncode != 0 and "--targets-column=K needs --targets=FILE" in r.stderr
    for bad in ("-1", "x", "1.5"):
        r = subprocess.run([cli, "design", snap, f"--targets={tg}", f"--targets-column={bad}"], input="0.5 0.5\n", capture_output=True, text=True,
                           timeout=60, cwd=tmp_path)
        assert r.returncode != 0 and "--targets-column=K needs a number" in r.stderr, bad
    r = subprocess.run([cli, "design", snap], input="0.5 0.5\n", capture_output=True, text=True, timeout=60, cwd=tmp_path)
    assert r.returncode != 0 and "power-exponential covariance only" in r.stderr and r.stdout == ""
    u = subprocess.run([cli, "no_such_mode", "x"], capture_output=True, text=True, timeout=60, cwd=tmp_path)
    assert u.returncode != 0 and "[--targets=FILE [--targets-column=K]]" in u.stderr


@pytest.mark.gpu
def test_cli_takes_a_matern_snapshot_with_targets(cli, gpu_ctx, tmp_path):
    X, y, snap, tg = matern_snapshot(tmp_path)
    Xq = np.array([[0.5, 0.5], [0.1, 0.9], [0.5, 0.5]])
    r = subprocess.run([cli, "design", snap, f"--targets={tg}", "--quiet"], input=lines_of(Xq), capture_output=True, text=True, timeout=300,
                       cwd=tmp_path)
    assert r.returncode == 0, r.stderr[-3000:]
    vals = np.array([ln.split() for ln in r.stdout.splitlines()], float)
    assert vals.shape == (3, 5) and np.array_equal(vals[0, 3:], vals[2, 3:])
    assert np.all(vals[:, 3] >= 0) and np.all(vals[:, 3] <= vals[:, 4])


def test_symbols_are_exported():
    import ctypes
    build.build_all()
    dev, host = ctypes.CDLL(build.HIP_LIB), ctypes.CDLL(build.HOST_LIB)
    for name in ("gpemu_design_target_set", "gpemu_design_target_set_dev", "gpemu_design_target_gain", "gpemu_design_target_gain_dev",
                 "gpemu_design_target_release", "gpemu_test_design_target_state"):
        assert hasattr(dev, name), name
    for name in ("emulate_design_target_set", "emulate_design_target_gain", "emulate_design_target_release",
                 "emulate_design_target_gain_multi"):
        assert hasattr(host, name), name
