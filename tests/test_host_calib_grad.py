"""The gradient of the calibration log density through the C host layer (libEmuMI.so: emulate_points_multi_logpdf_grad) on the
committed multi-output snapshot (N = 100, three components, six outputs).  The kernel is judged in
tests/test_gpu_calib_grad.py; here the layer above it:

  * the gradients against calibgradref's direct nt x nt form evaluated at the library's OWN PCA-space m, v, dm/dx and dv/dx
    (emulate_points_multi_grad(..., pca_space = 1, ...)), under calibgradref.BARS
  * stat_out bit for bit what emulate_points_multi_implausibility returns; repeated and reduced calls bit for bit
  * central differences of the layer's own logpdf with steps h and h / 2, h = 1e-4 of each parameter's design range: the gap
    to the gradient may be 8 |FD(h) - FD(h/2)| (the quotient's own truncation estimate) + 8 2^-52 max |logpdf| / h (its
    rounding) + the reference bar
"""
import subprocess

import numpy as np
import pytest

import calibgradref as G
from test_host_api import parse_snapshot  # noqa: F401
from test_host_calib import observation_set, rows
from test_host_mean import G6SNAP, compile_driver, multi_queries  # noqa: F401  (multi_queries: a fixture)

FD_POINTS = (5, 20, 41, 74)                               # inside the box, off the design (the first five queries are design points)


@pytest.fixture(scope="module")
def grad_driver(tmp_path_factory):
    return compile_driver(tmp_path_factory.mktemp("drv"), "host_calib_grad_driver.c", False)


@pytest.fixture(scope="module", params=[(0, 0), (1, 1)], ids=["diag", "full_rel"])
def run(request, grad_driver, multi_queries, tmp_path_factory):
    full, hasrel = request.param
    sd, qfile, nq = multi_queries
    z, sig, S, rel = observation_set(sd, full, hasrel)
    tmp = tmp_path_factory.mktemp("obs")
    path = tmp / "obs.dat"
    with open(path, "w") as f:
        f.write(f"{full} {hasrel}\n")
        for a in (z, S if full else sig) + ((rel,) if hasrel else ()):
            f.write(" ".join(repr(float(x)) for x in np.ravel(a)) + "\n")
    Q = np.loadtxt(qfile).reshape(nq, -1)
    X = sd["models"][0]["X"]
    h = 1e-4 * (X.max(axis=0) - X.min(axis=0))
    fd = []
    for q in FD_POINTS:
        for j in range(Q.shape[1]):
            for s in (1.0, -1.0, 0.5, -0.5):
                x = Q[q].copy()
                x[j] += s * h[j]
                fd.append(x)
    fd = np.array(fd)
    np.savetxt(tmp / "fd.dat", fd, fmt="%.17g")
    out = subprocess.run([grad_driver, G6SNAP, qfile, str(path), str(tmp / "fd.dat")], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stderr[-3000:]
    case = dict(name="g6", nt=sd["nt"], nr=sd["nr"], M=nq, z=z, S=S, sd=None if full else sig, rel=rel, d=Q.shape[1])
    case["obs_file"], case["qfile"], case["tmp"] = str(path), qfile, tmp
    return sd, nq, case, out.stdout, fd, h


@pytest.fixture(scope="module")
def reference(run):
    """calibgradref.direct64 at the library's own m, v, dm/dx and dv/dx, once per observation set"""
    sd, nq, c, out, fd, h = run
    nr, d = c["nr"], c["d"]
    c["ybar"], c["A"] = rows(out, "ybar")[0], np.ascontiguousarray(rows(out, "acol").T)
    c["mean"], c["var"] = np.ascontiguousarray(rows(out, "pca_m").T), np.ascontiguousarray(rows(out, "pca_v").T)
    for key, tag in (("gmean", "pca_gm"), ("gvar", "pca_gv")):
        c[key] = np.ascontiguousarray(rows(out, tag).reshape(nq, nr, d).transpose(1, 0, 2)).reshape(nr, nq * d)
    c["ldg"] = nq * d
    return G.direct64(c)


@pytest.mark.gpu
def test_gradients_against_the_direct_form(run, reference):
    sd, nq, c, out, fd, h = run
    ref, scale = reference
    got = np.stack([rows(out, "gchi"), rows(out, "glog")])
    assert got.shape == (2, nq, c["d"]) and np.all(np.isfinite(got))
    e = G.err(got, ref, scale).max(axis=(1, 2))
    print("host gradients against the direct form:", e, "bars", G.BARS)
    assert np.all(e <= G.BARS), e
    assert np.abs(got[1]).max() > 1.0                      # (not a comparison of zeros)


@pytest.mark.gpu
def test_stat_out_is_the_implausibility_entry_bit_for_bit(run):
    sd, nq, c, out, fd, h = run
    st, ref = rows(out, "stat"), rows(out, "ref")
    assert st.shape == (nq, 5) and st.tobytes() == ref.tobytes()
    assert rows(out, "same")[0, 0] == 0


@pytest.mark.gpu
def test_gradient_against_central_differences_of_the_layers_logpdf(run, reference):
    sd, nq, c, out, fd, h = run
    ref, scale = reference
    gl = rows(out, "glog")
    lp = rows(out, "fd")[:, 0].reshape(len(FD_POINTS), c["d"], 4)
    lpmax = np.abs(lp).max()
    for i, q in enumerate(FD_POINTS):
        for j in range(c["d"]):
            f1 = (lp[i, j, 0] - lp[i, j, 1]) / (2.0 * h[j])
            f2 = (lp[i, j, 2] - lp[i, j, 3]) / h[j]
            bar = 8.0 * abs(f1 - f2) + 8.0 * 2.0 ** -52 * lpmax / h[j] + G.BARS[1] * max(1.0, scale[1, q, j])
            print(f"point {q} coordinate {j}: gradient {gl[q, j]:.12e} FD(h/2) {f2:.12e} gap {abs(gl[q, j] - f2):.2e} allowed {bar:.2e}")
            assert abs(gl[q, j] - f2) <= bar, (q, j)


@pytest.fixture(scope="module")
def cpp_driver(tmp_path_factory):
    return compile_driver(tmp_path_factory.mktemp("drvpp"), "emupp_calib_grad_driver.cpp", True)


@pytest.mark.gpu
def test_cpp_entry_returns_the_c_entry_numbers(run, cpp_driver):
    sd, nq, c, out, fd, h = run
    pp = subprocess.run([cpp_driver, G6SNAP, c["qfile"], c["obs_file"]], capture_output=True, text=True, timeout=300)
    assert pp.returncode == 0, pp.stderr[-3000:]
    assert rows(pp.stdout, "ll")[:, 0].tobytes() == np.ascontiguousarray(rows(out, "stat")[:, 1]).tobytes()
    assert rows(pp.stdout, "grad").tobytes() == rows(out, "glog").tobytes()


@pytest.mark.gpu
def test_cli_gradient_flag_prints_the_c_entry_numbers(run):
    """`implausibility --gradient` with no cut: every point's line ends in the d components, to the printed digits; without the
    flag the lines are their first part"""
    sd, nq, c, out, fd, h = run
    nt, d = c["nt"], c["d"]
    sig = np.sqrt(np.diag(c["S"])) if c["S"] is not None else c["sd"]
    obs = c["tmp"] / "obs_cli.dat"
    with open(obs, "w") as f:
        f.write(f"{nt}\n")
        for t in range(nt):
            f.write(f"{float(c['z'][t])!r} {float(sig[t])!r}" + (f" {float(c['rel'][t])!r}" if c["rel"] is not None else "") + "\n")
        if c["S"] is not None:
            f.write("covariance\n" + "".join(" ".join(repr(float(x)) for x in row) + "\n" for row in c["S"]))
    from madaiemulator_amd import build
    args = [build.CLI_BIN, "implausibility", G6SNAP, f"--observations={obs}", "--cut=inf", "--quiet"]
    points = open(c["qfile"]).read()
    with_g = subprocess.run(args + ["--gradient"], input=points, capture_output=True, text=True, timeout=300)
    plain = subprocess.run(args, input=points, capture_output=True, text=True, timeout=300)
    assert with_g.returncode == 0 and plain.returncode == 0, with_g.stderr[-2000:]
    lg, lp = with_g.stdout.splitlines(), plain.stdout.splitlines()
    assert len(lg) == nq and len(lp) == nq
    gl = rows(out, "glog")
    for q in range(nq):
        tok = lg[q].split()
        assert int(tok[0]) == q and " ".join(tok[:-d]) == lp[q].strip()
        assert tok[-d:] == [format(x, ".17g") for x in gl[q]], q
