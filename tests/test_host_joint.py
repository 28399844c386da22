"""Hold-out validation and joint draws through the C host layer (libEmuMI.so: emulate_points_holdout and its halves,
emulate_points_draw, emulate_points_multi_holdout, emulate_points_multi_draw), the C++ class (emulator::ValidateHoldout,
emulator::DrawEmulator) and the command line (interactive_emulator validate SNAPSHOT --holdout=FILE), on the reference's
example inputs and the committed multi-output snapshot.  The device entries themselves are judged against an independent
reference in tests/test_gpu_predict_joint.py; here the layers above them are checked: they hand on the device entry's bits per
component; the projection of the observations is numpy's (Y - training_mean) evecs / sqrt(evals) to 1e-13 of the largest
projected value (nt = 6 terms); the summed log density is the sum; observable-space draws are the numpy back-projection
training_mean + draw_pca (evecs sqrt(evals))^T to 1e-12 (nr terms); and the command line's columns and summary are
tests/jointref.py's numbers within the bars of tests/test_gpu_predict_joint.py."""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest

import jointref
from madaiemulator_amd import abi, build, synth
from test_host_api import parse_snapshot
from test_host_mean import G6SNAP, UNI, UNI_Q, compile_driver

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
RTOL = jointref.RTOL
NP, ND = 40, 3


def rows(out, tag):
    n = len(tag.split())
    return np.array([line.split()[n:] for line in out.splitlines() if line.startswith(tag + " ")], float)


@pytest.fixture(scope="module")
def joint_driver(tmp_path_factory):
    return compile_driver(tmp_path_factory.mktemp("drv"), "host_joint_driver.c", False)


@pytest.fixture(scope="module")
def campaign(tmp_path_factory):
    """a held-out campaign for the committed snapshot: NP fresh points in the design's box (none on a training point, no two
    alike), observations = the training mean plus a smooth function and noise on the scale of the training outputs, and
    normals for ND draws per component.  -> (snapshot dict, Xq, Y, Z[nr, ND, NP], paths)"""
    sd = parse_snapshot(open(G6SNAP).read().split())
    Xq = jointref.fresh_queries(sd["models"][0]["X"], NP, 8100)
    rng = np.random.default_rng(8101)
    Y = sd["Y"].mean(axis=0) + sd["Y"].std(axis=0) * (np.sin(Xq.sum(axis=1))[:, None] + 0.3 * rng.standard_normal((NP, sd["nt"])))
    Z = rng.standard_normal((sd["nr"], ND, NP))
    tmp = tmp_path_factory.mktemp("campaign")
    paths = {k: str(tmp / f"{k}.dat") for k in ("q", "y", "z", "holdout")}
    np.savetxt(paths["q"], Xq, fmt="%.17g")
    np.savetxt(paths["y"], Y, fmt="%.17g")
    np.savetxt(paths["z"], Z.reshape(-1, NP), fmt="%.17g")
    with open(paths["holdout"], "w") as f:                         # the INPUT_MODEL_FILE format: "nt d N", design, outputs
        f.write(f"{sd['nt']}\n{sd['d']}\n{NP}\n")
        np.savetxt(f, Xq, fmt="%.17g")
        np.savetxt(f, Y, fmt="%.17g")
    return sd, Xq, Y, Z, paths


@pytest.fixture(scope="module")
def multi_out(joint_driver, campaign):
    sd, Xq, Y, Z, paths = campaign
    out = subprocess.run([joint_driver, "multi", G6SNAP, paths["q"], paths["y"], paths["z"]], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stderr[-3000:]
    return out.stdout


def projected(sd, Y):
    """nr x NP: numpy's projection from the snapshot's fields"""
    return ((Y - sd["Y"].mean(axis=0)) @ sd["evecs"] / np.sqrt(sd["evals"])).T


@pytest.mark.gpu
@pytest.mark.parametrize("cov,order", [(1, 1), (3, 0), (2, 3)])
def test_emulate_points_holdout_hands_on_the_device_entry(joint_driver, tmp_path, cov, order):
    """emulate_points_holdout / emulate_points_draw carry the bits of gpemu_predict_joint_factor / _draw on a context of the
    test's own; a second call, the enqueue / collect pair and NULL outputs change no bit"""
    th = np.array([0.3, -3.0, -0.4]) if cov == 1 else np.array([1.3, 0.02, np.log(0.8)])
    X, Y = synth.read_input_model_file(UNI)
    d = X.shape[1]
    Xq = np.array(open(UNI_Q).read().split(), float).reshape(-1, d)
    M = Xq.shape[0]
    rng = np.random.default_rng(8200 + cov)
    yobs = Y[:, 0].mean() + Y[:, 0].std() * rng.standard_normal(M)
    noise = 0.05 + 0.1 * rng.random(M)                              # the example's queries may coincide with training points
    z = rng.standard_normal((4, M))
    aux = tmp_path / "aux.dat"
    np.savetxt(aux, np.vstack([yobs, noise, z]), fmt="%.17g")
    out = subprocess.run([joint_driver, "uni", UNI, UNI_Q, str(aux), str(cov), str(order)] + [repr(float(t)) for t in th],
                         capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stderr[-3000:]
    assert rows(out.stdout, "same")[0, 0] == 0
    # (the file holds the numbers to 17 digits: what the driver read is what numpy reads back)
    back = np.loadtxt(aux)
    c = abi.Context(0)
    try:
        c.set_model(cov, order, X, Y[:, 0])
        _, rc = c.predict_setup(th)
        assert rc == abi.OK
        g = c.predict_joint_factor(Xq, back[1], back[0])
        draws = c.predict_joint_draw(back[2:])
    finally:
        c.close()
    assert g["status"] == abi.OK
    assert np.array_equal(rows(out.stdout, "mean")[0], g["mean"]) and np.array_equal(rows(out.stdout, "var")[0], g["var"])
    assert np.array_equal(rows(out.stdout, "werr")[0], g["werr"][0])
    assert np.array_equal(rows(out.stdout, "stat")[0], [g["maha"][0], g["logdet"], g["logpdf"][0]])
    assert np.array_equal(rows(out.stdout, "draw"), draws)


@pytest.mark.gpu
def test_emulate_points_multi_holdout(multi_out, campaign):
    sd, Xq, Y, Z, paths = campaign
    nr, nt = sd["nr"], sd["nt"]
    want = projected(sd, Y)
    pm, pv, pw = rows(multi_out, "pca_m"), rows(multi_out, "pca_v"), rows(multi_out, "pca_w")
    assert pm.shape == pv.shape == pw.shape == (NP, nr)
    total = 0.0
    for c in range(nr):
        proj = rows(multi_out, f"proj {c}")[0]
        ep = float(np.max(np.abs(proj - want[c])) / np.max(np.abs(want[c])))
        print(f"component {c}: projection against numpy {ep:.3e} (bar 1e-13)")
        assert ep <= 1e-13
        # PCA space: the per-component calls on the projected column, bit for bit
        assert np.array_equal(pm[:, c], rows(multi_out, f"comp_m {c}")[0]) and np.array_equal(pv[:, c], rows(multi_out, f"comp_v {c}")[0])
        assert np.array_equal(pw[:, c], rows(multi_out, f"comp_w {c}")[0])
        st = rows(multi_out, f"stat {c}")[0]
        assert np.array_equal(st, rows(multi_out, f"comp_stat {c}")[0])
        assert st[2] == -0.5 * (st[0] + st[1] + NP * 1.8378770664093453)
        total += st[2]
    assert abs(rows(multi_out, "sum")[0, 0] - total) <= 1e-12 * abs(total)


@pytest.mark.gpu
def test_emulate_points_multi_draw(multi_out, campaign):
    sd, Xq, Y, Z, paths = campaign
    nr, nt = sd["nr"], sd["nt"]
    f = sd["evecs"] * np.sqrt(sd["evals"])
    for s in range(ND):
        dp, do = rows(multi_out, f"draw_pca {s}"), rows(multi_out, f"draw_obs {s}")
        assert dp.shape == (NP, nr) and do.shape == (NP, nt)
        for c in range(nr):
            assert np.array_equal(dp[:, c], rows(multi_out, f"comp_draw {c}")[s])
        want = sd["Y"].mean(axis=0) + dp @ f.T
        err = float(np.max(np.abs(do - want) / np.maximum(1.0, np.abs(want))))
        print(f"draw {s}: observable space against the numpy back-projection {err:.3e} (bar 1e-12)")
        assert err <= 1e-12


@pytest.mark.gpu
@pytest.mark.parametrize("pca", [False, True])
def test_validate_holdout_and_draw_emulator(tmp_path, multi_out, campaign, pca):
    """the C++ class returns the numbers of emulate_points_multi_holdout (PCA space whatever PcaOnly says) and of
    emulate_points_multi_draw in the space the class was opened in"""
    sd, Xq, Y, Z, paths = campaign
    exe = compile_driver(tmp_path, "emupp_joint_driver.cpp", True)
    out = subprocess.run([exe, G6SNAP, paths["q"], paths["y"], paths["z"]] + (["pca"] if pca else []), capture_output=True, text=True,
                         timeout=300)
    assert out.returncode == 0, out.stderr[-3000:]
    for a, b in (("m", "pca_m"), ("v", "pca_v"), ("w", "pca_w"), ("sum", "sum")):
        assert np.array_equal(rows(out.stdout, a), rows(multi_out, b))
    for c in range(sd["nr"]):
        assert np.array_equal(rows(out.stdout, f"stat {c}"), rows(multi_out, f"stat {c}"))
    for s in range(ND):
        assert np.array_equal(rows(out.stdout, f"draw {s}"), rows(multi_out, f"draw_{'pca' if pca else 'obs'} {s}"))


@pytest.mark.gpu
def test_cli_validate_holdout(campaign):
    """`interactive_emulator validate SNAPSHOT --holdout=FILE` against tests/jointref.py per PCA component: the stdout columns
    mean_c variance_c werr_c and the stderr summary (Mahalanobis distance, log density, rmse, totals), within the bars of the
    device tests; --quiet drops the header and the summary and keeps the lines"""
    sd, Xq, Y, Z, paths = campaign
    nr, d = sd["nr"], sd["d"]
    out = subprocess.run([build.CLI_BIN, "validate", G6SNAP, "--holdout=" + paths["holdout"]], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stderr[-3000:]
    lines = out.stdout.splitlines()
    header = [str(d)] + [f"param_{i}" for i in range(d)] + [str(3 * nr)] + [f"{n}_{c}" for c in range(nr) for n in ("mean", "variance", "werr")]
    assert lines[:len(header)] == header and len(lines) == len(header) + NP
    got = np.array([ln.split() for ln in lines[len(header):]], float)
    assert got.shape == (NP, 3 * nr)
    zobs = projected(sd, Y)
    tot_maha = tot_lp = 0.0
    for c, comp in enumerate(sd["models"]):
        ref = jointref.reference(comp["cov"], comp["order"], comp["X"], comp["z"], comp["thetas"], Xq, None, yobs=zobs[c])
        m = re.search(rf"# holdout component {c}: points {NP} mahalanobis (\S+) log_density (\S+) rmse (\S+)", out.stderr)
        assert m, out.stderr[-2000:]
        maha, lp, rmse = (float(x) for x in m.groups())
        e = jointref.errors(dict(werr=got[:, 3 * c + 2][None, :], maha=np.array([maha]), logdet=-2.0 * lp - maha - NP * jointref.LOG2PI),
                            ref, NP)
        em = float(np.max(np.abs(got[:, 3 * c] - ref["mean"]) / np.maximum(1.0, np.abs(ref["mean"]))))
        ev = float(np.max(np.abs(got[:, 3 * c + 1] - ref["var"])) / ref["kappa"])
        er = abs(rmse - np.sqrt(np.mean((zobs[c] - ref["mean"]) ** 2)))
        print(f"component {c}: mean {em:.3e} var {ev:.3e} {e} rmse {er:.3e}  (bars {RTOL:.1e})")
        assert em <= RTOL and ev <= RTOL and er <= RTOL and all(v <= RTOL for v in e.values())
        tot_maha += maha
        tot_lp += lp
    m = re.search(rf"# holdout total: components {nr} points {NP} mahalanobis (\S+) log_density (\S+)", out.stderr)
    assert m and abs(float(m.group(1)) - tot_maha) <= 1e-12 * tot_maha and abs(float(m.group(2)) - tot_lp) <= 1e-12 * abs(tot_lp)
    quiet = subprocess.run([build.CLI_BIN, "validate", G6SNAP, "--holdout=" + paths["holdout"], "--quiet"], capture_output=True, text=True,
                           timeout=300)
    assert quiet.returncode == 0 and quiet.stdout.splitlines() == lines[len(header):] and "# holdout" not in quiet.stderr


@pytest.mark.gpu
def test_cli_validate_without_holdout_is_the_leave_one_out_mode():
    """without --holdout the mode is the leave-one-out one (judged in tests/test_host_loo.py): its header, N lines of mean and
    variance per output, its own summary and nothing of the hold-out mode"""
    sd = parse_snapshot(open(G6SNAP).read().split())
    out = subprocess.run([build.CLI_BIN, "validate", G6SNAP], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stderr[-3000:]
    lines = out.stdout.splitlines()
    nhead = 1 + sd["d"] + 1 + 2 * sd["nt"]
    assert lines[nhead - 2:nhead] == [f"mean_{sd['nt'] - 1}", f"variance_{sd['nt'] - 1}"] and len(lines) == nhead + sd["N"]
    assert all(len(ln.split()) == 2 * sd["nt"] for ln in lines[nhead:])
    assert out.stderr.count("# loo output") == sd["nt"] and "holdout" not in out.stderr and "werr" not in out.stdout


def test_symbols_are_exported_and_usage_names_the_option():
    build.build_all()
    dev, host, epp = ctypes.CDLL(build.HIP_LIB), ctypes.CDLL(build.HOST_LIB), open(build.EPP_LIB, "rb").read()
    for name in ("gpemu_predict_joint_factor", "gpemu_predict_joint_factor_dev", "gpemu_predict_joint_draw", "gpemu_predict_joint_draw_dev",
                 "gpemu_predict_joint_release"):
        assert hasattr(dev, name) and name in abi.SYMBOLS
    for name in ("emulate_points_holdout", "emulate_points_holdout_enqueue", "emulate_points_holdout_collect", "emulate_points_draw",
                 "emulate_points_multi_holdout", "emulate_points_multi_draw", "gpemu_host_project_observations"):
        assert hasattr(host, name)
    assert b"ValidateHoldout" in epp and b"DrawEmulator" in epp          # (mangled: the names are part of the symbols)
    assert abi.PROF_JOINT == 12
    for name in ("predict_joint_factor", "predict_joint_factor_dev", "predict_joint_draw", "predict_joint_draw_dev", "predict_joint_release"):
        assert hasattr(abi.Context, name)
    hdr = open(os.path.join(ROOT, "include", "gpemu.h")).read()
    assert "#define GPEMU_PROF_JOINT   12" in hdr
    usage = subprocess.run([build.CLI_BIN], capture_output=True, text=True, timeout=60)
    assert usage.returncode != 0 and "--holdout=FILE" in usage.stderr
