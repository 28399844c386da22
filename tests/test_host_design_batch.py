"""Greedy batches of K runs above the kernels: the ctypes bindings and the argument checks of the device entries
(no device needed), the command line's argument errors (raised before a device is touched), and -- marked gpu -- the C host
layer (libEmuMI.so: emulate_design_batch, emulate_design_batch_multi), the C++ class (emulator::QueryEmulatorDesignBatch) and
the CLI's `design --batch=K` against the device entry on contexts of the same components with the back-projection's weights.

The weights.  One run observes every PCA component; the summed IMSE of the outputs is sum_t sum_c B_tc^2 s_all^c, so the
quantity a pick maximises is sum_c weight_c gain_c with weight_c = sum_t B_tc^2 (all 1 in PCA space).  The test forms B from the
snapshot's decimals in numpy; the host layer takes B^2 from its back-projection, so in observable space the gains agree to a few
ulp (WEIGHT_RTOL = 8 * 2^-52 on each weight), not bit for bit; in PCA space and for a single emulator they are the device's
bits."""
import ctypes as C
import subprocess

import numpy as np
import pytest

from madaiemulator_amd import abi
from test_host_design import component_state, loadings, setting
from test_host_mean import compile_driver
from test_host_sens import cli, rows, two_components, write_box          # noqa: F401  (fixtures)

EPS = 2.0 ** -52
WEIGHT_RTOL = 8 * EPS
K = 4


# ---------------------------------------------------------------------------------------------------- no device
def test_abi_binds_the_entries():
    L = abi.load()
    for name in ("gpemu_design_batch", "gpemu_design_batch_dev", "gpemu_test_design_batch_state"):
        assert name in abi.SYMBOLS and getattr(L, name).restype is C.c_int
    assert len(abi.SYMBOLS["gpemu_design_batch"][1]) == 13 and len(abi.SYMBOLS["gpemu_design_batch_dev"][1]) == 13
    assert callable(abi.design_batch) and callable(abi.design_batch_dev) and hasattr(abi.Context, "design_batch_state")


def test_null_and_range_arguments_without_a_device():
    """GPEMU_ERR_ARG for NULL pointers and counts out of range before a context is looked at: the handles here are not contexts"""
    L, p = abi.load(), abi._p
    fake = (C.c_char * 64)()
    hs = (C.c_void_p * 2)(C.addressof(fake), C.addressof(fake))
    lo, hi, xq, pg = np.zeros(2), np.ones(2), np.zeros((8, 2)), np.zeros(4)
    pick = np.zeros(300, dtype=np.int32)
    pk = pick.ctypes.data_as(C.c_void_p)
    for fn in (L.gpemu_design_batch, L.gpemu_design_batch_dev):
        x = p(xq) if fn is L.gpemu_design_batch else xq.ctypes.data_as(C.c_void_p)
        g = p(pg) if fn is L.gpemu_design_batch else pg.ctypes.data_as(C.c_void_p)
        assert fn(None, 2, None, p(lo), p(hi), 8, x, 4, pk, g, None, None, None) == abi.ERR_ARG
        assert fn(hs, 0, None, p(lo), p(hi), 8, x, 4, pk, g, None, None, None) == abi.ERR_ARG
        assert fn(hs, -1, None, p(lo), p(hi), 8, x, 4, pk, g, None, None, None) == abi.ERR_ARG
        assert fn((C.c_void_p * 2)(C.addressof(fake), None), 2, None, p(lo), p(hi), 8, x, 4, pk, g, None, None, None) == abi.ERR_ARG
        assert fn(hs, 2, None, None, p(hi), 8, x, 4, pk, g, None, None, None) == abi.ERR_ARG
        assert fn(hs, 2, None, p(lo), None, 8, x, 4, pk, g, None, None, None) == abi.ERR_ARG
        assert fn(hs, 2, None, p(lo), p(hi), 8, None, 4, pk, g, None, None, None) == abi.ERR_ARG
        assert fn(hs, 2, None, p(lo), p(hi), 8, x, 4, None, g, None, None, None) == abi.ERR_ARG
        assert fn(hs, 2, None, p(lo), p(hi), 8, x, 4, pk, None, None, None, None) == abi.ERR_ARG
        for M, nb in ((0, 1), (-3, 1), (16385, 4), (8, 0), (8, -1), (8, 9), (300, 257)):
            assert fn(hs, 2, None, p(lo), p(hi), M, x, nb, pk, g, None, None, None) == abi.ERR_ARG, (M, nb)
    lam = np.zeros(4)
    assert L.gpemu_test_design_batch_state(None, 1, 1, p(lam), p(lam), p(lam)) == abi.ERR_ARG


def test_cli_argument_errors(cli, tmp_path):
    """--batch=0, a negative or non-numeric K, --batch with --best: refused before the snapshot is opened (it does not exist)"""
    def go(*args):
        return subprocess.run([cli, "design", str(tmp_path / "no_such_snapshot.txt")] + list(args), input="0.5 0.5\n", capture_output=True,
                              text=True, timeout=60, cwd=tmp_path)

    for bad in ("--batch=0", "--batch=-2", "--batch=three", "--batch=2x", "--batch=", "--batch=257"):
        r = go(bad)
        assert r.returncode != 0 and "--batch=K needs a number" in r.stderr and r.stdout == "", (bad, r.stderr)
    r = go("--batch=2", "--best=2")
    assert r.returncode != 0 and "exclude each other" in r.stderr and r.stdout == ""
    assert "Error opening file" in go("--batch=2").stderr                                    # a good K gets as far as the snapshot
    u = subprocess.run([cli, "no_such_mode", "x"], capture_output=True, text=True, timeout=60, cwd=tmp_path)
    assert "[--batch=K]" in u.stderr


# ---------------------------------------------------------------------------------------------------- on the device
@pytest.fixture(scope="module")
def batch_driver(tmp_path_factory):
    return compile_driver(tmp_path_factory.mktemp("drv"), "host_design_batch_driver.c", False)


@pytest.fixture(scope="module")
def second_ctx():
    ctx = abi.Context(0)
    yield ctx
    ctx.close()


def picks_of(text, tag="pick"):
    r = rows(text, tag)
    return r[:, -2].astype(int), r[:, -1]


@pytest.mark.gpu
@pytest.mark.parametrize("pca", [0, 1])
def test_host_entries_against_the_device_entry(batch_driver, two_components, gpu_ctx, second_ctx, tmp_path, pca):
    tc = two_components
    lo, hi, Xq, box, pts = setting(tc, tmp_path)
    out = subprocess.run([batch_driver, tc["path"], box, pts, str(pca), str(K)], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stderr[-3000:]
    ctxs = [gpu_ctx, second_ctx]
    for c, ctx in enumerate(ctxs):
        component_state(ctx, tc, c)
    comp = rows(out.stdout, "comp")
    for c, ctx in enumerate(ctxs):                                                           # one emulator: the device's bits
        dev = abi.design_batch([ctx], lo, hi, Xq, K)
        mine = comp[comp[:, 0] == c]
        assert np.array_equal(mine[:, 2].astype(int), dev["pick"]) and np.array_equal(mine[:, 3], dev["pick_gain"])
    weight = (loadings(tc, pca) ** 2).sum(axis=0)
    dev = abi.design_batch(ctxs, lo, hi, Xq, K, weight)
    pick, gain = picks_of(out.stdout)
    assert np.array_equal(pick, dev["pick"]) and len(set(pick)) == K
    if pca:
        assert np.array_equal(gain, dev["pick_gain"])
    else:
        assert np.all(np.abs(gain - dev["pick_gain"]) <= WEIGHT_RTOL * np.abs(dev["pick_gain_ctx"]) @ weight)
    # the first pick is the arg-max of emulate_design_gain_multi's total; the candidate repeated in the input is picked once at most
    first = sum(w * ctx.design_gain(lo, hi, Xq)["gain"] for w, ctx in zip(weight, ctxs))
    assert pick[0] == int(np.argmax(first))
    assert not (0 in pick[:2] and len(Xq) - 1 in pick[:2])


@pytest.mark.gpu
@pytest.mark.parametrize("pca", [0, 1])
def test_cpp_method(batch_driver, two_components, tmp_path, pca):
    tc = two_components
    lo, hi, Xq, box, pts = setting(tc, tmp_path)
    exe = compile_driver(tmp_path, "emupp_design_batch_driver.cpp", True)
    cpp = subprocess.run([exe, tc["path"], box, pts, str(K)] + (["pca"] if pca else []), capture_output=True, text=True, timeout=300)
    c = subprocess.run([batch_driver, tc["path"], box, pts, str(pca), str(K)], capture_output=True, text=True, timeout=300)
    assert cpp.returncode == 0 and c.returncode == 0, cpp.stderr[-3000:] + c.stderr[-3000:]
    assert np.array_equal(rows(cpp.stdout, "pick"), rows(c.stdout, "pick")) and len(rows(c.stdout, "pick")) == K
    bad = subprocess.run([exe, tc["path"], box, pts, "0"], capture_output=True, text=True, timeout=300)
    assert bad.returncode != 0 and "QueryEmulatorDesignBatch" in bad.stderr


@pytest.mark.gpu
def test_cli_batch(cli, batch_driver, two_components, gpu_ctx, tmp_path):
    """the K picks in pick order: index, the point, the conditional gain, the integrated variance after the pick"""
    tc = two_components
    lo, hi, Xq, box, pts = setting(tc, tmp_path)
    text = open(pts).read()

    def go(*args):
        return subprocess.run([cli, "design", tc["path"], f"--box={box}"] + list(args), input=text, capture_output=True, text=True, timeout=300,
                              cwd=tmp_path)

    drv = subprocess.run([batch_driver, tc["path"], box, pts, "0", str(K)], capture_output=True, text=True, timeout=300)
    assert drv.returncode == 0, drv.stderr[-3000:]
    pick, gain = picks_of(drv.stdout)
    s_all = []
    for c in range(2):
        component_state(gpu_ctx, tc, c)
        s_all.append(gpu_ctx.sens_post(lo, hi)["s_all"])
    imse = float(((loadings(tc, 0) ** 2) @ np.array(s_all)).sum())
    out = go(f"--batch={K}")
    assert out.returncode == 0, out.stderr[-3000:]
    lines = out.stdout.splitlines()
    assert lines[0] == "# index param_0 param_1 conditional_imse_reduction imse_after" and len(lines) == 1 + K
    vals = np.array([ln.split() for ln in lines[1:]], float)
    assert np.array_equal(vals[:, 0].astype(int), pick) and np.array_equal(vals[:, 1:3], Xq[pick]) and np.array_equal(vals[:, 3], gain)
    assert np.all(np.abs(vals[:, 4] - (imse - np.cumsum(gain))) <= 1e-12 * imse)
    assert np.all(np.diff(vals[:, 4]) < 0) and vals[-1, 4] > 0
    q = go(f"--batch={K}", "--quiet")
    assert q.returncode == 0 and q.stdout.splitlines() == lines[1:]
    assert go(f"--batch={len(Xq) + 1}").returncode != 0                                       # more picks than candidates
    full = go(f"--batch={len(Xq)}", "--quiet")
    assert full.returncode == 0 and sorted(int(ln.split()[0]) for ln in full.stdout.splitlines()) == list(range(len(Xq)))
