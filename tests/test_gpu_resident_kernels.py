"""The kernels that read the device-resident factor, ONE launch at a time through gpemu_test_resident_launch -- production's
launchers on operands of the test's: skinny_nt_kernel and gemv_tri_kernel (the few-query and one-query prediction
products), loo_colsq_kernel, loo_finish_kernel, lgo_gather_kernel, lgo_stage_kernel, lgo_finish_kernel, and the chunk tail
of gpemu_lgo with one indefinite matrix among good ones.  What they share is "the trap" (DESIGN.md 4.7 / 4.13): above its
diagonal L^-1 holds exact zeros only inside the diagonal tiles and nothing specified further out.  Here every element the
contract says is not read is NaN, as is every output before the launch (one payload, so UNCHANGED is a comparison of bytes):
a NaN in a VALUE element is a mask that reads too far.  Reference, classes and bars: tests/resref.py (checked on these cases
without a device by tests/test_resref.py).  Every test prints its worst error / bar."""
import numpy as np
import pytest

import lgoref
import resref as R
from madaiemulator_amd import abi

pytestmark = pytest.mark.gpu
LD = R.LD


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64).ravel()


def check(name, got, before, want, bar, cls):
    """UNCHANGED elements keep their bytes; VALUE elements are no NaN (unless NaN is wanted) and within their bar (a zero bar:
    equal) -> the worst error / bar"""
    got, before, cls = np.asarray(got).ravel(), np.asarray(before).ravel(), np.asarray(cls).ravel()
    want, bar = np.asarray(want, dtype=LD).ravel(), np.asarray(bar, dtype=LD).ravel()
    un = cls == R.UNCHANGED
    moved = np.flatnonzero(un & (bits(got) != bits(before)))
    assert moved.size == 0, f"{name}: {moved.size} elements outside the contract were written, first at {moved[:8]}"
    v = cls == R.VALUE
    wn = np.isnan(np.asarray(want, dtype=np.float64))
    assert np.all(np.isnan(got[v & wn])), f"{name}: NaN wanted"
    v &= ~wn
    nan = np.flatnonzero(v & np.isnan(got))
    assert nan.size == 0, f"{name}: {nan.size} NaN among the values (a read beside the operands), first at {nan[:8]}"
    r = R.ratio(np.abs(np.asarray(got[v], dtype=LD) - want[v]), bar[v])
    assert r <= 1.0, f"{name}: error / bar = {r}"
    return r


# ------------------------------------------------------------------ the prediction products
@pytest.mark.parametrize("kernel,M", [("skinny", 1), ("skinny", 2), ("skinny", 16), ("gemv", 1)])
@pytest.mark.parametrize("kind", R.KINDS)
@pytest.mark.parametrize("Np", sorted(R.PRODUCT_SPLITS))
def test_products(gpu_ctx, kernel, M, kind, Np):
    one = kernel == "gemv"
    case = R.product_case(1000 + Np + M, Np, M, kind, one_query=one)
    K, ntot = case["K"], case["ntot"]
    vrows, ldv = 18, ntot + 6                      # two guard rows per slice, six guard columns per row
    full, fullbar = R.product_reference(case, 1, K)
    worst = 0.0
    for nslice, klen in R.PRODUCT_SPLITS[Np]:
        vp0 = R.nans(nslice, vrows, ldv)
        out, _ = gpu_ctx.test_resident_launch(abi.RES_GEMV if one else abi.RES_SKINNY, kq=case["kq"], lin=case["lin"], vp=vp0,
                                              ldk=case["ldk"], ld=case["ld"], ldv=ldv, vrows=vrows, K=K, ntri=case["ntri"], ntot=ntot,
                                              nslice=nslice, klen=klen)
        assert np.array_equal(bits(out["kq"]), bits(case["kq"])) and np.array_equal(bits(out["lin"]), bits(case["lin"]))
        vp = out["vp"].reshape(nslice, vrows, ldv)
        want, bar = R.product_reference(case, nslice, klen)
        W, B = np.zeros((nslice, vrows, ldv), dtype=LD), np.zeros((nslice, vrows, ldv), dtype=LD)
        W[:, :16, :ntot], B[:, :16, :ntot] = want, bar
        if kind == "int":
            B[:] = 0                               # integers: the numpy product is the only right answer
        r = check(f"{kernel} M={M} {kind} Np={Np} nslice={nslice} klen={klen}", vp, vp0, W, B, R.product_classes(nslice, vrows, ldv, ntot, one))
        rows = 1 if one else 16
        tot = np.asarray(vp[:, :rows, :ntot], dtype=LD).sum(axis=0)
        tb = np.zeros_like(tot) if kind == "int" else bar[:, :rows].sum(axis=0)
        r = max(r, R.ratio(np.abs(tot - full[0, :rows]), tb))
        assert r <= 1.0, f"sum over {nslice} slices of {klen} against the unsplit product: error / bar = {r}"
        worst = max(worst, r)
    print(f"products {kernel} M={M} {kind} Np={Np}: worst error / bar {worst:.3f}")


# ------------------------------------------------------------------ leave-one-out
@pytest.mark.parametrize("N", R.COLSQ_N)
def test_loo_colsq(gpu_ctx, N):
    lin, Np, ld = R.linv_case(100 + N, N)
    part0 = R.nans(R.nchunks_of(N), Np)
    out, _ = gpu_ctx.test_resident_launch(abi.RES_LOO_COLSQ, lin=lin, part=part0, ld=ld, N=N, Np=Np)
    want, bar, cls = R.colsq_reference(lin, N, Np)
    r = check(f"loo_colsq N={N}", out["part"], part0, want, bar, cls)
    print(f"loo_colsq N={N}: worst error / bar {r:.3f}")


@pytest.mark.parametrize("N,nreg", R.LOO_FINISH_CASES)
def test_loo_finish(gpu_ctx, N, nreg):
    c = R.loo_finish_case(200 + N, N, nreg)
    Np = c["Np"]
    mean0, var0 = R.nans(Np), R.nans(Np)
    out, _ = gpu_ctx.test_resident_launch(abi.RES_LOO_FINISH, part=c["part"], lin=c["lin"], betaq=c["betaq"], y=c["y"], mean=mean0,
                                          var=var0, ld=c["ld"], N=N, Np=Np, nreg=nreg)
    ref = R.loo_finish_reference(c["part"], c["lin"][Np, :N], c["lin"][Np + 1:, :N].T, c["betaq"][nreg:].reshape(nreg, nreg), c["y"], N, Np)
    cls = np.where(np.arange(Np) < N, R.VALUE, R.UNCHANGED)
    pad = np.zeros(Np - N, dtype=LD)
    rm = check(f"loo_finish mean N={N} nreg={nreg}", out["mean"], mean0, np.concatenate([ref["mean"], pad]), np.concatenate([ref["bar_mean"], pad]), cls)
    rv = check(f"loo_finish var N={N} nreg={nreg}", out["var"], var0, np.concatenate([ref["var"], pad]), np.concatenate([ref["bar_var"], pad]), cls)
    print(f"loo_finish N={N} nreg={nreg}: worst error / bar mean {rm:.3f} var {rv:.3f}")


# ------------------------------------------------------------------ leave-group-out
@pytest.mark.parametrize("N,sizes,bp", R.GATHER_CASES)
def test_lgo_gather(gpu_ctx, N, sizes, bp):
    tab = R.group_tables(N, sizes, 300 + N, bp)
    lin, Np, ld = R.linv_case(310 + N, N)
    G = len(sizes)
    for g0, nbc in ((0, G), (0, G // 2), (G // 2, G - G // 2)):          # one chunk; the two chunks of a split call
        z0 = R.nans(nbc * bp, Np)
        out, _ = gpu_ctx.test_resident_launch(abi.RES_LGO_GATHER, lin=lin, z=z0, colrow=tab["colrow"], bsize=tab["bsize"], ld=ld, N=N,
                                              Np=Np, g0=g0, nbc=nbc, bp=bp, ngroups=G)
        Z = out["z"].reshape(nbc * bp, Np)
        want = R.gather_reference(lin, N, Np, tab, g0, nbc)
        assert not np.isnan(Z).any(), f"gather N={N} g0={g0}: NaN at {np.argwhere(np.isnan(Z))[:6]}"
        assert np.array_equal(Z, want), f"gather N={N} g0={g0}: {np.argwhere(Z != want)[:6]}"
    print(f"lgo_gather N={N} sizes={sizes}: exact")


@pytest.mark.parametrize("N,bp,sizes,nreg,g0", R.STAGE_CASES)
def test_lgo_stage(gpu_ctx, N, bp, sizes, nreg, g0):
    c = R.stage_case(400 + nreg, N, bp, sizes, nreg, g0)
    tab = c["tab"]
    out, _ = gpu_ctx.test_resident_launch(abi.RES_LGO_STAGE, t=c["t"], lin=c["lin"], betaq=c["betaq"], members=tab["members"],
                                          moff=tab["moff"], bsize=tab["bsize"], nmembers=tab["members"].size, ld=c["ld"], N=N, Np=c["Np"],
                                          nreg=nreg, g0=g0, nbc=c["nbc"], bp=bp, ngroups=len(sizes), tstride=c["tstride"])
    want, bar, cls = R.stage_reference(c)
    r = check(f"lgo_stage bp={bp} nreg={nreg} g0={g0}", out["t"], c["t"], want, bar, cls)
    print(f"lgo_stage bp={bp} sizes={sizes[g0:]} nreg={nreg}: worst error / bar {r:.3f}")


@pytest.mark.parametrize("optional", [True, False])
@pytest.mark.parametrize("N,bp,sizes,g0,words", R.FINISH_CASES)
def test_lgo_finish(gpu_ctx, N, bp, sizes, g0, words, optional):
    c = R.finish_case(500 + bp + g0, N, bp, sizes, g0, words)
    tab, G = c["tab"], len(sizes)
    pre = dict(mean=R.nans(N + 3), var=R.nans(N + 3), werr=R.nans(N + 3) if optional else None, stat=R.nans(3 * G) if optional else None)
    info0 = np.full(G, -77, dtype=np.int32)
    out, _ = gpu_ctx.test_resident_launch(abi.RES_LGO_FINISH, t=c["t"], res=c["res"], y=c["y"], info=c["info"], info_out=info0,
                                          members=tab["members"], moff=tab["moff"], bsize=tab["bsize"], nmembers=tab["members"].size,
                                          N=N, g0=g0, nbc=c["nbc"], bp=bp, ngroups=G, tstride=c["tstride"], **pre)
    assert np.array_equal(bits(out["t"]), bits(c["t"]))
    ref = R.finish_reference(c)
    worst = {}
    for k in ("mean", "var", "werr") if optional else ("mean", "var"):
        want, bar, cls = (np.concatenate([a, np.zeros(3, dtype=a.dtype)]) for a in ref[k])
        worst[k] = check(f"lgo_finish {k} bp={bp} g0={g0}", out[k], pre[k], want, bar, cls)
    if optional:
        worst["stat"] = check(f"lgo_finish stat bp={bp} g0={g0}", out["stat"], pre["stat"], *ref["stat"])
    want, cls = ref["info_out"]
    assert np.array_equal(out["info_out"], np.where(cls == R.VALUE, want, info0)), out["info_out"]
    print(f"lgo_finish bp={bp} sizes={sizes[g0:]} optional={optional}: worst error / bar {worst}")


@pytest.fixture(scope="module")
def tail_good(gpu_ctx):
    """the three positive definite matrices, their longdouble references, and the device's outputs for them"""
    mats = [R.spd(600 + g, b) for g, b in enumerate(R.TAIL_SIZES)]
    case = R.tail_case(610, R.TAIL_N, R.TAIL_BP, R.TAIL_SIZES, mats)
    refs = [R.tail_reference(case, g) for g in range(3)]
    out, rc = run_tail(gpu_ctx, case)
    return dict(mats=mats, case=case, refs=refs, out=out, rc=rc)


def run_tail(ctx, case):
    tab, N, G = case["tab"], case["N"], case["ngroups"]
    out, rc = ctx.test_resident_launch(abi.RES_LGO_TAIL, allow=(abi.ERR_NOT_PD,), t=case["t"], y=case["y"], mean=R.nans(N), var=R.nans(N),
                                       werr=R.nans(N), stat=R.nans(3 * G), info_out=np.full(G, -77, dtype=np.int32), members=tab["members"],
                                       moff=tab["moff"], bsize=tab["bsize"], nmembers=tab["members"].size, N=N,
                                       g0=0, nbc=G, bp=case["bp"], ngroups=G, tstride=case["tstride"])
    return out, rc


def tail_group(out, case, g):
    B, G = case["tab"]["groups"][g], case["ngroups"]
    return dict(mean=out["mean"][B], var=out["var"][B], werr=out["werr"][B], maha=float(out["stat"][g]), logdet=float(out["stat"][G + g]),
                logpdf=float(out["stat"][2 * G + g]))


def tail_errors(out, case, refs, groups):
    worst = {}
    for g in groups:
        ref, kappa, _ = refs[g]
        got = tail_group(out, case, g)
        assert not any(np.isnan(v).any() for v in got.values()), (g, got)
        e = lgoref.errors(got, ref, kappa)
        assert all(v <= lgoref.RTOL for v in e.values()), (g, e)      # (a NaN measure fails here)
        worst = {k: max(worst.get(k, 0.0), v) for k, v in e.items()}
    return worst


def test_lgo_tail_all_positive_definite(gpu_ctx, tail_good):
    assert tail_good["rc"] == abi.OK
    out, case = tail_good["out"], tail_good["case"]
    assert np.array_equal(out["info_out"], [0, 0, 0])
    worst = tail_errors(out, case, tail_good["refs"], (0, 1, 2))
    left_out = np.isin(np.arange(case["N"]), np.concatenate(case["tab"]["groups"]))
    for k in ("mean", "var", "werr"):
        assert np.all(R.is_prefill(out[k])[~left_out]) and not np.isnan(out[k][left_out]).any()
    print(f"lgo_tail, three good groups: worst error / RTOL { {k: v / lgoref.RTOL for k, v in worst.items()} }")


@pytest.mark.parametrize("p", R.TAIL_P)
def test_lgo_tail_with_an_indefinite_neighbour(gpu_ctx, tail_good, p):
    """the not-positive-definite branch of leave-group-out: the failed group gets its pivot's row and NaN, its neighbours in
    the lock-step batch keep their bits, and the status is gpemu_lgo's"""
    mats = list(tail_good["mats"])
    mats[1] = R.make_indefinite(mats[1], p)
    case = R.tail_case(610, R.TAIL_N, R.TAIL_BP, R.TAIL_SIZES, mats)
    assert R.tail_reference(case, 1)[2] == p
    out, rc = run_tail(gpu_ctx, case)
    assert rc == abi.ERR_NOT_PD
    assert b"leave-group-out" in gpu_ctx.L.gpemu_last_error(gpu_ctx.h)
    assert np.array_equal(out["info_out"], [0, p, 0]), out["info_out"]
    bad = tail_group(out, case, 1)
    assert all(np.all(np.isnan(v)) for v in bad.values()), bad
    worst = tail_errors(out, case, tail_good["refs"], (0, 2))
    good = tail_good["out"]
    for g in (0, 2):
        a, b = tail_group(out, case, g), tail_group(good, tail_good["case"], g)
        assert all(np.array_equal(bits(a[k]), bits(b[k])) for k in a), f"group {g} changed with a failed neighbour"
    print(f"lgo_tail, pivot {p} of the middle group fails: worst error / RTOL of the others { {k: v / lgoref.RTOL for k, v in worst.items()} }")


# ------------------------------------------------------------------ the entry's refusals
def test_refusals(gpu_ctx):
    def refused(op, args, **change):
        with pytest.raises(abi.GpemuError) as e:
            gpu_ctx.test_resident_launch(op, **dict(args, **change))
        assert e.value.code == abi.ERR_ARG, (op, change)

    L, C = gpu_ctx.L, abi.C
    assert L.gpemu_test_resident_launch(gpu_ctx.h, None) == abi.ERR_ARG
    assert L.gpemu_test_resident_launch(None, C.byref(abi.ResidentLaunchArgs())) == abi.ERR_ARG
    case = R.product_case(1, 192, 1, "int")
    prod = dict(kq=case["kq"], lin=case["lin"], vp=R.nans(2, 16, 256), ldk=case["ldk"], ld=case["ld"], ldv=256, vrows=16, K=192, ntri=192,
                ntot=256, nslice=2, klen=96)
    gpu_ctx.test_resident_launch(abi.RES_SKINNY, **prod)
    refused(8, prod)
    refused(-1, prod)
    for change in (dict(kq=None), dict(lin=None), dict(vp=None), dict(klen=88), dict(klen=80), dict(nslice=1), dict(K=200), dict(ntot=250),
                   dict(ntri=100), dict(ntri=272), dict(ldk=197), dict(ld=201), dict(ld=188), dict(ldv=255), dict(vrows=15),
                   dict(vp=R.nans(2 * 16 * 256 - 1)), dict(lin=case["lin"][:-1]), dict(kq=case["kq"][:15]), dict(nslice=0)):
        refused(abi.RES_SKINNY, prod, **change)
        refused(abi.RES_GEMV, prod, **change)
    lin, Np, ld = R.linv_case(2, 130)
    colsq = dict(lin=lin, part=R.nans(3, Np), ld=ld, N=130, Np=Np)
    gpu_ctx.test_resident_launch(abi.RES_LOO_COLSQ, **colsq)
    for change in (dict(N=0), dict(N=Np + 1), dict(Np=190), dict(ld=ld + 1), dict(ld=Np - 2), dict(part=R.nans(3 * Np - 1)), dict(lin=lin[:100]),
                   dict(part=None)):
        refused(abi.RES_LOO_COLSQ, colsq, **change)
    c = R.loo_finish_case(3, 130, 4)
    fin = dict(part=c["part"], lin=c["lin"], betaq=c["betaq"], y=c["y"], mean=R.nans(130), var=R.nans(130), ld=c["ld"], N=130, Np=192, nreg=4)
    gpu_ctx.test_resident_launch(abi.RES_LOO_FINISH, **fin)
    for change in (dict(nreg=0), dict(nreg=64, betaq=R.nans(64 + 64 * 64)), dict(mean=R.nans(129)), dict(lin=c["lin"][:-1]), dict(y=None), dict(betaq=None), dict(var=None)):
        refused(abi.RES_LOO_FINISH, fin, **change)
    tab = R.group_tables(130, (63, 65), 4, 128)
    gat = dict(lin=lin, z=R.nans(2 * 128, Np), colrow=tab["colrow"], bsize=tab["bsize"], ld=ld, N=130, Np=Np, g0=0, nbc=2, bp=128, ngroups=2)
    gpu_ctx.test_resident_launch(abi.RES_LGO_GATHER, **gat)
    far = tab["colrow"].copy()
    far[5] = 2 * 128
    for change in (dict(bp=100), dict(bp=0), dict(nbc=0), dict(nbc=3), dict(g0=1), dict(g0=-1), dict(bp=64), dict(colrow=far), dict(colrow=None),
                   dict(bsize=None), dict(z=R.nans(2 * 128 * Np - 1)), dict(bsize=np.array([63, 0], dtype=np.int32))):
        refused(abi.RES_LGO_GATHER, gat, **change)
    s = R.stage_case(5, 130, 64, (1, 63, 64), 4, 0)
    tb = s["tab"]
    stg = dict(t=s["t"], lin=s["lin"], betaq=s["betaq"], members=tb["members"], moff=tb["moff"], bsize=tb["bsize"], nmembers=tb["members"].size,
               ld=s["ld"], N=130, Np=192, nreg=4, g0=0, nbc=3, bp=64, ngroups=3, tstride=s["tstride"])
    gpu_ctx.test_resident_launch(abi.RES_LGO_STAGE, **stg)
    out_of_range = tb["members"].copy()
    out_of_range[2] = 130
    for change in (dict(tstride=s["tstride"] + 1), dict(tstride=R.tall_rows(64) * 64 - 2), dict(t=s["t"][:-11]), dict(members=out_of_range),
                   dict(nmembers=tb["members"].size - 1), dict(members=None), dict(moff=None), dict(moff=np.array([0, 1, -1], dtype=np.int32))):
        refused(abi.RES_LGO_STAGE, stg, **change)
        refused(abi.RES_LGO_TAIL, dict(stg, y=np.zeros(130), mean=R.nans(130), var=R.nans(130), info_out=np.zeros(3, dtype=np.int32)), **change)
    f = R.finish_case(6, 130, 64, (63, 64, 1), 0, (R.INFO_NONE,) * 3)
    tb = f["tab"]
    fa = dict(t=f["t"], res=f["res"], y=f["y"], info=f["info"], info_out=np.zeros(3, dtype=np.int32), mean=R.nans(130), var=R.nans(130),
              members=tb["members"], moff=tb["moff"], bsize=tb["bsize"], nmembers=tb["members"].size, N=130, g0=0, nbc=3, bp=64,
              ngroups=3, tstride=f["tstride"])
    gpu_ctx.test_resident_launch(abi.RES_LGO_FINISH, **fa)
    for change in (dict(info=None), dict(info_out=None), dict(res=None), dict(y=None), dict(mean=None), dict(mean=R.nans(129), var=R.nans(129)), dict(t=None)):
        refused(abi.RES_LGO_FINISH, fa, **change)
