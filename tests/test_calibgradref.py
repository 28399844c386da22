"""The references of the calibration gradient, on the CPU (no device):

  * calibgradref.direct64 against its 50-digit repeat on every input family the GPU tests use: the errors that
    calibgradref.BARS are 8 x of, recomputed here
  * the r x r form in float64 on gpemu_calib_project's tables against the same 50-digit numbers and, at every
    point, against direct64: inside the bars before a device runs
  * the formulas are derivatives: for smooth closed-form m_c(x), v_c(x) the 50-digit gradient agrees with 50-digit central
    differences of chi2 and logpdf (step 1e-15: truncation ~1e-30, rounding ~1e-35 relative; asserted 1e-20)
"""
import functools

import numpy as np
import pytest

import calibgradref as G
import calibref as R
from madaiemulator_amd import abi

NAMES = [a[0] for a in R.CASES] + ["special_" + k for k in R.SPECIALS]


@functools.lru_cache(maxsize=None)
def family(i):
    c = G.all_cases()[i]
    pts = R.mp_points(c)
    ref, scale = G.direct_mp(c, pts)
    g64, s64 = G.direct64(c)
    return c, pts, ref, scale, g64, s64


def test_dimensions_are_spread_over_the_cases():
    assert {G.dim_of(n) for n in NAMES} == set(G.DIMS)
    assert {G.dim_of(a[0]) for a in R.CASES if a[1] > 8} == set(G.DIMS)      # the two wide instantiations see every d


@pytest.mark.parametrize("i", range(len(NAMES)), ids=NAMES)
def test_float64_reference_against_50_digits(i):
    c, pts, ref, scale, g64, s64 = family(i)
    if c["name"] == "special_v_huge":
        assert np.all(np.isfinite(ref))                  # float64 cannot factor C at v = 1e30: 50 digits alone serve this family
        return
    e = G.err(g64[:, pts], ref, scale).max(axis=(1, 2))
    print(c["name"], c["d"], e)
    assert np.all(e <= G.MEASURED), (c["name"], e)
    assert np.all(G.err(s64[:, pts], scale, scale) <= 1e-12)                  # the two agree on the measure's denominator
    if c["name"] == "special_one_nan":
        assert np.all(np.isnan(g64[:, 17])) and np.all(np.isfinite(g64[:, :17]))


def test_bars_are_eight_times_the_measured_errors():
    assert np.array_equal(G.BARS, 8.0 * G.MEASURED)


@pytest.mark.parametrize("i", range(len(NAMES)), ids=NAMES)
def test_r_form_on_projected_tables_is_inside_the_bars(i):
    c, pts, ref, scale, g64, s64 = family(i)
    pj = abi.calib_project(c["ybar"], c["A"], c["z"], S=c["S"], sd=c["sd"])
    assert pj["status"] == abi.OK and pj["info"] == 0
    rf = G.rform64(c, pj)
    assert np.all(G.err(rf[:, pts], ref, scale) <= G.BARS[:, None, None])
    if c["name"] != "special_v_huge":
        e = G.err(rf, g64, s64).max(axis=(1, 2))
        print(c["name"], e)
        assert np.all(e <= G.BARS), e


def test_negative_variance_drops_its_gradient_terms():
    c = G.make("special_v_negative")
    g, _ = G.direct64(c)
    c2 = dict(c, gvar=7.0 * c["gvar"] + 1.0)
    g2, _ = G.direct64(c2)
    assert g.tobytes() == g2.tobytes()
    c0 = dict(c, var=np.where(c["var"] == 1e300, 1e300, 0.0), gvar=np.where(c["gvar"] == 1e300, 1e300, 0.0))
    g0, _ = G.direct64(c0)
    assert g.tobytes() == g0.tobytes()


@pytest.mark.parametrize("key", ["r3_nt3_rel", "r4_nt7_full", "r5_nt7"])
def test_the_formulas_are_derivatives(key):
    """m_c(x) = sin(a_c . x + p_c), v_c(x) = exp(b_c . x - 3) at 50 digits; central differences with a step of 1e-15"""
    import mpmath as mp
    mp.mp.dps = 50
    c = R.make_case(*next(a for a in R.CASES if a[0] == key))
    nr, d = c["nr"], 3
    rng = np.random.default_rng(11)
    a, p, b = rng.standard_normal((nr, d)), rng.uniform(0, 6, nr), 0.5 * rng.standard_normal((nr, d))
    x0 = [mp.mpf(float(t)) for t in rng.uniform(-1, 1, d)]
    f = mp.mpf
    arg = lambda k, x: mp.fsum(f(float(a[k, j])) * x[j] for j in range(d)) + f(float(p[k]))
    m_of = lambda x: [mp.sin(arg(k, x)) for k in range(nr)]
    v_of = lambda x: [mp.exp(mp.fsum(f(float(b[k, j])) * x[j] for j in range(d)) - 3) for k in range(nr)]
    gm = [[mp.cos(arg(k, x0)) * f(float(a[k, j])) for j in range(d)] for k in range(nr)]
    gv = [[v_of(x0)[k] * f(float(b[k, j])) for j in range(d)] for k in range(nr)]
    tabs = G._mp_tables(c)
    gc, gl, _, _ = G.grad_mp(c, m_of(x0), v_of(x0), gm, gv, tabs)
    h = mp.mpf(10) ** -15
    for j in range(d):
        xp = [x0[i] + (h if i == j else 0) for i in range(d)]
        xm = [x0[i] - (h if i == j else 0) for i in range(d)]
        cp, lp = G.stat_mp(c, m_of(xp), v_of(xp), tabs)
        cm, lm = G.stat_mp(c, m_of(xm), v_of(xm), tabs)
        for name, got, fd in (("chi2", gc[j], (cp - cm) / (2 * h)), ("logpdf", gl[j], (lp - lm) / (2 * h))):
            rel = abs(got - fd) / abs(fd)
            print(key, j, name, mp.nstr(got, 20), mp.nstr(rel, 3))
            assert rel <= mp.mpf(10) ** -20, (key, j, name)
    # stat_mp is calibref.direct_mp's chi2 and logpdf before the rounding: the two agree at float64 inputs
    c1 = dict(c, M=1, mean=np.array([[float(t)] for t in m_of(x0)]), var=np.array([[float(t)] for t in v_of(x0)]))
    ref, _ = R.direct_mp(c1, [0])
    chi2, logpdf = G.stat_mp(c, [f(float(t)) for t in c1["mean"][:, 0]], [f(float(t)) for t in c1["var"][:, 0]], tabs)
    assert float(chi2) == ref[0, 0] and float(logpdf) == ref[1, 0]


@pytest.mark.parametrize("extra,why", [(["--gradient", "--binary"], "--gradient"), (["--gradient"], None)])
def test_cli_gradient_flag_is_checked_before_any_device(tmp_path, extra, why):
    """--gradient with --binary, or outside `implausibility`: refused by the parser; a good command line fails later, if at all"""
    import os
    import subprocess
    from madaiemulator_amd import build
    build.build_all()
    snap = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "g6_multi_snapshot.txt")
    f = tmp_path / "obs.dat"
    f.write_text("6\n" + "".join(f"{1.0 + t} 0.1\n" for t in range(6)))
    out = subprocess.run([build.CLI_BIN, "implausibility", snap, f"--observations={f}"] + extra, input="", capture_output=True, text=True,
                         timeout=120)
    if why:
        assert out.returncode == 1 and why in out.stderr and out.stdout == ""
        other = subprocess.run([build.CLI_BIN, "print_thetas", snap, "--gradient"], input="", capture_output=True, text=True, timeout=120)
        assert other.returncode == 1 and why in other.stderr and other.stdout == ""
    else:
        assert "--gradient" not in out.stderr
        assert out.returncode == 0 or "HIP device" in out.stderr or "gpemu error" in out.stderr, out.stderr
