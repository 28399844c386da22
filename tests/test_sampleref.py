"""The ensemble sampler's replica (tests/sampleref.py) and the library's host-side generator, on the CPU (no device):

  * Philox4x32-10 against known answers; U strictly inside (0, 1) and equal to (n + 0.5) 2^-52
  * gpemu_philox4x32 and gpemu_sample_uniforms (libgpemu_hip.so, loaded without a device) against the replica, bit for bit
  * the replica samples correlated Gaussians at d = 1, 3, 5 and a flat likelihood in a box: the test's own seed inside
    sampleref.BARS, which are twice the largest error over 16 other seeds -- measure_bars below is what measured them, and
    test_bars_hold_for_their_seeds repeats a part of the measurement
  * the integrated autocorrelation time on AR(1) series against (1 + phi) / (1 - phi), the replica's and the host layer's
    gpemu_host_autocorr_time (libEmuMI.so, no device)
  * the replica on the posteriors the GPU end-to-end tests tabulate (tests/golden/sample_grid.npz, written by
    tests/test_gpu_sample.py with GPEMU_SAMPLE_GRID_OUT set): the bars those tests assert the device's chain against
"""
import ctypes
import os

import numpy as np
import pytest

import sampleref as R
from madaiemulator_amd import abi, build

GRID = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "sample_grid.npz")
GRID_D = {"e2e1": 1, "e2e2": 2}

KNOWN = [
    ((0, 0, 0, 0), (0, 0), (0x6627e8d5, 0xe169c58d, 0xbc57ac4c, 0x9b00dbd8)),
    ((0xffffffff,) * 4, (0xffffffff,) * 2, (0x408f276d, 0x41c83b0e, 0xa20bc7c6, 0x6d5451fd)),
    ((0x243f6a88, 0x85a308d3, 0x13198a2e, 0x03707344), (0xa4093822, 0x299f31d0), (0xd16cfe09, 0x94fdcceb, 0x5001e420, 0x24126ea1)),
]


def measure_bars(what=("gauss", "box", "ar1", "grid")):
    """what sampleref.BARS holds: the replica's largest error over sampleref.BAR_SEEDS, times 2"""
    bars = {}
    if "gauss" in what:
        for d in (1, 3, 5):
            e = np.array([R.gauss_errors(d, s) for s in R.BAR_SEEDS])
            bars["gauss_mean", d], bars["gauss_cov", d] = 2.0 * e[:, 0].max(), 2.0 * e[:, 1].max()
    if "box" in what:
        bars["box"] = 2.0 * max(R.box_errors(s) for s in R.BAR_SEEDS)
    if "ar1" in what:
        for phi in (0.5, 0.9):
            bars["ar1", phi] = 2.0 * max(ar1_error(phi, s) for s in R.BAR_SEEDS)
    if "grid" in what:
        g = np.load(GRID)
        for key, d in GRID_D.items():
            e = np.array([R.grid_errors(g[key], d, s) for s in R.BAR_SEEDS])
            bars["grid_mean", key], bars["grid_sd", key] = 2.0 * e[:, 0].max(), 2.0 * e[:, 1].max()
    return bars


def ar1_error(phi, seed):
    tau = R.autocorr_time(R.ar1(phi, R.AR1_N, seed))
    want = (1.0 + phi) / (1.0 - phi)
    return abs(tau - want) / want


@pytest.mark.parametrize("ctr,key,out", KNOWN)
def test_philox_known_answers(ctr, key, out):
    assert tuple(int(v) for v in R.philox4x32(*ctr, *key)) == out
    assert tuple(int(v) for v in abi.philox4x32(ctr, key)) == out


def test_uniform_is_inside_the_unit_interval_and_exact():
    assert R.uniform(0, 0) == 2.0 ** -53 and R.uniform(0xffffffff, 0xffffffff) == 1.0 - 2.0 ** -53
    rng = np.random.default_rng(5)
    a, b = rng.integers(0, 2 ** 32, 4000, dtype=np.uint64), rng.integers(0, 2 ** 32, 4000, dtype=np.uint64)
    u = R.uniform(a, b)
    assert np.all((u > 0.0) & (u < 1.0))
    n = (a.astype(object) << 20) | (b.astype(object) >> 12)
    from fractions import Fraction
    assert all(Fraction(float(x)) == Fraction(2 * int(m) + 1, 2 ** 53) for x, m in zip(u[:500], n[:500]))


def test_library_generator_equals_the_replica_bit_for_bit():
    rng = np.random.default_rng(11)
    ctr = rng.integers(0, 2 ** 32, (3000, 4), dtype=np.uint64)
    key = rng.integers(0, 2 ** 32, (3000, 2), dtype=np.uint64)
    want = np.stack(R.philox4x32(ctr[:, 0], ctr[:, 1], ctr[:, 2], ctr[:, 3], key[:, 0], key[:, 1]), axis=1)
    got = np.stack([abi.philox4x32(c, k) for c, k in zip(ctr, key)])
    assert np.array_equal(got, want)
    for seed in (0, 1, 0xdeadbeefcafef00d, 2 ** 64 - 1):
        for step in (0, 7, 2 ** 32 - 1, 2 ** 32 + 5, 2 ** 63 + 11):
            walkers = np.concatenate([np.arange(300), [2 ** 31, 2 ** 32 - 1]])
            want = np.stack(R.uniforms(seed, walkers, step), axis=1)
            got = np.stack([abi.sample_uniforms(seed, int(k), step) for k in walkers])
            assert got.tobytes() == want.tobytes(), (seed, step)
    assert abi.load().gpemu_philox4x32(None, None, None) == abi.ERR_ARG
    assert abi.load().gpemu_sample_uniforms(0, 0, 0, None) == abi.ERR_ARG


def test_no_counter_repeats_between_the_draws_of_a_run():
    """u1, u2 (counter word 3 = 0), u3 (1) and the default starts (2) of one seed are different streams"""
    k = np.arange(64)
    u1, u2, u3 = R.uniforms(3, k, 0)
    w = R.words(3, k, 0, 2)
    allu = np.concatenate([u1, u2, u3, R.uniform(w[0], w[1])])
    assert np.unique(allu).size == allu.size


@pytest.mark.parametrize("d", [1, 3, 5])
def test_replica_samples_a_correlated_gaussian(d):
    em, ec = R.gauss_errors(d, R.TEST_SEED)
    print(f"d {d}: mean {em:.4f}/{R.BARS['gauss_mean', d]:.4f} cov {ec:.4f}/{R.BARS['gauss_cov', d]:.4f}")
    assert em <= R.BARS["gauss_mean", d] and ec <= R.BARS["gauss_cov", d]


def test_replica_flat_likelihood_in_a_box_gives_uniform_marginals():
    e = R.box_errors(R.TEST_SEED)
    print(f"box: {e:.4f}/{R.BARS['box']:.4f}")
    assert e <= R.BARS["box"]


@pytest.mark.parametrize("phi", [0.5, 0.9])
def test_replica_autocorr_time_on_ar1(phi):
    e = ar1_error(phi, R.TEST_SEED)
    print(f"ar1 {phi}: {e:.4f}/{R.BARS['ar1', phi]:.4f}")
    assert e <= R.BARS["ar1", phi]


def test_host_autocorr_time_is_the_replicas():
    """gpemu_host_autocorr_time against (1 + phi) / (1 - phi) under the AR(1) bars, and against the replica's estimator: the same
    sums in another order"""
    build.build_all()
    host = ctypes.CDLL(build.HOST_LIB)
    fn = host.gpemu_host_autocorr_time
    fn.restype, fn.argtypes = ctypes.c_int, [ctypes.POINTER(ctypes.c_double), ctypes.c_int, ctypes.POINTER(ctypes.c_double)]
    tau = ctypes.c_double(0.0)
    for phi in (0.5, 0.9):
        s = R.ar1(phi, R.AR1_N, R.TEST_SEED)
        assert fn(s.ctypes.data_as(ctypes.POINTER(ctypes.c_double)), s.size, ctypes.byref(tau)) == 0
        want = (1.0 + phi) / (1.0 - phi)
        print(f"host tau at phi {phi}: {tau.value:.4f}, exact {want:.4f}")
        assert abs(tau.value - want) / want <= R.BARS["ar1", phi]
        assert abs(tau.value - R.autocorr_time(s)) <= 1e-9 * tau.value
    const = np.full(10, 3.0)
    assert fn(const.ctypes.data_as(ctypes.POINTER(ctypes.c_double)), 10, ctypes.byref(tau)) == 0 and tau.value == 1.0
    assert fn(None, 10, ctypes.byref(tau)) == 1 and np.isnan(tau.value)
    assert fn(const.ctypes.data_as(ctypes.POINTER(ctypes.c_double)), 0, ctypes.byref(tau)) == 1
    assert fn(const.ctypes.data_as(ctypes.POINTER(ctypes.c_double)), 10, None) == 1


@pytest.mark.parametrize("key", sorted(GRID_D))
def test_replica_on_the_tabulated_posteriors(key):
    em, es = R.grid_errors(np.load(GRID)[key], GRID_D[key], R.TEST_SEED)
    print(f"{key}: mean {em:.4f}/{R.BARS['grid_mean', key]:.4f} sd {es:.4f}/{R.BARS['grid_sd', key]:.4f}")
    assert em <= R.BARS["grid_mean", key] and es <= R.BARS["grid_sd", key]


def test_bars_hold_for_their_seeds():
    """the cheap part of the measurement repeated: the stored bars are what measure_bars gives (the logarithms of another libm
    may move a chain, so the comparison is not to the last bit)"""
    assert R.TEST_SEED not in R.BAR_SEEDS and len(R.BAR_SEEDS) == 16
    for k, v in measure_bars(("ar1",)).items():
        assert abs(v - R.BARS[k]) <= 0.5 * R.BARS[k], (k, v, R.BARS[k])
