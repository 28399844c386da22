"""gpemu_host_backproject (csrc/host/multi.c): the one place the host layer turns PCA-space results into observable-space
ones (multivar_support.c:118-157).  Every observable-space number of the emulate_*_multi entries goes through it, so its
summation order is pinned here bit for bit, without a device."""
import os
import subprocess

import numpy as np

from madaiemulator_amd import build

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MULTI = os.path.join(ROOT, "tests", "golden", "ref_inputs", "multi-simple.input_model_file.dat")


def test_backproject_is_the_literal_rule_bit_for_bit(tmp_path):
    """the four shapes the entries use -- mean (factor evecs sqrt(evals), training mean added, width 1), variance (evecs^2
    evals, width 1), mean gradient (width d) and the covariance layout (one row of width 9 = 3 x 3) -- against the rule as
    literal loops in the driver (factor first, sum over the components in index order from 0.0, mean added afterwards):
    memcmp-equal.  numpy's product guards those loops: a sum of nr <= nt products in double differs from any other order by
    a few ulp of its largest term at most, far inside rtol = 1e-13."""
    build.build_all()
    exe, binf = str(tmp_path / "host_backproject_driver"), tmp_path / "bp.bin"
    subprocess.check_call(["gcc", "-std=gnu99", "-O1", "-Wall", "-I", os.path.join(ROOT, "include"), "-I", build.HOST_SRC,
                           "-o", exe, os.path.join(ROOT, "tests", "c", "host_backproject_driver.c"),
                           "-L", build.LIBDIR, "-lEmuMI", "-lgpemu_hip", f"-Wl,-rpath,{build.LIBDIR}", "-lm"])
    out = subprocess.run([exe, MULTI, str(binf)], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stderr[-2000:]
    lines = [ln.split() for ln in out.stdout.splitlines() if ln.split() and ln.split()[0] in ("dims", "case")]
    nt, nr, d = (int(v) for v in lines[0][1:])
    cases = [(c[1], int(c[2]), int(c[3]), int(c[4]), int(c[5]), int(c[6])) for c in lines[1:]]
    assert [c[:5] for c in cases] == [("mean", 0, 1, 3, 1), ("variance", 1, 0, 3, 1), ("mean_gradient", 0, 0, 3, d),
                                      ("covariance_layout", 1, 0, 1, 9)]
    assert 1 < nr <= nt and d >= 1
    raw = np.fromfile(binf, dtype=np.float64)
    ybar, lam, U, pos = raw[:nt], raw[nt:nt + nr], raw[nt + nr:nt + nr + nt * nr].reshape(nt, nr), nt + nr + nt * nr
    for name, squared, add_mean, nrows, width, equal in cases:
        assert equal == 1, name                                        # the routine's bytes are the literal loops' bytes
        got_pca = raw[pos:pos + nrows * nr * width].reshape(nrows, nr, width)
        pos += got_pca.size
        got = raw[pos:pos + nrows * nt * width].reshape(nrows, nt, width)
        pos += got.size
        F = U ** 2 * lam if squared else U * np.sqrt(lam)
        want = np.stack([(got_pca[q].T @ F.T).T for q in range(nrows)])
        if add_mean:
            want[:, :, 0] += ybar
        assert np.all(np.isfinite(got)), name
        np.testing.assert_allclose(got, want, rtol=1e-13, atol=0, err_msg=name)
    assert pos == raw.size
