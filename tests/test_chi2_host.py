"""The host side of the reference's chi^2 test procedure (src/utils/chi2test.cpp) on the HIP path, CPU only: the
loader's ChiSquareTest properties (nh_test_get_chi2_params), hypothesis::chi2_test restated (nh_chi2_test) against
chi2_refs / scipy and the reference's own hypothesis.h where its probe is built, and the exported symbols.

p-values: |p - (1 - scipy.stats.chi2.cdf)| <= 1e-9, the bound test_ttest_host.py holds the t-test's p to."""
import ctypes as C
import math
import os

import numpy as np
import pytest
from scipy import stats

import chi2_refs
import nori_hip as nh
from test_oracle_kat import reference_verdicts

CHI2_XML = "scenes/pa3/tests/chi2test-microfacet.xml"
TTEST_XML = "scenes/pa3/tests/ttest-microfacet.xml"


# ---- the loader -------------------------------------------------------------------------------------------------------
def test_loader_defaults(scene_dir):
    t = nh.Test(os.path.join(scene_dir, CHI2_XML))
    # chi2test.cpp:52-73: none is set in the file; the automatic sample count is 10 * 20 * 5000
    assert (t.resolution, t.min_exp_frequency, t.test_count, t.chi2_sample_count) == (10, 5, 5, 1000000)
    assert t.sample_count == -1  # the descriptor keeps the file's own value


def test_loader_reads_the_properties(scene_dir, tmp_path):
    text = open(os.path.join(scene_dir, CHI2_XML)).read()
    props = ('<test type="chi2test">\n<integer name="resolution" value="7"/>\n<integer name="minExpFrequency" value="9"/>\n'
             '<integer name="testCount" value="3"/>\n')
    p = tmp_path / "props.xml"
    p.write_text(text.replace('<test type="chi2test">', props))
    t = nh.Test(str(p))
    assert (t.resolution, t.min_exp_frequency, t.test_count, t.chi2_sample_count) == (7, 9, 3, 7 * 14 * 5000)
    p.write_text(text.replace('<test type="chi2test">', props + '<integer name="sampleCount" value="4321"/>\n'))
    t = nh.Test(str(p))
    assert (t.resolution, t.chi2_sample_count, t.sample_count) == (7, 4321, 4321)
    for rel in chi2_refs.FILES:
        t = nh.Test(os.path.join(chi2_refs.materialize(str(tmp_path)), rel))
        assert (t.resolution, t.min_exp_frequency, t.test_count, t.chi2_sample_count) == (3, 5, 2, 20000)


def test_loader_refusals(scene_dir, tmp_path):
    text = open(os.path.join(scene_dir, CHI2_XML)).read()
    p = tmp_path / "scene_child.xml"
    p.write_text(text.replace("</test>", "<scene></scene>\n</test>"))
    with pytest.raises(nh.NoriError, match=r"ChiSquareTest::addChild\(<EScene>\) is not supported!"):
        nh.Test(str(p))
    t = nh.Test(os.path.join(scene_dir, TTEST_XML))
    assert t.resolution is None and t.test_count is None
    cp = nh.nh_chi2_params()
    assert nh.lib.nh_test_get_chi2_params(t._h, C.byref(cp)) == 1  # NH_ERR_INVALID
    assert b"not a chi2test" in nh.lib.nh_host_last_error()


# ---- nh_chi2_test -----------------------------------------------------------------------------------------------------
def tables():
    """(obs, exp, n, min_exp, alpha, num_tests): Poisson-like tables around their expectation, with and without cells to
    pool, a misfit, few cells (dof 1, 2, 3) and many, frequencies from 1e-3 to 1e5."""
    rng = np.random.default_rng(7)
    out = []
    for cells in (2, 3, 4, 18, 200, 8192):
        for scale in (0.5, 4.0, 30.0, 5000.0):
            for misfit in (0.0, 0.02, 0.3):
                w = rng.random(cells) ** 3 + 1e-4
                n = int(scale * cells)
                exp = w / w.sum() * n
                skew = 1.0 + misfit * np.cos(np.arange(cells))
                obs = rng.poisson(exp * skew).astype(np.float64)
                for min_exp, alpha, k in ((5.0, 0.01, 1), (5.0, 0.01, 15), (1.0, 0.05, 4)):
                    out.append((obs, exp, max(n, 1), min_exp, alpha, k))
    return out


def test_chi2_matches_refs_and_scipy():
    worst = 0.0
    kinds = set()
    for obs, exp, n, min_exp, alpha, k in tables():
        got = nh.chi2_test(obs, exp, n, min_exp, alpha, k)
        want = chi2_refs.chi2_statistic(obs, exp, n, min_exp, alpha, k)
        kinds.add(got["kind"])
        assert (got["dof"], got["pooled_cells"]) == (want["dof"], want["pooled_cells"]), (len(obs), n, got, want)
        if want["kind"] in (2, 3):
            assert got["kind"] == want["kind"] and not got["accepted"] and math.isnan(got["p_value"])
            continue
        assert got["statistic"] == pytest.approx(want["statistic"], rel=1e-12)
        ref = 1 - stats.chi2.cdf(got["statistic"], got["dof"])
        worst = max(worst, abs(got["p_value"] - ref))
        assert abs(got["p_value"] - ref) <= 1e-9, (len(obs), n, got, ref)
        if abs(ref - chi2_refs.sidak(alpha, k)) > 1e-8:  # (not on the verdict's edge)
            assert got["accepted"] == want["accepted"] and got["kind"] == want["kind"], (got, want)
    assert {nh.CHI2_ACCEPTED, nh.CHI2_REJECTED_P_VALUE} <= kinds
    print(f"largest |p - scipy| over the tables: {worst:.3e}")


def test_chi2_p_value_grid():
    """The distribution function alone, through one-term tables: dof cells + 1 equal cells, the statistic placed."""
    worst = 0.0
    for dof in (1, 2, 3, 4, 7, 50, 199, 1000, 8191):
        for z in (0.0, 1e-6, 0.1, 0.5, 0.9, 1.0, 1.1, 1.5, 2.0, 3.0, 6.0):
            cells, e = dof + 1, 100.0
            x = z * dof  # the statistic wanted, put into the first two cells
            d = math.sqrt(x * e / 2.0)
            obs = np.full(cells, e)
            obs[0] += d
            obs[1] -= d
            got = nh.chi2_test(obs, np.full(cells, e), int(cells * e), 5.0, 0.01, 1)
            assert got["dof"] == dof and got["pooled_cells"] == 0
            ref = 1 - stats.chi2.cdf(got["statistic"], dof)
            if dof == 2:  # hypothesis.h:46-47
                assert got["p_value"] == 1 - (1.0 - math.exp(-0.5 * got["statistic"]))
            worst = max(worst, abs(got["p_value"] - ref))
            assert abs(got["p_value"] - ref) <= 1e-9, (dof, z, got, ref)
    print(f"largest |p - scipy| over the grid: {worst:.3e}")


def test_chi2_rejection_kinds():
    n = 100000
    # all-zero tables: nothing counted, dof -1
    got = nh.chi2_test(np.zeros(12), np.zeros(12), n, 5.0, 0.01, 1)
    assert (got["accepted"], got["kind"], got["dof"]) == (False, nh.CHI2_REJECTED_DOF, -1) and math.isnan(got["p_value"])
    # one cell: dof 0
    got = nh.chi2_test([n], [float(n)], n, 5.0, 0.01, 1)
    assert (got["kind"], got["dof"]) == (nh.CHI2_REJECTED_DOF, 0)
    # a sample in a cell of expected frequency 0: rejected above n * 1e-5 (here 1), ignored at or below it
    exp = np.array([0.0, 25000.0, 25000.0, 25000.0, 25000.0])
    obs = np.array([2.0, 25010.0, 24990.0, 25100.0, 24898.0])
    got = nh.chi2_test(obs, exp, n, 5.0, 0.01, 1)
    assert (got["accepted"], got["kind"], got["statistic"]) == (False, nh.CHI2_REJECTED_ZERO_CELL, 2.0)
    assert math.isnan(got["p_value"])
    obs[0] = 1.0
    got = nh.chi2_test(obs, exp, n, 5.0, 0.01, 1)
    assert got["accepted"] and got["kind"] == nh.CHI2_ACCEPTED and got["dof"] == 3
    assert got == nh.chi2_test(obs[1:], exp[1:], n, 5.0, 0.01, 1)
    # a plain misfit
    got = nh.chi2_test([26000.0, 24000.0, 25000.0, 25000.0], exp[1:], n, 5.0, 0.01, 1)
    assert (got["accepted"], got["kind"]) == (False, nh.CHI2_REJECTED_P_VALUE) and got["p_value"] < 1e-10
    # pooling: the three low cells pool (the third joins because the pool is still under 5), 2 terms, dof 1
    got = nh.chi2_test([1.0, 2.0, 4.0, 50.0], [1.5, 1.5, 6.0, 48.0], 57, 5.0, 0.01, 1)
    assert (got["pooled_cells"], got["dof"]) == (3, 1)
    assert got["statistic"] == pytest.approx((7 - 9) ** 2 / 9 + (50 - 48) ** 2 / 48, rel=1e-14)
    # equal expected frequencies: cell order decides which of them joins the pool (a stable sort)
    a = nh.chi2_test([3.0, 9.0, 1.0, 40.0], [2.0, 6.0, 6.0, 40.0], 54, 5.0, 0.01, 1)
    assert a["pooled_cells"] == 2 and a["statistic"] == pytest.approx((12 - 8) ** 2 / 8 + (1 - 6) ** 2 / 6, rel=1e-14)


def test_chi2_non_finite_and_invalid():
    exp = np.array([10.0, 20.0, 30.0, 40.0])
    for bad in (float("nan"), float("inf")):
        for which in range(2):
            o, e = np.array([12.0, 18.0, 33.0, 37.0]), exp.copy()
            (o if which == 0 else e)[2] = bad
            got = nh.chi2_test(o, e, 100, 5.0, 0.01, 1)
            if which == 1 and math.isinf(bad):  # an infinite expectation makes a NaN term too: (inf)^2 / inf
                assert math.isnan(got["statistic"])
            assert not got["accepted"] and got["kind"] == nh.CHI2_REJECTED_P_VALUE, (bad, which, got)
    with pytest.raises(nh.NoriError):
        nh.chi2_test([], [], 10, 5.0, 0.01, 1)
    with pytest.raises(nh.NoriError):
        nh.chi2_test([1.0, 2.0], [1.0, 2.0], 10, 5.0, 0.01, 0)


def test_chi2_verdicts_match_reference(tmp_path):
    grid = [g for g in tables() if len(g[0]) <= 200]
    mine = [nh.chi2_test(*g)["accepted"] for g in grid]
    assert any(mine) and not all(mine)
    theirs = reference_verdicts([("chi2",) + g for g in grid], tmp_path)
    if theirs is not None:  # (only where the reference checkout is present, as test_oracle_kat's verdict checks)
        assert mine == theirs, [i for i, (a, b) in enumerate(zip(mine, theirs)) if a != b][:5]


def test_symbols_exported():
    host = ("nh_test_get_chi2_params", "nh_chi2_test")
    device = ("nh_chi2_histogram", "nh_chi2_expected", "nh_chi2_run", "nh_chi2_run_tables")
    host_lib = C.CDLL(os.path.join(os.path.dirname(nh.LIB_PATH), "libnori_host.so"))
    for s in host:
        assert hasattr(host_lib, s), s
    for s in device:
        assert not hasattr(host_lib, s), s  # the host library needs no GPU runtime
    for s in host + device:
        assert hasattr(nh.lib, s), s
