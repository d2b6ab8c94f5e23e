"""The reference's chi^2 test procedure (src/utils/chi2test.cpp) on the HIP path: the contingency table of
nh_chi2_histogram against the oracle count for count, the expected frequencies of nh_chi2_expected against the recursive
adaptive Simpson rule of chi2_refs over the oracle's pdf, whole files through nh_chi2_run against the golden
(tests/golden/chi2_golden.json) and live against chi2_refs, the CLI, the refusals.

The oracle has no Disney BSDF: chi2_refs.histogram restates its sample() -- the diffuse BSDF's direction and density,
skipped where pdf < Epsilon -- over the oracle's diffuse BSDF (chi2_refs.histogram says what it assumes).

Tolerances. Counts are integers: equal. Expected frequencies: both sides run the same refinement tree (equal evaluation
counts per cell) in fp64 in the same order, so bit equality is what to expect; the bound is the project's fp64 bound
REL = 1e-9 relative on every cell (a zero cell must be zero), which leaves room only for a device fp64 sin / cos that
differs from the host library's by an ulp and flips the fp32 rounding of a wo component (about 2^-29 per evaluation).
p-values against the golden: 1e-6, as test_gpu_ttest.py holds p to its golden."""
import json
import os
import subprocess

import numpy as np
import pytest

import chi2_refs
import disney_scenes as dz
import nori_hip as nh
import nori_oracle as no

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "chi2_golden.json")
REFERENCE_XML = "scenes/pa3/tests/chi2test-microfacet.xml"
REL = 1e-9
F32 = np.float32


@pytest.fixture(scope="module")
def ctx(gpu):
    return nh.Context(gpu)


@pytest.fixture(scope="module")
def work_dir(scene_dir):
    return chi2_refs.materialize(scene_dir, os.path.join(scene_dir, REFERENCE_XML))


@pytest.fixture(scope="module")
def golden():
    with open(GOLDEN) as f:
        return json.load(f)


def unit(x, y, z):
    v = np.array([x, y, z], np.float64)
    return (v / np.linalg.norm(v)).astype(F32)


def microfacet(alpha, int_ior=1.5, ext_ior=1.000277, kd=(0.2, 0.1, 0.6)):
    b = nh.nh_bsdf()
    b.type = nh.BSDF_MICROFACET
    b.alpha, b.int_ior, b.ext_ior = alpha, int_ior, ext_ior
    for i in range(3):
        b.kd[i] = kd[i]
    b.ks = float(F32(1) - max(F32(k) for k in kd))
    return b


def simple(kind):
    b = nh.nh_bsdf()
    b.type = kind
    for i in range(3):
        b.albedo[i] = (0.5, 0.6, 0.7)[i]
    b.int_ior, b.ext_ior = 1.5046, 1.000277
    return b


def disney(tmp, name, **params):
    """A Disney nh_bsdf through the loader (which clamps and defaults its parameters as disney.cpp does)."""
    p = os.path.join(tmp, f"{name}.xml")
    with open(p, "w") as f:
        f.write('<test type="chi2test">\n' + dz.bsdf_xml(params, albedo=(0.6, 0.4, 0.3)) + "\n</test>\n")
    return nh.Test(p).bsdfs[0]


def oracle_histogram(b, wi, n, res, first_draw=0):
    return chi2_refs.histogram(b, wi, chi2_refs.pcg_at(first_draw), n, res[0], res[1])


# ---- 1. the histogram -------------------------------------------------------------------------------------------------
WI_GRAZING, WI_STEEP = unit(0.9, 0.42, 0.08), unit(-0.2, 0.24, 0.95)


def bsdf_cases(tmp):
    return [("microfacet 0.1 grazing", microfacet(0.1, kd=(0.0, 0.0, 0.0)), WI_GRAZING),
            ("microfacet 0.1 steep", microfacet(0.1, kd=(0.0, 0.0, 0.0)), WI_STEEP),
            ("microfacet 0.3", microfacet(0.3), WI_STEEP),
            ("diffuse", simple(nh.BSDF_DIFFUSE), WI_STEEP),
            ("disney rough", disney(tmp, "rough", roughness=0.8, metallic=0.3, sheen=0.5), WI_STEEP),
            ("disney clearcoat", disney(tmp, "coat", roughness=0.3, clearcoat=1.0, clearcoatGloss=0.6), WI_GRAZING),
            ("mirror", simple(nh.BSDF_MIRROR), WI_STEEP),
            ("dielectric", simple(nh.BSDF_DIELECTRIC), WI_GRAZING)]


def test_histogram_equals_oracle_per_bsdf(ctx, tmp_path):
    n, res, first = 20000, (10, 20), 10
    for name, b, wi in bsdf_cases(str(tmp_path)):
        got = ctx.chi2_histogram(b, wi, n, res[0], res[1], first_draw=first)
        want = oracle_histogram(b, wi, n, res, first)
        np.testing.assert_array_equal(got, want, err_msg=name)
        assert 0 < got.sum() <= n, name
        print(f"{name}: {int(got.sum())} of {n} counted, {int((got > 0).sum())} cells hit, fullest {int(got.max())}")


@pytest.mark.parametrize("n", [1, 63, 64, 20000, 20007])
def test_histogram_sample_counts(ctx, n):
    """One lane, a wave less one, a wave, many workgroups, and a count that ends inside a lane's run of 16."""
    b, res = microfacet(0.3), (3, 6)
    got = ctx.chi2_histogram(b, WI_STEEP, n, res[0], res[1])
    np.testing.assert_array_equal(got, oracle_histogram(b, WI_STEEP, n, res))


def test_histogram_long_runs(ctx):
    """Above 2048 * 256 * 16 samples the lanes' runs grow instead of the grid: here to 18, the last one cut short."""
    b, n, res = simple(nh.BSDF_DIFFUSE), 2048 * 256 * 17 + 5, (3, 6)
    got = ctx.chi2_histogram(b, WI_STEEP, n, res[0], res[1], first_draw=4)
    np.testing.assert_array_equal(got, oracle_histogram(b, WI_STEEP, n, res, 4))
    assert got.sum() == n


@pytest.mark.parametrize("first_draw", [0, 10, 2 ** 33 + 2])
def test_histogram_first_draw(ctx, first_draw):
    b, n, res = microfacet(0.1), 4099, (10, 20)
    got = ctx.chi2_histogram(b, WI_STEEP, n, res[0], res[1], first_draw=first_draw)
    np.testing.assert_array_equal(got, oracle_histogram(b, WI_STEEP, n, res, first_draw))


@pytest.mark.parametrize("res", [(1, 2), (3, 6), (10, 20), (64, 128), (5, 7)])
def test_histogram_resolutions(ctx, res):
    """(64, 128) is the largest table, the one LDS table per workgroup; the others take one per wave."""
    b, n = microfacet(0.3), 20000
    got = ctx.chi2_histogram(b, WI_GRAZING, n, res[0], res[1], first_draw=2)
    assert got.shape == (res[0] * res[1],)
    np.testing.assert_array_equal(got, oracle_histogram(b, WI_GRAZING, n, res, 2))


def test_histogram_below_the_horizon_and_repeatable(ctx, tmp_path):
    below = unit(0.3, -0.2, -0.5)
    for b in (microfacet(0.3), simple(nh.BSDF_DIFFUSE), simple(nh.BSDF_MIRROR), disney(str(tmp_path), "d", roughness=0.5)):
        got = ctx.chi2_histogram(b, below, 5000, 10, 20)
        assert not got.any()
        np.testing.assert_array_equal(got, oracle_histogram(b, below, 5000, (10, 20)))
    b = microfacet(0.1, kd=(0.0, 0.0, 0.0))
    first = ctx.chi2_histogram(b, WI_GRAZING, 300000, 10, 20)
    again = ctx.chi2_histogram(b, WI_GRAZING, 300000, 10, 20)
    np.testing.assert_array_equal(first.view(np.uint64), again.view(np.uint64))
    assert first.sum() > 0


# ---- 2. the expected frequencies --------------------------------------------------------------------------------------
def check_expected(got, evals, want, want_evals, what):
    np.testing.assert_array_equal(evals, want_evals, err_msg=what)
    bad = [(i, g, w) for i, (g, w) in enumerate(zip(got, want)) if not (g == w or abs(g - w) <= REL * abs(w))]
    differ = int((got.view(np.uint64) != want.view(np.uint64)).sum())
    print(f"{what}: {len(got)} cells, {int(evals.sum())} evaluations, {differ} cells differ in bits")
    assert not bad, (what, bad[:5])


@pytest.mark.parametrize("res", [(3, 6), (10, 20)])
def test_expected_equals_refs(ctx, tmp_path, res):
    n = res[0] * res[1] * 5000
    cases = [("microfacet 0.1", microfacet(0.1, kd=(0.0, 0.0, 0.0))), ("microfacet 0.6", microfacet(0.6, 1.8, 1.3, (0.4, 0.2, 0.3))),
             ("disney", disney(str(tmp_path), "rough", roughness=0.8, metallic=0.3))]
    wis = np.stack([WI_GRAZING, WI_STEEP])
    for name, b in cases:
        exp, evals = ctx.chi2_expected(b, wis, res[0], res[1], n, evals=True)
        assert exp.shape == evals.shape == (2, res[0] * res[1])
        for k, wi in enumerate(wis):
            want, want_evals = chi2_refs.expected_frequencies(b, wi, res[0], res[1], n)
            check_expected(exp[k], evals[k], want, want_evals, f"{name}, wi {k}, {res}")
            assert 0.5 * n < exp[k].sum() < 1.001 * n  # (a density; a grazing lobe loses what reflects below)
    one = ctx.chi2_expected(cases[0][1], WI_STEEP, res[0], res[1], n)  # one direction: the same bits as in a batch
    np.testing.assert_array_equal(one.view(np.uint64), ctx.chi2_expected(cases[0][1], wis, res[0], res[1], n)[1].view(np.uint64))


# ---- 3. whole files ---------------------------------------------------------------------------------------------------
def check_against(res, want, hex_tables):
    assert len(res) == len(want)
    for i, (r, g) in enumerate(zip(res, want)):
        wi = [float.fromhex(x) for x in g["wi"]] if hex_tables else g["wi"]
        exp = np.array([float.fromhex(x) for x in g["exp"]]) if hex_tables else g["exp"]
        np.testing.assert_array_equal(r["wi"], np.array(wi, F32), err_msg=f"test {i}")
        np.testing.assert_array_equal(r["obs"], np.asarray(g["obs"], np.float64), err_msg=f"test {i}")
        bad = [(j, a, b) for j, (a, b) in enumerate(zip(r["exp"], exp)) if not (a == b or abs(a - b) <= REL * abs(b))]
        assert not bad, (i, bad[:5])
        assert (r["accepted"], r["kind"], r["dof"], r["pooled_cells"]) == \
            (g["accepted"], g["kind"], g["dof"], g["pooled_cells"]), (i, r, g)
        assert r["sample_count"] == g["sample_count"] and abs(r["level"] - g["level"]) <= 1e-15
        assert r["obs_sum"] == sum(g["obs"])
        if g["kind"] in (nh.CHI2_ACCEPTED, nh.CHI2_REJECTED_P_VALUE):
            assert abs(r["statistic"] - g["statistic"]) <= REL * abs(g["statistic"]), (i, r["statistic"], g["statistic"])
            assert abs(r["p_value"] - g["p_value"]) <= 1e-6, (i, r["p_value"], g["p_value"])
        elif g["kind"] == nh.CHI2_REJECTED_ZERO_CELL:
            assert r["statistic"] == g["statistic"]


def test_reference_file_passes(gpu, work_dir, golden):
    res = nh.run_chi2_tests(os.path.join(work_dir, REFERENCE_XML))
    check_against(res, golden[REFERENCE_XML], True)
    assert len(res) == 15 and all(r["accepted"] for r in res)
    print("smallest p-value", min(r["p_value"] for r in res), "level", res[0]["level"])


@pytest.mark.parametrize("rel", [chi2_refs.DISNEY_XML, chi2_refs.MIXED_XML])
def test_small_files_equal_golden(gpu, work_dir, golden, rel):
    res = nh.run_chi2_tests(os.path.join(work_dir, rel))
    check_against(res, golden[rel], True)
    if rel == chi2_refs.MIXED_XML:  # diffuse accepted; mirror and dielectric: discrete, every sample in a pdf-0 cell
        assert [r["kind"] for r in res] == [nh.CHI2_ACCEPTED] * 2 + [nh.CHI2_REJECTED_ZERO_CELL] * 4
        assert nh.CHI2_KINDS[res[2]["kind"]] == "expected frequency 0" and res[2]["statistic"] == 20000
        assert all(not r["exp"].any() for r in res[2:])
    else:
        assert all(r["accepted"] for r in res)


def test_small_microfacet_file_live(gpu, work_dir):
    path = os.path.join(work_dir, chi2_refs.SMALL_XML)
    res = nh.run_chi2_tests(path)
    want = chi2_refs.execute(path)
    assert len(res) == 6
    check_against(res, want, False)
    assert all(r["accepted"] for r in res)
    assert len(nh.run_chi2_tests(path, tables=False)) == 6


# ---- 4. the CLI -------------------------------------------------------------------------------------------------------
def test_cli(gpu, work_dir):
    cli = os.path.join(os.path.dirname(nh.LIB_PATH), "nori_hip")

    def run(path):
        return subprocess.run(["timeout", "-k", "10", "120", cli, path], capture_output=True, text=True, timeout=150)
    r = run(os.path.join(work_dir, REFERENCE_XML))
    assert r.returncode == 0, (r.stdout, r.stderr)
    assert "Passed 15/15 tests." in r.stdout
    assert r.stdout.count("Accepted the null hypothesis (p-value = ") == 15 and "Rejected" not in r.stdout
    assert r.stdout.count("Accumulating 1000000 samples into a 10x20 contingency table .. done.") == 15
    assert r.stdout.count("Integrating expected frequencies .. done.") == 15
    assert r.stdout.count("Chi^2 statistic = ") == 15 and "Pooled " in r.stdout
    # a BSDF whose histogram cannot fit its (zero) pdf: the first tests fail, the exit status says so
    r = run(os.path.join(work_dir, chi2_refs.MIXED_XML))
    assert r.returncode not in (0, 124, 137), (r.returncode, r.stdout, r.stderr)
    assert "Passed 2/6 tests." in r.stdout
    assert r.stdout.count("samples in a cell with expected frequency 0. Rejecting the null hypothesis!") == 4
    dielectric = os.path.join(work_dir, "chi2", "chi2test-dielectric-first.xml")
    text = open(os.path.join(work_dir, REFERENCE_XML)).read()
    with open(dielectric, "w") as f:
        f.write(text.replace('<test type="chi2test">', '<test type="chi2test">\n<integer name="sampleCount" value="20000"/>\n'
                             '<bsdf type="dielectric"/>', 1))
    r = run(dielectric)
    assert r.returncode not in (0, 124, 137), (r.returncode, r.stdout, r.stderr)
    assert "Passed 15/20 tests." in r.stdout and r.stdout.count("Encountered ") == 5


# ---- 5. refusals ------------------------------------------------------------------------------------------------------
def test_refusals(ctx, work_dir, tmp_path):
    b = microfacet(0.3)
    for res in ((64, 129), (8193, 1), (0, 4), (4, 0), (-1, -1)):
        with pytest.raises(nh.NoriError, match="at most 8192 cells"):
            ctx.chi2_histogram(b, WI_STEEP, 100, res[0], res[1])
        with pytest.raises(nh.NoriError, match="at most 8192 cells"):
            ctx.chi2_expected(b, WI_STEEP, res[0], res[1], 100)
    for n in (0, -5):
        with pytest.raises(nh.NoriError, match="n >= 1"):
            ctx.chi2_histogram(b, WI_STEEP, n, 3, 6)
    for kind in (-1, 5, 99):
        bad = microfacet(0.3)
        bad.type = kind
        with pytest.raises(nh.NoriError, match="unknown BSDF type"):
            ctx.chi2_histogram(bad, WI_STEEP, 100, 3, 6)
        with pytest.raises(nh.NoriError, match="unknown BSDF type"):
            ctx.chi2_expected(bad, WI_STEEP, 3, 6, 100)
    textured = tmp_path / "textured.xml"
    textured.write_text('<test type="chi2test">\n<bsdf type="diffuse"><texture type="checkerboard_color" name="albedo">'
                        '<color name="value1" value="0.8,0.8,0.8"/><color name="value2" value="0.2,0.2,0.2"/>'
                        '</texture></bsdf>\n</test>\n')
    with pytest.raises(nh.NoriError, match="a textured BSDF in a <test> is not supported"):
        nh.run_chi2_tests(str(textured))
    with pytest.raises(nh.NoriError, match="not a chi2test"):
        nh.run_chi2_tests(os.path.join(work_dir, "scenes/pa3/tests/ttest-microfacet.xml"))
    # the table is still usable afterwards
    assert ctx.chi2_histogram(b, WI_STEEP, 100, 3, 6).sum() == 100
