"""The reference's warp test (src/utils/warptest.cpp, runTest) on the HIP path: every warp and pdf through nh_warp_query
against the numpy restatement (warp_refs), the table of nh_warp_histogram against the binning applied to the device's
own query outputs and against the restatement, the expected frequencies of nh_warp_expected against the recursive
adaptive Simpson rule, whole runs against warp_refs.execute and the fixture (tests/golden/warp_runs.json), the CLI.

Tolerances. Queries: the rule of test_gpu_volume.check -- bit for bit against the fp32 restatement, else within 4 x the
restatement's own fp32-vs-fp64 gap with NaN positions equal; it prints which applied. Counts are integers: equal.
Expected frequencies: equal evaluation counts per cell, values equal or within REL = 1e-9 (test_gpu_chi2.py's bound for
the same integrator), NaN cells in the same places. p-values: 1e-6, statistics REL, as test_gpu_chi2.check_against.

Beckmann's `isinf(log(1 - x))` branch cannot be reached with a float below 1: log(1 - (1 - 2^-24)) = log(2^-24) is
finite. The nearest value, x = 1 - 2^-24, is among the inputs.

As written, squareToBeckmannPdf is 0 / 0 = NaN at z = 0 exactly (exp(-inf) over M_PI alpha^2 0^3), which runTest's
integrand reaches when a cell edge lies at y = 0.5, i.e. at an even yres -- never at the reference's 51. At (6, 12) and
(8, 16) row yres / 2 of Beckmann's expected table is NaN on both sides, and the verdict is a rejection for a p-value
that is not finite."""
import json
import math
import os
import subprocess

import numpy as np
import pytest

import nori_hip as nh
import warp_refs as wr
from test_gpu_volume import check

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "warp_runs.json")
REL = 1e-9
F32, F64 = np.float32, np.float64
TOP = F32(1) - F32(2.0 ** -24)

# type: the (parameter, angle slider) pairs its queries run at; the first is the one the table tests use
PARAMS = {
    nh.WARP_NONE: [(0.5, 0.5)], nh.WARP_DISK: [(0.5, 0.5)], nh.WARP_UNIFORM_SPHERE: [(0.5, 0.5)],
    nh.WARP_UNIFORM_SPHERE_VOL: [(0.5, 0.5)],
    nh.WARP_UNIFORM_SPHERE_CAP: [(0.5, 0.5), (0.0, 0.5), (0.999, 0.5)],
    nh.WARP_UNIFORM_HEMISPHERE: [(0.5, 0.5)], nh.WARP_COSINE_HEMISPHERE: [(0.5, 0.5)],
    nh.WARP_BECKMANN: [(0.3, 0.5), (0.05, 0.5), (1.0, 0.5)],
    nh.WARP_HENYEY_GREENSTEIN: [(0.3, 0.5), (0.0, 0.5), (-0.3, 0.5), (0.9, 0.5)],
    nh.WARP_MICROFACET_BRDF: [(0.5, 0.9), (0.1, 0.5), (0.1, 0.9), (0.5, 0.5)],
    nh.WARP_ISO_PHASE: [(0.0, 0.7)], nh.WARP_ANISO_PHASE: [(-0.3, 0.7), (0.9, 0.3)],
}
TYPES = sorted(PARAMS)


def name(t):
    return nh.WARP_NAMES[t]


@pytest.fixture(scope="module")
def ctx(gpu):
    return nh.Context(gpu)


@pytest.fixture(scope="module")
def golden():
    with open(GOLDEN) as f:
        return json.load(f)


def table_case(t):
    par, angle = PARAMS[t][0]
    return F32(par), wr.wi(angle)


# ---- 1. queries -------------------------------------------------------------------------------------------------------
def sample_inputs():
    """The corners, edges and faces of the unit cube at 0, 0.5 and 1 - 2^-24, and 256 random points."""
    e = [F32(0), F32(0.5), TOP]
    grid = np.array([[a, b, c] for a in e for b in e for c in e], F32)
    return np.concatenate([grid, np.minimum(np.random.default_rng(11).random((256, 3), dtype=np.float32), TOP)])


def pdf_inputs(t):
    rng = np.random.default_rng(12)
    if t == nh.WARP_NONE:  # inside, on and just outside the unit square
        up, dn = np.nextafter(F32(1), F32(2)), -np.nextafter(F32(0), F32(1))
        pts = [[0, 0], [1, 1], [0.5, 1], [up, 0.5], [0.5, up], [dn, 0.5], [0.5, dn], [0.3, 0.7], [2, 2], [-1, 0.5]]
        return np.array([[x, y, 0] for x, y in pts], F32)
    if t == nh.WARP_DISK:  # |p|^2 = 1 exactly and just above
        up = np.nextafter(F32(1), F32(2))
        pts = [[1, 0], [0, 1], [-1, 0], [0, -1], [up, 0], [0, -up], [0.6, 0.8], [0, 0], [0.5, 0.5], [0.8, 0.7]]
        return np.concatenate([np.array([[x, y, 0] for x, y in pts], F32),
                               np.concatenate([rng.random((64, 2), dtype=np.float32) * 2 - 1, np.zeros((64, 1), F32)], 1)])
    v = rng.normal(size=(192, 3))
    v = (v / np.linalg.norm(v, axis=1)[:, None]).astype(F32)  # unit vectors
    off = (v[:32].astype(F64) * (1 + 2e-4)).astype(F32)       # off the sphere by 2 Epsilon, outwards ...
    off_in = (v[32:64].astype(F64) * (1 - 2e-4)).astype(F32)  # ... and inwards
    flat = np.array([[1, 0, 0], [0, 1, 0], [0.6, 0.8, 0], [-1, 0, 0], [0, 0, 1], [0, 0, -1], [0, 0.6, -0.8]], F32)
    rim = np.array([[math.sqrt(0.75), 0, 0.5], [0, math.sqrt(1 - 0.999 ** 2), 0.999], [0, 1, 0]], F32)  # the caps' rims
    return np.concatenate([v, off, off_in, flat, rim, -np.abs(v[:16])])


@pytest.mark.parametrize("t", TYPES, ids=name)
def test_query_sample(ctx, t):
    s = sample_inputs()
    for par, angle in PARAMS[t]:
        w = wr.wi(angle)
        dev = ctx.warp_query(t, par, nh.WARP_QUERY_SAMPLE, s, wi=w)
        r32, r64 = (np.concatenate([p, wt[:, None]], 1) for p, wt in (wr.sample(t, par, s, T, w) for T in (F32, F64)))
        assert dev.shape == r32.shape == (len(s), 4)
        check(f"{name(t)} sample, parameter {par}, angle {angle}", dev, r32, r64)
        assert int(np.isnan(dev).sum()) == int(np.isnan(r32).sum())
        if t == nh.WARP_HENYEY_GREENSTEIN and par == 0.9:
            print("NaN points at g = 0.9:", int(np.isnan(dev).any(axis=1).sum()))
        if t != nh.WARP_MICROFACET_BRDF:
            assert (dev[:, 3] == 1).all()


@pytest.mark.parametrize("t", TYPES, ids=name)
def test_query_pdf(ctx, t):
    v = pdf_inputs(t)
    for par, angle in PARAMS[t]:
        w = wr.wi(angle)
        dev = ctx.warp_query(t, par, nh.WARP_QUERY_PDF, v, wi=w)
        assert dev.shape == (len(v),)
        check(f"{name(t)} pdf, parameter {par}, angle {angle}", dev, wr.pdf(t, par, v, F32, w), wr.pdf(t, par, v, F64, w))
    if t == nh.WARP_UNIFORM_SPHERE_CAP:  # as written: zero on the rim and below it, the cap's density above and off the sphere
        got = ctx.warp_query(t, 0.5, nh.WARP_QUERY_PDF, np.array([[0, 0, 1], [0, 1, 0], [0, 0, -2]], F32))
        assert got[0] == got[2] > 0 and got[1] == 0
    if t == nh.WARP_UNIFORM_SPHERE_VOL:
        assert (dev == F32(4) / F32(3) * F32(math.pi)).all()


# ---- 2. the histogram -------------------------------------------------------------------------------------------------
def own_chain(ctx, t, par, w, n, res, first=0, order=nh.LENS_DRAWS_RTL):
    """The numpy binning applied to the device's own nh_warp_query outputs on the same draws: (want, nan, skipped)."""
    pts = wr.points(first, n, order == nh.LENS_DRAWS_RTL)
    q = ctx.warp_query(t, par, nh.WARP_QUERY_SAMPLE, pts, wi=w)
    keep = ~(q[:, 3] == 0)
    cell, nan = wr.cells(t, q[keep, :3], res[1], res[0])
    return np.bincount(cell[~nan], minlength=res[0] * res[1]).astype(F64), int(nan.sum()), int(n - keep.sum())


@pytest.mark.parametrize("t", TYPES, ids=name)
def test_histogram_exact_chain(ctx, t):
    n, res = 20007, (6, 12)
    par, w = table_case(t)
    obs, nan = ctx.warp_histogram(t, par, n, res[1], res[0], wi=w)
    want, want_nan, skipped = own_chain(ctx, t, par, w, n, res)
    np.testing.assert_array_equal(obs, want)
    assert nan == want_nan and obs.sum() + nan + skipped == n
    ref, ref_nan, ref_skipped = wr.histogram(t, par, n, res[1], res[0], wi_=w)
    differ = int((obs != ref).sum())
    print(f"{name(t)}: {int(obs.sum())} counted, {skipped} skipped, {nan} NaN; {differ} cells differ from the restatement")
    np.testing.assert_array_equal(obs, ref)  # (follows from the query test wherever that one is bit for bit)
    assert (nan, skipped) == (ref_nan, ref_skipped)


@pytest.mark.parametrize("n", [1, 63, 64, 65, 20000, 20007])
def test_histogram_sizes(ctx, n):
    """One lane, a wave less one, a wave, a wave and one, many workgroups, and a count that ends inside a lane's run."""
    t, res = nh.WARP_BECKMANN, (3, 6)
    par, w = table_case(t)
    obs, nan = ctx.warp_histogram(t, par, n, res[1], res[0], first_draw=5)
    want, want_nan, _ = wr.histogram(t, par, n, res[1], res[0], first_draw=5)
    np.testing.assert_array_equal(obs, want)
    assert nan == want_nan and obs.sum() + nan == n


def test_histogram_long_runs(ctx):
    """The launcher shares the chi^2 histogram's limits (nh_internal.h kChi2MaxGroups 2048, kChi2Block 256, kChi2MinRun
    16): above 2048 * 256 * 16 points the lanes' runs grow instead of the grid, here to 18 with the last one cut short."""
    t, n, res = nh.WARP_NONE, 2048 * 256 * 17 + 5, (3, 6)
    obs, nan = ctx.warp_histogram(t, 0.5, n, res[1], res[0], first_draw=4)
    want, _, _ = wr.histogram(t, 0.5, n, res[1], res[0], first_draw=4)
    np.testing.assert_array_equal(obs, want)
    assert obs.sum() == n and nan == 0


@pytest.mark.parametrize("t,res", [(nh.WARP_DISK, (1, 1)), (nh.WARP_DISK, (1, 2)), (nh.WARP_DISK, (5, 7)),
                                   (nh.WARP_DISK, (51, 51)), (nh.WARP_UNIFORM_SPHERE_CAP, (51, 102))],
                         ids=lambda v: name(v) if isinstance(v, int) else f"{v[0]}x{v[1]}")
def test_histogram_resolutions(ctx, t, res):
    """(51, 102) = 5202 cells is the reference's own table and takes one LDS table per workgroup; (51, 51) and the
    smaller ones take one per wave."""
    n = 20000
    par, w = table_case(t)
    obs, nan = ctx.warp_histogram(t, par, n, res[1], res[0], first_draw=2)
    assert obs.shape == (res[0] * res[1],)
    want, want_nan, _ = wr.histogram(t, par, n, res[1], res[0], first_draw=2)
    np.testing.assert_array_equal(obs, want)
    assert nan == want_nan == 0 and obs.sum() == n


@pytest.mark.parametrize("first_draw", [0, 7, 2 ** 33 + 1])
def test_histogram_first_draw_and_order(ctx, first_draw):
    """The sphere volume is the type that reads the third draw: its table changes with the draw order."""
    t, n, res = nh.WARP_UNIFORM_SPHERE_VOL, 4099, (6, 12)
    got = {}
    for order in (nh.LENS_DRAWS_RTL, nh.LENS_DRAWS_LTR):
        obs, nan = ctx.warp_histogram(t, 0.5, n, res[1], res[0], first_draw=first_draw, draw_order=order)
        want, _, _ = wr.histogram(t, 0.5, n, res[1], res[0], first_draw=first_draw, rtl=order == nh.LENS_DRAWS_RTL)
        np.testing.assert_array_equal(obs, want)
        assert obs.sum() == n and nan == 0
        got[order] = obs
    assert (got[nh.LENS_DRAWS_RTL] != got[nh.LENS_DRAWS_LTR]).any()


@pytest.mark.parametrize("t,par,some", [(nh.WARP_HENYEY_GREENSTEIN, 0.9, False), (nh.WARP_HENYEY_GREENSTEIN, 0.999, True),
                                        (nh.WARP_UNIFORM_SPHERE_CAP, -1.5, True)], ids=["hg-0.9", "hg-0.999", "cap--1.5"])
def test_histogram_nan_tally(ctx, t, par, some):
    """squareToHenyeyGreenstein returns NaN points where 1 - cos^2 rounds below zero: at the corners of the square at
    g = 0.9 (test_query_sample counts them) but, by the restatement, for none of the stream's first 200000 points;
    for 1328 of them at g = 0.999. A sphere cap with cosThetaMax = -1.5 (finite, outside the slider's range) has z < -1
    for a fifth of the points. Tallied, not binned."""
    n, res = 200000, (6, 12)
    obs, nan = ctx.warp_histogram(t, F32(par), n, res[1], res[0])
    want, want_nan, skipped = wr.histogram(t, F32(par), n, res[1], res[0])
    print(f"{name(t)} {par}: {nan} NaN points of {n} (restatement {want_nan})")
    assert nan == want_nan and skipped == 0 and obs.sum() + nan + skipped == n
    assert (nan > 0) == some
    np.testing.assert_array_equal(obs, want)
    own, own_nan, _ = own_chain(ctx, t, F32(par), None, n, res)
    np.testing.assert_array_equal(obs, own)
    assert nan == own_nan


def test_histogram_repeatable(ctx):
    t = nh.WARP_MICROFACET_BRDF
    par, w = table_case(t)
    first = ctx.warp_histogram(t, par, 300000, 102, 51, wi=w)
    again = ctx.warp_histogram(t, par, 300000, 102, 51, wi=w)
    np.testing.assert_array_equal(first[0].view(np.uint64), again[0].view(np.uint64))
    assert first[1] == again[1] and 0 < first[0].sum() <= 300000


# ---- 3. the expected frequencies --------------------------------------------------------------------------------------
def check_expected(got, evals, want, want_evals, what):
    np.testing.assert_array_equal(evals, want_evals, err_msg=what)
    np.testing.assert_array_equal(np.isnan(got), np.isnan(want), err_msg=what)
    bad = [(i, g, w) for i, (g, w) in enumerate(zip(got, want))
           if not (g == w or abs(g - w) <= REL * abs(w) or (math.isnan(g) and math.isnan(w)))]
    differ = int((got.view(np.uint64) != want.view(np.uint64)).sum())
    print(f"{what}: {len(got)} cells, {int(evals.sum())} evaluations, {int(np.isnan(want).sum())} NaN cells, "
          f"{differ} cells differ in bits")
    assert not bad, (what, bad[:5])


@pytest.mark.parametrize("res", [(3, 6), (6, 12)], ids=lambda r: f"{r[0]}x{r[1]}")
@pytest.mark.parametrize("t", TYPES, ids=name)
def test_expected_equals_refs(ctx, t, res):
    n = 1000 * res[0] * res[1]
    par, w = table_case(t)
    exp, evals = ctx.warp_expected(t, par, res[1], res[0], n, wi=w, evals=True)
    want, want_evals = wr.expected(t, par, res[1], res[0], n, w)
    check_expected(exp, evals, want, want_evals, f"{name(t)} {res}")
    fin = ~np.isnan(want)
    a, b = float(sum(exp[fin].tolist())), float(sum(want[fin].tolist()))
    assert a == b or abs(a - b) <= REL * abs(b)
    if t == nh.WARP_DISK:  # cells outside the disk: exactly zero; at (6, 12) the square's corner cells are
        assert (exp[want == 0] == 0).all()
        if res == (6, 12):
            assert exp[0] == 0 and exp[11] == 0 and exp[-12] == 0 and exp[-1] == 0
    if t == nh.WARP_BECKMANN:  # the docstring's NaN row, at an even yres only
        assert int(np.isnan(exp).sum()) == (res[1] if res[0] % 2 == 0 else 0)


# ---- 4. verdicts ------------------------------------------------------------------------------------------------------
def same_verdict(r, g, what):
    assert (r["kind"], r["dof"], r["pooled_cells"], bool(r["accepted"])) == \
        (g["kind"], g["dof"], g["pooled_cells"], bool(g["accepted"])), (what, r, g)
    if g["kind"] in (nh.CHI2_ACCEPTED, nh.CHI2_REJECTED_P_VALUE):
        if math.isnan(g["statistic"]):
            assert math.isnan(r["statistic"]) and math.isnan(r["p_value"]), what
        else:
            assert abs(r["statistic"] - g["statistic"]) <= REL * abs(g["statistic"]), (what, r["statistic"], g["statistic"])
            assert abs(r["p_value"] - g["p_value"]) <= 1e-6, (what, r["p_value"], g["p_value"])
    elif g["kind"] == nh.CHI2_REJECTED_ZERO_CELL:
        assert r["statistic"] == g["statistic"], what


@pytest.mark.parametrize("t", TYPES, ids=name)
def test_run_equals_refs(gpu, t):
    res = (6, 12)
    n = 1000 * res[0] * res[1]
    ps, angle = {nh.WARP_HENYEY_GREENSTEIN: (0.65, 0.5), nh.WARP_ANISO_PHASE: (0.35, 0.6),
                 nh.WARP_MICROFACET_BRDF: (0.6, 0.8)}.get(t, (0.5, 0.5))
    r = nh.run_warp_test(t, ps, angle, xres=res[1], yres=res[0], sample_count=n)
    g = wr.execute(t, ps, angle, True, res[1], res[0], n)
    np.testing.assert_array_equal(r["obs"], g["obs"])
    np.testing.assert_array_equal(r["wi"], g["wi"])
    assert r["obs_sum"] == g["obs_sum"] and r["sample_count"] == n and abs(r["level"] - g["level"]) <= 1e-15
    same_verdict(r, g, name(t))
    print(f"{name(t)}: {nh.CHI2_KINDS[r['kind']]}, statistic {r['statistic']:.6g}, dof {r['dof']}, p {r['p_value']:.4g}")


@pytest.mark.parametrize("t", TYPES, ids=name)
def test_reference_defaults_equal_fixture(gpu, golden, t):
    g = golden["runs"][name(t)]
    r = nh.run_warp_test(t, g["parameter_slider"], g["angle_slider"])
    assert (r["yres"], r["xres"], r["sample_count"]) == (g["yres"], g["xres"], g["sample_count"]) == wr.default_table(t)
    assert r["obs_sum"] == g["obs_sum"] and wr.digest(r["obs"]) == g["obs_sha256"]
    cells = g["cells"]
    np.testing.assert_array_equal(r["obs"][cells], np.array(g["obs"], F64))
    want = np.array([float.fromhex(x) for x in g["exp"]])
    bad = [(c, a, b) for c, a, b in zip(cells, r["exp"][cells], want) if not (a == b or abs(a - b) <= REL * abs(b))]
    assert not bad, bad
    es = float.fromhex(g["exp_sum"])
    assert abs(r["exp_sum"] - es) <= REL * abs(es)
    same_verdict(r, g, name(t))
    print(f"{name(t)}: {nh.CHI2_KINDS[r['kind']]}, p {r['p_value']:.6g}")


def test_fixture_verdicts(golden):
    """What the reference decides at its own table, by the restatement: the sphere volume is rejected (its pdf, the
    constant 4/3 pi, is no density on the sphere) and so is the disk (in the rim's cells adaptiveSimpson2D meets its
    absolute tolerance after 25 evaluations of a discontinuous integrand; p = 8e-5). Everything else is accepted, the
    sphere cap included: on runTest's unit vectors its pdf as written is the cap's density."""
    rejected = sorted(k for k, g in golden["runs"].items() if not g["accepted"])
    assert rejected == ["disk", "spherevol"]
    assert all(g["kind"] == nh.CHI2_REJECTED_P_VALUE for g in golden["runs"].values() if not g["accepted"])


def test_power(ctx):
    """A Beckmann histogram at alpha = 0.3 against the expected table of alpha = 0.4. At (8, 16), as at every even
    yres, the expected table has the docstring's NaN row, so the rejection there is for a p-value that is not finite;
    at (7, 14) no cell is NaN and the restatement gives a statistic of 249.3 at 27 degrees of freedom -- a tail of about
    1e-37, which 1 - cdf returns as 0 -- against 7.8 at 13 (p = 0.86) for the matching table: nowhere near the level."""
    for res, nan_row in (((8, 16), True), ((7, 14), False)):
        n = 1000 * res[0] * res[1]
        obs, _ = ctx.warp_histogram(nh.WARP_BECKMANN, 0.3, n, res[1], res[0])
        exp = ctx.warp_expected(nh.WARP_BECKMANN, 0.4, res[1], res[0], n)
        assert bool(np.isnan(exp).any()) == nan_row
        r = nh.chi2_test(obs, exp, n, 5.0, 0.01, 1)
        assert not r["accepted"] and r["kind"] == nh.CHI2_REJECTED_P_VALUE, (res, r)
        if not nan_row:
            assert r["p_value"] < 1e-12 and r["statistic"] > 200, r
        same = nh.chi2_test(obs, ctx.warp_expected(nh.WARP_BECKMANN, 0.3, res[1], res[0], n), n, 5.0, 0.01, 1)
        assert same["accepted"] == (not nan_row), (res, same)


# ---- 5. the CLI -------------------------------------------------------------------------------------------------------
def test_cli(gpu, golden):
    cli = os.path.join(os.path.dirname(nh.LIB_PATH), "nori_hip")
    for warp in ("beckmann", "spherecap"):
        g = golden["runs"][warp]
        r = subprocess.run(["timeout", "-k", "10", "120", cli, "--warptest", warp, "--param", str(g["parameter_slider"])],
                           capture_output=True, text=True, timeout=150)
        assert r.returncode == (0 if g["accepted"] else 1), (warp, r.returncode, r.stdout, r.stderr)
        verdict = "Accepted the null hypothesis (p-value = " if g["accepted"] else "***** Rejected ***** the null hypothesis"
        assert verdict in r.stdout and f"Chi^2 statistic = {g['statistic']:g} (d.o.f. = {g['dof']})" in r.stdout, r.stdout
    assert golden["runs"]["beckmann"]["accepted"]  # (--warptest beckmann --param 0.5 exits 0)
    r = subprocess.run([cli, "--warptest", "schlick"], capture_output=True, text=True, timeout=60)
    assert r.returncode == 1 and "NH_WARP_SCHLICK" in r.stderr
