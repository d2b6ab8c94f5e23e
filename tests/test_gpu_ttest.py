"""The per-path radiance query (nh_radiance_query) and the reference's t-test procedure (src/utils/ttest.cpp) on the
GPU: the query against the CPU oracle's path bit for bit and against a render's framebuffer; the scene and BSDF
estimators (nh_ttest_scene, nh_ttest_bsdf) against the oracle per sample and against fsum moments; the reference's five
scene t-test files and its microfacet t-test through nh_test_run, with the verdicts predicted from the oracle
(tests/golden/ttest_seed2.json); the CLI; the refusals.

Tolerance of the moments: both sides are fp64 sums of n <= 1e5 terms, worst case n 2^-53 ~ 1e-11 relative; 1e-9 leaves two
orders for conditioning (the device sums in a tree, the fixture with math.fsum, the oracle's BSDF loop with Welford's
recurrence)."""
import importlib.util
import json
import math
import os
import subprocess

import numpy as np
import pytest

import light_scenes
import nori_hip as nh
import nori_oracle as no
import scenegen
import volume_refs as vr

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
_spec = importlib.util.spec_from_file_location("make_ttest_fixture", os.path.join(GOLDEN, "make_ttest_fixture.py"))
fixture_maker = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(fixture_maker)  # the fixture's own definitions: oracle_luminance, two_pass, FILES

F32 = np.float32
FILES = fixture_maker.FILES
COUNTS = dict(zip(FILES, (4, 10, 15, 6, 4)))
REL = 1e-9


def close(a, b, rel=REL):
    return a == b or abs(a - b) <= rel * abs(b)


def luminance(rgb):
    rgb = np.asarray(rgb, F32).reshape(-1, 3)
    return rgb[:, 0] * F32(0.212671) + rgb[:, 1] * F32(0.715160) + rgb[:, 2] * F32(0.072169)


def same_bits(a, b):
    """assert_array_equal on the bit patterns (NaN = the same NaN, -0 != +0)."""
    a, b = np.ascontiguousarray(a, F32), np.ascontiguousarray(b, F32)
    np.testing.assert_array_equal(a.view(np.uint32), b.view(np.uint32))


def uploaded(xml, size=None, integrator=None, index=0):
    s = nh.Scene(xml, index)
    if size:
        s.set_resolution(*size)
    if integrator is not None:
        s.set_integrator(integrator)
    b = nh.Bvh(s)
    ctx = nh.Context(0)
    ctx.upload(s, b)
    return s, b, ctx


def with_camera_children(xml, children, tag):
    """A copy of the scene file, next to it, with `children` inserted as the camera's first children."""
    text = open(xml).read()
    assert text.count('<camera type="perspective">') == 1
    out = os.path.join(os.path.dirname(xml), f"{tag}_{os.path.basename(xml)}")
    with open(out, "w") as f:
        f.write(text.replace('<camera type="perspective">', '<camera type="perspective">' + children))
    return out


@pytest.fixture(scope="module")
def work_dir(tmp_path_factory):
    d = str(tmp_path_factory.mktemp("ttest"))
    vr.materialize(d)
    light_scenes.materialize(d)
    return scenegen.materialize(d)


@pytest.fixture(scope="module")
def golden():
    with open(os.path.join(GOLDEN, "ttest_seed2.json")) as f:
        return json.load(f)


def random_pairs(n, n_pixels, n_samples, seed):
    rng = np.random.default_rng(seed)
    return rng.integers(0, n_pixels, n).astype(np.int32), rng.integers(0, n_samples, n).astype(np.int32)


# ---- 1. the query is the oracle's path, bit for bit ---------------------------------------------------------------
@pytest.mark.parametrize("integrator", [pytest.param(nh.INTEGRATOR_PATH_MIS, id="path_mis"),
                                        pytest.param(nh.INTEGRATOR_PATH_MATS, id="path_mats"),
                                        pytest.param(nh.INTEGRATOR_DIRECT_MIS, id="direct_mis")])
def test_query_equals_oracle_path(gpu, work_dir, integrator):
    W, H = 24, 16
    s, _, ctx = uploaded(scenegen.cbox_xml(work_dir, "c1"), (W, H), integrator)
    oracle = no.OracleScene(s)
    pixel, sample = random_pairs(512, W * H, 64, 7)
    got = ctx.radiance_query(pixel, sample, seed=7)
    want = [oracle.path(7, int(p) % W, int(p) // W, int(k)) for p, k in zip(pixel, sample)]
    same_bits(got["rgb"], np.array([w[0] for w in want]))
    same_bits(got["jitter"], np.array([w[1] for w in want]))
    assert np.any(got["rgb"] > 0)
    # the image-plane position spelled out: the same ray, the same draws
    ps = np.stack([(pixel % W).astype(F32) + got["jitter"][:, 0], (pixel // W).astype(F32) + got["jitter"][:, 1]], 1)
    again = ctx.radiance_query(pixel, sample, seed=7, pixel_sample=ps)
    same_bits(again["rgb"], got["rgb"])
    same_bits(again["jitter"], got["jitter"])
    # another seed is another set of paths
    assert not np.array_equal(ctx.radiance_query(pixel, sample, seed=8)["rgb"], got["rgb"])


def test_query_thin_lens_takes_the_renders_lens_sample(gpu, work_dir):
    W, H = 24, 16
    xml = with_camera_children(scenegen.cbox_xml(work_dir, "c2"), '<float name="lensRadius" value="0.08"/>'
                               '<float name="focalDistance" value="3.2"/>', "dof")
    s, _, ctx = uploaded(xml, (W, H))
    oracle = no.OracleScene(s)
    pixel, sample = random_pairs(128, W * H, 64, 11)
    got = ctx.radiance_query(pixel, sample, seed=3)
    want = [oracle.path(3, int(p) % W, int(p) // W, int(k)) for p, k in zip(pixel, sample)]
    same_bits(got["rgb"], np.array([w[0] for w in want]))
    same_bits(got["jitter"], np.array([w[1] for w in want]))


# ---- 2. the query is what a render accumulates, for what the oracle lacks -----------------------------------------
def check_query_equals_render(xml, integrator=None):
    W, H, SPP, SEED = 8, 6, 6, 5
    s, _, ctx = uploaded(with_camera_children(xml, '<rfilter type="box"/>', "box"), (W, H), integrator)
    assert s.border == 0
    ctx.render(0, SPP, seed=SEED, clear=True)
    fb = ctx.framebuffer()
    pixel = np.repeat(np.arange(W * H, dtype=np.int32), SPP)
    sample = np.tile(np.arange(SPP, dtype=np.int32), W * H)
    q = ctx.radiance_query(pixel, sample, seed=SEED)
    # the box filter's table ends in 0 at distance 0.5 exactly, i.e. at a zero jitter component: none here
    assert np.all(q["jitter"] > 0) and np.all(q["jitter"] < 1)
    rgb = q["rgb"].reshape(H, W, SPP, 3)
    valid = (np.isfinite(rgb) & (rgb >= 0)).all(axis=3)  # ImageBlock::put drops the others with their weight
    want = np.zeros((H, W, 4), F32)
    for k in range(SPP):  # fp32 sums in round order
        want[..., :3] += np.where(valid[:, :, k, None], rgb[:, :, k], F32(0))
        want[..., 3] += valid[:, :, k].astype(F32)
    same_bits(fb, want)
    assert np.any(want[..., :3] > 0)
    return valid


@pytest.mark.parametrize("integrator", [pytest.param(nh.INTEGRATOR_PATH_VOL_MATS, id="path_vol_mats"),
                                        pytest.param(nh.INTEGRATOR_PATH_VOL_MIS, id="path_vol_mis")])
def test_query_equals_render_volume(gpu, work_dir, integrator):
    check_query_equals_render(os.path.join(work_dir, "scenes/project/volume/cbox_homog_dielectric_medium.xml"), integrator)


def test_query_equals_render_spot_light(gpu, work_dir):
    check_query_equals_render(os.path.join(work_dir, light_scenes.SPOT_XML))


# ---- 3. the scene estimator on the reference's 1x1 scenes ---------------------------------------------------------
@pytest.mark.parametrize("name", FILES)
def test_ttest_scene_equals_oracle(gpu, work_dir, name):
    N, SEED = 4096, 2
    s, _, ctx = uploaded(os.path.join(work_dir, "scenes", name))
    assert (s.width, s.height) == (1, 1)
    want = fixture_maker.oracle_luminance(no.OracleScene(s), SEED, N)
    mean, var, lum = ctx.ttest_scene(N, seed=SEED, luminance=True)
    same_bits(lum, want)
    m2, v2 = fixture_maker.two_pass(want)
    print(f"{name}: mean {mean!r} (fsum {m2!r}), variance {var!r} (fsum {v2!r})")
    assert close(mean, m2) and close(var, v2), (mean, m2, var, v2)
    # a later window of the same streams
    m3, v3, part = ctx.ttest_scene(1000, seed=SEED, first=1000, luminance=True)
    same_bits(part, want[1000:2000])
    m4, v4 = fixture_maker.two_pass(want[1000:2000])
    assert close(m3, m4) and close(v3, v4)
    # the reduction's order depends on n alone
    assert ctx.ttest_scene(N, seed=SEED) == (mean, var)
    assert ctx.ttest_scene(N, seed=SEED, luminance=True)[:2] == (mean, var)


def test_reduction_edges(gpu, work_dir):
    """n around a wave, a workgroup's 4096 samples and several partials: every split of the device sum."""
    s, _, ctx = uploaded(scenegen.cbox_xml(work_dir, "c1"), (6, 4))
    _, _, want = ctx.ttest_scene(3 * 4096 + 77, seed=4, luminance=True)
    assert len(np.unique(want)) > 100  # (a sum worth the name)
    for n in (2, 3, 63, 64, 65, 255, 257, 4095, 4096, 4097, 3 * 4096 + 77):
        mean, var, lum = ctx.ttest_scene(n, seed=4, luminance=True)
        same_bits(lum, want[:n])
        m2, v2 = fixture_maker.two_pass(want[:n])
        assert close(mean, m2) and close(var, v2), (n, mean, m2, var, v2)


# ---- 4. the scene estimator on a camera of several pixels ---------------------------------------------------------
def test_ttest_scene_multi_pixel(gpu, work_dir):
    W, H, N, SEED = 6, 4, 4096, 9
    s, _, ctx = uploaded(scenegen.cbox_xml(work_dir, "c1"), (W, H))
    _, _, lum = ctx.ttest_scene(N, seed=SEED, luminance=True)
    ps = np.zeros((N, 2), F32)
    for k in range(N):
        r = no.Pcg32.per_path(SEED, 0, k)
        ps[k, 0] = F32(r.next_float()) * F32(W)
        ps[k, 1] = F32(r.next_float()) * F32(H)
    q = ctx.radiance_query(np.zeros(N, np.int32), np.arange(N, dtype=np.int32), seed=SEED, pixel_sample=ps)
    same_bits(lum, luminance(q["rgb"]))
    assert len(np.unique(lum)) > N // 16  # the samples do cover the image, not one pixel


# ---- 5. the reference's files pass, as predicted from the oracle --------------------------------------------------
@pytest.mark.parametrize("name", FILES)
def test_reference_scene_tests_pass(gpu, work_dir, golden, name):
    g = golden["files"][name]
    res = nh.run_tests(os.path.join(work_dir, "scenes", name), seed=golden["seed"])
    assert len(res) == COUNTS[name] == len(g["scenes"])
    for i, (r, want) in enumerate(zip(res, g["scenes"])):
        print(f"{name} scene {i}: mean {r['mean']!r} variance {r['variance']!r} p {r['p_value']:.6g} "
              f"(oracle {want['mean']!r} {want['variance']!r} {want['p_value']:.6g})")
    for i, (r, want) in enumerate(zip(res, g["scenes"])):
        assert r["sample_count"] == g["sample_count"] == 100000
        assert r["reference"] == g["references"][i]
        assert close(r["mean"], want["mean"]) and close(r["variance"], want["variance"]), (i, r, want)
        assert abs(r["p_value"] - want["p_value"]) <= 1e-6, (i, r, want)
        assert r["accepted"], (i, r)
    level = 1.0 - (1.0 - float(F32(0.01))) ** (1.0 / len(res))
    assert min(r["p_value"] for r in res) > 10 * level  # (the smallest, 0.116 of 6 tests, is 70 levels up)


# ---- 6. the BSDF estimator -----------------------------------------------------------------------------------------
def test_ttest_bsdf_equals_oracle(gpu, work_dir):
    path = os.path.join(work_dir, "scenes/pa3/tests/ttest-microfacet.xml")
    t = nh.Test(path)
    n = t.sample_count
    ctx = nh.Context(0)
    rng = no.Pcg32()  # one running default-state stream, as ttest.cpp's `random`
    mine = []
    for j, (angle, ref) in enumerate(zip(t.angles, t.references)):
        m2, v2 = no.ttest_bsdf(t.bsdfs[0], float(angle), rng, n)
        mean, var = ctx.ttest_bsdf(t.bsdfs[0], float(angle), n, first_draw=2 * n * j)
        print(f"angle {angle}: mean {mean!r} (oracle {m2!r}), variance {var!r} (oracle {v2!r})")
        assert close(mean, m2) and close(var, v2), (angle, mean, m2, var, v2)
        ok, p = nh.students_t_test(mean, var, float(ref), n, float(t.significance_level), len(t.references))
        assert ok, (angle, mean, ref, p)
        mine.append((mean, var))
    res = nh.run_tests(path)
    assert [(r["mean"], r["variance"]) for r in res] == mine
    assert [F32(r["angle"]) for r in res] == t.angles and all(r["accepted"] for r in res)
    # the stream is the reference's: draws 2k, 2k + 1 of the default-state pcg32
    _, _, lum = ctx.ttest_bsdf(t.bsdfs[0], 45.0, 64, first_draw=10, luminance=True)
    r = no.Pcg32()
    for _ in range(10):
        r.next_uint()
    wi = np.array([math.sin(float(F32(math.radians(45.0)))), 0.0, math.cos(float(F32(math.radians(45.0))))], F32)
    want = []
    for _ in range(64):
        sx, sy = r.next_float(), r.next_float()
        want.append(no.bsdf_sample(t.bsdfs[0], wi, (sx, sy))[1])
    same_bits(lum, luminance(np.array(want)))


# ---- 7. the CLI ----------------------------------------------------------------------------------------------------
def test_cli_runs_test_files(gpu, work_dir):
    cli = os.path.join(os.path.dirname(nh.LIB_PATH), "nori_hip")
    furnace = os.path.join(work_dir, "scenes/pa4/tests/test-furnace.xml")

    def run(path):
        return subprocess.run(["timeout", "-k", "10", "120", cli, path, "--seed", "2"], capture_output=True, text=True,
                              timeout=150)
    r = run(furnace)
    assert r.returncode == 0, (r.stdout, r.stderr)
    assert "Passed 4/4 tests." in r.stdout
    assert r.stdout.count("Accepted the null hypothesis") == 4 and "Rejected" not in r.stdout
    assert r.stdout.count("Sample mean = ") == 4 and r.stdout.count("Sample variance = ") == 4
    assert r.stdout.count("t-statistic = ") == 4 and "(d.o.f. = 99999)" in r.stdout
    text = open(furnace).read()
    head = text.index('value="', text.index('<string name="references"')) + len('value="')
    assert text[head:head + 2] == "2,"
    wrong = os.path.join(os.path.dirname(furnace), "test-furnace-wrong.xml")
    with open(wrong, "w") as f:
        f.write(text[:head] + "2.5" + text[head + 1:])
    r = run(wrong)
    assert r.returncode not in (0, 124, 137), (r.returncode, r.stdout, r.stderr)
    assert "Passed 3/4 tests." in r.stdout
    assert r.stdout.count("***** Rejected ***** the null hypothesis") == 1


# ---- 8. refusals ---------------------------------------------------------------------------------------------------
def test_refusals(gpu, work_dir):
    W, H = 24, 16
    xml = scenegen.cbox_xml(work_dir, "c2")
    s, _, ctx = uploaded(xml, (W, H))
    ok = ctx.radiance_query([W * H - 1], [0])
    assert ok["rgb"].shape == (1, 3)
    with pytest.raises(nh.NoriError, match="outside"):
        ctx.radiance_query([W * H], [0])
    with pytest.raises(nh.NoriError, match="outside"):
        ctx.radiance_query([-1], [0])
    with pytest.raises(nh.NoriError, match="negative sample"):
        ctx.radiance_query([0], [-1])
    with pytest.raises(nh.NoriError, match="n >= 2|2 <= n"):
        ctx.ttest_scene(1)
    with pytest.raises(nh.NoriError, match="must be uploaded"):
        nh.Context(0).radiance_query([0], [0])
    dof = with_camera_children(xml, '<float name="lensRadius" value="0.08"/><float name="focalDistance" value="3.2"/>',
                               "dof_refused")
    _, _, dctx = uploaded(dof, (W, H))
    with pytest.raises(nh.NoriError, match="thin-lens camera is not supported"):
        dctx.ttest_scene(64)
    with pytest.raises(nh.NoriError, match="chi2test is not supported by the HIP path"):
        nh.run_tests(os.path.join(work_dir, "scenes/pa3/tests/chi2test-microfacet.xml"))
