"""The av (AverageVisibilityIntegrator) and envmaptester integrators on the GPU.

av: the per-path radiance query against the numpy restatement av_refs.av_paths bit for bit; renders against the paths
(box filter: every sample lands in its own pixel with weight 1, and sums of small integers are exact in fp32); the split
pipeline (wavefront mode) against the megakernel bit for bit, over traversal orders, split ranges, block subsets, a deep
tree on the wide traversal and the queue's edge cases; the reference's own test-av.xml through nh_test_run against
tests/golden/av_ttest.json; the adaptive sampler. envmaptester: the query against emitter_refs' fp64 pdf / 100 under the
tolerance and texel-edge exclusion of tests/test_gpu_emitter_envmap.py. The refusals are host-side checks made before any
launch."""
import importlib.util
import json
import os
import subprocess

import numpy as np
import pytest

import av_refs
import emitter_refs as er
import nori_hip as nh
import nori_oracle as no
import scenegen

HERE = os.path.dirname(os.path.abspath(__file__))
GOLDEN = os.path.join(HERE, "golden")
_spec = importlib.util.spec_from_file_location("envq", os.path.join(HERE, "test_gpu_emitter_envmap.py"))
envq = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(envq)  # its tolerance and exclusion: bound, rel_gap, MAX_LEFT_OUT; er.near_texel_edge

F32, F64 = np.float32, np.float64
MK, WF = nh.MODE_MEGAKERNEL, nh.MODE_WAVEFRONT
W, H, SPP = 24, 16, 8
LENGTHS = (0.05, 0.5, 1000.0)
SEED = 11


def occluder_obj(path):
    """208 flat triangles, `v` and `f` lines only: 8 x 13 small quads hovering over the floor and in front of the back
    wall, tilted so that neighbouring ones shade each other"""
    rng = np.random.default_rng(3)
    v, f = [], []
    for i in range(8):
        for j in range(13):
            c = np.array([-0.8 + 1.6 * j / 12, 0.15 + 1.4 * i / 7, -0.6 + 0.9 * rng.random()])
            a, b = rng.standard_normal(3), rng.standard_normal(3)
            a, b = 0.09 * a / np.linalg.norm(a), 0.09 * b / np.linalg.norm(b)
            k = len(v)
            v += [c - a - b, c + a - b, c + a + b, c - a + b]
            f += [(k + 1, k + 2, k + 3), (k + 1, k + 3, k + 4)]
    with open(path, "w") as g:
        g.write("".join("v %.7g %.7g %.7g\n" % tuple(p) for p in v))
        g.write("".join("f %d %d %d\n" % t for t in f))
    return len(f)


def dome_obj(path):
    """a small smooth-shaded cap with `vn` lines (the interpolated-pole branch of setHitInformation)"""
    n = 12
    with open(path, "w") as g:
        g.write("v 0 0.4 0.7\nvn 0 1 0\n")
        for k in range(n):
            a = 2 * np.pi * k / n
            d = np.array([0.5 * np.cos(a), 0.8, 0.5 * np.sin(a)])
            g.write("v %.7g %.7g %.7g\nvn %.7g %.7g %.7g\n" % (0.35 * np.cos(a), 0.05, 0.7 + 0.35 * np.sin(a),
                                                               *(d / np.linalg.norm(d))))
        for k in range(n):
            g.write("f 1//1 %d//%d %d//%d\n" % (2 + (k + 1) % n, 2 + (k + 1) % n, 2 + k, 2 + k))


@pytest.fixture(scope="module")
def work_dir(tmp_path_factory):
    return str(tmp_path_factory.mktemp("av_gpu"))


def av_scene_xml(work_dir, rfilter=""):
    """the Cornell box's walls and its two analytic spheres, the occluder quads and the smooth cap"""
    scenegen.materialize(work_dir)
    meshes = os.path.join(work_dir, "scenes/pa4/cbox/meshes")
    if not os.path.exists(os.path.join(meshes, "occluders.obj")):
        assert occluder_obj(os.path.join(meshes, "occluders.obj")) == 208
        dome_obj(os.path.join(meshes, "dome.obj"))
    extra = "".join(f'<shape type="obj"><string name="filename" value="meshes/{m}.obj"/><bsdf type="diffuse"/></shape>'
                    for m in ("occluders", "dome"))
    xml = scenegen.cbox_xml(work_dir, "c2", extra_shapes=extra)
    if rfilter:  # a reconstruction filter is a child of the camera
        text = open(xml).read()
        assert text.count("</camera>") == 1
        xml = xml[:-4] + "_rf.xml"
        with open(xml, "w") as f:
            f.write(text.replace("</camera>", rfilter + "</camera>"))
    return xml


def uploaded(xml, size, length=None, integrator=nh.INTEGRATOR_AV, index=0, sampler=None):
    s = nh.Scene(xml, index)
    if size:
        s.set_resolution(*size)
    if integrator is not None:
        s.set_integrator(integrator)
    if length is not None:
        s.set_av_params(length)
    if sampler:
        s.set_sample_count(sampler[0])
        s.set_sampler(nh.SAMPLER_ADAPTIVE, sampler[1])
    b = nh.Bvh(s)
    ctx = nh.Context(0)
    ctx.upload(s, b)
    return s, b, ctx


def all_paths(w, h, spp):
    pix = np.tile(np.arange(w * h, dtype=np.int32), spp)
    smp = np.repeat(np.arange(spp, dtype=np.int32), w * h)
    return pix, smp


def same_bits(a, b):
    a, b = np.ascontiguousarray(a, F32), np.ascontiguousarray(b, F32)
    np.testing.assert_array_equal(a.view(np.uint32), b.view(np.uint32))


def render(ctx, s0, s1, mode, traversal=nh.TRAVERSAL_REFERENCE, blocks=None, clear=True, seed=SEED, stats=False):
    ctx.render(s0, s1, seed=seed, mode=mode, traversal=traversal, blocks=blocks, clear=clear, stats=stats)
    ctx.synchronize()
    return ctx.framebuffer()


@pytest.fixture(scope="module")
def reference_paths(work_dir):
    """av_refs.av_paths of every path of the 24 x 16 x 8 scene, per length: computed once, shared, never written to"""
    xml = av_scene_xml(work_dir)
    pix, smp = all_paths(W, H, SPP)
    out = {}
    for length in LENGTHS:
        s = nh.Scene(xml)
        s.set_resolution(W, H)
        s.set_integrator(nh.INTEGRATOR_AV)
        s.set_av_params(length)
        r = av_refs.av_paths(s, no.OracleScene(s), SEED, pix, smp, detail=True)
        for v in r.values():
            if isinstance(v, np.ndarray):
                v.setflags(write=False)
        out[length] = r
    return out


# ---- 1. per-path parity, exact -------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("length", LENGTHS)
def test_radiance_query_equals_the_restatement(gpu, work_dir, reference_paths, length):
    ref = reference_paths[length]
    assert 0 < (ref["value"] == 0).sum() < ref["found"].sum() < len(ref["found"])  # occluded, open, escaped
    assert ref["draws"].max() > 7  # a rejected try
    hit = ref["shape"][ref["found"]]
    assert (hit == 3).sum() > 50 and (hit == 6).sum() > 50 and (hit == 7).sum() > 50  # a sphere, the quads, the cap
    if length == 1000.0:
        assert (ref["value"] == 0).sum() > (reference_paths[0.05]["value"] == 0).sum()
    _, _, ctx = uploaded(av_scene_xml(work_dir), (W, H), length)
    pix, smp = all_paths(W, H, SPP)
    g = ctx.radiance_query(pix, smp, seed=SEED)
    np.testing.assert_array_equal(g["rgb"][:, 0], ref["value"])
    np.testing.assert_array_equal(g["rgb"][:, 1], ref["value"])
    np.testing.assert_array_equal(g["rgb"][:, 2], ref["value"])


# ---- 2. a render is the sum of its paths (box filter) ----------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("mode", [MK, WF], ids=["megakernel", "wavefront"])
def test_box_filter_render_counts_the_ones(gpu, work_dir, reference_paths, mode):
    xml = av_scene_xml(work_dir, rfilter='<rfilter type="box"/>')
    s, _, ctx = uploaded(xml, (W, H), 0.5)
    b = s.desc.filter.border
    fb = render(ctx, 0, SPP, mode)[b:b + H, b:b + W]
    k = reference_paths[0.5]["value"].reshape(SPP, H, W).sum(0)
    want = np.stack([k, k, k, np.full((H, W), SPP, F32)], -1).astype(F32)
    np.testing.assert_array_equal(fb, want)


# ---- 3. the two modes under the default filter ---------------------------------------------------------------------
@pytest.mark.gpu
def test_modes_agree_bit_for_bit(gpu, work_dir):
    _, _, ctx = uploaded(av_scene_xml(work_dir), (70, 45), 0.5)
    base = render(ctx, 0, 3, MK)
    assert 0 < base[..., 0].sum() < base[..., 3].sum()
    for trav in (nh.TRAVERSAL_REFERENCE, nh.TRAVERSAL_ORDERED, nh.TRAVERSAL_WIDE):
        same_bits(render(ctx, 0, 3, MK, trav), base)
        same_bits(render(ctx, 0, 3, WF, trav), base)
    for mode in (MK, WF):
        render(ctx, 0, 1, mode)
        same_bits(render(ctx, 1, 3, mode, clear=False), base)
    blocks = [1, 3, 4]  # of the 3 x 2 block grid: the ragged right column and bottom row included
    same_bits(render(ctx, 0, 3, WF, blocks=blocks), render(ctx, 0, 3, MK, blocks=blocks))
    sub = render(ctx, 0, 3, WF, blocks=[4])
    b = ctx.scene.desc.filter.border
    # pixels more than a filter radius inside block 4 (x 32..63, y 32..44) receive that block's samples only
    np.testing.assert_array_equal(sub[b + 32 + 2:b + 45 - 2, b + 32 + 2:b + 64 - 2], base[b + 34:b + 43, b + 34:b + 62])


# ---- 4. a deep tree: the wide traversal ------------------------------------------------------------------------------
LADDER = [(128, 64), (132, 66), (136, 68), (160, 80)]  # BVH depths 17, 18, 19, 19: around the threshold


def pipeline_depth_threshold():
    """the tree depth above which the pools (and the av pipeline) pick the wide / persistent traversal, as written in
    nh_pipeline.hip"""
    import re
    src = open(os.path.join(os.path.dirname(HERE), "optix-renderer_amd/csrc/nh_pipeline.hip")).read()
    m = re.search(r"p\.persistent = c->depth > (\d+);", src)
    a = re.search(r"av_wide\(.*?c->depth > (\d+)", src, flags=re.S)
    assert m and a and m.group(1) == a.group(1)
    return int(m.group(1))


@pytest.mark.gpu
def test_deep_tree_runs_the_wide_traversal(gpu, work_dir):
    assert pipeline_depth_threshold() == 20
    chosen = None
    for n_phi, n_theta in LADDER:  # the smallest mesh of the ladder at which the context itself chooses the wide tree
        xml, _ = scenegen.bumpy_cbox_xml(work_dir, n_phi, n_theta)
        s, _, ctx = uploaded(xml, (48, 48), 0.15)
        wf = render(ctx, 0, 4, WF, nh.TRAVERSAL_ORDERED)
        if ctx.stats()["node_bytes"] != 64:
            chosen = (s, ctx, wf)
            break
        same_bits(wf, render(ctx, 0, 4, MK, nh.TRAVERSAL_ORDERED))  # below the threshold: the binary tree, still equal
    assert chosen is not None and (n_phi, n_theta) != LADDER[0], "the ladder must straddle the threshold"
    s, ctx, wf = chosen
    same_bits(wf, render(ctx, 0, 4, MK, nh.TRAVERSAL_ORDERED))
    same_bits(render(ctx, 0, 4, WF, nh.TRAVERSAL_WIDE), wf)
    rng = np.random.default_rng(9)
    pix = rng.integers(0, 48 * 48, 2048).astype(np.int32)
    smp = rng.integers(0, 64, 2048).astype(np.int32)
    ref = av_refs.av_paths(s, no.OracleScene(s), SEED, pix, smp)
    assert 100 < (ref == 0).sum() < 1900
    np.testing.assert_array_equal(ctx.radiance_query(pix, smp, seed=SEED)["rgb"][:, 0], ref)


# ---- 5. the queue's edges ------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_queue_edges(gpu, work_dir):
    xml = av_scene_xml(work_dir, rfilter='<rfilter type="box"/>')
    # 23 x 7 pixels, 3 rounds: 483 paths, not a multiple of 64. length 1e-3: every camera hit queues a ray, next to
    # nothing is within reach (the restatement says what is)
    s, _, ctx = uploaded(xml, (23, 7), 1e-3)
    b = s.desc.filter.border
    pix, smp = all_paths(23, 7, 3)
    ref = av_refs.av_paths(s, no.OracleScene(s), SEED, pix, smp, detail=True)
    found = int(ref["found"].sum())
    assert found > 400 and (ref["value"] == 0).sum() <= 2
    k = ref["value"].reshape(3, 7, 23).sum(0)
    want = np.stack([k, k, k, np.full((7, 23), 3, F32)], -1).astype(F32)
    fb = render(ctx, 0, 3, WF, stats=True)
    np.testing.assert_array_equal(fb[b:b + 7, b:b + 23], want)
    st = ctx.stats()
    assert st["ray_queries"] == 483 + found and st["shadow_queries"] == found  # 1 or 2 queries per path
    np.testing.assert_array_equal(render(ctx, 0, 3, WF)[b:b + 7, b:b + 23], want)  # and without the counters
    ctx.reset_stats()
    render(ctx, 0, 3, MK, stats=True)
    assert ctx.stats()["ray_queries"] == 483 + found
    # the camera turned away from everything: no camera ray hits, the queue stays empty, no any-hit launch is made
    text = open(xml).read()
    assert text.count('target="0, 0.893051, 4.41198"') == 1
    away = os.path.join(os.path.dirname(xml), "away.xml")
    with open(away, "w") as f:
        f.write(text.replace('target="0, 0.893051, 4.41198"', 'target="0, 0.919769, 6.5"'))
    s, _, ctx = uploaded(away, (23, 7), 0.5)
    ones = np.full((7, 23, 4), 3, F32)
    for stats in (False, True):
        ctx.reset_stats()
        fb = render(ctx, 0, 3, WF, stats=stats)
        np.testing.assert_array_equal(fb[b:b + 7, b:b + 23], ones)
        if stats:
            st = ctx.stats()
            assert st["ray_queries"] == 483 and st["shadow_queries"] == 0
    same_bits(fb, render(ctx, 0, 3, MK))


# ---- 6. the reference's own test -------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_reference_test_av(gpu, work_dir):
    with open(os.path.join(GOLDEN, "av_ttest.json")) as f:
        fx = json.load(f)
    path = os.path.join(av_refs.materialize(work_dir), "scenes/pa1/test-av.xml")
    res = nh.run_tests(path, seed=fx["seed"])
    assert len(res) == 4
    n = fx["sample_count"]
    for r, want, ref in zip(res, fx["scenes"], fx["references"]):
        assert r["accepted"] and r["sample_count"] == n and r["reference"] == ref
        assert r["mean"] == want["ones"] / n == want["mean"]
        assert r["variance"] == want["variance"] or abs(r["variance"] - want["variance"]) <= 1e-12 * want["variance"]
        assert abs(r["p_value"] - want["p_value"]) < 1e-6
    cli = os.path.join(os.path.dirname(nh.LIB_PATH), "nori_hip")
    out = subprocess.run([cli, path, "--seed", str(fx["seed"])], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stdout + out.stderr
    assert "Passed 4/4 tests." in out.stdout


# ---- 7. the adaptive sampler -----------------------------------------------------------------------------------------
FLAT = """<scene>
  <integrator type="av"><float name="length" value="0.001"/></integrator>
  <camera type="perspective">
    <transform name="toWorld"><lookat target="0, 0.4, 0" origin="0, 1.2, 3.2" up="0, 1, 0"/></transform>
    <float name="fov" value="40"/><integer name="width" value="16"/><integer name="height" value="12"/>
  </camera>
  <shape type="obj"><string name="filename" value="ground.obj"/><bsdf type="diffuse"/></shape>
</scene>
"""


@pytest.mark.gpu
def test_adaptive_sampler_constant_image(gpu, work_dir):
    """A ground quad in the plane y = 0 under an empty sky, length 1e-3. Every hit point has y == 0 exactly (a
    barycentric sum of zeros), so an occlusion ray meets the quad's plane at t == 0 < mint or not at all: every sample
    is one wherever the sampler puts it -- hits and escapes alike -- and every pixel's colour sum equals its weight sum
    bit for bit. (A curved or tilted surface would not do: a grazing ray re-enters it within 1e-3 about once in a
    thousand hits, in the reference as here.)"""
    d = os.path.join(work_dir, "flat")
    os.makedirs(d, exist_ok=True)
    with open(os.path.join(d, "ground.obj"), "w") as f:
        f.write("v -4 0 -4\nv 4 0 -4\nv 4 0 4\nv -4 0 4\nf 1 4 3 2\n")
    xml = os.path.join(d, "flat.xml")
    with open(xml, "w") as f:
        f.write(FLAT)
    fbs = []
    for _ in range(2):
        s, _, ctx = uploaded(xml, None, integrator=None, sampler=(4, 2))
        assert s.desc.integrator == nh.INTEGRATOR_AV and s.av_params() == float(F32(1e-3))
        fb = render(ctx, 0, 4, MK)
        assert ctx.adaptive_stats()["total_samples"] >= 16 * 12 * 4
        b = s.desc.filter.border
        core = fb[b:b + 12, b:b + 16]
        assert np.all(core[..., 3] > 0)
        np.testing.assert_array_equal(core[..., :3], np.repeat(core[..., 3:], 3, -1))  # every pixel is one
        fbs.append(fb)
    same_bits(fbs[0], fbs[1])


# ---- 8. envmaptester -------------------------------------------------------------------------------------------------
EW, EH = 64, 48


def env_pixel_samples():
    rng = np.random.default_rng(17)
    return (rng.random((2048, 2)) * np.array([EW, EH])).astype(F32)


def camera_directions_f64(camera, ps):
    """the camera ray's direction with every operation in fp64 on the float32 matrices and sample positions"""
    s2c = np.array(list(camera.sample_to_camera), F32).reshape(4, 4).astype(F64)
    c2w = np.array(list(camera.camera_to_world), F32).reshape(4, 4).astype(F64)
    inv = np.array(list(camera.inv_output_size), F32).astype(F64)
    x = np.stack([ps[:, 0].astype(F64) * inv[0], ps[:, 1].astype(F64) * inv[1], np.zeros(len(ps)), np.ones(len(ps))], -1)
    r = x @ s2c.T
    d = r[:, :3] / r[:, 3:]
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    return d @ c2w[:3, :3].T


def env_refs(scene):
    e = scene.desc.env
    rgba = np.ctypeslib.as_array(e.rgba, shape=(e.width * e.height, 4)).copy()
    kw = dict(scale=(e.scale_u, e.scale_v), offset=(e.offset_u, e.offset_v), spherical=bool(e.spherical),
              rotation=tuple(e.rotation[k] for k in range(9)), constant=bool(e.constant), normalization=e.normalization)
    rad = tuple(e.radiance[k] for k in range(3))
    return (er.EnvRef(e.width, e.height, rgba, rad, T, **kw) for T in (F32, F64))


def envmaptester_expectation(scene):
    ps = env_pixel_samples()
    r32, r64 = env_refs(scene)
    d32 = av_refs.camera_rays(scene.desc.camera, ps)[1]
    d64 = camera_directions_f64(scene.desc.camera, ps)
    _, i32, _, _ = r32.eval(d32)
    _, i64, pu, pv = r64.eval(d64)
    keep = envq.kept({"texel": i32}, {"texel": i64, "pu": pu, "pv": pv})  # the cap MAX_LEFT_OUT, asserted there
    return ps, keep, r32.pdf(d32) / F32(100), r64.pdf(d64) / 100.0


def env_scene(work_dir):
    xml = scenegen.envmap_xml(os.path.join(work_dir, "env"), EW, EH, 2, area_light=False)
    s = nh.Scene(xml)
    s.set_integrator(nh.INTEGRATOR_ENVMAPTESTER)
    return s


def test_envmaptester_samples_respect_the_exclusion_cap(work_dir):
    """CPU: at most MAX_LEFT_OUT of the chosen pixel samples have an fp64 texel coordinate within 1e-3 of an integer,
    and on the others fp32 and fp64 name the same texel (asserted by the other test file's kept())"""
    ps, keep, p32, p64 = envmaptester_expectation(env_scene(work_dir))
    assert 1.0 - keep.mean() <= envq.MAX_LEFT_OUT and (p64[keep] > 0).sum() > 1000


@pytest.mark.gpu
def test_envmaptester(gpu, work_dir):
    s = env_scene(work_dir)
    ps, keep, p32, p64 = envmaptester_expectation(s)
    b = nh.Bvh(s)
    ctx = nh.Context(0)
    ctx.upload(s, b)
    g = ctx.radiance_query(np.zeros(len(ps), np.int32), np.zeros(len(ps), np.int32), seed=1, pixel_sample=ps)["rgb"]
    np.testing.assert_array_equal(g[:, 0], g[:, 1])
    np.testing.assert_array_equal(g[:, 0], g[:, 2])
    gap, err = envq.rel_gap(p32[keep], p64[keep]), envq.rel_gap(g[keep, 0], p64[keep])
    print(f"envmaptester: fp32 gap {gap:.3g}, device {err:.3g}, {100 * (1 - keep.mean()):.2f} % left out")
    assert err <= envq.bound(gap), (err, gap)
    assert np.all(g[keep & (p64 == 0), 0] == 0)
    s.set_resolution(16, 12)
    ctx.upload(s, nh.Bvh(s))
    mk = render(ctx, 0, 2, MK)
    assert mk[..., 3].sum() > 0 and mk[..., 0].sum() > 0
    same_bits(render(ctx, 0, 2, WF), mk)


# ---- 9. refusals -----------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_refusals(gpu, work_dir):
    s = nh.Scene(av_scene_xml(work_dir))
    s.set_resolution(W, H)
    s.set_integrator(nh.INTEGRATOR_AV)
    s.set_av_params(0.5)
    ctx = nh.Context(0)
    ctx.upload(s, nh.Bvh(s), av_params=False)
    for call in (lambda: ctx.render(0, 1, mode=MK), lambda: ctx.render(0, 1, mode=WF),
                 lambda: ctx.radiance_query([0], [0]), lambda: ctx.ttest_scene(64)):
        with pytest.raises(nh.NoriError, match="nh_set_av_params"):
            call()
    with pytest.raises(nh.NoriError):
        ctx.set_av_params(float("nan"))
    ctx.set_av_params()
    assert ctx.radiance_query([0], [0])["rgb"].shape == (1, 3)
    ctx.upload(s, nh.Bvh(s), av_params=False)  # every scene upload forgets the length
    with pytest.raises(nh.NoriError, match="nh_set_av_params"):
        ctx.render(0, 1)
    # envmaptester on a descriptor built by hand, without an environment map
    s.set_integrator(nh.INTEGRATOR_ENVMAPTESTER)
    assert s.desc.envmap < 0
    ctx.upload(s, nh.Bvh(s))
    for call in (lambda: ctx.render(0, 1), lambda: ctx.radiance_query([0], [0])):
        with pytest.raises(nh.NoriError, match="This integrator requires an env map."):
            call()
