"""The adaptive sampler's render loop on the GPU against its fp32 restatement (optix-renderer_amd/adaptive_refs.py,
paths from the CPU oracle at the same per-path seeds): the RGBW master by np.array_equal, and with every render
nh_get_adaptive_stats and nh_get_adaptive_variance. Then the refusals, and an independent-sampler render before and
after an adaptive one on the same context.

Every test loads or sets the adaptive sampler: none can pass on a build whose loader refuses it."""
import numpy as np
import pytest

import adaptive_refs as ar
import nori_hip as nh
import nori_oracle as no
import scenegen

pytestmark = pytest.mark.gpu

# Seeds picked on the CPU with the restatement so that the renders reach the branches named in `reaches_branches`
SEED = 2


def cbox(scene_dir, size, integrator, initial_uniform=2, spp=2):
    s = nh.Scene(scenegen.cbox_xml(scene_dir, "c1", spp=spp))
    s.set_resolution(*size)
    s.set_integrator(integrator)
    s.set_sampler(nh.SAMPLER_ADAPTIVE, initial_uniform)
    return s


CONSTANT_ENV = """<scene>
<integrator type="path_mats"/>
<sampler type="adaptive"><integer name="sampleCount" value="2"/></sampler>
<camera type="perspective">
<transform name="toWorld"><lookat target="0, 0, 1" origin="0, 0, 0" up="0, 1, 0"/></transform>
<float name="fov" value="40"/><integer name="width" value="8"/><integer name="height" value="8"/>
</camera>
<shape type="sphere"><point name="center" value="0, 0, -100"/><float name="radius" value="1"/><bsdf type="diffuse"/></shape>
<emitter type="envmap"><texture type="constant_color" name="albedo"><color name="value" value="0.25, 0.5, 0.75"/></texture></emitter>
</scene>
"""


def uploaded(scene):
    ctx = nh.Context(0)
    ctx.upload(scene, nh.Bvh(scene))
    return ctx


_refs = {}


def reference(key, scene, seed, oracle_scene=None):
    """The restatement's render of outer samples [0, 2) of `scene`, computed once per key and never changed
    afterwards. oracle_scene: the scene the CPU oracle traces the paths in, when it is not `scene` itself."""
    if key not in _refs:
        r = ar.for_scene(scene, no.OracleScene(oracle_scene or scene), seed)
        r.render(0, 2)
        master = r.master.copy()
        master.setflags(write=False)
        _refs[key] = (master, r.stats(), r.variance(), r.log)
    return _refs[key]


def check(ctx, ref):
    master, stats, variance, _ = ref
    assert np.array_equal(ctx.framebuffer(), master)
    assert ctx.adaptive_stats() == stats
    assert np.array_equal(ctx.adaptive_variance(), variance)


def reaches_branches(log):
    """A block that stops by var_diff > oldNorm after an adaptive pass, and a block that runs more than 4 passes."""
    return (any(reason == "norm" and n_adaptive >= 1 for _, _, _, reason, n_adaptive, _ in log) and
            any(passes > 4 for _, _, passes, _, _, _ in log))


@pytest.mark.parametrize("integrator", [pytest.param(nh.INTEGRATOR_PATH_MIS, id="path_mis"),
                                        pytest.param(nh.INTEGRATOR_PATH_MATS, id="path_mats")])
def test_cbox_16x16(gpu, scene_dir, integrator):
    """16 full blocks, sampleCount 2."""
    s = cbox(scene_dir, (16, 16), integrator)
    ref = reference(("cbox16", integrator), s, SEED)
    assert reaches_branches(ref[3])
    assert ref[1]["n_blocks"] == 16
    ctx = uploaded(s)
    ctx.render(0, 2, seed=SEED, clear=True)
    check(ctx, ref)


def test_ragged_blocks(gpu, scene_dir):
    """10x6: blocks clipped in both directions, whose transposed positions leave the block and the image."""
    s = cbox(scene_dir, (10, 6), nh.INTEGRATOR_PATH_MIS)
    ref = reference("cbox10x6", s, SEED)
    assert reaches_branches(ref[3])
    assert ref[1]["n_blocks"] == 6
    ctx = uploaded(s)
    ctx.render(0, 2, seed=SEED, clear=True)
    check(ctx, ref)


def test_initial_uniform_1(gpu, scene_dir):
    """initialUniform 1: the third pass of a block is already adaptive."""
    s = cbox(scene_dir, (16, 16), nh.INTEGRATOR_PATH_MIS, initial_uniform=1)
    assert s.desc.adaptive_initial_uniform == 1
    ref = reference("cbox16_iu1", s, SEED)
    assert reaches_branches(ref[3])
    ctx = uploaded(s)
    ctx.render(0, 2, seed=SEED, clear=True)
    check(ctx, ref)


def test_volumetric_integrator(gpu, scene_dir):
    """The adaptive path kernel's volumetric branch: on a scene without media path_vol_mats computes path_mats (as
    tests/test_gpu_volume.py pins for the independent sampler), which the oracle has."""
    s = cbox(scene_dir, (8, 8), nh.INTEGRATOR_PATH_VOL_MATS)
    ref = reference("cbox8_vol", s, SEED, oracle_scene=cbox(scene_dir, (8, 8), nh.INTEGRATOR_PATH_MATS))
    ctx = uploaded(s)
    ctx.render(0, 2, seed=SEED, clear=True)
    check(ctx, ref)


def test_mode_and_traversal_change_nothing(gpu, scene_dir):
    s = cbox(scene_dir, (16, 16), nh.INTEGRATOR_PATH_MIS)
    ref = reference(("cbox16", nh.INTEGRATOR_PATH_MIS), s, SEED)
    ctx = uploaded(s)
    ctx.render(0, 2, seed=SEED, clear=True, mode=nh.MODE_WAVEFRONT, traversal=nh.TRAVERSAL_WIDE)
    check(ctx, ref)


def test_constant_environment(gpu, tmp_path):
    """Every ray sees the same radiance: the variance image of a pass is flat, the distribution zero, and the one
    adaptive pass of a block puts all 16 samples on element 15."""
    p = tmp_path / "constant_env.xml"
    p.write_text(CONSTANT_ENV)
    s = nh.Scene(str(p))
    ref = reference("constant_env", s, 5)
    picks = [e for _, _, _, _, _, passes in ref[3] for pk in passes for e in pk]
    assert picks and all(e == 15 for e in picks)
    assert all(passes == 4 for _, _, passes, _, _, _ in ref[3])
    ctx = uploaded(s)
    ctx.render(0, 2, seed=5, clear=True)
    check(ctx, ref)


def test_split_range(gpu, scene_dir):
    """One call over [0, 2) against the calls [0, 1) and [1, 2): the block streams live across calls."""
    s = cbox(scene_dir, (16, 16), nh.INTEGRATOR_PATH_MIS)
    ref = reference(("cbox16", nh.INTEGRATOR_PATH_MIS), s, SEED)
    ctx = uploaded(s)
    ctx.render(0, 1, seed=SEED, clear=True)
    ctx.render(1, 2, seed=SEED)
    check(ctx, ref)


def test_refusals(gpu, scene_dir):
    s = cbox(scene_dir, (16, 16), nh.INTEGRATOR_PATH_MIS)
    ctx = uploaded(s)
    with pytest.raises(nh.NoriError, match="adaptive sampler: a render of chosen 32x32 blocks"):
        ctx.render(0, 1, seed=SEED, blocks=[0])
    with pytest.raises(nh.NoriError, match="must start at 0 or continue"):
        ctx.render(1, 2, seed=SEED)
    ctx.render(0, 1, seed=SEED, clear=True)
    with pytest.raises(nh.NoriError, match="must start at 0 or continue"):
        ctx.render(2, 3, seed=SEED)
    with pytest.raises(nh.NoriError, match="overflows the int32 path sample index"):
        ctx.render(1, nh.ADAPTIVE_MAX_SAMPLES + 1, seed=SEED)
    xml = scenegen.cbox_xml(scene_dir, "c1", spp=2)
    text = open(xml).read().replace('<camera type="perspective">',
                                    '<camera type="perspective"><float name="lensRadius" value="0.05"/>')
    lens = xml.replace(".xml", "_lens.xml")
    with open(lens, "w") as f:
        f.write(text)
    t = nh.Scene(lens)
    t.set_resolution(16, 16)
    t.set_sampler(nh.SAMPLER_ADAPTIVE, 2)
    ctx2 = uploaded(t)
    with pytest.raises(nh.NoriError, match="thin-lens camera is not supported"):
        ctx2.render(0, 1, seed=SEED, clear=True)


def test_staging_budget_refusal(gpu, scene_dir, monkeypatch):
    """Under path_mats the box's black corner blocks run all 1001 passes: over 4000 staged block images in an outer
    sample, more than a 1 MiB budget (1024 images) holds. The render is refused, and so is a range continuing it."""
    s = cbox(scene_dir, (16, 16), nh.INTEGRATOR_PATH_MATS)
    assert reference(("cbox16", nh.INTEGRATOR_PATH_MATS), s, SEED)[1]["max_passes"] == 1001
    ctx = uploaded(s)
    monkeypatch.setenv("NH_ADAPTIVE_STAGING_MB", "1")
    with pytest.raises(nh.NoriError, match="exceed the staging budget of 1 MiB"):
        ctx.render(0, 1, seed=SEED, clear=True)
    monkeypatch.delenv("NH_ADAPTIVE_STAGING_MB")
    with pytest.raises(nh.NoriError, match="must start at 0 or continue"):
        ctx.render(1, 2, seed=SEED)
    ctx.render(0, 2, seed=SEED, clear=True)
    check(ctx, reference(("cbox16", nh.INTEGRATOR_PATH_MATS), s, SEED))


def test_independent_render_unchanged_around_an_adaptive_one(gpu, scene_dir):
    plain = nh.Scene(scenegen.cbox_xml(scene_dir, "c1", spp=2))
    plain.set_resolution(16, 16)
    adaptive = cbox(scene_dir, (16, 16), nh.INTEGRATOR_PATH_MIS)
    bvh = nh.Bvh(plain)
    ctx = nh.Context(0)
    ctx.upload(plain, bvh)
    ctx.render(0, 2, seed=SEED, clear=True)
    before = ctx.framebuffer()
    with pytest.raises(nh.NoriError, match="no adaptive render"):
        ctx.adaptive_stats()
    ctx.upload(adaptive, bvh)
    ctx.render(0, 2, seed=SEED, clear=True)
    check(ctx, reference(("cbox16", nh.INTEGRATOR_PATH_MIS), adaptive, SEED))
    ctx.upload(plain, bvh)
    ctx.render(0, 2, seed=SEED, clear=True)
    assert np.array_equal(ctx.framebuffer(), before)
