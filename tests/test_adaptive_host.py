"""The adaptive sampler off the GPU: the loader and the appended nh_scene_desc fields, the reference's two adaptive
scenes, and the fp32 restatement (optix-renderer_amd/adaptive_refs.py) against what can be stated without a render --
the recorded Eigen reductions, the uniform passes' order, the zero-variance branch."""
import ctypes
import json
import os

import numpy as np
import pytest

import adaptive_refs as ar
import nori_hip as nh

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")

SCENE = """<scene>
<integrator type="path_mis"/>
<sampler type="{type}">{props}</sampler>
<camera type="perspective"><integer name="width" value="8"/><integer name="height" value="8"/></camera>
<shape type="sphere"><point name="center" value="0, 0, 5"/><float name="radius" value="1"/><bsdf type="diffuse"/>
<emitter type="area"><color name="radiance" value="1, 1, 1"/></emitter></shape>
</scene>
"""


def load(tmp_path, type, props=""):
    p = tmp_path / "s.xml"
    p.write_text(SCENE.format(type=type, props=props))
    return nh.Scene(str(p))


def ints(**kw):
    return "".join(f'<integer name="{k}" value="{v}"/>' for k, v in kw.items())


@pytest.mark.parametrize("props, count, uniform", [
    ("", 1, 1),                                          # sampleCount 1, initialUniform 2 clamped to it
    (ints(sampleCount=100), 100, 2),                     # the default initialUniform
    (ints(sampleCount=100, initialUniform=7), 100, 7),
    (ints(sampleCount=3, initialUniform=9), 3, 3),
    (ints(sampleCount=3, initialUniform=0), 3, 1),
    (ints(sampleCount=3, initialUniform=-4), 3, 1),
])
def test_loader_accepts_adaptive_and_clamps(tmp_path, props, count, uniform):
    s = load(tmp_path, "adaptive", props)
    d = s.desc
    assert (d.sampler, d.sample_count, d.adaptive_initial_uniform) == (nh.SAMPLER_ADAPTIVE, count, uniform)
    assert ar.clamp_initial_uniform(uniform, count) == uniform


def test_independent_and_unknown_samplers(tmp_path):
    s = load(tmp_path, "independent", ints(sampleCount=4))
    d = s.desc
    assert (d.sampler, d.sample_count, d.adaptive_initial_uniform) == (nh.SAMPLER_INDEPENDENT, 4, 0)
    with pytest.raises(nh.NoriError, match=r'sampler "stratified" is not supported \(the HIP path uses per-path pcg32\)'):
        load(tmp_path, "stratified")


def test_set_sampler(tmp_path):
    s = load(tmp_path, "independent", ints(sampleCount=4))
    s.set_sampler(nh.SAMPLER_ADAPTIVE, 9)
    assert (s.desc.sampler, s.desc.adaptive_initial_uniform) == (nh.SAMPLER_ADAPTIVE, 4)
    s.set_sampler(nh.SAMPLER_ADAPTIVE, 0)
    assert s.desc.adaptive_initial_uniform == 1
    s.set_sampler(nh.SAMPLER_INDEPENDENT)
    assert (s.desc.sampler, s.desc.adaptive_initial_uniform) == (nh.SAMPLER_INDEPENDENT, 0)
    with pytest.raises(nh.NoriError, match="invalid sampler type"):
        s.set_sampler(2)


def test_desc_fields_are_appended():
    """sampler and adaptive_initial_uniform are the last two fields, after everything the struct held before."""
    names = [n for n, _ in nh.nh_scene_desc._fields_]
    assert names[-3:] == ["ambient_medium", "sampler", "adaptive_initial_uniform"]
    D = nh.nh_scene_desc
    assert D.sampler.offset == D.ambient_medium.offset + 4
    assert D.adaptive_initial_uniform.offset == D.sampler.offset + 4
    assert ctypes.sizeof(D) == (D.adaptive_initial_uniform.offset + 4 + 7) // 8 * 8


@pytest.mark.parametrize("xml, integrator, shapes", [
    (ar.DISNEY_SPHERE_XML, nh.INTEGRATOR_PATH_MATS, 3),
    (ar.DISNEY_TEST_XML, nh.INTEGRATOR_PATH_MIS, 1),
])
def test_reference_adaptive_scenes_load(tmp_path, xml, integrator, shapes):
    """scenes/project/disney/disney_sphere.xml and disney-test.xml as they are (their mesh and images are stand-ins)."""
    s = nh.Scene(os.path.join(ar.materialize(str(tmp_path)), xml))
    d = s.desc  # (points into s)
    assert (d.sampler, d.sample_count, d.adaptive_initial_uniform) == (nh.SAMPLER_ADAPTIVE, 100, 2)
    assert (d.camera.width, d.camera.height, d.integrator, d.n_shapes) == (800, 800, integrator, shapes)
    assert any(d.bsdfs[i].type == nh.BSDF_DISNEY for i in range(d.n_bsdfs))
    assert d.envmap >= 0


def bits(x):
    return np.ascontiguousarray(x, np.float32).view(np.uint32)


def bit(x):
    return int(np.float32(x).view(np.uint32))


def test_reductions_equal_the_eigen_recording():
    """sum(), squaredNorm() and normalize() of the restatement against the results recorded from the reference's
    vendored Eigen (tests/golden/adaptive_eigen_redux.json), every block shape from 1x1 to 4x4, bit for bit."""
    with open(os.path.join(GOLDEN, "adaptive_eigen_redux.json")) as f:
        rec = json.load(f)
    assert rec["eigen"] == "3.3.8" and len(rec["cases"]) == 64
    shapes, serial_differs = set(), 0
    for c in rec["cases"]:
        r, n = c["rows"], c["cols"]
        shapes.add((r, n))
        a = np.array(c["a"], np.uint32).view(np.float32).reshape(r, n)
        b = np.array(c["b"], np.uint32).view(np.float32).reshape(r, n)
        assert bit(ar.eigen_redux_sum(ar._colmajor(a) - ar._colmajor(b))) == c["diff_sum"]
        assert bit(ar.eigen_redux_sum(ar._colmajor(a))) == c["a_sum"]
        z = ar.eigen_squared_norm(ar._colmajor(b))
        assert bit(z) == c["b_squared_norm"]
        assert np.array_equal(bits((b / np.sqrt(z, dtype=np.float32)).astype(np.float32)).ravel(), c["b_normalized"])
        left_to_right = np.float32(0)
        for v in ar._colmajor(a):
            left_to_right = np.float32(left_to_right + v)
        serial_differs += int(bit(left_to_right) != c["a_sum"])
    assert len(shapes) == 16
    assert serial_differs > 0  # the recording tells the packet order from a plain loop


FLT = (np.float32(2.0), np.float32(16.0), np.concatenate([np.linspace(1, 0.03, 32), [0]]).astype(np.float32))


def constant_paths(calls):
    def path(x, y, sample):
        calls.append((x, y, sample))
        return np.array([0.25, 0.5, 0.75], np.float32), np.array([0.5, 0.5], np.float32)
    return path


def test_uniform_passes_are_transposed_x_major():
    """On a 4-divisible image the uniform passes visit a block's pixels with the pair's first member as x: x outer,
    y inner (the independent sampler's order), path i of pass k of outer sample s at sample index (s 1002 + k) 16 + i."""
    calls = []
    r = ar.AdaptiveRender(8, 8, FLT, 2, 2, constant_paths(calls))
    r.render(0, 1)
    blocks = ar.spiral_blocks(8, 8)
    assert blocks == [(4, 4, 4, 4), (0, 4, 4, 4), (0, 0, 4, 4), (4, 0, 4, 4)]  # BlockGenerator: centre, left, up, right
    at = 0
    for (ox, oy, sx, sy), (_, _, passes, _, _, _) in zip(blocks, r.log):
        for k in range(passes):
            chunk = calls[at:at + 16]
            at += 16
            assert [c[2] for c in chunk] == [k * 16 + i for i in range(16)]
            if k < 3:  # initialUniform 2: passes 0 to 2 are uniform
                assert [(c[0], c[1]) for c in chunk] == [(ox + x, oy + y) for x in range(4) for y in range(4)]
    assert at == len(calls) == r.stats()["total_samples"]


def test_constant_radiance_puts_every_adaptive_sample_on_element_15():
    """A flat block image gives a zero variance matrix (max - min < Epsilon), normalize() leaves it, the DiscretePDF
    stays zero, and lower_bound sends every draw to the last element: pixel (3, 3), read back as x = 3, y = 3. The next
    test then sees the pixels that pass left without weight and stops the block: 3 uniform passes and 1 adaptive."""
    calls = []
    r = ar.AdaptiveRender(8, 8, FLT, 2, 2, constant_paths(calls))
    r.render(0, 2)
    assert len(r.log) == 8
    for _, bi, passes, reason, n_adaptive, picks in r.log:
        assert (passes, reason, n_adaptive) == (4, "norm", 1)
        assert picks == [[15] * 16]
    ox, oy = r.blocks[0][:2]
    assert [(c[0], c[1]) for c in calls[48:64]] == [(ox + 3, oy + 3)] * 16
    assert r.stats() == {"total_samples": 8 * 4 * 16, "passes": 32, "max_passes": 4, "n_blocks": 4}
    assert np.all(r.variance() == 0)


def test_ragged_blocks_leave_the_block():
    """A 6x3 image: the 2x3 edge block's uniform pass reads {i < size.y, j < size.x} as (x, y), so x runs to 2 in a
    block 2 wide, and y only to 1 in a block 3 tall."""
    calls = []
    r = ar.AdaptiveRender(6, 3, FLT, 2, 2, constant_paths(calls))
    r.render(0, 1)
    edge = r.blocks.index((4, 0, 2, 3))
    at = sum(sum(b[2] * b[3] for _ in range(l[2])) for b, l in zip(r.blocks[:edge], r.log[:edge]))
    assert [(c[0], c[1]) for c in calls[at:at + 6]] == [(4 + i, j) for i in range(3) for j in range(2)]


def test_sample_index_bound():
    top = ((ar.max_sample_count() - 1) * ar.PASS_STRIDE + ar.MAX_ROUND + 1) * ar.PATHS_PER_PASS + 15
    assert top < 2 ** 31 and ar.max_sample_count() == nh.ADAPTIVE_MAX_SAMPLES
