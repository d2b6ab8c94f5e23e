"""The fused kernels' pair records arranged by kind (host/gpu_layout.cpp pair_layout, leaf_test<.., PAIRS>): the
wavefront framebuffer equals, element for element, the same render with NH_PAIR_KINDS=0 (the reference arrangement) and
the megakernel's. nh_render_stats::pair_kinds says which arrangement ran: 1 by default, 0 with the knob and for the
megakernel. Renders have collect_stats off unless stated (the counting kernels keep the reference arrangement). Every
case also checks on the host that its scene's leaves hold the pairs the case is about.
"""
import os

import numpy as np
import pytest

import nori_hip as nh
import scenegen
from pair_kind_helpers import leaf_table
from primary_mask_records import device_records

pytestmark = pytest.mark.gpu

W = H = 64
INSIDE = '<lookat target="-0.3, 0.6, -1" origin="0.1, 1.0, 0.5" up="0, 1, 0"/>'
LOOKAT = '<lookat target="0, 0.893051, 4.41198" origin="0, 0.919769, 5.41159" up="0, 1, 0"/>'

MESHES = {
    # Triangles that each span the box [-1, 1] x [0, 1.6] x [-1, 1] from corner to corner (and spheres below that nearly
    # fill it): no split of such primitives lowers the builder's cost, so a scene of them is one leaf.
    "pk_tri_a.obj": "v -1 0 -1\nv 1 0 1\nv 0 1.6 0\nf 1 2 3\n",
    "pk_tri_b.obj": "v -1 0 1\nv 1 0 -1\nv 0 1.6 0.2\nf 1 2 3\n",
    "pk_tri_c.obj": "v -1 1.6 -1\nv 1 1.5 1\nv 0.2 0 0\nf 1 2 3\n",
    "pk_tri_d.obj": "v 1 1.6 -1\nv -1 1.4 1\nv -0.2 0 -0.1\nf 1 3 2\n",
    "pk_quad.obj": "v -1 0 1\nv 1 0 1\nv 1 1.6 -1\nv -1 1.6 -1\nf 1 2 3\nf 1 3 4\n",
    "pk_tri_light.obj": "v -1 1.6 1\nv 1 1.6 -1\nv 0 0.1 -0.9\nf 1 3 2\n",
    "pk_small_light.obj": "v 0.23 1.58 -0.22\nv 0.23 1.58 0.16\nv -0.24 1.58 0.16\nf 1 2 3\n",
}
LIGHT = '<emitter type="area"><color name="radiance" value="4 4 4"/></emitter>'


def _mesh(name, inner):
    return f'<shape type="obj"><string name="filename" value="meshes/{name}"/>{inner}</shape>\n'


def _diffuse(albedo):
    return f'<bsdf type="diffuse"><color name="albedo" value="{albedo}"/></bsdf>'


def _sphere(center, radius, inner):
    return (f'<shape type="sphere"><point name="center" value="{center}"/><float name="radius" value="{radius}"/>'
            f'{inner}</shape>\n')


THREE_SPHERES = (_sphere("-0.15 0.8 0", 0.85, _diffuse("0.7 0.2 0.2")) + _sphere("0.15 0.8 0", 0.85, _diffuse("0.2 0.7 0.2")) +
                 _sphere("0 0.9 0.1", 0.8, _diffuse("0.6 0.6 0.1")))
# name -> (shapes, (triangle pairs, sphere pairs) of the scene's one leaf)
GENERATED = {
    "sphere_and_triangle": (
        _sphere("0 0.4 0", 0.4, _diffuse("0.6 0.5 0.3")) +
        _mesh("pk_small_light.obj", '<emitter type="area"><color name="radiance" value="15 15 15"/></emitter>'), (1, 1)),
    "three_spheres_five_triangles": (
        _mesh("pk_tri_light.obj", LIGHT) + _mesh("pk_tri_a.obj", _diffuse("0.7 0.7 0.7")) +
        _mesh("pk_tri_b.obj", _diffuse("0.2 0.5 0.7")) + _mesh("pk_tri_c.obj", _diffuse("0.7 0.4 0.6")) +
        _mesh("pk_tri_d.obj", _diffuse("0.3 0.3 0.8")) + THREE_SPHERES, (3, 2)),
    "spheres_only": (
        _sphere("0 1.4 0", 0.2, '<emitter type="area"><color name="radiance" value="12 12 12"/></emitter>') +
        _sphere("-0.4 0.4 0", 0.4, _diffuse("0.7 0.3 0.2")) + _sphere("0.45 0.35 0.3", 0.35, _diffuse("0.2 0.4 0.7")), (0, 2)),
    # a quad a second time, as a shape of its own with another albedo: every hit of it is an equal-t tie, which goes
    # to the later record -- between the slots of a pair, or between two pairs
    "duplicated_quad": (
        _mesh("pk_tri_light.obj", LIGHT) + _mesh("pk_quad.obj", _diffuse("0.7 0.7 0.7")) +
        _mesh("pk_quad.obj", _diffuse("0.1 0.6 0.2")) + _sphere("0.1 0.8 0", 0.85, _diffuse("0.6 0.6 0.6")), (3, 1)),
    "duplicated_sphere": (
        _mesh("pk_tri_light.obj", LIGHT) + _mesh("pk_tri_a.obj", _diffuse("0.7 0.7 0.7")) +
        _sphere("0 0.8 0", 0.85, _diffuse("0.8 0.1 0.1")) + _sphere("0 0.8 0", 0.85, _diffuse("0.1 0.2 0.8")), (1, 1)),
}


def _generated_xml(tmp, name):
    """A scene of GENERATED: the Cornell box's camera, sampler and integrator around the case's shapes."""
    c2 = scenegen.cbox_xml(str(tmp), "c2")
    text = open(c2).read()
    head = text[:text.index("<shape")]
    for mesh, obj in MESHES.items():
        with open(os.path.join(os.path.dirname(c2), "meshes", mesh), "w") as f:
            f.write(obj)
    path = os.path.join(os.path.dirname(c2), f"pk_{name}.xml")
    with open(path, "w") as f:
        f.write(head + GENERATED[name][0] + "</scene>\n")
    return path


def _scene(xml, old=None, new=None):
    if old is not None:
        text = open(xml).read()
        assert text.count(old) == 1, old
        xml = os.path.join(os.path.dirname(xml), "pk_edit.xml")
        with open(xml, "w") as f:
            f.write(text.replace(old, new))
    s = nh.Scene(xml)
    s.set_resolution(W, H)
    return s, nh.Bvh(s)


def _leaf_pairs(s, b):
    """(triangle pairs, sphere pairs) per leaf of the arrangement by kind, from the host function nh_upload_bvh uses."""
    return [tuple(int(x) for x in row[1:]) for row in nh.pair_layout(device_records(s, b), leaf_table(b))[1]]


def _render(s, b, mode, calls, seed, blocks=None, stats=False):
    ctx = nh.Context(0)
    ctx.upload(s, b)  # (reads NH_PAIR_KINDS)
    for i, (s0, s1) in enumerate(calls):
        ctx.render(s0, s1, seed=seed, traversal=nh.TRAVERSAL_ORDERED, clear=i == 0, stats=stats, mode=mode, blocks=blocks)
    ctx.synchronize()
    fb, st = ctx.framebuffer(), ctx.stats()
    ctx.close()
    return fb, st


def _check(monkeypatch, s, b, calls, seed, blocks=None, traits=None):
    monkeypatch.delenv("NH_PAIR_KINDS", raising=False)
    on, st_on = _render(s, b, nh.MODE_WAVEFRONT, calls, seed, blocks)
    mk, st_mk = _render(s, b, nh.MODE_MEGAKERNEL, calls, seed, blocks)
    monkeypatch.setenv("NH_PAIR_KINDS", "0")
    off, st_off = _render(s, b, nh.MODE_WAVEFRONT, calls, seed, blocks)
    assert (st_on["pair_kinds"], st_off["pair_kinds"], st_mk["pair_kinds"]) == (1, 0, 0)
    assert st_on["fused_bounce"] == 1 and st_off["fused_bounce"] == 1
    if traits is not None:
        assert st_on["bounce_traits"] == traits and st_off["bounce_traits"] == traits
    assert np.abs(on).sum() > 0
    np.testing.assert_array_equal(on, off)
    np.testing.assert_array_equal(on, mk)


def test_c2_trait_kernels(gpu, tmp_path, monkeypatch):
    """C2: the diffuse area-light kernels; leaf 0 holds 4 triangle pairs and the pair of the two spheres."""
    s, b = _scene(scenegen.cbox_xml(str(tmp_path), "c2"))
    assert _leaf_pairs(s, b) == [(4, 1), (2, 0)]
    _check(monkeypatch, s, b, [(0, 8)], 3, traits=2)


def test_c1_general_kernels(gpu, tmp_path, monkeypatch):
    """C1 (mirror and dielectric spheres): the general bounce kernels and the specular tail."""
    s, b = _scene(scenegen.cbox_xml(str(tmp_path), "c1"))
    assert _leaf_pairs(s, b) == [(4, 1), (2, 0)]
    _check(monkeypatch, s, b, [(0, 8)], 5, traits=1)


def test_c2_traits_off(gpu, tmp_path, monkeypatch):
    """C2 with NH_BOUNCE_TRAITS=0: the lean general kernels."""
    monkeypatch.setenv("NH_BOUNCE_TRAITS", "0")
    s, b = _scene(scenegen.cbox_xml(str(tmp_path), "c2"))
    _check(monkeypatch, s, b, [(0, 6)], 7, traits=1)


@pytest.mark.parametrize("name", list(GENERATED))
def test_generated_scene(gpu, tmp_path, monkeypatch, name):
    """Scenes of one leaf with at most 10 records (GENERATED)."""
    s, b = _scene(_generated_xml(tmp_path, name))
    assert len(leaf_table(b)) == 1 and leaf_table(b)[0][1] <= 10
    assert _leaf_pairs(s, b) == [GENERATED[name][1]]
    _check(monkeypatch, s, b, [(0, 6)], 11)


def test_camera_inside_a_sphere(gpu, tmp_path, monkeypatch):
    """C2 with a sphere around the box and the camera: that sphere's nearer root lies behind every ray's start, so its
    farther one is the candidate."""
    o, c, r = np.array([0, 0.919769, 5.41159]), np.array([0, 0.9, 2.5]), 4.0
    assert np.linalg.norm(o - c) < r
    around = _sphere("0 0.9 2.5", r, _diffuse("0.5 0.5 0.5"))
    s, b = _scene(scenegen.cbox_xml(str(tmp_path), "c2", extra_shapes=around))
    assert sum(n_sph for _, n_sph in _leaf_pairs(s, b)) >= 2
    _check(monkeypatch, s, b, [(0, 6)], 29, traits=2)


def test_camera_inside_the_box(gpu, tmp_path, monkeypatch):
    """C2 seen from between the spheres: rays start close to them, walls lie behind the camera."""
    s, b = _scene(scenegen.cbox_xml(str(tmp_path), "c2"), LOOKAT, INSIDE)
    _check(monkeypatch, s, b, [(0, 6)], 13, traits=2)


def test_several_calls(gpu, tmp_path, monkeypatch):
    """One render in three calls, the first starting at round 5."""
    s, b = _scene(scenegen.cbox_xml(str(tmp_path), "c2"))
    _check(monkeypatch, s, b, [(5, 8), (8, 10), (10, 13)], 17, traits=2)


def test_block_subset(gpu, tmp_path, monkeypatch):
    """Every other 32x32 block of the image."""
    s, b = _scene(scenegen.cbox_xml(str(tmp_path), "c2"))
    blocks = nh.tile_shard(W, H, 2, 1)
    assert 0 < len(blocks) < 4
    _check(monkeypatch, s, b, [(0, 8)], 19, blocks=blocks, traits=2)


@pytest.mark.parametrize("variant", ["c2", "c1"])
def test_counting_kernels_keep_the_reference_arrangement(gpu, tmp_path, monkeypatch, variant):
    """collect_stats on: the same framebuffer and the same counters with the knob on and off (an any-hit query counts
    the primitives up to its first hit, which depends on the order they are tested in); pair_kinds reads 0 both times."""
    s, b = _scene(scenegen.cbox_xml(str(tmp_path), variant))
    monkeypatch.delenv("NH_PAIR_KINDS", raising=False)
    on, st_on = _render(s, b, nh.MODE_WAVEFRONT, [(0, 6)], 23, stats=True)
    plain, st_plain = _render(s, b, nh.MODE_WAVEFRONT, [(0, 6)], 23)
    monkeypatch.setenv("NH_PAIR_KINDS", "0")
    off, st_off = _render(s, b, nh.MODE_WAVEFRONT, [(0, 6)], 23, stats=True)
    assert st_on["pair_kinds"] == 0 and st_off["pair_kinds"] == 0 and st_plain["pair_kinds"] == 1
    assert st_on["prims_tested"] > 0 and st_on["shadow_prims_tested"] > 0
    for k in ("ray_queries", "nodes_visited", "boxes_tested", "prims_tested", "shadow_queries", "shadow_nodes_visited",
              "shadow_boxes_tested", "shadow_prims_tested", "samples", "invalid_samples"):
        assert st_on[k] == st_off[k], k
    np.testing.assert_array_equal(on, off)
    np.testing.assert_array_equal(on, plain)
