"""The light samples' any-hit queries from the flat image's any-hit section (host/shadow_masks.cpp shadow_any_word,
host/gpu_layout.cpp flat_image, csrc/nh_traverse.h trace_flat<.., ANY>): the wavefront framebuffer equals, element for
element, the same render with NH_ANY_LIST=0 (those queries test the closest-hit pair records) and the megakernel's.
nh_render_stats::any_list says how many records the queries could test: 4 on the Cornell box by default; 0 with the
knob, for the megakernel, and for a scene without a section (nothing can be left out, or the scene is not flat). Every
case checks on the host what its scene's word keeps, so an equal image shows that leaving records out changes nothing,
not that nothing was left out. 64 x 64 pixels at 4 spp.
"""
import os

import numpy as np
import pytest

import nori_hip as nh
import scenegen
from flat_trace_helpers import LIGHT, cluster_scene, diffuse, is_flat_tree, load, mesh, sphere, write_scene
from pair_kind_helpers import leaf_table
from primary_mask_records import device_records, is_sphere
from test_gpu_flat_trace import THREE_SPHERES, TWO_SPHERES, _two_leaf_scene

pytestmark = pytest.mark.gpu

W = H = 64
SPP = 4
ALL = (1 << 64) - 1


def _render(s, b, mode, seed):
    ctx = nh.Context(0)
    ctx.upload(s, b)  # (reads NH_ANY_LIST)
    ctx.render(0, SPP, seed=seed, traversal=nh.TRAVERSAL_ORDERED, clear=True, mode=mode)
    ctx.synchronize()
    fb, st = ctx.framebuffer(), ctx.stats()
    ctx.close()
    return fb, st


def _write_mesh(xml, name, text):
    with open(os.path.join(os.path.dirname(xml), "meshes", name), "w") as f:
        f.write(text)


def _kept(s, b):
    """the records the scene's any-hit word keeps, or None when it leaves nothing out"""
    rec = device_records(s, b)
    word = nh.shadow_any_word(s.desc.camera, rec, nh.shadow_emitter_faces(s.desc))
    if word & ((1 << len(rec)) - 1) == (1 << len(rec)) - 1:
        return None
    return [k for k in range(len(rec)) if (word >> k) & 1]


def _check(monkeypatch, s, b, seed, any_list, flat=1):
    monkeypatch.delenv("NH_ANY_LIST", raising=False)
    on, st_on = _render(s, b, nh.MODE_WAVEFRONT, seed)
    mk, st_mk = _render(s, b, nh.MODE_MEGAKERNEL, seed)
    monkeypatch.setenv("NH_ANY_LIST", "0")
    off, st_off = _render(s, b, nh.MODE_WAVEFRONT, seed)
    assert (st_on["any_list"], st_off["any_list"], st_mk["any_list"]) == (any_list, 0, 0)
    assert (st_on["flat_trace"], st_off["flat_trace"]) == (flat, flat)
    assert np.abs(on).sum() > 0
    assert np.array_equal(on, off)
    assert np.array_equal(on, mk)


@pytest.mark.parametrize("variant", ["c2", "c1"])
def test_cornell_box(gpu, tmp_path, monkeypatch, variant):
    """C2 (the diffuse area-light kernels) and C1 (the general ones): the queries test the spheres' pair in the left
    leaf and the light's in the right one, 4 records of 14."""
    s, b = load(scenegen.cbox_xml(str(tmp_path), variant), W, H)
    rec = device_records(s, b)
    kept = _kept(s, b)
    assert kept is not None and len(kept) == 4 and sum(is_sphere(rec[k]) for k in kept) == 2
    _check(monkeypatch, s, b, 3, 4)


def test_c2_lean_general_kernels(gpu, tmp_path, monkeypatch):
    monkeypatch.setenv("NH_BOUNCE_TRAITS", "0")
    s, b = load(scenegen.cbox_xml(str(tmp_path), "c2"), W, H)
    _check(monkeypatch, s, b, 7, 4)


def test_left_leaf_keeps_nothing(gpu, tmp_path, monkeypatch):
    """The Cornell box without its spheres: the left leaf is eight wall triangles and keeps no record (its box is the
    root's), the right one keeps the light's two."""
    s, b = load(scenegen.cbox_xml(str(tmp_path), "c2", drop_spheres=True), W, H)
    assert leaf_table(b) == [(0, 8), (8, 4)]
    assert _kept(s, b) == [9, 10]
    _check(monkeypatch, s, b, 5, 2)


def test_right_leaf_keeps_nothing(gpu, tmp_path, monkeypatch):
    """The same box lit from a light that lies on the floor and faces up: the light shares the left leaf with the
    floor, the right leaf is the other eight wall triangles and keeps no record."""
    xml = scenegen.cbox_xml(str(tmp_path), "c2", drop_spheres=True)
    _write_mesh(xml, "al_floor_light.obj", "v -0.24 0.01 -0.22\nv 0.23 0.01 -0.22\nv 0.23 0.01 0.16\nv -0.24 0.01 0.16\n"
                                           "f 1 3 2\nf 1 4 3\n")
    text = open(xml).read()
    assert text.count("meshes/light.obj") == 1
    xml = os.path.join(os.path.dirname(xml), "al_floor.xml")
    with open(xml, "w") as f:
        f.write(text.replace("meshes/light.obj", "meshes/al_floor_light.obj"))
    s, b = load(xml, W, H)
    assert leaf_table(b) == [(0, 4), (4, 8)]
    assert _kept(s, b) == [1, 2]
    _check(monkeypatch, s, b, 9, 2)


def test_single_leaf(gpu, tmp_path, monkeypatch):
    """A tetrahedral room, a light triangle and a sphere: one leaf of 6 records, the word keeps the light and the
    sphere."""
    A, B, C, D = "-1 0 -0.75", "1 0 -0.75", "0 0 1.25", "0 1.5 0"
    meshes = {"al_t0.obj": f"v {A}\nv {B}\nv {C}\nf 1 2 3\n", "al_t1.obj": f"v {A}\nv {B}\nv {D}\nf 1 2 3\n",
              "al_t2.obj": f"v {B}\nv {C}\nv {D}\nf 1 2 3\n", "al_t3.obj": f"v {C}\nv {A}\nv {D}\nf 1 2 3\n",
              "al_tl.obj": "v -0.1 0.75 -0.1\nv 0.1 0.75 -0.1\nv 0 0.75 0.15\nf 1 2 3\n"}
    shapes = ("".join(mesh(k, diffuse("0.6 0.6 0.6")) for k in list(meshes)[:4]) + mesh("al_tl.obj", LIGHT.format(12)) +
              sphere("0 0.25 0.1", 0.15, diffuse("0.3 0.5 0.6")))
    xml = write_scene(tmp_path, "al_tet", shapes, meshes, lookat='<lookat target="0, 0.3, 0" origin="0, 0.35, 0.8" up="0, 1, 0"/>')
    s, b = load(xml, W, H)
    rec = device_records(s, b)
    kept = _kept(s, b)
    assert leaf_table(b) == [(0, 6)] and len(kept) == 2 and sum(is_sphere(rec[k]) for k in kept) == 1
    _check(monkeypatch, s, b, 11, 2)


def test_single_leaf_without_a_list(gpu, tmp_path, monkeypatch):
    """One leaf of 7 records that is no enclosure: nothing is left out, no section."""
    xml, _ = cluster_scene(tmp_path, "one", [(-1.0, 1.0)], THREE_SPHERES, plane_pair=False)
    s, b = load(xml, W, H)
    assert leaf_table(b) == [(0, 7)] and _kept(s, b) is None
    _check(monkeypatch, s, b, 11, 0)


def test_two_leaves_camera_in_the_right_box(gpu, tmp_path, monkeypatch):
    """The hand-built two-leaf scene whose camera rays enter the right box first: no enclosure, no section."""
    s, b = _two_leaf_scene(tmp_path)
    assert _kept(s, b) is None
    _check(monkeypatch, s, b, 13, 0)


def test_poked_wall(gpu, tmp_path, monkeypatch):
    """C2 with a slab (one triangle: the tree stays two leaves) that pokes 0.05 through the right wall: the word is all
    ones, the image has no section and the any-hit queries read the closest-hit records."""
    xml = scenegen.cbox_xml(str(tmp_path), "c2")  # (the right wall is the plane x = 1)
    _write_mesh(xml, "al_slab.obj", "v 0.6 0.5 -0.2\nv 1.05 0.5 -0.2\nv 1.05 0.5 0.2\nf 1 2 3\n")
    slab = ('<shape type="obj"><string name="filename" value="meshes/al_slab.obj"/>' + diffuse("0.5 0.5 0.5") + "</shape>")
    s, b = load(scenegen.cbox_xml(str(tmp_path), "c2", extra_shapes=slab), W, H)
    rec = device_records(s, b)
    assert len(rec) == 15 and leaf_table(b) == [(0, 11), (11, 4)] and _kept(s, b) is None
    _check(monkeypatch, s, b, 17, 0)


def test_three_leaves_walk_the_tree(gpu, tmp_path, monkeypatch):
    """Three leaves, not flat: no image, no section."""
    xml, _ = cluster_scene(tmp_path, "three", [(-4.5, -2.7), (-2.0, -0.2), (0.2, 2.0)], TWO_SPHERES)
    s, b = load(xml, W, H)
    assert len(leaf_table(b)) == 3 and not is_flat_tree(b)
    _check(monkeypatch, s, b, 19, 0, flat=0)
