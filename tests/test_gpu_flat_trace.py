"""Flat traversal in the fused bounce kernels (csrc/nh_traverse.h trace_flat; host/gpu_layout.cpp flat_image): for a
scene whose tree is one leaf, or a root with two leaves, the wavefront framebuffer equals, element for element, the same
render with NH_FLAT_TRACE=0 (every query walks the tree) and the megakernel's. nh_render_stats::flat_trace says which
ran: 1 by default for such a scene, 0 with the knob, for the megakernel and for a deeper tree. Every case checks on the
host that its scene has the tree the case is about.
"""
import os

import numpy as np
import pytest

import nori_hip as nh
import scenegen
from flat_trace_helpers import (CLUSTER_ORIGIN, cluster_scene, diffuse, is_flat_tree, leaf_of_record, load, same_bits,
                                sphere, tree_boxes)
from pair_kind_helpers import leaf_table
from primary_mask_records import device_records, is_sphere

pytestmark = pytest.mark.gpu

W = H = 64
SPP = 4
TWO_SPHERES = (sphere("-1.2 0.5 0.1", 0.35, diffuse("0.6 0.5 0.3")) + sphere("1.3 0.45 -0.2", 0.3, diffuse("0.3 0.5 0.6")))
THREE_SPHERES = (sphere("0 0.8 0", 0.85, diffuse("0.6 0.5 0.3")) + sphere("0.15 0.8 0", 0.85, diffuse("0.3 0.5 0.6")) +
                 sphere("0 0.9 0.1", 0.8, diffuse("0.6 0.6 0.1")))


def _render(s, b, mode, traversal, seed):
    ctx = nh.Context(0)
    ctx.upload(s, b)  # (reads NH_FLAT_TRACE)
    ctx.render(0, SPP, seed=seed, traversal=traversal, clear=True, mode=mode)
    ctx.synchronize()
    fb, st = ctx.framebuffer(), ctx.stats()
    ctx.close()
    return fb, st


def _check(monkeypatch, s, b, seed, traversal=nh.TRAVERSAL_ORDERED, flat=1, traits=None):
    monkeypatch.delenv("NH_FLAT_TRACE", raising=False)
    on, st_on = _render(s, b, nh.MODE_WAVEFRONT, traversal, seed)
    mk, st_mk = _render(s, b, nh.MODE_MEGAKERNEL, traversal, seed)
    monkeypatch.setenv("NH_FLAT_TRACE", "0")
    off, st_off = _render(s, b, nh.MODE_WAVEFRONT, traversal, seed)
    assert (st_on["flat_trace"], st_off["flat_trace"], st_mk["flat_trace"]) == (flat, 0, 0)
    assert st_on["fused_bounce"] == 1 and st_off["fused_bounce"] == 1 and st_on["pair_kinds"] == 1
    if traits is not None:
        assert st_on["bounce_traits"] == traits and st_off["bounce_traits"] == traits
    assert np.abs(on).sum() > 0
    assert np.array_equal(on, off)
    assert np.array_equal(on, mk)


@pytest.mark.parametrize("traversal", [nh.TRAVERSAL_ORDERED, nh.TRAVERSAL_REFERENCE])
@pytest.mark.parametrize("variant,traits", [("c2", 2), ("c1", 1)])
def test_cornell_box(gpu, tmp_path, monkeypatch, variant, traits, traversal):
    """C2 (the diffuse area-light kernels) and C1 (the general ones, mirror and dielectric spheres): two leaves, the
    left child's box the root's. The reference's visit order runs the general kernels."""
    s, b = load(scenegen.cbox_xml(str(tmp_path), variant), W, H)
    assert is_flat_tree(b) and leaf_table(b) == [(0, 10), (10, 4)]
    boxes = tree_boxes(b)
    assert same_bits(boxes[6:12], boxes[0:6]) and not same_bits(boxes[12:18], boxes[0:6])
    _check(monkeypatch, s, b, 3, traversal, traits=traits if traversal == nh.TRAVERSAL_ORDERED else 1)


def test_c2_lean_general_kernels(gpu, tmp_path, monkeypatch):
    """C2 with NH_BOUNCE_TRAITS=0: the lean general kernels."""
    monkeypatch.setenv("NH_BOUNCE_TRAITS", "0")
    s, b = load(scenegen.cbox_xml(str(tmp_path), "c2"), W, H)
    _check(monkeypatch, s, b, 7, traits=1)


def test_single_leaf(gpu, tmp_path, monkeypatch):
    """One leaf of 7 records: a light, three triangles and three spheres."""
    xml, _ = cluster_scene(tmp_path, "one", [(-1.0, 1.0)], THREE_SPHERES, plane_pair=False)
    s, b = load(xml, W, H)
    rec = device_records(s, b)
    assert leaf_table(b) == [(0, 7)] and sum(is_sphere(r) for r in rec) == 3
    _check(monkeypatch, s, b, 11)


def _two_leaf_scene(tmp_path):
    """Two clusters side by side, a sphere in each, and two triangles in the plane y = 0.8 that cover each other
    between the clusters, one in each leaf. The camera sits inside the right child's box and outside the left one's, so
    its rays enter the right box first."""
    xml, names = cluster_scene(tmp_path, "two", [(-2.0, -0.2), (0.2, 2.0)], TWO_SPHERES)
    s, b = load(xml, W, H)
    leaves = leaf_table(b)
    assert is_flat_tree(b) and len(leaves) == 2
    rec, leaf_of = device_records(s, b), leaf_of_record(b)
    shape_leaf = {int(r[7]): leaf_of[k] for k, r in enumerate(rec) if not is_sphere(r)}  # (one triangle per mesh)
    pl, pr = names.index("plane_l"), names.index("plane_r")
    assert shape_leaf[pl] == 0 and shape_leaf[pr] == 1  # the coincident triangles lie in different leaves
    # they lie in one plane and their boxes overlap in x and z
    rl, rr = rec[[k for k, r in enumerate(rec) if int(r[7]) == pl and not is_sphere(r)][0]], \
        rec[[k for k, r in enumerate(rec) if int(r[7]) == pr and not is_sphere(r)][0]]
    assert {float(rl[1]), float(rl[5]), float(rl[9]), float(rr[1]), float(rr[5]), float(rr[9])} == {np.float32(0.8)}
    assert max(rl[0], rl[4], rl[8]) > min(rr[0], rr[4], rr[8])
    assert sum(is_sphere(r) for k, r in enumerate(rec) if leaf_of[k] == 0) == 1
    assert sum(is_sphere(r) for k, r in enumerate(rec) if leaf_of[k] == 1) == 1
    boxes = tree_boxes(b).reshape(3, 6)
    o = np.array(CLUSTER_ORIGIN, np.float32)
    assert (boxes[2][:3] < o).all() and (o < boxes[2][3:]).all()  # inside the right child's box
    assert not ((boxes[1][:3] <= o).all() and (o <= boxes[1][3:]).all())  # outside the left one's
    assert not same_bits(boxes[1], boxes[0]) and not same_bits(boxes[2], boxes[0])
    return s, b


@pytest.mark.parametrize("traversal", [nh.TRAVERSAL_ORDERED, nh.TRAVERSAL_REFERENCE])
def test_two_leaves_camera_in_the_right_box(gpu, tmp_path, monkeypatch, traversal):
    s, b = _two_leaf_scene(tmp_path)
    _check(monkeypatch, s, b, 13, traversal)


def test_zero_direction_component(gpu, tmp_path, monkeypatch):
    """C2 through a camera whose toWorld scales y by 0: every camera ray's direction has y = 0 exactly, so its
    reciprocal is infinite and the box tests take the reference's branchy form."""
    xml = scenegen.cbox_xml(str(tmp_path), "c2")
    text = open(xml).read()
    assert text.count('<scale value="-1,1,1"/>') == 1
    a = text.index("<lookat")
    text = text[:a] + '<lookat target="0, 0.8, 0" origin="0.1, 0.8, 5" up="0, 1, 0"/>' + text[text.index("/>", a) + 2:]
    xml = os.path.join(os.path.dirname(xml), "flat_zero_dy.xml")
    with open(xml, "w") as f:
        f.write(text.replace('<scale value="-1,1,1"/>', '<scale value="-1,0,1"/>'))
    s, b = load(xml, W, H)
    c2w = np.array(s.desc.camera.camera_to_world[:], np.float32).reshape(4, 4)
    assert (c2w[1, :3] == 0).all() and (c2w[0, :3] != 0).any() and (c2w[2, :3] != 0).any()
    _check(monkeypatch, s, b, 17, traits=2)


def test_three_leaves_walk_the_tree(gpu, tmp_path, monkeypatch):
    """A third cluster: three leaves, not flat -- the scene renders as before and flat_trace reads 0."""
    xml, _ = cluster_scene(tmp_path, "three", [(-4.5, -2.7), (-2.0, -0.2), (0.2, 2.0)], TWO_SPHERES)
    s, b = load(xml, W, H)
    assert len(leaf_table(b)) == 3 and not is_flat_tree(b)
    _check(monkeypatch, s, b, 19, flat=0)
