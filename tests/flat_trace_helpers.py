"""Helpers of the flat-traversal tests: what nh_flat_image is given for a scene's BVH (leaf table, the root's and its
children's boxes) and the image it must return, restated in numpy; and the hand-built scenes of those tests."""
import os

import numpy as np

import nori_hip as nh
import scenegen
from pair_kind_helpers import leaf_table

HEADER_F4, PAIR_F4, MAX_PAIRS = 6, 6, 16  # csrc/nh_layout.h kFlatHeaderF4, kPairF4, kFlatMaxPairs


def node_box(nodes, i) -> np.ndarray:
    """(min xyz, max xyz) of reference node i (include/nori_hip.h nh_bvh_node: words 2-7 are the box's floats)."""
    return nodes[i][2:8].copy().view(np.float32)


def tree_boxes(bvh) -> np.ndarray:
    """The 18 floats nh_flat_image takes: the root's box, its left child's and its right child's (a leaf root: its own
    box three times). The left child follows its parent, word1 of an inner node is its right child."""
    nodes = bvh.nodes()
    root = node_box(nodes, 0)
    if int(nodes[0][0]) & 1:
        return np.concatenate([root, root, root])
    return np.concatenate([root, node_box(nodes, 1), node_box(nodes, int(nodes[0][1]))])


def is_flat_tree(bvh) -> bool:
    """One leaf, or a root whose two children are leaves."""
    nodes = bvh.nodes()
    if int(nodes[0][0]) & 1:
        return True
    return bool(int(nodes[1][0]) & 1) and bool(int(nodes[int(nodes[0][1])][0]) & 1)


def as_int(x) -> int:
    return int(np.asarray(x, np.float32).reshape(1).view(np.int32)[0])


def expected_image(rec, leaves, boxes):
    """The flat image of one or two leaves over the (n, 12) records, from nh.pair_layout's arrangement by kind: header,
    then each leaf's pair records with the edges p1 - p0, p2 - p0 as float32 differences."""
    rec = np.asarray(rec, np.float32).reshape(-1, 12)
    slots, lp = nh.pair_layout(rec, leaves, by_kind=True)
    boxes = np.asarray(boxes, np.float32).reshape(3, 6)
    if len(leaves) == 1:
        boxes = np.stack([boxes[0]] * 3)
    eq = 1 if len(leaves) == 1 else (1 if boxes[1].tobytes() == boxes[0].tobytes() else 0) | (
        2 if boxes[2].tobytes() == boxes[0].tobytes() else 0)
    counts = [int(n_tri) | (int(n_sph) << 16) for _, n_tri, n_sph in lp] + [0]
    rows = []

    def row(xyz, word):
        rows.append(np.concatenate([np.asarray(xyz, np.float32), np.array([word], np.int32).view(np.float32)]))

    row(boxes[0][:3], eq)
    row(boxes[0][3:], len(leaves))
    row(boxes[1][:3], counts[0])
    row(boxes[1][3:], 0)
    row(boxes[2][:3], counts[1])
    row(boxes[2][3:], 0)
    for first, n_tri, n_sph in lp:
        for p in range(first, first + n_tri + n_sph):
            k, k1 = int(slots[p][0]), int(slots[p][1])
            k1 = k if k1 < 0 else k1
            a, b, c = rec[k, 0:4], rec[k, 4:8], rec[k, 8:12]
            a1, b1, c1 = rec[k1, 0:4], rec[k1, 4:8], rec[k1, 8:12]
            f = np.float32
            rows.append(np.array([a[0], a1[0], a[1], a1[1]], f))
            rows.append(np.array([a[2], a1[2], a[3], a1[3]], f))
            rows.append(np.array([b[0] - a[0], b1[0] - a1[0], b[1] - a[1], b1[1] - a1[1]], f))
            rows.append(np.array([b[2] - a[2], b1[2] - a1[2], c[0] - a[0], c1[0] - a1[0]], f))
            rows.append(np.array([c[1] - a[1], c1[1] - a1[1], c[2] - a[2], c1[2] - a1[2]], f))
            rows.append(np.concatenate([np.array([c[3], c1[3]], f), np.array([k, k1], np.int32).view(f)]))
    return np.array(rows, np.float32), eq


def same_bits(a, b) -> bool:
    a, b = np.ascontiguousarray(a, np.float32), np.ascontiguousarray(b, np.float32)
    return a.shape == b.shape and a.tobytes() == b.tobytes()


# ---- hand-built scenes --------------------------------------------------------------------------------------------
LIGHT = '<emitter type="area"><color name="radiance" value="{0} {0} {0}"/></emitter>'


def diffuse(albedo):
    return f'<bsdf type="diffuse"><color name="albedo" value="{albedo}"/></bsdf>'


def mesh(name, inner):
    return f'<shape type="obj"><string name="filename" value="meshes/{name}"/>{inner}</shape>\n'


def sphere(center, radius, inner):
    return (f'<shape type="sphere"><point name="center" value="{center}"/><float name="radius" value="{radius}"/>'
            f'{inner}</shape>\n')


def write_scene(tmp, name, shapes, meshes, lookat=None):
    """The Cornell box's sampler and integrator (path_mis) around `shapes`; meshes: file name -> OBJ text; lookat
    replaces the camera's."""
    c2 = scenegen.cbox_xml(str(tmp), "c2")
    text = open(c2).read()
    head = text[:text.index("<shape")]
    if lookat is not None:
        a, b = head.index("<lookat"), head.index("/>", head.index("<lookat")) + 2
        head = head[:a] + lookat + head[b:]
    for fn, obj in meshes.items():
        with open(os.path.join(os.path.dirname(c2), "meshes", fn), "w") as f:
            f.write(obj)
    path = os.path.join(os.path.dirname(c2), f"flat_{name}.xml")
    with open(path, "w") as f:
        f.write(head + shapes + "</scene>\n")
    return path


def load(xml, w, h):
    s = nh.Scene(xml)
    s.set_resolution(w, h)
    return s, nh.Bvh(s)


def leaf_of_record(bvh):
    """leaf index of every record position."""
    out = {}
    for l, (start, count) in enumerate(leaf_table(bvh)):
        for k in range(start, start + count):
            out[k] = l
    return out


def corner_triangles(x0, x1, y0, y1, z0, z1):
    """Three triangles that each span the box from corner to corner: no split of them lowers the builder's cost."""
    xm, zm = (x0 + x1) / 2, (z0 + z1) / 2
    return [f"v {x0} {y0} {z0}\nv {x1} {y0} {z1}\nv {xm} {y1} {zm}\nf 1 2 3\n",
            f"v {x0} {y0} {z1}\nv {x1} {y0} {z0}\nv {xm} {y1} {zm + 0.1}\nf 1 2 3\n",
            f"v {x0} {y1} {z0}\nv {x1} {y1 - 0.1} {z1}\nv {xm + 0.1} {y0} {zm}\nf 1 2 3\n"]


ALBEDOS = ["0.7 0.7 0.7", "0.2 0.5 0.7", "0.7 0.4 0.6", "0.3 0.3 0.8", "0.6 0.6 0.1", "0.7 0.2 0.2", "0.8 0.8 0.2",
           "0.2 0.8 0.8", "0.5 0.5 0.5", "0.4 0.7 0.3", "0.6 0.3 0.2", "0.3 0.6 0.6"]
# the camera of the cluster scenes: inside the right cluster's box, outside the left one's, looking at the left one
CLUSTER_ORIGIN = (1.0, 0.9, 0.2)
CLUSTER_LOOKAT = '<lookat target="-1.0, 0.7, 0" origin="1.0, 0.9, 0.2" up="0, 1, 0"/>'
# two triangles in the plane y = 0.8 that cover each other for -0.5 < x < 0.5, one centred left of x = 0, one right
PLANE_LEFT = "v -1.9 0.8 -0.9\nv 0.5 0.8 -0.9\nv -0.7 0.8 0.9\nf 1 2 3\n"
PLANE_RIGHT = "v -0.5 0.8 -0.9\nv 1.9 0.8 -0.9\nv 0.7 0.8 0.9\nf 1 2 3\n"


def cluster_scene(tmp, name, clusters, spheres="", plane_pair=True):
    """Clusters of corner-to-corner triangles, one per x range of `clusters`, under a light in the last one; with
    plane_pair the two coincident triangles PLANE_LEFT / PLANE_RIGHT; `spheres`: further shapes. Returns (xml, names of
    the shapes in order)."""
    meshes, shapes, names = {}, "", []
    x0, x1 = clusters[-1]
    meshes["fl_light.obj"] = f"v {x0 + 0.1} 1.7 -0.5\nv {x1 - 0.1} 1.7 -0.5\nv {(x0 + x1) / 2} 1.7 0.6\nf 1 3 2\n"
    shapes += mesh("fl_light.obj", LIGHT.format(12))
    names.append("light")
    for c, (x0, x1) in enumerate(clusters):
        for i, obj in enumerate(corner_triangles(x0, x1, 0, 1.6, -1, 1)):
            meshes[f"fl_c{c}_{i}.obj"] = obj
            shapes += mesh(f"fl_c{c}_{i}.obj", diffuse(ALBEDOS[(3 * c + i) % len(ALBEDOS)]))
            names.append(f"c{c}_{i}")
    if plane_pair:
        meshes["fl_plane_l.obj"], meshes["fl_plane_r.obj"] = PLANE_LEFT, PLANE_RIGHT
        shapes += mesh("fl_plane_l.obj", diffuse("0.8 0.8 0.2")) + mesh("fl_plane_r.obj", diffuse("0.2 0.8 0.8"))
        names += ["plane_l", "plane_r"]
    return write_scene(tmp, name, shapes + spheres, meshes, lookat=CLUSTER_LOOKAT), names
