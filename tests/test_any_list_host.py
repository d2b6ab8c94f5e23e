"""The scene-wide any-hit word (host/shadow_masks.cpp shadow_any_word, through the binding) and the flat image's any-hit
section (host/gpu_layout.cpp flat_image), on the records in the order a context traverses them. CPU only.

  - On the Cornell box (C2, C1) the word keeps exactly the two spheres and the light's two triangles: the ceiling lies
    behind the light (the emitter-side rule), the floor, the back wall and the side walls are supporting walls.
  - Nothing is left out (all ones) when a slab pokes through a side wall, a mesh lies outside the room, the light
    stands 1e-4 from a side wall, the emitter has vertex normals, or the scene has 65 records.
  - Soundness: a float32 numpy restatement of tri_test_nb, operation for operation (shadow_mask_helpers.accepts32),
    accepts no left-out record for segments formed as the kernels form them (emitter_sample: origin on an emitter
    face by the emit_faces arithmetic, direction and maxt from the float32 difference to the far end) -- from the faces'
    corners, edges and random interior points to far ends on every record: random points, the left-out records' corners
    and edges (which the walls share), points on the left-out records themselves, and each of these moved +-eps_f along
    that record's normal, eps_f = 8 * 2^-24 * the largest coordinate (how far a float hit point lies from its record).
    More than 200 000 segments per scene; the same restatement accepts kept records in the same set.
  - The image: the any-hit section's counts, its pairing by kind and its record indices; the closest-hit part and the
    box-equality bits are those of the image without a word; no section for an all-ones word or with NH_ANY_LIST=0.
"""
import os

import numpy as np
import pytest

import nori_hip as nh
from flat_trace_helpers import HEADER_F4, MAX_PAIRS, PAIR_F4, as_int, same_bits, tree_boxes
from pair_kind_helpers import leaf_table
from primary_mask_records import device_records, is_sphere
from shadow_mask_helpers import F, accepts32, face_normals32, face_points32, shadow_segments32
from test_shadow_masks_host import ALL, _scene

ANY_LIST, ANY_OFF = 4, HEADER_F4 + PAIR_F4 * MAX_PAIRS  # csrc/nh_layout.h kFlatAnyList, kFlatAnyOff
U = 2.0 ** -24


def _load(tmp, variant, **kw):
    s = _scene(tmp, variant, "reference", 96, 80, **kw)
    b = nh.Bvh(s)
    rec = device_records(s, b)
    faces = nh.shadow_emitter_faces(s.desc)
    return s, b, rec, faces


def _word(s, rec, faces):
    return nh.shadow_any_word(s.desc.camera, rec, faces)


def _light_records(rec, faces):
    """the records whose three vertices are an emitter face's"""
    fs = [set(map(tuple, f.reshape(3, 3))) for f in faces]
    return [k for k, r in enumerate(rec)
            if not is_sphere(r) and {tuple(r[0:3]), tuple(r[4:7]), tuple(r[8:11])} in fs]


def _kept(word, n):
    return [k for k in range(n) if (word >> k) & 1]


@pytest.mark.parametrize("variant", ["c2", "c1"])
def test_word_on_the_cornell_box(tmp_path, variant):
    s, b, rec, faces = _load(tmp_path, variant)
    assert len(rec) == 14 and len(faces) == 2
    word = _word(s, rec, faces)
    spheres = [k for k, r in enumerate(rec) if is_sphere(r)]
    light = _light_records(rec, faces)
    assert len(spheres) == 2 and len(light) == 2
    assert _kept(word, len(rec)) == sorted(spheres + light), hex(word)
    assert word >> len(rec) == ALL >> len(rec)  # the bits above the last record are set
    # it holds the emitter-side word's zeros
    emitter_word, _ = nh.shadow_masks(s.desc.camera, rec, faces, np.arange(0))
    assert word & ~emitter_word == 0


def _write_mesh(tmp, name, text):
    d = os.path.join(str(tmp), "scenes/pa4/cbox/meshes")
    os.makedirs(d, exist_ok=True)
    with open(os.path.join(d, name), "w") as f:
        f.write(text)


def _obj_shape(name):
    return (f'<shape type="obj"><string name="filename" value="meshes/{name}"/>'
            '<bsdf type="diffuse"><color name="albedo" value="0.5 0.5 0.5"/></bsdf></shape>')


def _light_obj(tmp):
    """(vertex rows, other lines) of the Cornell box's light mesh"""
    _scene(tmp, "c2", "reference", 96, 80)  # (materializes the fixture)
    lines = open(os.path.join(str(tmp), "scenes/pa4/cbox/meshes/light.obj")).read().splitlines()
    v = np.array([[float(x) for x in l.split()[1:4]] for l in lines if l.startswith("v ")])
    return v, [l for l in lines if l.startswith("f ")]


def test_nothing_left_out(tmp_path):
    s, b, rec, faces = _load(tmp_path, "c2")
    pts = np.concatenate([rec[k].reshape(3, 4)[:, :3] for k in range(len(rec)) if not is_sphere(rec[k])])
    x_wall = float(pts[:, 0].max())  # the right wall's farthest vertex
    # a slab that pokes 0.05 through the right wall
    _write_mesh(tmp_path, "al_slab.obj", f"v 0.6 0.5 -0.2\nv {x_wall + 0.05} 0.5 -0.2\nv {x_wall + 0.05} 0.5 0.2\n"
                                         "v 0.6 0.5 0.2\nf 1 2 3\nf 1 3 4\n")
    # a mesh outside the room
    _write_mesh(tmp_path, "al_out.obj", "v 3 0.2 0\nv 4 0.2 0\nv 3.5 1.0 0.3\nf 1 2 3\n")
    # the light moved to 1e-4 from the right wall (the wall leans: the distance is set at the light's own height)
    v, f = _light_obj(tmp_path)
    right = [r.reshape(3, 4)[:, :3].astype(np.float64) for r in rec
             if not is_sphere(r) and r.reshape(3, 4)[:, 0].min() > 0.9]
    assert len(right) == 2
    p0, n = right[0][0], np.cross(right[0][1] - right[0][0], right[0][2] - right[0][0])
    n /= np.linalg.norm(n)
    n = -n if n[0] > 0 else n  # into the room
    gap = ((v - p0) @ n).min()
    assert gap > 0.5
    moved = v - (gap - 1e-4) * n
    _write_mesh(tmp_path, "al_light_near.obj", "\n".join([f"v {x!r} {y!r} {z!r}" for x, y, z in moved.tolist()] + f) + "\n")
    # the light with vertex normals
    fn = [" ".join(["f"] + [f"{i.split('/')[0]}//1" for i in l.split()[1:]]) for l in f]
    _write_mesh(tmp_path, "al_light_vn.obj", "\n".join([f"v {x!r} {y!r} {z!r}" for x, y, z in v.tolist()]
                                                       + ["vn 0 -1 0"] + fn) + "\n")
    cases = {
        "slab": (dict(extra=_obj_shape("al_slab.obj")), 16, 2),
        "outside": (dict(extra=_obj_shape("al_out.obj")), 15, 2),
        "near": (dict(edits=[("meshes/light.obj", "meshes/al_light_near.obj")]), 14, 2),
        "normals": (dict(edits=[("meshes/light.obj", "meshes/al_light_vn.obj")]), 14, 0),
    }
    for name, (kw, n_rec, n_faces) in cases.items():
        s, b, rec, faces = _load(tmp_path, "c2", name="al_" + name, **kw)
        assert len(rec) == n_rec and len(faces) == n_faces, name
        assert _word(s, rec, faces) == ALL, name
    # 65 records
    s, b, rec, faces = _load(tmp_path, "c2")
    assert _word(s, rec, faces) != ALL
    assert _word(s, np.concatenate([rec] * 5)[:65], faces) == ALL


def _points_on(r, rng, n):
    """n random points on record r, float64"""
    r = r.astype(np.float64)
    if is_sphere(r.astype(np.float32)):
        d = rng.standard_normal((n, 3))
        return r[0:3] + r[3] * d / np.linalg.norm(d, axis=1, keepdims=True)
    a, b = rng.random(n), rng.random(n)
    su = np.sqrt(a)
    w = np.stack([1 - su, b * su, su * (1 - b)], axis=1)
    return w @ np.stack([r[0:3], r[4:7], r[8:11]])


@pytest.mark.parametrize("variant", ["c2", "c1"])
def test_left_out_records_accept_no_shadow_segment(tmp_path, variant):
    s, b, rec, faces = _load(tmp_path, variant)
    word = _word(s, rec, faces)
    n = len(rec)
    out = [k for k in range(n) if not (word >> k) & 1]
    assert len(out) == 10 and not any(is_sphere(rec[k]) for k in out)
    rng = np.random.default_rng(5)
    # emitter points: corners and random interior points (emit_faces arithmetic), and points on the faces' edges
    lp, lf = face_points32(faces, rng, 12)
    f3 = faces.reshape(-1, 3, 3)
    edge_p, edge_f = [], []
    for i, (p0, p1, p2) in enumerate(f3):
        for bu, bv in [(F(0.5), F(0.5)), (F(0.5), F(0)), (F(0), F(0.5)), (F(0.25), F(0.75)), (F(0), F(0.125)),
                       (F(0.875), F(0))]:
            edge_p.append((bu * p0 + bv * p1) + (F(1) - bu - bv) * p2)
            edge_f.append(i)
    lp, lf = np.concatenate([lp, np.array(edge_p, F)]), np.concatenate([lf, np.array(edge_f)])
    ln = face_normals32(faces)[lf]
    # far ends
    cw = np.array(s.desc.camera.camera_to_world[:], np.float64).reshape(4, 4)
    tri = np.concatenate([rec[k].reshape(3, 4)[:, :3] for k in range(n) if not is_sphere(rec[k])]).astype(np.float64)
    eps_f = 8 * U * max(np.abs(tri).max(), np.abs(cw[:3, 3] / cw[3, 3]).max())
    far = [_points_on(rec[k], rng, 150) for k in range(n)]
    for k in out:
        r = rec[k].astype(np.float64)
        p = np.stack([r[0:3], r[4:7], r[8:11]])
        nk = np.cross(p[1] - p[0], p[2] - p[0])
        nk /= np.linalg.norm(nk)
        t = rng.random((40, 1))
        on = np.concatenate([p, (p[0] + p[1]) / 2 * np.ones((1, 3)), (p[1] + p[2]) / 2 * np.ones((1, 3)),
                             (p[0] + p[2]) / 2 * np.ones((1, 3)), p[0] + t * (p[1] - p[0]), p[1] + t * (p[2] - p[1]),
                             p[2] + t * (p[0] - p[2]), _points_on(rec[k], rng, 100)])
        far += [on, on + eps_f * nk, on - eps_f * nk]
    far = np.concatenate(far).astype(F)
    m = len(lp)
    so, sd, mint, maxt, traced = shadow_segments32(np.tile(lp, (len(far), 1)), np.tile(ln, (len(far), 1)),
                                                   np.repeat(far, m, axis=0))
    so, sd, mint, maxt = so[traced], sd[traced], mint[traced], maxt[traced]
    print(f"{variant}: {len(so)} segments ({m} emitter points x {len(far)} far ends), eps_f {eps_f:.3e}")
    assert len(so) >= 200_000
    for k in out:
        acc = accepts32(rec[k], so, sd, mint, maxt)
        assert not acc.any(), ("the float32 test accepts a left-out record", k, int(np.argmax(acc)))
    n_kept = sum(int(accepts32(rec[k], so, sd, mint, maxt).sum()) for k in _kept(word, n))
    print(f"{n_kept} (segment, kept record) acceptances")
    assert n_kept > 0


def _pair_rows(rec, k, k1):
    """the pair record of records k, k1 (flat_trace_helpers.expected_image's rows)"""
    a, b, c = rec[k, 0:4], rec[k, 4:8], rec[k, 8:12]
    a1, b1, c1 = rec[k1, 0:4], rec[k1, 4:8], rec[k1, 8:12]
    return np.array([[a[0], a1[0], a[1], a1[1]], [a[2], a1[2], a[3], a1[3]],
                     [b[0] - a[0], b1[0] - a1[0], b[1] - a[1], b1[1] - a1[1]],
                     [b[2] - a[2], b1[2] - a1[2], c[0] - a[0], c1[0] - a1[0]],
                     [c[1] - a[1], c1[1] - a1[1], c[2] - a[2], c1[2] - a1[2]]], F)


def _check_section(rec, leaves, img, plain, eq, word):
    """img: the image with the word; plain: the one without."""
    n_plain = len(plain)
    assert as_int(img[0][3]) == eq | ANY_LIST and as_int(plain[0][3]) == eq
    # everything but the three header words is the plain image's, then zeros up to the section
    a, p = img[:n_plain].copy(), plain.copy()
    for row in (0, 3, 5):
        a[row][3] = p[row][3] = 0
    assert same_bits(a, p)
    assert not img[n_plain:ANY_OFF].view(np.int32).any()
    at = ANY_OFF
    for l, (start, count) in enumerate(leaves):
        kept = [k for k in range(start, start + count) if (word >> k) & 1]
        tris, sphs = [k for k in kept if not is_sphere(rec[k])], [k for k in kept if is_sphere(rec[k])]
        counts = as_int(img[3 + 2 * l][3])
        assert (counts & 0xffff, counts >> 16) == ((len(tris) + 1) // 2, (len(sphs) + 1) // 2), l
        for ks in (tris, sphs):
            for i in range(0, len(ks), 2):
                k, k1 = ks[i], ks[i + 1] if i + 1 < len(ks) else ks[i]
                assert (as_int(img[at + 5][2]), as_int(img[at + 5][3])) == (k, k1)
                assert same_bits(img[at:at + 5], _pair_rows(rec, k, k1))
                assert same_bits(img[at + 5][:2], np.array([rec[k][11], rec[k1][11]], F))
                at += PAIR_F4
    if len(leaves) == 1:
        assert as_int(img[5][3]) == 0
    assert at == len(img)


def test_any_hit_section(tmp_path, monkeypatch):
    monkeypatch.delenv("NH_ANY_LIST", raising=False)
    monkeypatch.delenv("NH_FLAT_TRACE", raising=False)
    for variant in ("c2", "c1"):
        s, b, rec, faces = _load(tmp_path, variant)
        leaves, boxes = leaf_table(b), tree_boxes(b)
        assert len(leaves) == 2
        word = _word(s, rec, faces)
        plain, eq = nh.flat_image(rec, leaves, boxes)
        img, eq_w = nh.flat_image(rec, leaves, boxes, any_word=word)
        assert plain is not None and img is not None and eq_w == eq
        _check_section(rec, leaves, img, plain, eq, word)
        # C2 / C1: the spheres' pair in the left leaf, the light's in the right one
        assert [as_int(img[3][3]), as_int(img[5][3])] == [1 << 16, 1] and len(img) == ANY_OFF + 2 * PAIR_F4
        # no section: an all-ones word (also over the records alone), and the knob
        for w in (ALL, (1 << len(rec)) - 1):
            none, eq_n = nh.flat_image(rec, leaves, boxes, any_word=w)
            assert same_bits(none, plain) and eq_n == eq
        monkeypatch.setenv("NH_ANY_LIST", "0")
        none, _ = nh.flat_image(rec, leaves, boxes, any_word=word)
        assert same_bits(none, plain)
        monkeypatch.delenv("NH_ANY_LIST")
    # other words: a lone triangle and a lone sphere repeated, a leaf that keeps nothing, one leaf
    s, b, rec, faces = _load(tmp_path, "c2")
    leaves, boxes = leaf_table(b), tree_boxes(b)
    plain, eq = nh.flat_image(rec, leaves, boxes)
    sph = [k for k in range(len(rec)) if is_sphere(rec[k])]
    (s0, c0), (s1, c1) = leaves
    for word in ((1 << s0) | (1 << sph[0]) | (1 << s1), ((1 << c0) - 1) << s0 & ~(1 << sph[1]), 0, 0b10101 << s1):
        img, _ = nh.flat_image(rec, leaves, boxes, any_word=word | (ALL << len(rec) & ALL))
        _check_section(rec, leaves, img, plain, eq, word)
    one = [(0, len(rec))]
    root = np.concatenate([boxes[:6]] * 3)
    plain1, eq1 = nh.flat_image(rec, one, root)
    img1, _ = nh.flat_image(rec, one, root, any_word=0b1111000011)
    assert eq1 == 1
    _check_section(rec, one, img1, plain1, eq1, 0b1111000011)
