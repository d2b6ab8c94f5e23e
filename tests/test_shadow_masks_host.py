"""The candidate masks of the light samples' any-hit queries (host/shadow_masks.cpp, through the binding), on the records
in the order a context traverses them (primary_mask_records.device_records). CPU only.

Shadow segments are formed as the kernels form them (shadow_mask_helpers.shadow_segments32: origin on an emitter face,
direction and maxt from the float32 difference to the far end; only those the kernel would query, float dot(n, sd) >= 0).
Conservative, twice over: a record the segment meets in float64 within a tenth of the world-space pad has its bit, and
the float32 restatement of the kernels' own primitive tests accepts no record whose bit is clear.
  - per-block words: the far end is the float64 first hit of a camera ray of the block (corners at jitter 0 and
    1 - 2^-24, random positions, positions up to one pixel outside);
  - the emitter-side word: the far end is anywhere in the scene's box, and within 1e-6 of an emitter face's plane on
    its front side (grazing rays).
Useful: on the Cornell box the ceiling pair's bits are clear in every word, and at 1024x1024 a block keeps on average
strictly fewer records than the same rule keeps without clipping (the whole boxes of the block's primary records
joined with the light's).
"""
import os

import numpy as np
import pytest

import nori_hip as nh
import scenegen
from light_scenes import point_xml
from primary_mask_records import device_records, is_sphere
from shadow_mask_helpers import (F, accepts32, face_normals32, face_points32, first_hits64, meets64, record_box, scene_box,
                                 shadow_segments32)
from test_primary_masks_host import CAMERAS, LOOKAT, _camera_rays

ALL = (1 << 64) - 1
LENS = ('<camera type="perspective"><float name="lensRadius" value="0.08"/>'
        '<float name="focalDistance" value="3.2"/>')
AREA = '<emitter type="area"><color name="radiance" value="2 2 2"/></emitter>'


def _scene(tmp, variant, camera, w, h, edits=(), extra="", name=""):
    xml = scenegen.cbox_xml(str(tmp), variant, extra_shapes=extra)
    text = open(xml).read()
    assert text.count(LOOKAT) == 1
    text = text.replace(LOOKAT, CAMERAS[camera])
    for old, new in edits:
        assert text.count(old) == 1, old
        text = text.replace(old, new)
    path = os.path.join(os.path.dirname(xml), f"sm_{variant}_{camera}{name}.xml")
    with open(path, "w") as f:
        f.write(text)
    s = nh.Scene(path)
    s.set_resolution(w, h)
    return s


def _popcount(a, n=64):
    """set bits among the low n of each word (the bits above the last record are set in every word)"""
    return np.array([bin(int(x) & ((1 << n) - 1)).count("1") for x in a])


def _block_positions(nbx, nby, w, h, rng, n_in, n_out):
    """(n_blocks, n, 2) raster positions per block, formed in float32 as the kernels form pixel + jitter: the corner
    pixels at jitter 0 and at the largest float below 1, n_in random positions inside, n_out up to one pixel outside."""
    top = np.nextafter(np.float32(1), np.float32(0))
    out = []
    for by in range(nby):
        for bx in range(nbx):
            x0, y0, x1, y1 = 32 * bx, 32 * by, min(32 * bx + 32, w), min(32 * by + 32, h)
            pos = [(np.float32(px) + jx, np.float32(py) + jy) for px in (x0, x1 - 1) for py in (y0, y1 - 1)
                   for jx in (np.float32(0), top) for jy in (np.float32(0), top)]
            inside = np.stack([rng.uniform(x0, x1, n_in), rng.uniform(y0, y1, n_in)], axis=1)
            outside = np.stack([rng.uniform(x0 - 1, x1 + 1, n_out), rng.uniform(y0 - 1, y1 + 1, n_out)], axis=1)
            out.append(np.concatenate([np.array(pos, np.float32), inside.astype(np.float32), outside.astype(np.float32)]))
    return np.array(out, np.float64)


def _check_segments(rec, words, p, n, ref, tol, what):
    """Both assertions for segments from light points p (normals n) to ref, each with its own word. Returns how many
    (segment, record) pairs were met in float64."""
    so, sd, mint, maxt, traced = shadow_segments32(p, n, ref)
    so, sd, mint, maxt, words = so[traced], sd[traced], mint[traced], maxt[traced], np.asarray(words, np.uint64)[traced]
    assert len(so) > 0
    n_met = 0
    for k, r in enumerate(rec):
        bit = ((words >> np.uint64(k)) & np.uint64(1)).astype(bool)
        met = meets64(r, so, sd, mint, maxt, tol)
        acc = accepts32(r, so, sd, mint, maxt)
        assert not (met & ~bit).any(), (what, "float64 meets a record whose bit is clear", k, int(np.argmax(met & ~bit)))
        assert not (acc & ~bit).any(), (what, "the float32 test accepts a record whose bit is clear", k,
                                        int(np.argmax(acc & ~bit)))
        n_met += int(met.sum())
    return n_met


@pytest.mark.parametrize("camera", list(CAMERAS))
@pytest.mark.parametrize("size", [(1024, 1024), (96, 80)])
@pytest.mark.parametrize("variant", ["c1", "c2"])
def test_block_words_conservative(tmp_path, variant, size, camera):
    w, h = size
    s = _scene(tmp_path, variant, camera, w, h)
    cam, rec = s.desc.camera, device_records(s, nh.Bvh(s))
    faces = nh.shadow_emitter_faces(s.desc)
    assert len(rec) == 14 and len(faces) == 2
    nbx, nby = (w + 31) // 32, (h + 31) // 32
    word, masks = nh.shadow_masks(cam, rec, faces, np.arange(nbx * nby))
    pm = nh.primary_masks(cam, rec, np.arange(nbx * nby))
    assert masks is not None and len(masks) == nbx * nby
    assert ((masks & ~np.uint64(word)) == 0).all()  # each holds the emitter-side word's zeros
    assert (masks[pm == 0] == 0).all()
    lo, hi = scene_box(rec)
    tol = 1e-4 * (hi - lo).max() / 10
    rng = np.random.default_rng(11)
    big = w >= 1024
    pos = _block_positions(nbx, nby, w, h, rng, 4 if big else 40, 4 if big else 20)
    nb, npos = pos.shape[:2]
    o, d = _camera_rays(cam, pos.reshape(-1, 2))
    found, ref = first_hits64(rec, o, d)
    blk = np.repeat(np.arange(nb), npos)
    # a ray that hits something belongs to a block with candidates (the primary masks' own guarantee)
    assert (pm[blk[found]] != 0).all()
    lp, lf = face_points32(faces, rng, 2)
    ln = face_normals32(faces)[lf]
    ref, blk = ref[found].astype(F), blk[found]
    m = len(lp)
    p = np.tile(lp, (len(ref), 1))
    n = np.tile(ln, (len(ref), 1))
    n_met = _check_segments(rec, np.repeat(masks[blk], m), p, n, np.repeat(ref, m, axis=0), tol, (variant, size, camera))
    print(f"{len(ref) * m} segments, {n_met} (segment, record) meetings")
    assert n_met > 0 or camera != "reference"  # (the reference camera sees the spheres' shadows)


@pytest.mark.parametrize("variant", ["c1", "c2"])
def test_emitter_word_conservative(tmp_path, variant):
    s = _scene(tmp_path, variant, "reference", 96, 80)
    rec = device_records(s, nh.Bvh(s))
    faces = nh.shadow_emitter_faces(s.desc)
    word, _ = nh.shadow_masks(s.desc.camera, rec, faces, np.arange(0))
    ceiling = [k for k, r in enumerate(rec) if not is_sphere(r) and min(r[1], r[5], r[9]) > 1.585]
    assert len(ceiling) == 2
    assert all(not (word >> k) & 1 for k in ceiling), hex(word)
    lo, hi = scene_box(rec)
    tol = 1e-4 * (hi - lo).max() / 10
    rng = np.random.default_rng(3)
    lp, lf = face_points32(faces, rng, 6)
    ln = face_normals32(faces)[lf]
    far = rng.uniform(lo, hi, (6000, 3))
    # grazing far ends: on an emitter face's plane, moved up to 1e-6 to its front side
    f64 = faces.astype(np.float64).reshape(-1, 3, 3)
    for f in f64:
        nn = np.cross(f[1] - f[0], f[2] - f[0])
        nn /= np.linalg.norm(nn)
        x = rng.uniform(lo, hi, (3000, 3))
        x = x - ((x - f[0]) @ nn)[:, None] * nn + rng.uniform(0, 1e-6, (3000, 1)) * nn
        far = np.concatenate([far, x[((x >= lo) & (x <= hi)).all(axis=1)]])
    far = far.astype(F)
    m = len(lp)
    n_met = _check_segments(rec, np.full(len(far) * m, word, np.uint64), np.tile(lp, (len(far), 1)),
                            np.tile(ln, (len(far), 1)), np.repeat(far, m, axis=0), tol, variant)
    assert n_met > 0


def test_useful_on_the_benchmark_scene(tmp_path):
    """C2 at 1024x1024: the ceiling pair is in no word, and clipping pays: the mean number of records a block keeps is
    strictly below what the same rule keeps from the unclipped boxes of the block's primary records and the light."""
    w = h = 1024
    s = _scene(tmp_path, "c2", "reference", w, h)
    cam, rec = s.desc.camera, device_records(s, nh.Bvh(s))
    faces = nh.shadow_emitter_faces(s.desc)
    word, masks = nh.shadow_masks(cam, rec, faces, np.arange(32 * 32))
    pm = nh.primary_masks(cam, rec, np.arange(32 * 32))
    ceiling = [k for k, r in enumerate(rec) if not is_sphere(r) and min(r[1], r[5], r[9]) > 1.585]
    assert len(ceiling) == 2 and all(not (int(x) >> k) & 1 for k in ceiling for x in list(masks) + [word])
    boxes = [record_box(r) for r in rec]
    f = faces.astype(np.float64).reshape(-1, 3)
    unclipped = []
    for x in pm[pm != 0]:
        ks = [k for k in range(len(rec)) if (int(x) >> k) & 1]
        lo = np.minimum(f.min(0), np.min([boxes[k][0] for k in ks], axis=0))
        hi = np.maximum(f.max(0), np.max([boxes[k][1] for k in ks], axis=0))
        unclipped.append(sum(1 for a, b in boxes if (a <= hi).all() and (b >= lo).all()))
    kept = _popcount(masks[pm != 0], len(rec))
    print(f"records kept per block with candidates: mean {kept.mean():.3f} of {len(rec)} "
          f"(unclipped boxes: {np.mean(unclipped):.3f}; primary masks: {_popcount(pm[pm != 0]).mean():.3f}); "
          f"emitter-side word keeps {bin(word & ((1 << len(rec)) - 1)).count('1')}")
    assert kept.mean() < np.mean(unclipped)
    assert kept.mean() <= 6.0


def test_nothing_left_out(tmp_path):
    """A point light, area lights on opposite walls, a sphere light: every word all ones. A lens: no per-block table."""
    blocks = np.arange(9)
    right = '<color name="albedo" value="0.161 0.133 0.427"/>\n\t\t</bsdf>'
    left = '<color name="albedo" value="0.630 0.065 0.05"/>\n\t\t</bsdf>'
    cases = {
        "point": (dict(extra=point_xml((0.0, 1.2, 0.0), (5, 5, 5))), 0),
        "sphere": (dict(extra='<shape type="sphere"><point name="center" value="0 1.0 0"/><float name="radius" '
                              f'value="0.1"/><bsdf type="diffuse"/>{AREA}</shape>'), 0),
        # both side walls lit as well: three planar lights, two of them facing each other
        "walls": (dict(edits=[(right, right + AREA), (left, left + AREA)]), 6),
    }
    for name, (kw, n_faces) in cases.items():
        s = _scene(tmp_path, "c2", "reference", 96, 80, name=name, **kw)
        rec = device_records(s, nh.Bvh(s))
        faces = nh.shadow_emitter_faces(s.desc)
        assert len(faces) == n_faces, name
        word, masks = nh.shadow_masks(s.desc.camera, rec, faces, blocks)
        pm = nh.primary_masks(s.desc.camera, rec, blocks)
        assert word == ALL, (name, hex(word))
        assert masks is not None and (masks[pm != 0] == np.uint64(ALL)).all(), name
    s = _scene(tmp_path, "c2", "reference", 96, 80, edits=[('<camera type="perspective">', LENS)], name="lens")
    rec = device_records(s, nh.Bvh(s))
    word, masks = nh.shadow_masks(s.desc.camera, rec, nh.shadow_emitter_faces(s.desc), blocks)
    assert masks is None
    # more than 64 records: nothing is left out
    s = _scene(tmp_path, "c2", "reference", 96, 80)
    rec = device_records(s, nh.Bvh(s))
    word, masks = nh.shadow_masks(s.desc.camera, np.concatenate([rec] * 5)[:65], nh.shadow_emitter_faces(s.desc), blocks)
    assert word == ALL and masks is None
