"""The per-block candidate masks of the camera rays' first closest hit (host/primary_masks.cpp, through the binding),
on the records in the order a context traverses them (primary_mask_records.device_records). CPU only.

Conservative: whatever a float64 intersection of a camera ray with a primitive accepts, the ray's block has that
primitive's bit. Useful: on the all-diffuse Cornell box at 1024x1024 a block keeps at most 3 of the 14 records on
average, and the blocks beside the box keep none.
"""
import os

import numpy as np
import pytest

import nori_hip as nh
import scenegen
from primary_mask_records import device_records, is_sphere

LOOKAT = '<lookat target="0, 0.893051, 4.41198" origin="0, 0.919769, 5.41159" up="0, 1, 0"/>'
# the reference's camera, two cameras moved and turned, and one inside the box (walls behind it)
CAMERAS = {
    "reference": LOOKAT,
    "right_above": '<lookat target="0, 0.8, 0" origin="1.5, 1.6, 4.5" up="0, 1, 0"/>',
    "low_tilted": '<lookat target="0.3, 1.0, 0" origin="-0.8, 0.3, 3.9" up="0.2, 1, 0"/>',
    "inside": '<lookat target="-0.3, 0.6, -1" origin="0.1, 1.0, 0.5" up="0, 1, 0"/>',
}


def _scene(tmp, camera, w, h, variant="c2"):
    xml = scenegen.cbox_xml(str(tmp), variant)
    text = open(xml).read()
    assert text.count(LOOKAT) == 1
    path = os.path.join(os.path.dirname(xml), f"pm_{camera}.xml")
    with open(path, "w") as f:
        f.write(text.replace(LOOKAT, CAMERAS[camera]))
    s = nh.Scene(path)
    s.set_resolution(w, h)
    return s


def _camera_rays(cam, xy):
    """PerspectiveCamera::sampleRay for raster positions xy (n, 2), in float64 on the camera's float32 matrices."""
    s2c = np.array(cam.sample_to_camera[:], np.float64).reshape(4, 4)
    c2w = np.array(cam.camera_to_world[:], np.float64).reshape(4, 4)
    n = len(xy)
    smp = np.stack([xy[:, 0] * float(cam.inv_output_size[0]), xy[:, 1] * float(cam.inv_output_size[1]),
                    np.zeros(n), np.ones(n)], axis=1)
    r = smp @ s2c.T
    dl = r[:, :3] / r[:, 3:4]
    dl /= np.linalg.norm(dl, axis=1, keepdims=True)
    return c2w[:3, 3] / c2w[3, 3], dl @ c2w[:3, :3].T


def _hits(records, o, d):
    """(n_rays, n_records) bool: the ray meets the primitive at some t > 0, in float64."""
    out = np.zeros((len(d), len(records)), bool)
    for k, r in enumerate(records.astype(np.float64)):
        if is_sphere(records[k]):
            L = o - r[0:3]
            qa, qb, qc = (d * d).sum(1), 2.0 * (d @ L), L @ L - r[3] * r[3]
            disc = qb * qb - 4.0 * qa * qc
            out[:, k] = (disc >= 0) & ((-qb + np.sqrt(np.maximum(disc, 0.0))) > 0)
            continue
        p0, e1, e2 = r[0:3], r[4:7] - r[0:3], r[8:11] - r[0:3]
        pvec = np.cross(d, e2)
        det = pvec @ e1
        with np.errstate(divide="ignore", invalid="ignore"):
            u = (pvec @ (o - p0)) / det
            qvec = np.cross(o - p0, e1)
            v = (d @ qvec) / det
            t = (e2 @ qvec) / det
        out[:, k] = (det != 0) & (u >= 0) & (v >= 0) & (u + v <= 1) & (t > 0)
    return out


def _block_positions(bx, by, w, h, rng):
    """Raster positions of block (bx, by): its corner pixels at jitter 0 and at the largest float below 1, 300 random
    positions inside, and 100 up to one pixel outside its rectangle. Formed in float32 as the kernels form pixel + jitter."""
    x0, y0, x1, y1 = 32 * bx, 32 * by, min(32 * bx + 32, w), min(32 * by + 32, h)
    top = np.nextafter(np.float32(1), np.float32(0))
    pos = [(np.float32(px) + jx, np.float32(py) + jy) for px in (x0, x1 - 1) for py in (y0, y1 - 1)
           for jx in (np.float32(0), top) for jy in (np.float32(0), top)]
    inside = np.stack([rng.uniform(x0, x1, 300), rng.uniform(y0, y1, 300)], axis=1)
    outside = np.stack([rng.uniform(x0 - 1, x1 + 1, 100), rng.uniform(y0 - 1, y1 + 1, 100)], axis=1)
    return np.concatenate([np.array(pos, np.float32), inside.astype(np.float32), outside.astype(np.float32)]).astype(np.float64)


@pytest.mark.parametrize("camera", list(CAMERAS))
def test_conservative(tmp_path, camera):
    """200x150 (partial blocks on two sides): every primitive a block's ray hits in float64 has its bit in the block's mask."""
    w, h = 200, 150
    s = _scene(tmp_path, camera, w, h)
    cam, rec = s.desc.camera, device_records(s, nh.Bvh(s))
    assert len(rec) == 14
    nbx, nby = (w + 31) // 32, (h + 31) // 32
    masks = nh.primary_masks(cam, rec, np.arange(nbx * nby))
    assert masks is not None and len(masks) == nbx * nby
    rng = np.random.default_rng(5)
    n_hits = 0
    for by in range(nby):
        for bx in range(nbx):
            o, d = _camera_rays(cam, _block_positions(bx, by, w, h, rng))
            hit = _hits(rec, o, d).any(axis=0)
            m = int(masks[by * nbx + bx])
            for k in np.nonzero(hit)[0]:
                assert (m >> int(k)) & 1, (camera, bx, by, int(k), hex(m))
            n_hits += int(hit.sum())
    assert n_hits > 0


def test_useful_on_the_benchmark_scene(tmp_path):
    """C2 at 1024x1024: a mean of at most 3 candidate records per block (the geometry alone gives 1.97 at the 4-pixel
    pad), and no candidate in a block whose padded rectangle misses the projection of the whole scene."""
    w = h = 1024
    s = _scene(tmp_path, "reference", w, h)
    cam, rec = s.desc.camera, device_records(s, nh.Bvh(s))
    pad = nh.primary_mask_pad(w, h)
    assert pad == 4 and nh.primary_mask_pad(64, 64) == 2 and nh.primary_mask_pad(4096, 2048) == 16
    masks = nh.primary_masks(cam, rec, np.arange(32 * 32))
    pop = np.array([bin(int(m)).count("1") for m in masks])
    print(f"mean popcount {pop.mean():.3f}, blocks with mask 0: {(pop == 0).mean():.3f}")
    assert pop.mean() <= 3.0
    # the scene's projection: every vertex and sphere-box corner (all in front of this camera), by the inverse of
    # _camera_rays -- raster x, y from the camera-space direction
    pts = [rec[:, 0:3], rec[:, 4:7], rec[:, 8:11]]
    sph = np.array([is_sphere(r) for r in rec], bool)
    tri_pts = np.concatenate([p[~sph] for p in pts]).astype(np.float64)
    corners = [rec[sph, 0:3].astype(np.float64) + 1.01 * rec[sph, 3:4].astype(np.float64) * (2.0 * np.array(sg) - 1.0)
               for sg in np.ndindex(2, 2, 2)]
    world = np.concatenate([tri_pts] + corners)
    c2w = np.array(cam.camera_to_world[:], np.float64).reshape(4, 4)
    s2c = np.array(cam.sample_to_camera[:], np.float64).reshape(4, 4)
    pc = (np.linalg.inv(c2w) @ np.concatenate([world, np.ones((len(world), 1))], axis=1).T).T
    assert (pc[:, 2] / pc[:, 3] > 0.1).all()
    ps = (np.linalg.inv(s2c) @ np.concatenate([pc[:, :3] / pc[:, 3:4], np.ones((len(pc), 1))], axis=1).T).T
    rx, ry = ps[:, 0] / ps[:, 3] * w, ps[:, 1] / ps[:, 3] * h
    n_outside = 0
    for by in range(32):
        for bx in range(32):
            x0, y0, x1, y1 = 32 * bx - pad - 1, 32 * by - pad - 1, 32 * bx + 32 + pad + 1, 32 * by + 32 + pad + 1
            if x1 < rx.min() or x0 > rx.max() or y1 < ry.min() or y0 > ry.max():
                n_outside += 1
                assert masks[by * 32 + bx] == 0, (bx, by, hex(int(masks[by * 32 + bx])))
    assert n_outside > 0


def test_behind_the_camera(tmp_path):
    """The camera inside the box: a record with a vertex behind the camera plane is a candidate of every block."""
    w, h = 200, 150
    s = _scene(tmp_path, "inside", w, h)
    cam, rec = s.desc.camera, device_records(s, nh.Bvh(s))
    masks = nh.primary_masks(cam, rec, np.arange(7 * 5))
    w2c = np.linalg.inv(np.array(cam.camera_to_world[:], np.float64).reshape(4, 4))
    n_behind = 0
    for k, r in enumerate(rec):
        if is_sphere(r):
            continue
        z = [(w2c @ np.append(r[4 * j:4 * j + 3].astype(np.float64), 1.0))[2] for j in range(3)]
        if min(z) <= 0:
            n_behind += 1
            assert all((int(m) >> k) & 1 for m in masks), k
    assert n_behind >= 4
    assert any(int(m) != int(masks[0]) for m in masks)  # (the records in front are still culled)


def test_feature_absent(tmp_path):
    """More than 64 records, or a camera with a lens: no table."""
    s = _scene(tmp_path, "reference", 64, 64)
    cam, rec = s.desc.camera, device_records(s, nh.Bvh(s))
    blocks = np.arange(4)
    assert nh.primary_masks(cam, rec, blocks) is not None
    many = np.concatenate([rec] * 5)
    assert nh.primary_masks(cam, many[:64], blocks) is not None
    assert nh.primary_masks(cam, many[:65], blocks) is None
    lens = nh.nh_camera.from_buffer_copy(cam)
    lens.lens_radius, lens.focal_distance = 0.08, 3.2
    assert nh.primary_masks(lens, rec, blocks) is None

