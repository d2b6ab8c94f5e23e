"""Bounce 0 with the per-block candidate masks (host/primary_masks.cpp, leaf_test<.., MASKED>): the wavefront framebuffer
equals, element for element, the same render with NH_PRIMARY_MASKS=0 and the megakernel's. nh_render_stats::primary_masks
says whether bounce 0 ran with masks: 1 by default on these scenes, 0 with NH_PRIMARY_MASKS=0 and for a camera with a lens.
Every render has collect_stats off (the counting kernels never use masks). Every case with masks also checks on the
host, for its own scene, resolution and blocks, that the table leaves records out: an image equal to the unmasked one
then shows that skipping them changes nothing, not that nothing was skipped.
"""
import os

import numpy as np
import pytest

import nori_hip as nh
import scenegen
from primary_mask_records import device_records

pytestmark = pytest.mark.gpu

LOOKAT = '<lookat target="0, 0.893051, 4.41198" origin="0, 0.919769, 5.41159" up="0, 1, 0"/>'
INSIDE = '<lookat target="-0.3, 0.6, -1" origin="0.1, 1.0, 0.5" up="0, 1, 0"/>'
LENS = ('<camera type="perspective"><float name="lensRadius" value="0.08"/>'
        '<float name="focalDistance" value="3.2"/>')


def _scene(tmp, variant, w, h, old=None, new=None):
    xml = scenegen.cbox_xml(str(tmp), variant)
    if old is not None:
        text = open(xml).read()
        assert text.count(old) == 1, old
        xml = os.path.join(os.path.dirname(xml), "pm_edit.xml")
        with open(xml, "w") as f:
            f.write(text.replace(old, new))
    s = nh.Scene(xml)
    s.set_resolution(w, h)
    return s, nh.Bvh(s)


def _render(s, b, mode, calls, seed, blocks=None):
    ctx = nh.Context(0)
    ctx.upload(s, b)
    for i, (s0, s1) in enumerate(calls):
        ctx.render(s0, s1, seed=seed, traversal=nh.TRAVERSAL_ORDERED, clear=i == 0, stats=False, mode=mode, blocks=blocks)
    ctx.synchronize()
    fb, st = ctx.framebuffer(), ctx.stats()
    ctx.close()
    return fb, st


def _culled(s, b, blocks):
    """(records left out, summed over the rendered blocks; blocks that leave at least one out) of the table the host
    builds for this scene -- nh_render builds its table with the same function from the same camera and records."""
    w, h = s.width, s.height
    ids = np.arange(((w + 31) // 32) * ((h + 31) // 32)) if blocks is None else np.asarray(blocks)
    rec = device_records(s, b)
    m = nh.primary_masks(s.desc.camera, rec, ids)
    if m is None:
        return 0, 0
    out = [len(rec) - bin(int(x)).count("1") for x in m]
    return sum(out), sum(1 for x in out if x)


def _check(monkeypatch, s, b, calls, seed, traits, blocks=None, masks=1):
    if masks:
        n_out, n_blocks = _culled(s, b, blocks)
        print(f"records left out over the rendered blocks: {n_out}, in {n_blocks} block(s)")
        assert n_out >= 1 and n_blocks >= 1, (n_out, n_blocks)
    else:
        assert _culled(s, b, blocks) == (0, 0)
    monkeypatch.delenv("NH_PRIMARY_MASKS", raising=False)
    on, st_on = _render(s, b, nh.MODE_WAVEFRONT, calls, seed, blocks)
    monkeypatch.setenv("NH_PRIMARY_MASKS", "0")
    off, st_off = _render(s, b, nh.MODE_WAVEFRONT, calls, seed, blocks)
    mk, st_mk = _render(s, b, nh.MODE_MEGAKERNEL, calls, seed, blocks)
    assert st_on["primary_masks"] == masks and st_off["primary_masks"] == 0 and st_mk["primary_masks"] == 0
    assert st_on["bounce_traits"] == traits and st_off["bounce_traits"] == traits
    assert np.abs(on).sum() > 0
    np.testing.assert_array_equal(on, off)
    np.testing.assert_array_equal(on, mk)


def test_partial_blocks(gpu, tmp_path, monkeypatch):
    """C2 at 40x24: both blocks partial."""
    s, b = _scene(tmp_path, "c2", 40, 24)
    _check(monkeypatch, s, b, [(0, 12)], 13, 2)


def test_list_not_a_multiple_of_64(gpu, tmp_path, monkeypatch):
    """C2 at 70x50: 3500 pixels, so waves straddle blocks and rounds, and the last wave of a launch is partial."""
    s, b = _scene(tmp_path, "c2", 70, 50)
    _check(monkeypatch, s, b, [(0, 9)], 21, 2)


def test_general_kernels_c1(gpu, tmp_path, monkeypatch):
    """C1 (mirror and dielectric spheres) at 40x24: the general bounce kernels' first_vertex."""
    s, b = _scene(tmp_path, "c1", 40, 24)
    _check(monkeypatch, s, b, [(0, 8)], 3, 1)


def test_traits_off(gpu, tmp_path, monkeypatch):
    """C2 with NH_BOUNCE_TRAITS=0: the lean general kernels."""
    monkeypatch.setenv("NH_BOUNCE_TRAITS", "0")
    s, b = _scene(tmp_path, "c2", 48, 40)
    _check(monkeypatch, s, b, [(0, 8)], 5, 1)


def test_camera_inside_the_box(gpu, tmp_path, monkeypatch):
    """Walls behind the camera: their records stay candidates of every block."""
    s, b = _scene(tmp_path, "c2", 72, 40, LOOKAT, INSIDE)
    _check(monkeypatch, s, b, [(0, 8)], 7, 2)


def test_block_subset(gpu, tmp_path, monkeypatch):
    """Every other block of a 96x64 image: the mask table covers the image's block grid, the list only some of it."""
    s, b = _scene(tmp_path, "c2", 96, 64)
    blocks = nh.tile_shard(96, 64, 2, 1)
    assert 0 < len(blocks) < 6
    _check(monkeypatch, s, b, [(0, 8)], 9, 2, blocks=blocks)


def test_round_offset_two_calls(gpu, tmp_path, monkeypatch):
    """A render that starts at round 5, in two calls."""
    s, b = _scene(tmp_path, "c2", 40, 24)
    _check(monkeypatch, s, b, [(5, 11), (11, 17)], 11, 2)


def test_lens_scene_runs_without_masks(gpu, tmp_path, monkeypatch):
    """A thin-lens camera's rays do not leave one point: no table, the field reads 0."""
    s, b = _scene(tmp_path, "c2", 40, 24, '<camera type="perspective">', LENS)
    _check(monkeypatch, s, b, [(0, 8)], 15, 1, masks=0)
