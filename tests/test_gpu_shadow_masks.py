"""Bounce 0's light samples with candidate masks (host/shadow_masks.cpp, rr_step<.., SMASK>): the wavefront framebuffer
equals, element for element, the same render with NH_SHADOW_MASKS=1 and with NH_SHADOW_MASKS=0 (every record tested)
and the megakernel's. nh_render_stats::shadow_masks says which masks the bounce kernels ran with: 2 by default and with
NH_SHADOW_MASKS=2, 0 with NH_SHADOW_MASKS=0 -- and with 1: the emitter-side word alone at every bounce was measured and
is not built, so that level runs without masks; 0 for a scene with a point light, for a camera
with a lens and for a collect_stats render. Every masked case first checks on the host, for its own scene, resolution and blocks, that its tables leave
records out: an equal image then shows that skipping them changes nothing, not that nothing was skipped.
"""
import os

import numpy as np
import pytest

import nori_hip as nh
import scenegen
from light_scenes import point_xml
from primary_mask_records import device_records

pytestmark = pytest.mark.gpu

LOOKAT = '<lookat target="0, 0.893051, 4.41198" origin="0, 0.919769, 5.41159" up="0, 1, 0"/>'
INSIDE = '<lookat target="-0.3, 0.6, -1" origin="0.1, 1.0, 0.5" up="0, 1, 0"/>'
LENS = ('<camera type="perspective"><float name="lensRadius" value="0.08"/>'
        '<float name="focalDistance" value="3.2"/>')
W, H = 96, 80
CALLS = [(0, 3), (3, 4)]


def _scene(tmp, variant, old=None, new=None, extra=""):
    xml = scenegen.cbox_xml(str(tmp), variant, extra_shapes=extra)
    if old is not None:
        text = open(xml).read()
        assert text.count(old) == 1, old
        xml = os.path.join(os.path.dirname(xml), "sm_edit.xml")
        with open(xml, "w") as f:
            f.write(text.replace(old, new))
    s = nh.Scene(xml)
    s.set_resolution(W, H)
    return s, nh.Bvh(s)


def _render(s, b, mode, seed, blocks=None, stats=False):
    ctx = nh.Context(0)
    ctx.upload(s, b)
    for i, (s0, s1) in enumerate(CALLS):
        ctx.render(s0, s1, seed=seed, traversal=nh.TRAVERSAL_ORDERED, clear=i == 0, stats=stats, mode=mode, blocks=blocks)
    ctx.synchronize()
    fb, st = ctx.framebuffer(), ctx.stats()
    ctx.close()
    return fb, st


def _left_out(s, b, blocks):
    """(records the emitter-side word leaves out; records the per-block words leave out, summed over the rendered blocks
    that have candidates) of the tables the host builds -- nh_render builds its own with the same functions."""
    ids = np.arange(((W + 31) // 32) * ((H + 31) // 32)) if blocks is None else np.asarray(blocks)
    rec = device_records(s, b)
    word, masks = nh.shadow_masks(s.desc.camera, rec, nh.shadow_emitter_faces(s.desc), ids)
    pm = nh.primary_masks(s.desc.camera, rec, ids)
    n_word = len(rec) - bin(word & ((1 << len(rec)) - 1)).count("1")
    if masks is None:
        return n_word, 0
    return n_word, sum(len(rec) - bin(int(x) & ((1 << len(rec)) - 1)).count("1") for x, p in zip(masks, pm) if p)


@pytest.mark.parametrize("flat", ["default", "0"])
@pytest.mark.parametrize("subset", [False, True])
@pytest.mark.parametrize("camera", ["lookat", "inside"])
@pytest.mark.parametrize("variant", ["c2", "c1"])
def test_masks_change_nothing(gpu, tmp_path, monkeypatch, variant, camera, subset, flat):
    if flat == "0":
        monkeypatch.setenv("NH_FLAT_TRACE", "0")
    else:
        monkeypatch.delenv("NH_FLAT_TRACE", raising=False)
    s, b = _scene(tmp_path, variant, *((LOOKAT, INSIDE) if camera == "inside" else ()))
    blocks = nh.tile_shard(W, H, 2, 1) if subset else None
    n_word, n_blocks = _left_out(s, b, blocks)
    print(f"left out: {n_word} by the emitter-side word, {n_blocks} over the rendered blocks")
    assert n_word >= 1 and n_blocks >= 1
    seed = 17
    fbs, sts = {}, {}
    for level in ("2", "1", "0"):
        monkeypatch.setenv("NH_SHADOW_MASKS", level)
        fbs[level], sts[level] = _render(s, b, nh.MODE_WAVEFRONT, seed, blocks)
    monkeypatch.delenv("NH_SHADOW_MASKS")
    fbs["default"], sts["default"] = _render(s, b, nh.MODE_WAVEFRONT, seed, blocks)
    fbs["mk"], sts["mk"] = _render(s, b, nh.MODE_MEGAKERNEL, seed, blocks)
    assert [sts[k]["shadow_masks"] for k in ("default", "2", "1", "0", "mk")] == [2, 2, 0, 0, 0]
    assert sts["2"]["flat_trace"] == sts["0"]["flat_trace"] and (flat == "default" or sts["2"]["flat_trace"] == 0)
    assert variant != "c2" or sts["2"]["flat_trace"] == (1 if flat == "default" else 0)
    assert np.abs(fbs["2"]).sum() > 0
    for k in ("default", "1", "0", "mk"):
        np.testing.assert_array_equal(fbs["2"], fbs[k], err_msg=k)


def test_not_used(gpu, tmp_path, monkeypatch):
    """A point light beside the area light, a thin-lens camera, a collect_stats render: the field reads 0, and the image
    is the megakernel's."""
    monkeypatch.delenv("NH_SHADOW_MASKS", raising=False)
    cases = [(_scene(tmp_path, "c2", extra=point_xml((0.0, 1.2, 0.0), (5, 5, 5))), False),
             (_scene(tmp_path, "c2", '<camera type="perspective">', LENS), False),
             (_scene(tmp_path, "c2"), True)]
    for (s, b), stats in cases:
        fb, st = _render(s, b, nh.MODE_WAVEFRONT, 23, stats=stats)
        mk, _ = _render(s, b, nh.MODE_MEGAKERNEL, 23, stats=stats)
        assert st["shadow_masks"] == 0
        np.testing.assert_array_equal(fb, mk)
