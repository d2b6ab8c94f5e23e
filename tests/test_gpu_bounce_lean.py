"""The bounce kernels' lean head (wf_bounce_rr: the Intersection of the next hit is computed only where the hit shape
is an emitter, since the next launch recomputes it from the stored hit), under cameras that steer the lanes through
each of its branches: emitter hits in most lanes, rays in the plane of a wall, mostly misses.

Every case checks, with collect_stats on and off (different instantiations): the wavefront framebuffer equals the
megakernel's and the oracle's element for element, (stats on) both schedules count the same ray queries, node visits
and primitive tests, and the run with NH_BOUNCE_TRAITS=0 (the general lean kernels) gives the same array. 40x24 = 960
paths per round: the last 256-path workgroup of a bounce is partial.
"""
import os

import numpy as np
import pytest

import nori_hip as nh
import nori_oracle as no
import scenegen

pytestmark = pytest.mark.gpu

COUNTERS = ("ray_queries", "nodes_visited", "prims_tested")
W, H = 40, 24

_LOOKAT = '<lookat target="0, 0.893051, 4.41198" origin="0, 0.919769, 5.41159" up="0, 1, 0"/>'
# the right wall is the plane x = 1 exactly (rightwall.obj), the box spans z in [-1.04, 0.99] and is open at +z
CAMERAS = {
    # the reference's view of the box
    "default": _LOOKAT,
    # from the floor up at the light: emitter hits dominate the first vertex's head and the early bounces' heads
    "at_light": '<lookat target="-0.005, 1.58, -0.03" origin="0.1, 0.25, 0.7" up="0, 1, 0"/>',
    # the origin in the right wall's plane, looking straight down -z: rays in and next to the plane (det and t
    # numerators at and near zero), the view's middle column along the axis, half the image outside the box
    "in_wall_plane": '<lookat target="1, 0.8, 2" origin="1, 0.8, 3" up="0, 1, 0"/>',
    # far outside, the box at the image's edge: most camera rays miss everything
    "outside": '<lookat target="2.2, 0.9, 0" origin="0, 0.92, 9" up="0, 1, 0"/>',
}


def _xml(tmp, camera):
    """C2 with its camera's lookat replaced (edited in the text scenegen.cbox_xml returns)."""
    src = scenegen.cbox_xml(tmp, "c2")
    text = open(src).read()
    assert text.count(_LOOKAT) == 1
    path = os.path.join(os.path.dirname(src), f"lean_{camera}.xml")
    with open(path, "w") as f:
        f.write(text.replace(_LOOKAT, CAMERAS[camera]))
    return path


def _scene(xml):
    s = nh.Scene(xml)
    s.set_resolution(W, H)
    return s, nh.Bvh(s)


def _render(s, b, mode, stats, calls, seed, ctx=None):
    if ctx is None:
        ctx = nh.Context(0)
    ctx.upload(s, b)
    for i, (s0, s1) in enumerate(calls):
        ctx.render(s0, s1, seed=seed, traversal=nh.TRAVERSAL_ORDERED, clear=i == 0, stats=stats, mode=mode)
    ctx.synchronize()
    return ctx.framebuffer(), ctx.stats()


_ORACLE = {}


def _oracle(key, s, calls, seed):
    """The oracle's framebuffer of a case, rendered once and shared by the stats on / off runs."""
    if key not in _ORACLE:
        orc = no.OracleScene(s)
        fb = None
        for s0, s1 in calls:
            fb = orc.render(s0, s1, seed=seed, rgbw=fb)
        fb.setflags(write=False)
        _ORACLE[key] = fb
    return _ORACLE[key]


def _check(key, s, b, stats, calls, seed, monkeypatch):
    monkeypatch.delenv("NH_BOUNCE_TRAITS", raising=False)
    mk, st_mk = _render(s, b, nh.MODE_MEGAKERNEL, stats, calls, seed)
    wf, st_wf = _render(s, b, nh.MODE_WAVEFRONT, stats, calls, seed)
    assert st_wf["bounce_traits"] == 2 and st_wf["fused_bounce"] == 1, key
    monkeypatch.setenv("NH_BOUNCE_TRAITS", "0")
    gen, st_gen = _render(s, b, nh.MODE_WAVEFRONT, stats, calls, seed)
    assert st_gen["bounce_traits"] == 1, key
    monkeypatch.delenv("NH_BOUNCE_TRAITS", raising=False)
    np.testing.assert_array_equal(wf, mk, err_msg=str(key))
    np.testing.assert_array_equal(wf, _oracle(key, s, calls, seed), err_msg=str(key))
    np.testing.assert_array_equal(wf, gen, err_msg=str(key))
    assert np.abs(wf).sum() > 0
    if stats:
        assert st_wf["ray_queries"] > 0
        for k in COUNTERS:
            assert st_wf[k] == st_mk[k] == st_gen[k], (key, k, st_wf[k], st_mk[k], st_gen[k])
    return wf


@pytest.mark.parametrize("camera", list(CAMERAS))
@pytest.mark.parametrize("stats", [True, False], ids=["stats", "plain"])
def test_cameras(gpu, tmp_path, monkeypatch, stats, camera):
    """One call of 6 rounds under each camera; the default view also in a call that starts at round 3."""
    s, b = _scene(_xml(str(tmp_path), camera))
    fb = _check((camera, 0), s, b, stats, [(0, 6)], 11, monkeypatch)
    if camera == "default":
        _check((camera, 3), s, b, stats, [(3, 8)], 11, monkeypatch)
    if camera == "outside":  # most pixels saw nothing, some saw the box
        lum = fb[..., :3].sum(axis=-1)
        assert 0 < np.count_nonzero(lum) < lum.size // 2
    if camera == "at_light":  # the light's radiance reaches most of the image directly
        assert np.count_nonzero(fb[..., 0] > 5.0 * np.maximum(fb[..., 3], 1e-9)) > fb[..., 0].size // 4


@pytest.mark.parametrize("stats", [True, False], ids=["stats", "plain"])
def test_second_upload_other_camera(gpu, tmp_path, stats):
    """A context that rendered one camera's scene and is then given the same box under another camera renders what a
    fresh context renders: nothing built for the first camera at upload survives the second upload."""
    tmp = str(tmp_path)
    s1, b1 = _scene(_xml(tmp, "default"))
    s2, b2 = _scene(_xml(tmp, "in_wall_plane"))
    ctx = nh.Context(0)
    first, _ = _render(s1, b1, nh.MODE_WAVEFRONT, stats, [(0, 4)], 5, ctx=ctx)
    again, st = _render(s2, b2, nh.MODE_WAVEFRONT, stats, [(0, 4)], 5, ctx=ctx)
    fresh, _ = _render(s2, b2, nh.MODE_WAVEFRONT, stats, [(0, 4)], 5)
    assert st["bounce_traits"] == 2
    np.testing.assert_array_equal(again, fresh)
    assert not np.array_equal(first, fresh)
    np.testing.assert_array_equal(fresh, _oracle(("second", 0), s2, [(0, 4)], 5))
