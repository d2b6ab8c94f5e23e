"""The diffuse area-light instantiations of the RR-ahead kernels (wf_bounce_rr / wf_tail_rr<.., TRAIT>, their own
kernels for bounce 0 and the later bounces, scene tables staged in LDS) and the staging of a small scene as a copy of
an image built at upload.

Unless stated otherwise every case checks, with collect_stats on and off (different instantiations): the wavefront
framebuffer equals the megakernel's and the oracle's element for element, and (stats on) both schedules count the same
ray queries, node visits and primitive tests. nh_render_stats::bounce_traits names the bounce instantiation that ran:
2 the trait kernels, 1 the general ones.
"""
import os

import numpy as np
import pytest

import nori_hip as nh
import nori_oracle as no
import scenegen

pytestmark = pytest.mark.gpu

COUNTERS = ("ray_queries", "nodes_visited", "prims_tested")


def _render(s, b, mode, stats, calls, seed, blocks=None):
    ctx = nh.Context(0)
    ctx.upload(s, b)
    for i, (s0, s1) in enumerate(calls):
        ctx.render(s0, s1, seed=seed, traversal=nh.TRAVERSAL_ORDERED, clear=i == 0, stats=stats, mode=mode,
                   blocks=blocks)
    ctx.synchronize()
    return ctx.framebuffer(), ctx.stats()


_ORACLE = {}


def _oracle(key, s, calls, seed, blocks=None):
    """The oracle's framebuffer of a case, rendered once and shared by the stats on / off runs."""
    if key not in _ORACLE:
        orc = no.OracleScene(s)
        fb = None
        for s0, s1 in calls:
            fb = orc.render(s0, s1, seed=seed, blocks=blocks, rgbw=fb)
        fb.setflags(write=False)
        _ORACLE[key] = fb
    return _ORACLE[key]


def _check(key, s, b, stats, calls, seed, expect, blocks=None):
    """Wavefront vs megakernel vs oracle; returns the wavefront framebuffer and stats."""
    mk, st_mk = _render(s, b, nh.MODE_MEGAKERNEL, stats, calls, seed, blocks)
    wf, st_wf = _render(s, b, nh.MODE_WAVEFRONT, stats, calls, seed, blocks)
    assert st_wf["bounce_traits"] == expect, (key, st_wf["bounce_traits"])
    np.testing.assert_array_equal(wf, mk, err_msg=str(key))
    np.testing.assert_array_equal(wf, _oracle(key, s, calls, seed, blocks), err_msg=str(key))
    assert np.abs(wf).sum() > 0
    if stats:
        assert st_wf["ray_queries"] > 0
        for k in COUNTERS:
            assert st_wf[k] == st_mk[k], (key, k)
    return wf, st_wf


def _scene(xml, w, h):
    s = nh.Scene(xml)
    s.set_resolution(w, h)
    return s, nh.Bvh(s)


@pytest.mark.parametrize("stats", [True, False], ids=["stats", "plain"])
def test_partial_workgroup(gpu, tmp_path, monkeypatch, stats):
    """40x24: 960 paths per round, so the last 256-path workgroup of a bounce is partial -- in one call of 6 rounds and
    in a call that starts at round 5. NH_BOUNCE_TRAITS=0 runs the general kernels: the same array."""
    s, b = _scene(scenegen.cbox_xml(str(tmp_path), "c2"), 40, 24)
    for calls in ([(0, 6)], [(5, 9)]):
        monkeypatch.delenv("NH_BOUNCE_TRAITS", raising=False)
        fb, _ = _check(("partial", calls[0]), s, b, stats, calls, 13, 2)
        monkeypatch.setenv("NH_BOUNCE_TRAITS", "0")
        off, _ = _check(("partial", calls[0]), s, b, stats, calls, 13, 1)
        np.testing.assert_array_equal(fb, off)


@pytest.mark.parametrize("pools", ["1", "2"])
@pytest.mark.parametrize("stats", [True, False], ids=["stats", "plain"])
def test_block_subset(gpu, tmp_path, monkeypatch, stats, pools):
    """Every other block of a 96x64 image: the pixel list is not the image, so a path's sample round (its stream
    increment) is its id divided by the list's length."""
    monkeypatch.setenv("NH_POOLS", pools)
    s, b = _scene(scenegen.cbox_xml(str(tmp_path), "c2"), 96, 64)
    blocks = nh.tile_shard(96, 64, 2, 1)
    assert 0 < len(blocks) < 6
    _check("subset", s, b, stats, [(0, 5)], 7, 2, blocks=blocks)


@pytest.mark.parametrize("tail", ["64", "200000"])
@pytest.mark.parametrize("stats", [True, False], ids=["stats", "plain"])
def test_tail_threshold(gpu, tmp_path, monkeypatch, stats, tail):
    """NH_TAIL small: the trait bounce kernels finish nearly every path; large: the trait tail takes the chunk over
    after bounce 0 (test_cooperative_tail_matches_oracle's thresholds for C2)."""
    monkeypatch.setenv("NH_TAIL", tail)
    s, b = _scene(scenegen.cbox_xml(str(tmp_path), "c2"), 64, 48)
    _, st = _check("tail", s, b, stats, [(0, 8)], 17, 2)
    assert st["fused_bounce"] == 1
    if tail == "200000":
        assert st["launches_tail"] >= 1 and st["launches_shade"] == 1  # bounce 0, then the tail
    else:
        assert st["launches_shade"] > 2
    if stats:
        assert st["bounce_bounces"] > 0
        assert tail != "200000" or st["tail_bounces"] > 0


def _edited(xml, name, old, new):
    text = open(xml).read()
    assert text.count(old) >= 1, old
    path = os.path.join(os.path.dirname(xml), name)
    with open(path, "w") as f:
        f.write(text.replace(old, new, 1))
    return path


def _fallback_xml(tmp, case):
    c2 = scenegen.cbox_xml(tmp, "c2")
    if case == "c1":  # mirror and dielectric spheres
        return scenegen.cbox_xml(tmp, "c1")
    if case == "microfacet":
        return _edited(c2, "fb_microfacet.xml", f'<bsdf type="diffuse"><color name="albedo" value="{scenegen.C2_ALBEDO}"/></bsdf>',
                       '<bsdf type="microfacet"><float name="alpha" value="0.3"/><color name="kd" value="0.3 0.2 0.1"/></bsdf>')
    if case == "point_light":
        return _edited(c2, "fb_point.xml", "</scene>",
                       '<emitter type="point"><point name="position" value="0 1.2 0"/>'
                       '<color name="power" value="8 8 8"/></emitter>\n</scene>')
    if case == "sphere_emitter":
        return _edited(c2, "fb_sphere.xml", "</scene>",
                       '<shape type="sphere"><point name="center" value="0 1.1 0"/><float name="radius" value="0.12"/>'
                       '<emitter type="area"><color name="radiance" value="6 6 6"/></emitter></shape>\n</scene>')
    if case == "path_mats":
        return _edited(c2, "fb_mats.xml", '<integrator type="path_mis"/>', '<integrator type="path_mats"/>')
    if case == "thin_lens":
        return _edited(c2, "fb_lens.xml", '<camera type="perspective">',
                       '<camera type="perspective"><float name="lensRadius" value="0.08"/>'
                       '<float name="focalDistance" value="3.2"/>')
    raise ValueError(case)


@pytest.mark.parametrize("case", ["c1", "microfacet", "point_light", "sphere_emitter", "path_mats", "thin_lens"])
@pytest.mark.parametrize("stats", [True, False], ids=["stats", "plain"])
def test_fallbacks(gpu, tmp_path, stats, case):
    """Scenes outside the trait (each one condition off) take the general kernels and still match."""
    s, b = _scene(_fallback_xml(str(tmp_path), case), 32, 32)
    _check(("fallback", case), s, b, stats, [(0, 4)], 3, 1)


def _table_bytes(s):
    """The LDS bytes of a scene's staged tables (include/nori_hip.h NH_SMALL_TABLES_BYTES)."""
    d = s.desc
    cdf = faces = 0
    for i in range(d.n_emitters):
        sh = d.shapes[d.emitters[i].shape]
        cdf += sh.n_faces + 1
        faces += sh.n_faces
    return 64 * d.n_shapes + 48 * d.n_bsdfs + 32 * d.n_emitters + 16 * ((cdf + 3) // 4) + 48 * faces


def _quads_xml(tmp, k):
    """The diffuse box with k extra tiny diffuse quads (one shape and one BSDF each) on the floor."""
    mesh = os.path.join(tmp, "scenes/pa4/cbox/meshes/tiny_quad.obj")
    scenegen.materialize(tmp)
    with open(mesh, "w") as f:
        f.write("v 0 0 0\nv 0.02 0 0\nv 0.02 0 0.02\nv 0 0 0.02\nf 1 3 2\nf 1 4 3\n")
    shapes = "".join(
        f'<shape type="obj"><string name="filename" value="meshes/tiny_quad.obj"/>'
        f'<transform name="toWorld"><translate value="{-0.6 + 0.04 * i:.2f}, 0.01, 0.8"/></transform>'
        f'<bsdf type="diffuse"><color name="albedo" value="0.2 0.6 0.3"/></bsdf></shape>\n' for i in range(k))
    return scenegen.cbox_xml(tmp, "c2", extra_shapes=shapes)


@pytest.mark.parametrize("stats", [True, False], ids=["stats", "plain"])
def test_table_budget(gpu, tmp_path, stats):
    """The largest scene whose tables fit the LDS budget runs the trait kernels on its staged tables; one more shape
    puts the tables over the budget and the scene on the general kernels, which read them from global memory. Both
    match."""
    base = _table_bytes(nh.Scene(_quads_xml(str(tmp_path), 0)))
    per = _table_bytes(nh.Scene(_quads_xml(str(tmp_path), 1))) - base
    assert per == 64 + 48
    k = (nh.SMALL_TABLES_BYTES - base) // per  # the last count that fits
    for n, expect in ((k, 2), (k + 1, 1)):
        s, b = _scene(_quads_xml(str(tmp_path), n), 32, 32)
        assert (_table_bytes(s) <= nh.SMALL_TABLES_BYTES) == (expect == 2)
        _, st = _check(("budget", n), s, b, stats, [(0, 4)], 5, expect)
        assert st["lds_scene"] == 1 and st["fused_bounce"] == 1
