"""The photon mapper's host side -- loader, refusals, automatic radius, decode tables, C-ABI surface. CPU only."""
import ctypes
import json
import math
import os

import numpy as np
import pytest

import nori_hip as nh
import photon_refs as pr
import volume_refs as vr

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F32 = np.float32

CAMERA = ('<camera type="perspective"><transform name="toWorld"><lookat target="0,0,0" origin="0,3,6" up="0,1,0"/>'
          '</transform><integer name="width" value="16"/><integer name="height" value="16"/></camera>')
LIGHT = ('<shape type="sphere"><point name="center" value="0,3,0"/><float name="radius" value="0.5"/>'
         '<emitter type="area"><color name="radiance" value="10,10,10"/></emitter></shape>')
FLOOR = ('<shape type="sphere"><point name="center" value="0,-100,0"/><float name="radius" value="100"/>'
         '<bsdf type="diffuse"/></shape>')


def scene_text(integrator='<integrator type="photonmapper"/>', body=LIGHT + FLOOR, sampler=""):
    return f"<scene>{integrator}{sampler}{CAMERA}{body}</scene>"


def load(tmp_path, text, name="s.xml"):
    p = tmp_path / name
    p.write_text(text)
    return nh.Scene(str(p))


@pytest.fixture(scope="module")
def photon_dir(tmp_path_factory):
    """the reference's photon mapper scenes, in a directory of this module's own"""
    return pr.materialize(str(tmp_path_factory.mktemp("photon_scenes")))


def test_loader_defaults_and_values(tmp_path, photon_dir):
    s = load(tmp_path, scene_text())
    assert s.desc.integrator == nh.INTEGRATOR_PHOTONMAPPER == 9
    n, r = s.photon_params()
    assert n == 1000000 and r > 0  # photonRadius defaults to 0 = automatic, resolved by the getter
    s = load(tmp_path, scene_text('<integrator type="photonmapper"><integer name="photonCount" value="1234"/>'
                                  '<float name="photonRadius" value="0.25"/></integrator>'))
    assert s.photon_params() == (1234, 0.25)
    s.set_photon_params(77, 0.5)
    assert s.photon_params() == (77, 0.5)
    with pytest.raises(nh.NoriError):
        s.set_photon_params(0, 0.5)
    with pytest.raises(nh.NoriError):
        s.set_photon_params(10, -1.0)
    # the reference's own scene: scenes/pa4/cbox/cbox_pmap.xml
    c = nh.Scene(os.path.join(photon_dir, pr.CBOX_PMAP))
    assert c.desc.integrator == nh.INTEGRATOR_PHOTONMAPPER and c.desc.sample_count == 32
    assert c.photon_params() == (10000000, float(F32(0.05)))
    # another integrator: the defaults
    assert nh.Scene(os.path.join(photon_dir, "scenes/pa4/cbox/cbox_path_mis.xml")).photon_params()[0] == 1000000


REFUSALS = {
    "no emitter": (scene_text(body=FLOOR), "without an emitter is not supported"),
    "point light": (scene_text(body=LIGHT + FLOOR + '<emitter type="point"><point name="position" value="0,2,0"/>'
                                                       '<color name="power" value="1,1,1"/></emitter>'),
                    "not an area light is not supported"),
    "spot light": (scene_text(body=LIGHT + FLOOR + '<emitter type="spot"><point name="position" value="0,2,0"/>'
                                                      '<vector name="direction" value="0,-1,0"/>'
                                                      '<color name="power" value="1,1,1"/>'
                                                      '<float name="falloffstart" value="10"/>'
                                                      '<float name="totalwidth" value="30"/></emitter>'),
                   "not an area light is not supported"),
    "directional light": (scene_text(body=LIGHT + FLOOR + '<emitter type="directional">'
                                                             '<vector name="direction" value="0,-1,0"/>'
                                                             '<color name="radiance" value="1,1,1"/></emitter>'),
                          "not an area light is not supported"),
    "envmap": (scene_text(body=LIGHT + FLOOR + '<emitter type="envmap"/>'), "not an area light is not supported"),
    "shape medium": (scene_text(body=LIGHT + FLOOR + '<shape type="sphere"><point name="center" value="0,1,0"/>'
                                                        '<medium type="homog"/></shape>'),
                     "medium is not supported"),
    "ambient medium": (scene_text(body=LIGHT + FLOOR + '<medium type="homog"/>'), "medium is not supported"),
    "textured diffuse": (scene_text(body=LIGHT + '<shape type="sphere"><point name="center" value="0,-100,0"/>'
                                                 '<float name="radius" value="100"/><bsdf type="diffuse">'
                                                 '<texture type="checkerboard_color" name="albedo"/></bsdf></shape>'),
                         "textured diffuse or Disney albedo is not supported"),
    "textured disney": (scene_text(body=LIGHT + '<shape type="sphere"><point name="center" value="0,-100,0"/>'
                                                '<float name="radius" value="100"/><bsdf type="disney">'
                                                '<texture type="checkerboard_color" name="albedo"/></bsdf></shape>'),
                        "textured diffuse or Disney albedo is not supported"),
    "adaptive sampler": (scene_text(sampler='<sampler type="adaptive"><integer name="sampleCount" value="4"/></sampler>'),
                         "adaptive sampler is not supported"),
}


@pytest.mark.parametrize("case", sorted(REFUSALS))
def test_loader_refuses_what_the_reference_cannot_run(tmp_path, case):
    text, message = REFUSALS[case]
    with pytest.raises(nh.NoriError, match=message):
        load(tmp_path, text)
    # the same scene loads under a path tracer, so it is the photon mapper that refuses it (a scene without an
    # emitter or with a medium aside: path_mats loads them too)
    other = "path_vol_mats" if "medium" in case else "path_mats"
    load(tmp_path, text.replace('<integrator type="photonmapper"/>', f'<integrator type="{other}"/>'), "other.xml")


def test_no_emitter_comes_before_the_other_end_of_scene_errors(tmp_path):
    with pytest.raises(nh.NoriError, match="not supported"):
        load(tmp_path, '<scene><integrator type="photonmapper"/><camera type="perspective"/></scene>')
    with pytest.raises(nh.NoriError, match="without an emitter is not supported"):
        load(tmp_path, '<scene><integrator type="photonmapper"/></scene>')  # (no camera either)


def test_is_diffuse_bsdfs_load(tmp_path):
    """mirror, dielectric, microfacet and an untextured Disney BSDF are all legal under the photon mapper"""
    body = LIGHT + FLOOR + "".join(
        f'<shape type="sphere"><point name="center" value="{x},1,0"/><float name="radius" value="0.4"/>'
        f'<bsdf type="{t}"/></shape>' for x, t in ((-2, "mirror"), (-1, "dielectric"), (1, "microfacet"), (2, "disney")))
    assert load(tmp_path, scene_text(body=body)).desc.n_shapes == 6


@pytest.mark.parametrize("case", ["spheres", "cbox"])
def test_automatic_radius_is_the_reference_expression(tmp_path, photon_dir, case):
    """getBoundingBox().getExtents().norm() / 500.0f in fp32 with Eigen's grouping, over the BVH root box, bit for bit"""
    s = load(tmp_path, scene_text()) if case == "spheres" else nh.Scene(os.path.join(photon_dir, pr.CBOX_PMAP))
    s.set_photon_params(1000, 0.0)
    b = nh.Bvh(s).desc
    want = pr.auto_radius(list(b.bbox_min), list(b.bbox_max))
    got = F32(s.photon_params()[1])
    assert got.view(np.uint32) == want.view(np.uint32), (got, want)
    assert 0 < got < 1


def test_tables_match_fp64_rounded_once_within_one_ulp():
    got, want = nh.photon_tables(), pr.tables()
    for k in want:
        ulps = np.abs(got[k].view(np.int32).astype(np.int64) - want[k].view(np.int32).astype(np.int64))
        assert ulps.max() <= 1, (k, int(ulps.max()))
    assert got["exp"][0] == 0 and got["exp"][136] == 1 and np.array_equal(got["exp"], want["exp"])


def test_codec_restatement_edge_cases():
    """the restatement itself, on inputs whose bytes follow from the source by hand"""
    d = np.array([[0, 0, 1], [0, 0, -1], [1, 0, 0], [-1, -0.0, 0], [0, -1, 0]], F32)
    w = np.array([[1, 0.5, 0.25], [1e-33, 0, 0], [2, 2, 2], [0.75, 1e-4, 0], [3, 1, 2]], F32)
    b = pr.encode(d, w)
    assert list(b[0]) == [0, 0, 128, 64, 32, 129]       # acos(1) = 0; frexp(1) = (0.5, 1): scale 128
    assert list(b[1]) == [255, 0, 0, 0, 0, 0]           # acos(-1) * 256 / pi = 256 -> the 255 clamp; below 1e-32
    assert list(b[2]) == [128, 0, 128, 128, 128, 130]   # a power of two: mantissa 0.5
    assert b[3][1] == 128 and b[4][1] == 192            # atan2 = -pi -> -128 -> 128; -pi / 2 -> -64 -> 192
    assert list(b[3][2:]) == [192, 0, 0, 128]           # 1e-4 * 256 truncates to 0
    dd, ww = pr.decode(b, pr.tables())
    assert np.array_equal(ww[0], F32([1, 0.5, 0.25])) and np.array_equal(ww[1], F32([0, 0, 0]))
    assert dd[0][2] == 1 and abs(dd[2][0] - 1) < 1e-6


def test_new_symbols_are_exported_and_the_desc_did_not_grow():
    lib = ctypes.CDLL(nh.LIB_PATH)
    for name in ("nh_scene_get_photon_params", "nh_scene_set_photon_params", "nh_photon_tables", "nh_photon_map_build",
                 "nh_get_photon_stats", "nh_get_photons", "nh_photon_query"):
        assert hasattr(lib, name), name
    assert ctypes.sizeof(nh.nh_scene_desc) == 664  # its size in the commit before the photon mapper
    assert ctypes.sizeof(nh.nh_photon_params) == 8 and ctypes.sizeof(nh.nh_photon_stats) == 24
    hdr = open(os.path.join(REPO, "include", "nori_hip.h")).read()
    assert "NH_INTEGRATOR_PHOTONMAPPER = 9" in hdr and "NH_EMITTER_QUERY_SAMPLE_PHOTON = 3" in hdr


def test_table_pmap_loads(photon_dir):
    """scenes/pa4/table/table_pmap.xml as it is: two area lights, a microfacet table top, three dielectric glasses"""
    s = nh.Scene(os.path.join(photon_dir, pr.TABLE_PMAP))
    d = s.desc
    assert (d.integrator, d.n_shapes, d.n_emitters) == (nh.INTEGRATOR_PHOTONMAPPER, 7, 2)
    assert s.photon_params() == (5000000, 1.0)
    types = [d.bsdfs[d.shapes[i].bsdf].type for i in range(d.n_shapes)]
    assert types.count(nh.BSDF_DIELECTRIC) == 3 and types.count(nh.BSDF_MICROFACET) == 1


# ---------------------------------------------------------------------------------------------------------------------
# the estimator's t-test, restatement against restatement (tests/test_gpu_photon.py runs it against the device)
# ---------------------------------------------------------------------------------------------------------------------
M_MAPS = 32      # maps per scene on the device side of the test
N_COMPARISONS = 3  # comparisons in tests/test_gpu_photon.py: the Sidak correction's count


def mc_fixture():
    with open(pr.PHOTON_MC_FIXTURE) as f:
        return json.load(f)


def compare(values, fixture_values, n_tests=N_COMPARISONS):
    """volume_refs' two-sample t-test at the reference's 0.01, Sidak-corrected, of a few values against the fixture's"""
    ma, sa, da = vr.seeds_estimate(values)
    mb, sb, _ = vr.seeds_estimate(fixture_values)
    return vr.t_test(ma, sa, da, mb, sb, n_tests)


def test_fixture_is_what_the_generator_writes():
    fx = mc_fixture()
    assert (fx["photon_count"], fx["radius"]) == (pr.MC_PHOTONS, pr.MC_RADIUS)
    assert sorted(fx["scenes"]) == ["glass", "one", "two"] and fx["scenes"]["two"]["weights"] == [1.0, 3.0]
    for name, rec in fx["scenes"].items():
        assert len(rec["quirks"]["luminance"]) == fx["n_samples"] >= 200
        assert rec["quirks"]["mean_photons_in_ball"] >= 50, name  # the issue's floor on the photons in the ball
    S, w = pr.mc_scenes()["one"]
    again = pr.photon_mc(S, w, pr.MC_PHOTONS, pr.MC_RADIUS, 3, 101)
    assert again["luminance"] == fx["scenes"]["one"]["quirks"]["luminance"][:3]  # fixed numpy seeds


def test_ttest_accepts_the_restatement_and_rejects_the_no_quirks_estimator():
    """M_MAPS fresh samples of the restatement pass against the fixture on every scene; M_MAPS samples of the
    quirks=False estimator (true selection probability instead of `* lights.size()`) are rejected on the two-light
    scene, and so is the fixture's own quirks=False list: M_MAPS maps are enough to tell the quirk"""
    fx = mc_fixture()["scenes"]
    for name, (S, w) in pr.mc_scenes().items():
        fresh = pr.photon_mc(S, w, pr.MC_PHOTONS, pr.MC_RADIUS, M_MAPS, 7)["luminance"]
        r = compare(fresh, fx[name]["quirks"]["luminance"])
        print(name, r)
        assert r["pass"], (name, r)
    S, w = pr.mc_scenes()["two"]
    wrong = pr.photon_mc(S, w, pr.MC_PHOTONS, pr.MC_RADIUS, M_MAPS, 8, quirks=False)["luminance"]
    r = compare(wrong, fx["two"]["quirks"]["luminance"])
    assert not r["pass"] and r["pval"] < 1e-6, r
    assert not compare(fx["two"]["no_quirks"]["luminance"][:M_MAPS], fx["two"]["quirks"]["luminance"])["pass"]
    assert math.isfinite(r["t"])
