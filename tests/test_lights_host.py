"""Spot and directional lights in the scene loader (spotlight.cpp:14-23, :50, :65-69; directionalLight.cpp:32-39) -- CPU
only. The reference's own scenes come from tests/golden/light_scenes.json.gz (light_scenes.materialize)."""
import os

import numpy as np
import pytest

import light_scenes
import nori_hip as nh

F = np.float32
PI_F = F(3.14159265358979323846)  # Nori's M_PI is a float constant (common.h:61)


def deg_to_rad(v):  # common.h:218
    return F(v) * (PI_F / F(180.0))


def cos_f(x):  # std::cos(float), correctly rounded
    return F(np.cos(np.float64(F(x))))


def spot_intensity(power, falloffstart, totalwidth):
    """m_power / 2.f / M_PI / (1.f - .5f * (cosTotalWidth + cosFalloffStart)) in float arithmetic"""
    cf, ct = cos_f(deg_to_rad(falloffstart)), cos_f(deg_to_rad(F(totalwidth) / F(2)))
    return F(F(F(power) / F(2)) / PI_F) / F(F(1) - F(F(0.5) * F(ct + cf))), ct, cf


@pytest.fixture(scope="module")
def light_dir(tmp_path_factory):
    return light_scenes.materialize(str(tmp_path_factory.mktemp("lights")))


def _load_cut(light_dir, rel):
    """The scene at rel with its heavy <shape> elements cut out of the XML text (no mesh substituted)."""
    text = open(os.path.join(light_dir, rel)).read()
    cut = light_scenes.cut_shapes(text)
    assert cut.count("<shape") < text.count("<shape")
    p = os.path.join(light_dir, rel[:-4] + "-cut.xml")
    with open(p, "w") as f:
        f.write(cut)
    return nh.Scene(p)


def test_float_cos_of_180_degrees_is_minus_one():
    """What makes a spot with totalwidth = 360, falloffstart = 180 a point light (tests/test_gpu_lights.py part 2):
    cos(degToRad(180.f)) is exactly -1 in float, so I = power / (4 pi) and falloff == 1."""
    assert cos_f(deg_to_rad(180.0)) == F(-1)
    assert cos_f(deg_to_rad(F(360.0) / F(2))) == F(-1)
    i, ct, cf = spot_intensity(100.0, 180.0, 360.0)
    assert ct == F(-1) and cf == F(-1)
    assert i == F(100.0) / F(F(4) * PI_F)  # PointLight::update, as the loader folds it


def test_spot_xml_loads(light_dir):
    s = nh.Scene(os.path.join(light_dir, light_scenes.SPOT_XML))
    d = s.desc
    assert d.integrator == nh.INTEGRATOR_PATH_MIS and d.n_shapes == 2 and d.n_emitters == 1 and d.envmap == -1
    e = d.emitters[0]
    assert e.type == nh.EMITTER_SPOT and e.shape == -1 and e.light_prob == 1.0
    assert list(e.position) == [-50.0, 50.0, -50.0]
    i, ct, cf = spot_intensity(200.0, 20.0, 30.0)
    assert [F(v) for v in e.radiance] == [i, i, i]
    assert abs(float(i) - 200 / (2 * np.pi) / (1 - 0.5 * (np.cos(np.radians(15)) + np.cos(np.radians(20))))) < 1e-3
    assert bool(d.emitter_ext)
    x = d.emitter_ext[0]
    assert F(x.cos_total_width) == ct and F(x.cos_falloff_start) == cf
    assert abs(float(ct) - np.cos(np.radians(15))) < 1e-6 and abs(float(cf) - np.cos(np.radians(20))) < 1e-6
    np.testing.assert_allclose(list(x.direction), np.array([1, -1, 1]) / np.sqrt(3), rtol=0, atol=1e-7)
    # Frame(direction): orthonormal, n along the direction, s x t = n
    fs, ft, fn = (np.array(list(v), np.float64) for v in (x.frame_s, x.frame_t, x.frame_n))
    np.testing.assert_allclose(fn, np.array([1, -1, 1]) / np.sqrt(3), rtol=0, atol=2e-7)
    np.testing.assert_allclose(np.cross(fs, ft), fn, rtol=0, atol=1e-6)
    assert abs(fs @ ft) < 1e-6 and abs(fs @ fs - 1) < 1e-6 and abs(ft @ ft - 1) < 1e-6
    assert list(d.emitter_cdf[0:2]) == [0.0, 1.0]


def test_spotlight_validation_loads_without_its_heavy_shapes(light_dir):
    d_scene = _load_cut(light_dir, light_scenes.SPOT_VALIDATION_XML)
    d = d_scene.desc
    assert d.integrator == nh.INTEGRATOR_DIRECT_MIS
    assert d.n_shapes == 2  # the checkerboard table and the water surface
    assert d.n_emitters == 5 and d.envmap == 4
    assert [d.emitters[i].type for i in range(5)] == [nh.EMITTER_SPOT] * 4 + [nh.EMITTER_ENVMAP]
    assert [d.emitters[i].shape for i in range(4)] == [-1] * 4
    np.testing.assert_allclose(list(d.emitter_cdf[0:6]), [k / 5 for k in range(6)], rtol=0, atol=1e-7)
    assert d.emitter_cdf[5] == 1.0
    # the hard-edged cones: falloffstart (100, 200 degrees) is past totalwidth / 2 (15, 20 degrees)
    for k, (fs, tw, pw) in enumerate([(100, 30, (0, 0, 10000)), (100, 30, (10000, 0, 0)), (100, 30, (0, 10000, 0)),
                                      (200, 40, (100000,) * 3)]):
        x = d.emitter_ext[k]
        for c in range(3):
            i, ct, cf = spot_intensity(pw[c], fs, tw)
            assert F(d.emitters[k].radiance[c]) == i
        assert F(x.cos_total_width) == ct and F(x.cos_falloff_start) == cf and cf < ct
    assert list(d.emitter_ext[0].direction) == [0.0, 0.0, -1.0]
    np.testing.assert_allclose(list(d.emitter_ext[3].direction), np.array([1, -1, -1]) / np.sqrt(3), rtol=0, atol=1e-7)
    assert d.env.constant == 1


def test_blender_validation_loads_without_its_camel(light_dir):
    s = _load_cut(light_dir, light_scenes.BLENDER_VALIDATION_XML)  # (kept alive: the desc points into it)
    d = s.desc
    assert d.integrator == nh.INTEGRATOR_DIRECT_EMS and d.n_shapes == 1
    assert d.n_emitters == 2 and d.envmap == 1 and d.env.constant == 1
    e = d.emitters[0]
    assert e.type == nh.EMITTER_DIRECTIONAL and e.shape == -1 and list(e.radiance) == [100.0, 100.0, 100.0]
    x = d.emitter_ext[0]
    assert list(x.direction) == [0.0, 0.0, -1.0] and list(x.frame_n) == [0.0, 0.0, -1.0]
    assert F(x.cos_theta_max) == cos_f(deg_to_rad(2.0))
    assert list(d.emitter_cdf[0:3]) == [0.0, 0.5, 1.0]


def _scene(tmp_path, emitters):
    return nh.Scene(light_scenes.floor_scene_xml(str(tmp_path / "s.xml"), emitters))


def test_spot_needs_its_angles(tmp_path):
    with pytest.raises(nh.NoriError, match='"falloffstart" is missing'):
        _scene(tmp_path, light_scenes.spot_xml((0, 1, 0), (0, -1, 0), (1, 1, 1), totalwidth=30))
    with pytest.raises(nh.NoriError, match='"totalwidth" is missing'):
        _scene(tmp_path, light_scenes.spot_xml((0, 1, 0), (0, -1, 0), (1, 1, 1), falloffstart=10))


def test_zero_direction_is_refused(tmp_path):
    with pytest.raises(nh.NoriError, match="direction"):
        _scene(tmp_path, light_scenes.spot_xml((0, 1, 0), (0, 0, 0), (1, 1, 1), falloffstart=10, totalwidth=30))
    with pytest.raises(nh.NoriError, match="direction"):
        _scene(tmp_path, light_scenes.directional_xml(direction=(0, 0, 0), radiance=(1, 1, 1)))


def test_directional_defaults_and_ignored_light_weight(tmp_path):
    em = light_scenes.directional_xml(light_weight=7.0) + light_scenes.spot_xml(
        (0, 1, 0), (0, -2, 0), (1, 1, 1), falloffstart=10, totalwidth=30, light_weight=3.0)
    s = _scene(tmp_path, em)
    d = s.desc
    a, b = d.emitters[0], d.emitters[1]
    assert a.type == nh.EMITTER_DIRECTIONAL and a.light_prob == 1.0  # lightWeight is never read
    assert list(a.radiance) == [0.0, 0.0, 0.0] and list(d.emitter_ext[0].direction) == [0.0, 0.0, 1.0]
    assert F(d.emitter_ext[0].cos_theta_max) == cos_f(deg_to_rad(1.0))
    assert b.type == nh.EMITTER_SPOT and b.light_prob == 3.0 and list(d.emitter_ext[1].direction) == [0.0, -1.0, 0.0]
    assert list(d.emitter_cdf[0:3]) == [0.0, 0.25, 1.0]


def test_scenes_without_the_new_lights_carry_no_side_table(scene_dir):
    s = nh.Scene(os.path.join(scene_dir, "scenes/pa4/cbox/cbox_path_mis.xml"))
    d = s.desc
    assert not bool(d.emitter_ext)
