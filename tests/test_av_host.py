"""The av and envmaptester integrators on the host (no GPU): the loader, the descriptor's side parameters, and the numpy
restatement av_refs on the reference's own test-av.xml (tests/golden/av_scenes.json, av_ttest.json)."""
import ctypes
import json
import os

import numpy as np
import pytest

import av_refs
import nori_hip as nh
import nori_oracle as no
import scenegen

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
F32 = np.float32
QUAD = "v -1 0 -1\nv 1 0 -1\nv 1 0 1\nv -1 0 1\nf 1 4 3 2\n"


@pytest.fixture(scope="module")
def av_dir(tmp_path_factory):
    return av_refs.materialize(str(tmp_path_factory.mktemp("av")))


@pytest.fixture(scope="module")
def fixture():
    with open(os.path.join(GOLDEN, "av_ttest.json")) as f:
        return json.load(f)


def write(path, text):
    with open(path, "w") as f:
        f.write(text)
    return path


def scene_xml(integrator, extra=""):
    return f"""<scene>{integrator}
  <camera type="perspective"><integer name="width" value="8"/><integer name="height" value="8"/></camera>
  <shape type="obj"><string name="filename" value="quad.obj"/><bsdf type="diffuse"/></shape>{extra}
</scene>"""


# ---- loader --------------------------------------------------------------------------------------------------------
def test_ajax_av_loads_with_stand_in_meshes(av_dir):
    for name in ("ajax.obj", "plane.obj"):
        write(os.path.join(av_dir, "scenes/pa1", name), QUAD)
    s = nh.Scene(os.path.join(av_dir, "scenes/pa1/ajax-av.xml"))
    assert s.desc.integrator == nh.INTEGRATOR_AV == 10
    assert s.av_params() == 10.0
    assert s.desc.sample_count == 1024


def test_reference_av_scenes_fail_on_their_meshes_only(tmp_path):
    d = av_refs.materialize(str(tmp_path))
    for name in ("ajax-av.xml", "sponza-av.xml"):
        with pytest.raises(nh.NoriError) as e:
            nh.Scene(os.path.join(d, "scenes/pa1", name))
        assert "is not supported" not in str(e.value) and "unable to open OBJ file" in str(e.value), str(e.value)


def test_length_is_required(tmp_path):
    write(str(tmp_path / "quad.obj"), QUAD)
    xml = write(str(tmp_path / "no_length.xml"), scene_xml('<integrator type="av"/>'))
    with pytest.raises(nh.NoriError, match='"length" is missing'):
        nh.Scene(xml)


def test_envmaptester_needs_an_envmap(tmp_path):
    write(str(tmp_path / "quad.obj"), QUAD)
    xml = write(str(tmp_path / "no_env.xml"), scene_xml('<integrator type="envmaptester"/>'))
    with pytest.raises(nh.NoriError, match="This integrator requires an env map."):
        nh.Scene(xml)
    ok = write(str(tmp_path / "env.xml"), scene_xml('<integrator type="envmaptester"/>', '<emitter type="envmap"/>'))
    s = nh.Scene(ok)
    assert s.desc.integrator == nh.INTEGRATOR_ENVMAPTESTER == 11 and s.desc.envmap >= 0
    assert s.av_params() == 0.0


def test_set_integrator_and_params_round_trip(tmp_path):
    write(str(tmp_path / "quad.obj"), QUAD)
    s = nh.Scene(write(str(tmp_path / "av.xml"),
                       scene_xml('<integrator type="av"><float name="length" value="0.25"/></integrator>')))
    assert s.av_params() == 0.25
    s.set_av_params(1.99)
    assert s.av_params() == float(F32(1.99))
    with pytest.raises(nh.NoriError):
        s.set_av_params(float("nan"))
    for integ in (nh.INTEGRATOR_ENVMAPTESTER, nh.INTEGRATOR_AV):
        s.set_integrator(integ)
        assert s.desc.integrator == integ
    with pytest.raises(nh.NoriError):
        s.set_integrator(9)
    with pytest.raises(nh.NoriError):
        s.set_integrator(12)
    assert ctypes.sizeof(nh.nh_scene_desc) == 664 and ctypes.sizeof(nh.nh_av_params) == 4
    hdr = open(os.path.join(os.path.dirname(GOLDEN), "..", "include", "nori_hip.h")).read()
    assert "NH_INTEGRATOR_AV = 10, NH_INTEGRATOR_ENVMAPTESTER = 11" in hdr
    for name in ("nh_scene_get_av_params", "nh_scene_set_av_params", "nh_set_av_params"):
        assert name in hdr and hasattr(nh._lib, name)


# ---- av_refs on the reference's test-av.xml ---------------------------------------------------------------------
def test_av_refs_scene_4_is_all_ones(av_dir):
    path = os.path.join(av_dir, "scenes/pa1/test-av.xml")
    s = nh.Scene(path, 3)
    assert s.av_params() == float(F32(1.99))
    r = av_refs.ttest_estimator(s, no.OracleScene(s), 2, 4096)
    assert r["ones"] == 4096 and r["mean"] == 1.0 and r["variance"] == 0.0


def test_av_refs_reproduces_the_fixture(av_dir, fixture):
    path = os.path.join(av_dir, "scenes/pa1/test-av.xml")
    t = nh.Test(path)
    assert t.n_scenes == 4 and t.sample_count == fixture["sample_count"]
    assert [float(r) for r in t.references] == fixture["references"]
    for i in range(3):
        s = nh.Scene(path, i)
        r = av_refs.ttest_estimator(s, no.OracleScene(s), fixture["seed"], fixture["sample_count"])
        fx = fixture["scenes"][i]
        assert r["ones"] == fx["ones"]
        assert r["mean"] == fx["mean"] == fx["ones"] / fixture["sample_count"]
        assert r["variance"] == fx["variance"]
        ok, p = nh.students_t_test(r["mean"], r["variance"], fixture["references"][i], fixture["sample_count"],
                                   t.significance_level, 4)
        assert ok and fx["accepted"] and abs(p - fx["p_value"]) < 1e-6


# ---- the rejection sampler -----------------------------------------------------------------------------------------
def test_rejection_sampler():
    n = 20000
    rng = np.random.default_rng(5)
    st = av_refs.Streams(rng.integers(0, 2 ** 63, n, dtype=np.uint64), rng.integers(0, 2 ** 62, n, dtype=np.uint64) * 2 + 1)
    pole = av_refs.normalized3(rng.standard_normal((n, 3)).astype(F32))
    d = av_refs.sample_hemisphere(st, pole, np.ones(n, bool))
    norm = np.sqrt(av_refs.dot3(d, d))
    assert np.all(np.abs(norm.astype(np.float64) - 1.0) <= float(np.spacing(F32(1))))  # within 1 ulp of 1
    assert np.all(av_refs.dot3(d, pole) >= 0)
    assert np.all(st.draws % 3 == 0) and st.draws.min() == 3 and st.draws.max() > 3
    # acceptance is the unit ball's share of the cube, pi / 6: the mean number of tries is its inverse
    assert abs(st.draws.mean() / 3 - 6 / np.pi) < 0.05
    # uniform over the hemisphere: E[d . pole] = 1 / 2
    assert abs(float(av_refs.dot3(d, pole).mean()) - 0.5) < 0.01


def test_streams_match_the_oracle_pcg32():
    st = av_refs.Streams.per_path(no, 7, [0, 5, 1234], [0, 3, 99])
    for i, (p, s) in enumerate([(0, 0), (5, 3), (1234, 99)]):
        r = no.Pcg32.per_path(7, p, s)
        assert [r.next_float() for _ in range(5)] == [float(x) for x in
                                                       av_refs.Streams(st.state[i:i + 1], st.inc[i:i + 1]).next_floats(5)]
