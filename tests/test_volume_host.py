"""Participating media on the host: the loader (media records, phases, BSDF-less shapes, the ambient medium, the
refusals), the C-ABI layout of the appended fields, and the fp64 Monte-Carlo restatement of the volumetric integrators
(volume_refs) validated against the oracle's path_mats / path_mis with every medium a vacuum."""
import ctypes
import json
import math
import os
import shutil
import subprocess

import numpy as np
import pytest

import nori_hip as nh
import nori_oracle as no
import volume_refs as vr
from emitter_refs import F64, luminance

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def vol_dir(tmp_path_factory):
    return vr.materialize(str(tmp_path_factory.mktemp("vol")))


def shape_bsdfs(d):
    return [d.shapes[i].bsdf for i in range(d.n_shapes)]


@pytest.mark.parametrize("rel", vr.VOLUME_SCENES)
def test_reference_scene_loads(vol_dir, rel):
    s = nh.Scene(os.path.join(vol_dir, rel))
    d = s.desc
    want = nh.INTEGRATOR_PATH_VOL_MIS if 'type="path_vol_mis"' in open(os.path.join(vol_dir, rel)).read() \
        else nh.INTEGRATOR_PATH_VOL_MATS
    assert d.integrator == want
    # a shape has no BSDF only when it has a medium
    for i, (b, m) in enumerate(zip(shape_bsdfs(d), s.shape_media())):
        assert b >= -1 and (b >= 0 or m >= 0), (i, b, m)
    nh.Bvh(s)  # the builder takes BSDF-less shapes


def test_media_records(vol_dir):
    base = os.path.join(vol_dir, "scenes/project/volume")
    s = nh.Scene(os.path.join(base, "cbox_homog.xml"))
    (m,) = s.media()
    want = vr.fold_medium()  # sigma_a 0.5, sigma_s 0, intensities 1, density 1
    assert m["type"] == nh.MEDIUM_HOMOG and m["phase"] == nh.PHASE_ISO and m["g"] == 0 and m["density"] == 1
    for k in ("mu_a", "mu_s", "mu_t"):
        np.testing.assert_array_equal(m[k], want[k])
    assert list(m["mu_t"]) == [0.5, 0.5, 0.5] and list(m["mu_s"]) == [0, 0, 0]
    assert s.ambient_medium == -1 and s.shape_media() == [0, -1, -1, -1, -1, -1]
    assert shape_bsdfs(s.desc)[0] == -1 and all(b >= 0 for b in shape_bsdfs(s.desc)[1:])  # the medium-only sphere

    a = nh.Scene(os.path.join(base, "cbox_homog_aniso.xml"))
    (m,) = a.media()
    assert m["phase"] == nh.PHASE_HG and m["g"] == np.float32(-0.75)

    amb = nh.Scene(os.path.join(base, "cbox_homog_ambient.xml"))
    assert amb.ambient_medium == 0 and amb.shape_media()[0] == 1
    np.testing.assert_array_equal(amb.media()[0]["mu_t"], vr.fold_medium(sigma_a=(0.05, 0.05, 0.05))["mu_t"])

    die = nh.Scene(os.path.join(base, "cbox_homog_dielectric_medium.xml"))
    d = die.desc
    both = [i for i, (b, m) in enumerate(zip(shape_bsdfs(d), die.shape_media())) if b >= 0 and m >= 0]
    assert len(both) == 1 and d.bsdfs[d.shapes[both[0]].bsdf].type == nh.BSDF_DIELECTRIC
    assert shape_bsdfs(d)[0] == -1 and die.shape_media()[0] == 0


SCENE = """<scene><integrator type="path_vol_mats"/><camera type="perspective"/>{ambient}
<shape type="sphere"><emitter type="area"><color name="radiance" value="1, 1, 1"/></emitter>{media}</shape></scene>"""


def load_text(tmp_path, text):
    p = tmp_path / "scene.xml"
    p.write_text(text)
    return nh.Scene(str(p))


def test_explicit_fold_bit_for_bit(tmp_path):
    kw = dict(sigma_a=(0.3, 0.7, 0.11), sigma_s=(0.9, 0.013, 0.57), sigma_a_intensity=1.7, sigma_s_intensity=0.3,
              density=2.3)
    xml = ('<medium type="homog"><color name="sigma_a" value="0.3, 0.7, 0.11"/><color name="sigma_s" '
           'value="0.9, 0.013, 0.57"/><float name="sigma_a_intensity" value="1.7"/><float name="sigma_s_intensity" '
           'value="0.3"/><float name="density" value="2.3"/><phase type="anisophase"><float name="g" value="0.4"/>'
           '</phase></medium>')
    s = load_text(tmp_path, SCENE.format(ambient="", media=xml))
    (m,) = s.media()
    want = vr.fold_medium(**kw)
    for k in ("mu_a", "mu_s", "mu_t"):
        np.testing.assert_array_equal(m[k], want[k])
    assert m["density"] == np.float32(2.3) and m["phase"] == nh.PHASE_HG and m["g"] == np.float32(0.4)
    assert shape_bsdfs(s.desc) == [-1]
    # a vacuum medium is a medium too: the shape gets no default BSDF; no medium at all: the default diffuse
    assert shape_bsdfs(load_text(tmp_path, SCENE.format(ambient="", media='<medium type="vacuum"/>')).desc) == [-1]
    assert shape_bsdfs(load_text(tmp_path, SCENE.format(ambient="", media="")).desc) == [0]


HOMOG = '<medium type="homog"/>'


@pytest.mark.parametrize("ambient,media,message", [
    ("", '<medium type="heterog"/>', 'medium "heterog"'),
    ("", '<medium type="homog"><phase type="schlick"/></medium>', 'phase function "schlick" is not supported'),
    ("", '<medium type="homog"><emitter type="volumelight"/></medium>', "a medium's <emitter>"),
    ("", HOMOG + HOMOG, "Shape: tried to register multiple Medium instances."),
    (HOMOG + HOMOG, "", "There can only be one ambient medium per scene."),
    ("", '<medium type="homog"><phase type="isophase"/><phase type="isophase"/></medium>',
     "Medium: tried to register multiple PhaseFunction instances!"),
    ("", '<medium type="homog"><bsdf type="diffuse"/></medium>', "Medium::addChild(<bsdf>) is not supported!"),
])
def test_refusals(tmp_path, ambient, media, message):
    with pytest.raises(nh.NoriError) as e:
        load_text(tmp_path, SCENE.format(ambient=ambient, media=media))
    assert message in str(e.value)


def test_volume_emission_scene_is_refused(vol_dir):
    with pytest.raises(nh.NoriError, match="a medium's <emitter>"):
        nh.Scene(os.path.join(vol_dir, vr.EMISSION_SCENE))


def test_set_integrator_accepts_the_volumetric_ones(vol_dir):
    s = nh.Scene(os.path.join(vol_dir, "scenes/pa4/cbox/cbox_path_mis.xml"))
    for integ in (nh.INTEGRATOR_PATH_VOL_MATS, nh.INTEGRATOR_PATH_VOL_MIS):
        s.set_integrator(integ)
        assert s.desc.integrator == integ
    with pytest.raises(nh.NoriError):
        s.set_integrator(9)
    d = s.desc  # a scene without media: the appended fields are the zero tail
    assert d.n_media == 0 and not d.media and not d.shape_medium and d.ambient_medium == 0


def test_ctypes_records_match_the_c_structs(tmp_path):
    cc = shutil.which("cc") or shutil.which("gcc")
    assert cc, "no C compiler"
    fields_m = ["type", "mu_a", "mu_s", "mu_t", "density", "phase", "g"]
    fields_d = ["emitter_ext", "n_media", "media", "shape_medium", "ambient_medium"]
    fmt = " ".join(["%zu"] * (2 + len(fields_m) + len(fields_d)))
    args = ["sizeof(nh_medium)", "sizeof(nh_scene_desc)"] + [f"offsetof(nh_medium, {f})" for f in fields_m] + \
        [f"offsetof(nh_scene_desc, {f})" for f in fields_d]
    src = tmp_path / "size.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "nori_hip.h"\n'
                   f'int main(void) {{ printf("{fmt}\\n", {", ".join(args)}); return 0; }}\n')
    exe = tmp_path / "size"
    subprocess.run([cc, "-std=c99", "-I", os.path.join(REPO, "include"), "-o", str(exe), str(src)], check=True)
    out = list(map(int, subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.split()))
    assert ctypes.sizeof(nh.nh_medium) == out[0] and ctypes.sizeof(nh.nh_scene_desc) == out[1]
    assert [getattr(nh.nh_medium, f).offset for f in fields_m] == out[2:2 + len(fields_m)]
    assert [getattr(nh.nh_scene_desc, f).offset for f in fields_d] == out[2 + len(fields_m):]
    # appended: the media fields come after everything the older clients fill
    assert out[2 + len(fields_m)] < out[3 + len(fields_m)] < out[-1]


def test_students_t_cdf():
    # tabulated two-sided critical values: P(|T| > t) = 0.05
    for dof, t in ((1, 12.706), (7, 2.365), (30, 2.042), (1000, 1.962)):
        assert abs(2 * (1 - vr.students_t_cdf(t, dof)) - 0.05) < 2e-4
    assert vr.students_t_cdf(0.0, 5) == 0.5 and abs(vr.students_t_cdf(-2.0, 7) + vr.students_t_cdf(2.0, 7) - 1) < 1e-12


def test_mc_fixture_matches_the_scenes():
    with open(vr.MC_FIXTURE) as f:
        mc = json.load(f)
    assert sorted(mc) == sorted(f"{c}/{i}" for c in vr.mc_scenes() for i in ("path_vol_mats", "path_vol_mis"))
    for key, rec in mc.items():
        assert rec["separation"] > 8.0, key
    # the fixture is what the restatement gives today: one scene re-estimated with fewer paths
    S = vr.mc_scenes()["a_iso"]
    est = vr.estimate(S, 1 << 16, 77, True)
    ref = mc["a_iso/path_vol_mis"]["quirks"]
    assert abs(est["mean"] - ref["mean"]) < 5 * math.hypot(est["stderr"], ref["stderr"])


def oracle_estimate(xml_path, k_seeds=8, spp=64):
    s = nh.Scene(xml_path)
    o = no.OracleScene(s)
    vals = []
    for k in range(k_seeds):
        rgb = nh.to_rgb(o.render(0, spp, seed=vr.render_seed(200, k)), s.border).astype(np.float64).reshape(-1, 3)
        vals.append(float(luminance(rgb, F64).mean()))
    return vr.seeds_estimate(vals)


@pytest.mark.parametrize("integrator,mis", [("path_mats", False), ("path_mis", True)])
@pytest.mark.parametrize("view", ["a", "floor"])
def test_restatement_against_the_oracle(tmp_path, view, integrator, mis):
    """With every medium a vacuum the restatement must agree with the oracle's path_mats / path_mis (the reference's
    t-test, 4 comparisons): on scene (a)'s geometry, where the camera sees the light through the now empty sphere, and
    on a view of a diffuse floor lit by a sphere light (volume_refs.floor_scene), where paths bounce. The oracle's integrators dereference every
    shape's BSDF, so its scene leaves the BSDF-less sphere out: with a vacuum inside, it is a pass-through."""
    if view == "a":
        S = vr.mc_scenes()["a_iso"].vacuum_copy()
    else:
        S = vr.floor_scene(vr.medium(kind="vacuum"))
    solid = vr.SphereScene([s for s in S.spheres if s["bsdf"] is not None], [], None, S.origin, S.direction)
    p = tmp_path / "oracle.xml"
    p.write_text(vr.scene_xml(solid, integrator, 32, 64))
    mean, se, dof = oracle_estimate(str(p))
    est = vr.estimate(S, 1 << 18, 5, mis)
    res = vr.t_test(mean, se, dof, est["mean"], est["stderr"], 4)
    print(f"{view} {integrator}: oracle {mean:.5f} +- {se:.5f}, restatement {est['mean']:.5f} +- {est['stderr']:.5f}: "
          f"t = {res['t']:.2f}, p = {res['pval']:.3g}")
    assert mean > 0.05 and res["pass"], res
