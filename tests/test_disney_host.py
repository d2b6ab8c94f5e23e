"""<bsdf type="disney"> through the loader and the C-ABI record (no GPU): Disney's constructor (src/bsdf/disney.cpp:22-42),
cloneAndInit's albedo fallback (:44-52) and addChild (:88-109)."""
import ctypes
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

import disney_scenes as dz
import nori_hip as nh

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DEFAULTS = (0.0, 0.0, 0.5, 0.5, 0.0, 0.0, 0.0, 0.5, 0.0, 1.0)  # disney.cpp:32-41, in nh_bsdf's order


def load_sphere(tmp_path, bsdf, name="s.xml"):
    s = nh.Scene(dz.sphere_scene_xml(str(tmp_path / name), bsdf))
    d = s.desc
    assert d.n_shapes == 1
    b = nh.nh_bsdf()  # a copy: the scene owns the record
    ctypes.memmove(ctypes.byref(b), ctypes.byref(d.bsdfs[d.shapes[0].bsdf]), ctypes.sizeof(b))
    return s, b


def params_of(b):
    return [getattr(b, n) for n in nh.DISNEY_PARAMS]


def f32(x):
    return float(np.float32(x))


def test_params_order_matches_the_header():
    hdr = open(os.path.join(REPO, "include", "nori_hip.h")).read()
    body = re.search(r"typedef struct nh_bsdf \{(.*?)\} nh_bsdf;", hdr, re.S).group(1)
    tail = body[body.index("albedo_texture"):]
    decl = re.search(r"float\s+(metallic[^;]*);", tail).group(1)
    assert tuple(x.strip() for x in decl.split(",")) == nh.DISNEY_PARAMS
    assert nh.BSDF_DISNEY == 4 and re.search(r"NH_BSDF_DISNEY = 4\b", hdr)
    assert len(dz.XML_PARAMS) == len(nh.DISNEY_PARAMS) == 10


def test_defaults_and_albedo_rules(tmp_path):
    # neither a colour nor a texture: cloneAndInit's constant 0.5
    _, b = load_sphere(tmp_path, dz.bsdf_xml())
    assert b.type == nh.BSDF_DISNEY and b.albedo_texture == 0
    assert list(b.albedo) == [0.5, 0.5, 0.5]
    assert params_of(b) == [f32(v) for v in DEFAULTS]
    # an "albedo" colour is the constant albedo
    _, b = load_sphere(tmp_path, dz.bsdf_xml(albedo=(0.25, 0.5, 0.75)))
    assert b.albedo_texture == 0 and list(b.albedo) == [0.25, 0.5, 0.75]
    # a <texture name="albedo"> child is the albedo
    s, b = load_sphere(tmp_path, dz.bsdf_xml(albedo_texture=(0.125, 0.25, 0.5)))
    d = s.desc
    assert b.albedo_texture == 1 and d.n_textures == 1
    t = d.textures[0]
    assert t.type == nh.TEXTURE_CONSTANT and list(t.value1) == [0.125, 0.25, 0.5]


def test_albedo_child_errors(tmp_path):
    """Disney::addChild's three messages (disney.cpp:88-109), as Diffuse::addChild's."""
    with pytest.raises(nh.NoriError, match="There is already an albedo defined!"):
        load_sphere(tmp_path, dz.bsdf_xml(albedo=(0.5, 0.5, 0.5), albedo_texture=(0.1, 0.1, 0.1)))
    with pytest.raises(nh.NoriError, match="There is already an albedo defined!"):
        two = ('<texture type="constant_color" name="albedo"><color name="value" value="0.1, 0.1, 0.1"/></texture>')
        load_sphere(tmp_path, dz.bsdf_xml(albedo_texture=(0.2, 0.2, 0.2), extra=two))
    with pytest.raises(nh.NoriError, match="The name of this texture does not match any field!"):
        other = '<texture type="constant_color" name="colour"><color name="value" value="0.1, 0.1, 0.1"/></texture>'
        load_sphere(tmp_path, dz.bsdf_xml(extra=other))
    with pytest.raises(nh.NoriError, match=r"Disney::addChild\(<bsdf>\) is not supported!"):
        load_sphere(tmp_path, dz.bsdf_xml(extra='<bsdf type="diffuse"/>'))


def test_clamps(tmp_path):
    """clamp(.., 0, 1) on each of the ten floats: all above, all below, and values inside kept to the bit."""
    _, b = load_sphere(tmp_path, dz.bsdf_xml({k: 1.5 + i for i, k in enumerate(dz.XML_PARAMS)}))
    assert params_of(b) == [1.0] * 10
    _, b = load_sphere(tmp_path, dz.bsdf_xml({k: -0.25 - i for i, k in enumerate(dz.XML_PARAMS)}))
    assert params_of(b) == [0.0] * 10
    inside = {k: 0.05 + 0.09 * i for i, k in enumerate(dz.XML_PARAMS)}
    _, b = load_sphere(tmp_path, dz.bsdf_xml(inside))
    assert params_of(b) == [f32(v) for v in inside.values()]
    # one out of range among defaults
    _, b = load_sphere(tmp_path, dz.bsdf_xml({"sheenTint": 7.0, "clearcoatGloss": -3.0}))
    want = [f32(v) for v in DEFAULTS]
    want[7], want[9] = 1.0, 0.0
    assert params_of(b) == want


def test_base_color_is_ignored(tmp_path):
    """The reference's scenes set "baseColor", which Disney never reads: it loads, and the albedo stays 0.5."""
    _, a = load_sphere(tmp_path, dz.bsdf_xml({"metallic": 0.3}), "a.xml")
    _, b = load_sphere(tmp_path, dz.bsdf_xml({"metallic": 0.3}, base_color=(0.9, 0.1, 0.2)), "b.xml")
    assert bytes(a) == bytes(b)
    assert list(b.albedo) == [0.5, 0.5, 0.5] and b.albedo_texture == 0


def test_validation_scene_loads(tmp_path):
    """disney-validation-blender.xml from the bundle: 121 Disney records whose parameters equal the XML's."""
    root = dz.materialize(str(tmp_path))
    path = os.path.join(root, dz.VALIDATION_XML)
    s = nh.Scene(path)
    d = s.desc
    assert (d.camera.width, d.camera.height, d.sample_count, d.integrator) == (1024, 1024, 512, nh.INTEGRATOR_PATH_MIS)
    assert d.n_shapes == 122 and d.n_emitters == 2 and d.envmap >= 0 and d.env.constant == 1
    text = open(path).read()
    blocks = re.findall(r'<bsdf type="disney">(.*?)</bsdf>', text, re.S)
    assert len(blocks) == 121
    got = [d.bsdfs[d.shapes[i].bsdf] for i in range(d.n_shapes) if d.shapes[i].type == nh.SHAPE_SPHERE]
    assert len(got) == 121 and all(b.type == nh.BSDF_DISNEY for b in got)
    assert sum(d.bsdfs[i].type == nh.BSDF_DISNEY for i in range(d.n_bsdfs)) == 121
    xml_of = dict(zip(dz.XML_PARAMS, nh.DISNEY_PARAMS))
    for blk, b in zip(blocks, got):
        want = dict(zip(nh.DISNEY_PARAMS, DEFAULTS))
        for k, v in re.findall(r'<float name="(\w+)" value="([^"]+)"/>', blk):
            want[xml_of[k]] = min(max(f32(v), 0.0), 1.0)
        assert params_of(b) == [f32(want[n]) for n in nh.DISNEY_PARAMS]
        # the albedo is a constant_color texture child (its filename property is never read)
        col = [f32(x) for x in re.search(r'<color name="value" value="([^"]+)"/>', blk).group(1).split(",")]
        assert b.albedo_texture >= 1 and list(d.textures[b.albedo_texture - 1].value1) == col
    # the cube area light keeps its diffuse BSDF: the scene mixes two BSDF classes
    assert {d.bsdfs[d.shapes[i].bsdf].type for i in range(d.n_shapes)} == {nh.BSDF_DIFFUSE, nh.BSDF_DISNEY}


def test_ctypes_record_matches_the_c_struct(tmp_path):
    cc = shutil.which("cc") or shutil.which("gcc")
    assert cc, "no C compiler"
    src = tmp_path / "size.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "nori_hip.h"\n'
                   'int main(void) { printf("%zu %zu %zu\\n", sizeof(nh_bsdf), offsetof(nh_bsdf, albedo_texture), '
                   'offsetof(nh_bsdf, metallic)); return 0; }\n')
    exe = tmp_path / "size"
    subprocess.run([cc, "-std=c99", "-I", os.path.join(REPO, "include"), "-o", str(exe), str(src)], check=True)
    size, off_tex, off_met = map(int, subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.split())
    assert ctypes.sizeof(nh.nh_bsdf) == size
    assert nh.nh_bsdf.albedo_texture.offset == off_tex and nh.nh_bsdf.metallic.offset == off_met
    assert off_met == off_tex + 4  # appended after albedo_texture
