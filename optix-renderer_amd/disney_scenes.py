"""Disney-BSDF scene inputs for tests and tools.

`materialize()` writes the reference's own Disney scene (tests/golden/disney_scenes.json.gz:
scenes/project/disney/disney-validation-blender.xml with its mesh and image) to a directory, in the form
scenegen.materialize() writes the other bundles. The other functions generate small XML scenes around one
`<bsdf type="disney">` (src/bsdf/disney.cpp:22-42).
"""
from __future__ import annotations

import base64
import gzip
import json
import os

_REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DISNEY_FIXTURE = os.path.join(_REPO, "tests", "golden", "disney_scenes.json.gz")
VALIDATION_XML = "scenes/project/disney/disney-validation-blender.xml"

# the XML property names in nh_bsdf's field order (nori_hip.DISNEY_PARAMS)
XML_PARAMS = ("metallic", "subsurface", "specular", "roughness", "specularTint", "anisotropic", "sheen", "sheenTint",
              "clearcoat", "clearcoatGloss")


def materialize(out_dir: str) -> str:
    """Write the Disney scene bundle under out_dir; returns out_dir."""
    with gzip.open(DISNEY_FIXTURE, "rt") as f:
        files = json.load(f)
    for rel, text in files.items():
        p = os.path.join(out_dir, rel)
        os.makedirs(os.path.dirname(p), exist_ok=True)
        if isinstance(text, dict):  # binary file (a PNG)
            with open(p, "wb") as g:
                g.write(base64.b64decode(text["base64"]))
        else:
            with open(p, "w") as g:
                g.write(text)
    return out_dir


def _triple(c) -> str:
    return ", ".join(repr(float(x)) for x in c)


def bsdf_xml(params: dict | None = None, albedo=None, albedo_texture=None, base_color=None, extra: str = "") -> str:
    """A <bsdf type="disney">. params: XML property name -> value (written as given, unclamped); albedo: an "albedo"
    colour property; albedo_texture: the colour of a <texture type="constant_color" name="albedo"> child;
    base_color: a "baseColor" colour property (the reference's scenes set it; Disney never reads it); extra: further
    child XML."""
    out = ['<bsdf type="disney">']
    for k, v in (params or {}).items():
        out.append(f'<float name="{k}" value="{float(v)!r}"/>')
    if albedo is not None:
        out.append(f'<color name="albedo" value="{_triple(albedo)}"/>')
    if base_color is not None:
        out.append(f'<color name="baseColor" value="{_triple(base_color)}"/>')
    if albedo_texture is not None:
        out.append(f'<texture type="constant_color" name="albedo"><color name="value" value="{_triple(albedo_texture)}"/>'
                   '</texture>')
    out.append(extra)
    out.append("</bsdf>")
    return "\n".join(out)


def sphere_scene_xml(path: str, bsdf: str, integrator: str = "path_mis", width: int = 32, height: int = 32,
                     spp: int = 8, fov: float = 40.0, distance: float = 4.0, emitters: str = "",
                     rfilter: str = "", extra_shapes: str = "") -> str:
    """A unit sphere at the origin with the given <bsdf>, seen from (0, 0, distance) along -z. emitters /
    extra_shapes: XML added to the scene; rfilter: a reconstruction filter type (default: the camera's gaussian)."""
    rf = f'<rfilter type="{rfilter}"/>' if rfilter else ""
    text = f"""<scene>
<integrator type="{integrator}"/>
<sampler type="independent"><integer name="sampleCount" value="{spp}"/></sampler>
<camera type="perspective">
<transform name="toWorld"><lookat target="0, 0, 0" origin="0, 0, {float(distance)!r}" up="0, 1, 0"/></transform>
<float name="fov" value="{float(fov)!r}"/>
<integer name="width" value="{width}"/>
<integer name="height" value="{height}"/>
{rf}
</camera>
<shape type="sphere">
<point name="center" value="0, 0, 0"/>
<float name="radius" value="1"/>
{bsdf}
</shape>
{extra_shapes}
{emitters}
</scene>
"""
    os.makedirs(os.path.dirname(path) or ".", exist_ok=True)
    with open(path, "w") as f:
        f.write(text)
    return path


def constant_envmap_xml(color) -> str:
    return ('<emitter type="envmap"><texture type="constant_color" name="albedo">'
            f'<color name="value" value="{_triple(color)}"/></texture></emitter>')


def point_light_xml(position, power) -> str:
    return (f'<emitter type="point"><point name="position" value="{_triple(position)}"/>'
            f'<color name="power" value="{_triple(power)}"/></emitter>')
