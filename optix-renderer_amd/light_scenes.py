"""Spot / directional light scene inputs for tests and tools.

`materialize()` writes the reference's own light scenes (tests/golden/light_scenes.json.gz:
scenes/project/spotlight/{spot,spotlight-validation,blender-validation}.xml and plane_camel.obj) to a directory,
together with the meshes they share with the older bundles, in the form scenegen.materialize() writes those.
`cut_shapes()` removes the <shape> elements that load given OBJ files from a scene's text. The other functions
generate small XML scenes around one <emitter type="spot"> (src/emitters/spotlight.cpp:14-23) or
<emitter type="directional"> (src/emitters/directionalLight.cpp:32-39).
"""
from __future__ import annotations

import gzip
import json
import os
import re

_REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_GOLDEN = os.path.join(_REPO, "tests", "golden")
LIGHT_FIXTURE = os.path.join(_GOLDEN, "light_scenes.json.gz")
SPOT_XML = "scenes/project/spotlight/spot.xml"
SPOT_VALIDATION_XML = "scenes/project/spotlight/spotlight-validation.xml"
BLENDER_VALIDATION_XML = "scenes/project/spotlight/blender-validation.xml"

# meshes of the light scenes that an older bundle already carries, by the path the scenes name
SHARED_MESHES = {
    "scenes/pa1/plane.obj": "textured_scenes.json.gz",
    "scenes/project/meshes/camelhead.obj": "normalmap_scenes.json.gz",
    "scenes/project/meshes/table/plane.obj": "project_scenes.json.gz",
    "scenes/project/meshes/table/circle.obj": "project_scenes.json.gz",
}
# the heavy meshes of the two validation scenes (the three bowls, the two glasses, the camel): tests cut their shapes
HEAVY_MESHES = ("curvy_bowl.obj", "wine_glass.obj", "wine_glass_inner.obj", "camel_export_blender.obj")


def materialize(out_dir: str) -> str:
    """Write the light scene bundle and the shared meshes under out_dir; returns out_dir."""
    with gzip.open(LIGHT_FIXTURE, "rt") as f:
        files = json.load(f)
    bundles = {}
    for rel, name in SHARED_MESHES.items():
        if name not in bundles:
            with gzip.open(os.path.join(_GOLDEN, name), "rt") as f:
                bundles[name] = json.load(f)
        files[rel] = bundles[name][rel]
    for rel, text in files.items():
        p = os.path.join(out_dir, rel)
        os.makedirs(os.path.dirname(p), exist_ok=True)
        with open(p, "w") as g:
            g.write(text)
    return out_dir


def cut_shapes(xml_text: str, filenames=HEAVY_MESHES) -> str:
    """xml_text without the <shape> elements whose filename property ends in one of `filenames`."""
    def keep(m):
        fn = re.search(r'name="filename"\s+value="([^"]*)"', m.group(0))
        return "" if fn and fn.group(1).rsplit("/", 1)[-1] in filenames else m.group(0)
    return re.sub(r"<shape\b.*?</shape>", keep, xml_text, flags=re.S)


def _triple(c) -> str:
    return ", ".join(repr(float(x)) for x in c)


def spot_xml(position, direction, power, falloffstart=None, totalwidth=None, light_weight=None) -> str:
    """An <emitter type="spot">; falloffstart / totalwidth (degrees) are left out when None (the loader must refuse)."""
    out = [f'<emitter type="spot"><point name="position" value="{_triple(position)}"/>',
           f'<vector name="direction" value="{_triple(direction)}"/>',
           f'<color name="power" value="{_triple(power)}"/>']
    if falloffstart is not None:
        out.append(f'<float name="falloffstart" value="{float(falloffstart)!r}"/>')
    if totalwidth is not None:
        out.append(f'<float name="totalwidth" value="{float(totalwidth)!r}"/>')
    if light_weight is not None:
        out.append(f'<float name="lightWeight" value="{float(light_weight)!r}"/>')
    out.append("</emitter>")
    return "".join(out)


def directional_xml(direction=None, radiance=None, angle=None, light_weight=None) -> str:
    """An <emitter type="directional">; properties left at None take the reference's defaults."""
    out = ['<emitter type="directional">']
    if direction is not None:
        out.append(f'<vector name="direction" value="{_triple(direction)}"/>')
    if radiance is not None:
        out.append(f'<color name="radiance" value="{_triple(radiance)}"/>')
    if angle is not None:
        out.append(f'<float name="angle" value="{float(angle)!r}"/>')
    if light_weight is not None:
        out.append(f'<float name="lightWeight" value="{float(light_weight)!r}"/>')
    out.append("</emitter>")
    return "".join(out)


def point_xml(position, power) -> str:
    return (f'<emitter type="point"><point name="position" value="{_triple(position)}"/>'
            f'<color name="power" value="{_triple(power)}"/></emitter>')


def quad_obj(path: str, corners) -> str:
    """A quad (two triangles) through four corners given counter-clockwise about its normal."""
    os.makedirs(os.path.dirname(path) or ".", exist_ok=True)
    with open(path, "w") as f:
        for c in corners:
            f.write("v %r %r %r\n" % tuple(float(x) for x in c))
        f.write("f 1 2 3\nf 1 3 4\n")
    return path


def floor_scene_xml(path: str, emitters: str, integrator: str = "direct_ems", width: int = 32, height: int = 32,
                    spp: int = 16, half: float = 4.0, cam_height: float = 10.0, fov: float = 40.0,
                    albedo=(0.5, 0.5, 0.5), rfilter: str = "box", occluder=None) -> str:
    """A diffuse floor, the square |x|, |z| <= half of the plane y = 0 (normal +y), seen from straight above by a
    camera at (0, cam_height, 0). occluder: (cx, cy, cz, h) adds a diffuse horizontal square of half-width h centred
    there, facing up. emitters: emitter XML."""
    d = os.path.dirname(path) or "."
    base = os.path.splitext(os.path.basename(path))[0]
    quad_obj(os.path.join(d, base + "_floor.obj"), [(-half, 0, -half), (-half, 0, half), (half, 0, half), (half, 0, -half)])
    occ = ""
    if occluder is not None:
        cx, cy, cz, h = occluder
        quad_obj(os.path.join(d, base + "_occ.obj"),
                 [(cx - h, cy, cz - h), (cx - h, cy, cz + h), (cx + h, cy, cz + h), (cx + h, cy, cz - h)])
        occ = (f'<shape type="obj"><string name="filename" value="{base}_occ.obj"/>'
               '<bsdf type="diffuse"><color name="albedo" value="0.5, 0.5, 0.5"/></bsdf></shape>')
    text = f"""<scene>
<integrator type="{integrator}"/>
<sampler type="independent"><integer name="sampleCount" value="{spp}"/></sampler>
<camera type="perspective">
<transform name="toWorld"><lookat target="0, 0, 0" origin="0, {float(cam_height)!r}, 0" up="0, 0, 1"/></transform>
<float name="fov" value="{float(fov)!r}"/>
<integer name="width" value="{width}"/>
<integer name="height" value="{height}"/>
<rfilter type="{rfilter}"/>
</camera>
<shape type="obj"><string name="filename" value="{base}_floor.obj"/>
<bsdf type="diffuse"><color name="albedo" value="{_triple(albedo)}"/></bsdf></shape>
{occ}
{emitters}
</scene>
"""
    with open(path, "w") as f:
        f.write(text)
    return path
