"""Regenerates tests/golden/light_scenes.json.gz from a checkout of the reference renderer (scene data only).

    python tests/golden/make_light_fixture.py REFERENCE_ROOT

The bundle has the form of the other *_scenes.json.gz fixtures: gzip of {relative path: file text}. It holds the
reference's three spot / directional light scenes, scenes/project/spotlight/{spot,spotlight-validation,
blender-validation}.xml, and the one mesh they name that no other bundle carries, scenes/project/meshes/plane_camel.obj.

The other meshes the tests load are reused by path from the older bundles (light_scenes.SHARED_MESHES):
scenes/pa1/plane.obj (textured_scenes), scenes/project/meshes/camelhead.obj (normalmap_scenes) and
scenes/project/meshes/table/{plane,circle}.obj (project_scenes). Left out: camel_export_blender.obj (several MB); the
tests cut the shapes that name it, and the bowls and glasses of spotlight-validation.xml, out of the XML text.
"""
import gzip
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))

LIGHT_FILES = [
    "scenes/project/spotlight/spot.xml",
    "scenes/project/spotlight/spotlight-validation.xml",
    "scenes/project/spotlight/blender-validation.xml",
    "scenes/project/meshes/plane_camel.obj",
]


def main():
    if len(sys.argv) != 2:
        sys.exit(__doc__)
    ref = sys.argv[1]
    bundle = {p: open(os.path.join(ref, p), "rb").read().decode("utf-8") for p in LIGHT_FILES}
    out = os.path.join(HERE, "light_scenes.json.gz")
    with open(out, "wb") as f:
        f.write(gzip.compress(json.dumps(bundle, indent=0).encode(), mtime=0))
    size = os.path.getsize(out)
    assert size < (1 << 20), f"{out}: {size} bytes, over the 1 MiB limit for a newly committed file"
    print(f"wrote {out} ({size} bytes)")


if __name__ == "__main__":
    main()
