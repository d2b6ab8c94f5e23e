"""Regenerates tests/golden/disney_scenes.json.gz from a checkout of the reference renderer (scene data only).

    python tests/golden/make_disney_fixture.py REFERENCE_ROOT

The bundle has the form of the other *_scenes.json.gz fixtures: gzip of {relative path: file text | {"base64": ..}}.
It holds scenes/project/disney/disney-validation-blender.xml (121 Disney spheres, a cube area light, a constant
envmap, path_mis) with the two files it names: scenes/pa3/odyssey/cube.obj and scenes/project/res/photo_studio_01.png.

scenes/project/disney/disney.xml is left out: its envmap image res/rooitou_park.png alone is 1.4 MB, and this project
takes no new committed file above 1 MiB (the three older bundles above that size predate the rule).
"""
import base64
import gzip
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))

DISNEY_FILES = [
    "scenes/project/disney/disney-validation-blender.xml",
    "scenes/pa3/odyssey/cube.obj",
    "scenes/project/res/photo_studio_01.png",
]


def read_fixture(ref, rel):
    data = open(os.path.join(ref, rel), "rb").read()
    try:
        return data.decode("utf-8")
    except UnicodeDecodeError:
        return {"base64": base64.b64encode(data).decode("ascii")}


def main():
    if len(sys.argv) != 2:
        sys.exit(__doc__)
    ref = sys.argv[1]
    bundle = {p: read_fixture(ref, p) for p in DISNEY_FILES}
    out = os.path.join(HERE, "disney_scenes.json.gz")
    with open(out, "wb") as f:
        f.write(gzip.compress(json.dumps(bundle, indent=0).encode(), mtime=0))
    size = os.path.getsize(out)
    assert size < (1 << 20), f"{out}: {size} bytes, over the 1 MiB limit for a newly committed file"
    print(f"wrote {out} ({size} bytes)")


if __name__ == "__main__":
    main()
