"""Regenerates tests/golden/adaptive_scenes.json.gz from a checkout of the reference renderer (scene data only).

    python tests/golden/make_adaptive_fixture.py REFERENCE_ROOT

The bundle has the form of the other *_scenes.json.gz fixtures: gzip of {relative path: file text | {"base64": ..}}.
It holds the reference's two scenes that use <sampler type="adaptive">, as they are:
scenes/project/disney/disney_sphere.xml and scenes/project/disney/disney-test.xml.

The files they name are stand-ins, each under its own name, because the real ones cannot be committed:
  scenes/project/meshes/camelhead2.obj   1.9 MB in the reference; stand-in: the reference's scenes/project/meshes/cube.obj
  scenes/project/res/rooitou_park.png    1.4 MB in the reference; stand-in: the reference's res/envmap-test.png
  scenes/project/res/small_cave_2k.hdr   not in the reference checkout at all; stand-in: a 16x8 flat-encoded Radiance
                                         picture of a vertical gradient, generated here
This project takes no new committed file above 1 MiB.
"""
import base64
import gzip
import json
import os
import struct
import sys

HERE = os.path.dirname(os.path.abspath(__file__))

SCENES = ["scenes/project/disney/disney_sphere.xml", "scenes/project/disney/disney-test.xml"]
STAND_INS = {
    "scenes/project/meshes/camelhead2.obj": "scenes/project/meshes/cube.obj",
    "scenes/project/res/rooitou_park.png": "scenes/project/res/envmap-test.png",
}
HDR_NAME = "scenes/project/res/small_cave_2k.hdr"


def encode(data: bytes):
    try:
        return data.decode("utf-8")
    except UnicodeDecodeError:
        return {"base64": base64.b64encode(data).decode("ascii")}


def gradient_hdr(width=16, height=8) -> bytes:
    """A flat (uncompressed) RGBE picture: rows from bright (top) to dim."""
    out = b"#?RADIANCE\nFORMAT=32-bit_rle_rgbe\n\n" + f"-Y {height} +X {width}\n".encode()
    for y in range(height):
        m = 255 - 24 * y
        for x in range(width):
            out += struct.pack("4B", m, max(m - 8 * x, 1), 128, 129)
    return out


def main():
    if len(sys.argv) != 2:
        sys.exit(__doc__)
    ref = sys.argv[1]
    bundle = {p: encode(open(os.path.join(ref, p), "rb").read()) for p in SCENES}
    for name, src in STAND_INS.items():
        bundle[name] = encode(open(os.path.join(ref, src), "rb").read())
    bundle[HDR_NAME] = encode(gradient_hdr())
    out = os.path.join(HERE, "adaptive_scenes.json.gz")
    with open(out, "wb") as f:
        f.write(gzip.compress(json.dumps(bundle, indent=0).encode(), mtime=0))
    size = os.path.getsize(out)
    assert size < (1 << 20), f"{out}: {size} bytes, over the 1 MiB limit for a newly committed file"
    print(f"wrote {out} ({size} bytes)")


if __name__ == "__main__":
    main()
