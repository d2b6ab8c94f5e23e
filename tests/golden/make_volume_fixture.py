"""Regenerates tests/golden/volume_scenes.json.gz and tests/golden/volume_mc.json.

    python tests/golden/make_volume_fixture.py REFERENCE_ROOT

volume_scenes.json.gz has the form of the other *_scenes.json.gz fixtures: gzip of {relative path: file text}. It holds
the reference's homogeneous-media scenes (scene data only) -- scenes/project/volume/{cbox_homog, cbox_homog_ambient,
cbox_homog_aniso, cbox_homog_caustic, cbox_homog_dielectric_medium, cbox_val_mats, cbox_val_mis, homog_test}.xml,
scenes/pa4/cbox/cbox_path_vol_{mats,mis}.xml, scenes/project/optix/sphere-analytic.xml -- the Cornell box meshes the
project scenes name (scenes/project/meshes/cbox/*.obj) and, for the loader's refusal, one volume-light scene with its
plane (scenes/project/volume-emission/volumelight-test-mats.xml, plane.obj). The pa4 scenes' meshes are in
reference_scenes.json; cube.obj and plane.obj of scenes/project/meshes are reused from normalmap_scenes.json.gz
(volume_refs.SHARED_MESHES).

volume_mc.json: for every Monte-Carlo scene of volume_refs.mc_scenes() and both integrators, the seed, N, mean luminance
and standard error of the fp64 restatement of the reference's integrator (volume_refs.estimate), as written ("quirks")
and with the free-path density and scattering coefficient applied ("textbook"). The power conditions the GPU test
relies on are checked here: wherever the two variants differ in expectation they must lie more than 8 combined standard
errors apart, and scene (a) under path_vol_mis must be such a scene.
"""
import gzip
import json
import math
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(HERE)), "optix-renderer_amd"))

import volume_refs as vr  # noqa: E402

MESHES = ["scenes/project/meshes/cbox/%s.obj" % n for n in ("walls", "leftwall", "rightwall", "light")]
EXTRA = [vr.EMISSION_SCENE, "scenes/project/volume-emission/plane.obj"]
N_PATHS = 1 << 20
MIN_SEPARATION = 8.0


def main():
    if len(sys.argv) != 2:
        sys.exit(__doc__)
    ref = sys.argv[1]
    bundle = {p: open(os.path.join(ref, p), "rb").read().decode("utf-8") for p in vr.VOLUME_SCENES + MESHES + EXTRA}
    with open(vr.VOLUME_FIXTURE, "wb") as f:
        f.write(gzip.compress(json.dumps(bundle, indent=0).encode(), mtime=0))
    size = os.path.getsize(vr.VOLUME_FIXTURE)
    assert size < (1 << 20), f"{vr.VOLUME_FIXTURE}: {size} bytes, over the 1 MiB limit for a committed file"
    print(f"wrote {vr.VOLUME_FIXTURE} ({size} bytes)")

    mc = {}
    seed = 1000
    for name, scene in vr.mc_scenes().items():
        for integ, mis in (("path_vol_mats", False), ("path_vol_mis", True)):
            on = vr.estimate(scene, N_PATHS, seed, mis, quirks=True)
            off = vr.estimate(scene, N_PATHS, seed + 1, mis, quirks=False)
            seed += 2
            sep = abs(on["mean"] - off["mean"]) / math.sqrt(on["stderr"] ** 2 + off["stderr"] ** 2)
            mc[f"{name}/{integ}"] = {"quirks": on, "textbook": off, "separation": sep}
            print(f"{name} {integ}: quirks {on['mean']:.5f} +- {on['stderr']:.5f}, textbook {off['mean']:.5f} +- "
                  f"{off['stderr']:.5f}, {sep:.1f} combined standard errors apart")
            assert sep > MIN_SEPARATION, (name, integ, sep)
    with open(vr.MC_FIXTURE, "w") as f:
        json.dump(mc, f, indent=1, sort_keys=True)
        f.write("\n")
    print(f"wrote {vr.MC_FIXTURE}")


if __name__ == "__main__":
    main()
