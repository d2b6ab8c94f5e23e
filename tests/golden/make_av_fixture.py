"""Regenerates tests/golden/av_scenes.json and tests/golden/av_ttest.json on the CPU (no GPU, under a minute).

    python tests/golden/make_av_fixture.py [reference checkout]

av_scenes.json: {relative path: text} of the reference's av files -- scenes/pa1/test-av.xml with its disk.obj, and
ajax-av.xml / sponza-av.xml (their meshes are not shipped: the loader test only checks what they fail on). This is the
only thing here that reads the reference checkout.

av_ttest.json: for each of the four <scene>s of test-av.xml, av_refs.ttest_estimator -- the estimator of nh_ttest_scene
over the numpy restatement av_refs.av_paths (pixelSample = (a W, b H), sampleCount samples on the streams
path_rng(seed, 0, k)): the count of ones, the mean, the unbiased variance, and the two-sided p-value of scipy's Student t.

Seed: 2, like ttest_seed2.json, if the restatement accepts all four scenes there; otherwise the smallest seed >= 2 at
which it does. The seed found is 2 (recorded in the fixture).
"""
import json
import math
import os
import sys

from scipy import stats

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, os.path.join(REPO, "optix-renderer_amd"))
sys.path.insert(0, os.path.join(REPO, "oracle"))

FILES = ["scenes/pa1/test-av.xml", "scenes/pa1/disk.obj", "scenes/pa1/ajax-av.xml", "scenes/pa1/sponza-av.xml"]
FIRST_SEED = 2


def run_seed(path: str, seed: int):
    import av_refs
    import nori_hip as nh
    import nori_oracle as no
    t = nh.Test(path)
    n = t.sample_count
    scenes = []
    for i in range(t.n_scenes):
        s = nh.Scene(path, i)
        r = av_refs.ttest_estimator(s, no.OracleScene(s), seed, n)
        ref = float(t.references[i])
        accepted, p_host = nh.students_t_test(r["mean"], r["variance"], ref, n, t.significance_level, len(t.references))
        tstat = abs(r["mean"] - ref) * math.sqrt(n / max(r["variance"], 1e-5))
        scenes.append({"ones": r["ones"], "mean": r["mean"], "variance": r["variance"],
                       "p_value": 2.0 * float(stats.t.sf(tstat, n - 1)), "accepted": bool(accepted)})
        print(seed, i, scenes[-1], flush=True)
    return {"seed": seed, "sample_count": n, "references": [float(r) for r in t.references], "scenes": scenes}


def main():
    import tempfile

    import av_refs
    ref_root = sys.argv[1] if len(sys.argv) > 1 else "/root/reference"
    files = {}
    for rel in FILES:
        with open(os.path.join(ref_root, rel)) as f:
            files[rel] = f.read()
    with open(os.path.join(HERE, "av_scenes.json"), "w") as f:
        json.dump(files, f, indent=0)
        f.write("\n")
    with tempfile.TemporaryDirectory() as tmp:
        av_refs.materialize(tmp)
        path = os.path.join(tmp, "scenes/pa1/test-av.xml")
        seed = FIRST_SEED
        while True:
            out = run_seed(path, seed)
            if all(s["accepted"] for s in out["scenes"]):
                break
            seed += 1
    with open(os.path.join(HERE, "av_ttest.json"), "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
