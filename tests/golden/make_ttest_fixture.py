"""Regenerates tests/golden/ttest_seed2.json from the CPU oracle alone (no GPU, about a minute).

    python tests/golden/make_ttest_fixture.py

For every <scene> of the reference's five scene t-test files (tests/golden/reference_scenes.json) it runs the estimator
of nh_ttest_scene on the oracle: sample k < sampleCount is OracleScene.path(seed = 2, pixel (0, 0), sample k) -- on these
1x1 cameras the test's pixelSample (a * 1.0f, b * 1.0f) is the pixel jitter itself -- reduced to Color3f::getLuminance
in fp32, then to the math.fsum two-pass mean and unbiased variance. Stored per file: the references, per scene the mean,
the variance and the two-sided p-value of scipy's Student t (what tests/test_gpu_ttest.py predicts the verdicts from).
"""
import ctypes as C
import json
import math
import os
import sys
import tempfile

import numpy as np
from scipy import stats

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, os.path.join(REPO, "optix-renderer_amd"))
sys.path.insert(0, os.path.join(REPO, "oracle"))

FILES = ["pa4/tests/test-furnace.xml", "pa4/tests/test-direct.xml", "pa3/tests/test-mesh.xml",
         "pa3/tests/test-mesh-furnace.xml", "pa1/test-direct.xml"]
SEED = 2


def oracle_luminance(oracle, seed: int, n: int, first: int = 0) -> np.ndarray:
    """getLuminance (fp32, the reference's operation order) of OracleScene.path(seed, 0, 0, k), first <= k < first + n."""
    import nori_oracle as no
    rgb = np.zeros((n, 3), np.float32)
    jit = np.zeros(2, np.float32)
    fp = C.POINTER(C.c_float)
    jp = jit.ctypes.data_as(fp)
    base = rgb.ctypes.data
    for k in range(n):
        no._lib.no_path_radiance(oracle._h, seed, 0, 0, first + k, C.cast(base + 12 * k, fp), jp)
    return rgb[:, 0] * np.float32(0.212671) + rgb[:, 1] * np.float32(0.715160) + rgb[:, 2] * np.float32(0.072169)


def two_pass(lum: np.ndarray):
    x = [float(v) for v in lum]
    mean = math.fsum(x) / len(x)
    return mean, math.fsum((v - mean) * (v - mean) for v in x) / (len(x) - 1)


def main():
    import nori_hip as nh
    import nori_oracle as no
    import scenegen
    out = {"seed": SEED, "files": {}}
    with tempfile.TemporaryDirectory() as tmp:
        scenegen.materialize(tmp)
        for name in FILES:
            path = os.path.join(tmp, "scenes", name)
            t = nh.Test(path)
            n = t.sample_count
            scenes = []
            for i in range(t.n_scenes):
                s = nh.Scene(path, i)
                mean, var = two_pass(oracle_luminance(no.OracleScene(s), SEED, n))
                tstat = abs(mean - float(t.references[i])) * math.sqrt(n / max(var, 1e-5))
                scenes.append({"mean": mean, "variance": var, "p_value": 2.0 * float(stats.t.sf(tstat, n - 1))})
                print(name, i, scenes[-1], flush=True)
            out["files"][name] = {"sample_count": n, "references": [float(r) for r in t.references], "scenes": scenes}
    with open(os.path.join(HERE, "ttest_seed2.json"), "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
