"""Writes tests/golden/photon_mc.json: samples of the photon mapper's estimator (one photon map and one camera path
each) from the fp64 Monte-Carlo restatement photon_refs.photon_mc on the sphere scenes photon_refs.mc_scenes(), with
fixed numpy seeds. The two-light scene is also sampled with quirks=False (the true light selection probability in
place of `* lights.size()`): tests/test_photon_host.py checks that the t-test tells the two apart.

    python tests/golden/make_photon_fixture.py
"""
import json
import os
import sys

REPO = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.join(REPO, "optix-renderer_amd"))
sys.path.insert(0, os.path.join(REPO, "oracle"))

import photon_refs as pr  # noqa: E402

N_SAMPLES = 256
SEEDS = {"one": 101, "two": 102, "glass": 103}

if __name__ == "__main__":
    out = {"photon_count": pr.MC_PHOTONS, "radius": pr.MC_RADIUS, "n_samples": N_SAMPLES, "scenes": {}}
    for name, (S, weights) in pr.mc_scenes().items():
        rec = {"weights": weights, "quirks": pr.photon_mc(S, weights, pr.MC_PHOTONS, pr.MC_RADIUS, N_SAMPLES, SEEDS[name])}
        if len(weights) > 1:
            rec["no_quirks"] = pr.photon_mc(S, weights, pr.MC_PHOTONS, pr.MC_RADIUS, N_SAMPLES, SEEDS[name] + 1000,
                                            quirks=False)
        out["scenes"][name] = rec
        print(name, {k: (sum(v["luminance"]) / N_SAMPLES, v["mean_photons_in_ball"]) for k, v in rec.items() if k != "weights"})
    with open(pr.PHOTON_MC_FIXTURE, "w") as f:
        json.dump(out, f, indent=0)
