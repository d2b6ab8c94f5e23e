"""Regenerates tests/golden/chi2_golden.json on the CPU, with the oracle alone (no GPU, about a minute).

    python tests/golden/make_chi2_fixture.py

For scenes/pa3/tests/chi2test-microfacet.xml (from tests/golden/reference_scenes.json) and for the small Disney and
mixed (diffuse, mirror, dielectric) files of chi2_refs.FILES, chi2_refs.execute -- ChiSquareTest::execute restated on the
oracle: per test its wi, the observed counts, the expected frequencies as hex doubles, the pdf evaluations the adaptive
Simpson rule took in all, the statistic, dof, pooled cells, p-value and the verdict with its kind. Prints the figures
DESIGN.md section 7d quotes: tests accepted, the smallest p-value and the Sidak level, the evaluations per test.
"""
import json
import os
import sys
import tempfile

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, os.path.join(REPO, "optix-renderer_amd"))
sys.path.insert(0, os.path.join(REPO, "oracle"))

REFERENCE_XML = "scenes/pa3/tests/chi2test-microfacet.xml"


def record(results):
    tests = []
    for r in results:
        tests.append({"wi": [float(x).hex() for x in r["wi"]], "obs": [int(x) for x in r["obs"]],
                      "exp": [float(x).hex() for x in r["exp"]], "evals": int(r["evals"].sum()),
                      "max_cell_evals": int(r["evals"].max()), "statistic": r["statistic"], "dof": r["dof"],
                      "pooled_cells": r["pooled_cells"], "p_value": r["p_value"], "level": r["level"],
                      "accepted": bool(r["accepted"]), "kind": r["kind"], "sample_count": r["sample_count"]})
    return tests


def main():
    import chi2_refs
    import scenegen
    out = {}
    with tempfile.TemporaryDirectory() as tmp:
        scenegen.materialize(tmp)
        chi2_refs.materialize(tmp)
        for rel in (REFERENCE_XML, chi2_refs.DISNEY_XML, chi2_refs.MIXED_XML):
            tests = record(chi2_refs.execute(os.path.join(tmp, rel)))
            out[rel] = tests
            ps = [t["p_value"] for t in tests if t["kind"] in (0, 1)]
            print(f"{rel}: {sum(t['accepted'] for t in tests)}/{len(tests)} accepted, smallest p "
                  f"{min(ps) if ps else float('nan'):.4g}, level {tests[0]['level']:.3e}, evaluations per test "
                  f"{min(t['evals'] for t in tests)}..{max(t['evals'] for t in tests)}, per cell at most "
                  f"{max(t['max_cell_evals'] for t in tests)}", flush=True)
    assert all(t["accepted"] for t in out[REFERENCE_XML]) and len(out[REFERENCE_XML]) == 15
    with open(os.path.join(HERE, "chi2_golden.json"), "w") as f:
        json.dump(out, f, indent=0)
        f.write("\n")


if __name__ == "__main__":
    main()
