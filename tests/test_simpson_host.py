"""The iterative adaptive Simpson rule of the chi^2 test's expected frequencies (optix-renderer_amd/csrc/nh_simpson.h)
checked on the CPU: tests/c/simpson_check runs the host build against the recursion of hypothesis::adaptiveSimpson
written out -- a cubic (one leaf), a narrow Gaussian, an integrand that drives every branch to the depth limit, a step,
the zero function, NaN-returning integrands (which must terminate), every depth from -1 to 6, a reversed interval and
the nested 2-D form. Results are bit-identical and the evaluation counts equal."""
import os
import re
import subprocess

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CHECK = os.path.join(REPO, "tests", "c", "bin", "simpson_check")


def test_simpson_matches_recursion():
    r = subprocess.run([CHECK], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "simpson_check: all cases OK" in r.stdout and "MISMATCH" not in r.stdout, r.stdout
    lines = {m.group(1): (int(m.group(2)), int(m.group(3)))
             for m in re.finditer(r"^(.+?): \S+ OK, (\d+) evaluations, (\d+) leaves$", r.stdout, re.M)}
    # a leaf-only run evaluates 3 + 2 points; the full tree 3 + 2 (2^7 - 1): every frame of 7 levels adds two
    assert lines["cubic"] == (5, 1) and lines["zero"] == (5, 1)
    assert lines["nan"] == (3 + 2 * 127, 64) and lines["rough"] == (3 + 2 * 127, 64)
    assert lines["depth -1"] == (5, 1) and lines["depth 0"] == (5, 1) and lines["depth 3"] == (3 + 2 * 15, 8)
    assert lines["gaussian"] == (3 + 2 * 127, 64)
    assert 1 < lines["step"][1] < 64 and 1 < lines["narrow"][1] < 64  # refined where the integrand moves only
    assert len(re.findall(r"^2d .*OK", r.stdout, re.M)) == 4, r.stdout
