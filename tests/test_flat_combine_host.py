"""The combine step of the flat two-leaf traversal (optix-renderer_amd/csrc/nh_flat_combine.h) checked on the CPU:
tests/c/flat_combine_check runs the host build against the walk written out -- first leaf, the deferred child's
re-test, second leaf, every candidate accepted in order -- over found / not found per leaf, the second leaf's t below,
at and above the first's, its record index below and above, the deferred child's entry distance below, at and above the
first hit, both visit orders, one box missed, and any-hit."""
import os
import re
import subprocess

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CHECK = os.path.join(REPO, "tests", "c", "bin", "flat_combine_check")


def test_flat_combine():
    r = subprocess.run([CHECK], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    m = re.search(r"flat_combine_check: (\d+) cases OK", r.stdout)
    # 5^4 candidate sets x 5^2 entry distances x 4 box outcomes x (2 visit orders + any-hit)
    assert m and int(m.group(1)) == 625 * 25 * 4 * 3, r.stdout
