"""The launchers' dispatch helpers (optix-renderer_amd/csrc/nh_dispatch.h) checked on the CPU: tests/c/dispatch_check
calls nh_dispatch with 1 to 5 flags in every combination of values -- the callee must run once, with constants equal
to the run-time values in argument order -- and nh_dispatch_depth with every bucket boundary of each list in use."""
import os
import re
import subprocess

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CHECK = os.path.join(REPO, "tests", "c", "bin", "dispatch_check")


def test_dispatch_helpers():
    r = subprocess.run([CHECK], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    m = re.search(r"(\d+) flag combinations, (\d+) depth values, (\d+) failures", r.stdout)
    assert m, r.stdout
    # 2 + 4 + 8 + 16 + 32 combinations; 11 depths for each of 4 lists
    assert (int(m.group(1)), int(m.group(2)), int(m.group(3))) == (62, 44, 0), r.stdout
