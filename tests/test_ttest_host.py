"""The host side of the reference's t-test procedure (src/utils/ttest.cpp) on the HIP path, CPU only: the <test>
loader (nh_test_load_xml), hypothesis::students_t_test restated (nh_students_t_test) and the exported symbols."""
import ctypes as C
import math
import os

import numpy as np
import pytest
from scipy import stats

import nori_hip as nh
import scenegen
from test_oracle_kat import reference_verdicts

SCENE_TESTS = [("pa4/tests/test-furnace.xml", 4), ("pa4/tests/test-direct.xml", 10), ("pa3/tests/test-mesh.xml", 15),
               ("pa3/tests/test-mesh-furnace.xml", 6), ("pa1/test-direct.xml", 4)]
ANGLES_ERR = "Specified a different number of angles and reference values!"
BOTH_ERR = "Cannot test BSDFs and scenes at the same time!"
SCENES_ERR = "Specified a different number of scenes and reference values!"
CHILD_ERR = "StudentsTTest::addChild(<%s>) is not supported!"


@pytest.mark.parametrize("name,count", SCENE_TESTS)
def test_loader_scene_tests(scene_dir, name, count):
    path = os.path.join(scene_dir, "scenes", name)
    t = nh.Test(path)
    assert t.type == "ttest"
    assert t.n_scenes == count and not t.bsdfs
    # no `angles` here: tokenize("") is one empty token, which the reference's toFloat reads as 0 (common.cpp:105-112)
    assert t.angles == [np.float32(0)]
    refs = scenegen.test_references(path)
    assert len(refs) == count
    assert t.references == [np.float32(r) for r in refs]
    # none of the files sets them: the constructor's defaults (ttest.cpp:65, :78)
    assert t.significance_level == np.float32(0.01) and t.sample_count == 100000
    # the scenes themselves still load one by one, as before
    assert nh.Scene(path, count - 1).width == 1
    with pytest.raises(nh.NoriError):
        nh.Scene(path, count)


def test_loader_bsdf_test(scene_dir):
    t = nh.Test(os.path.join(scene_dir, "scenes/pa3/tests/ttest-microfacet.xml"))
    assert t.type == "ttest" and t.n_scenes == 0
    assert t.angles == [np.float32(a) for a in (0, 45, 60, 80, 85)]
    assert t.references == [np.float32(r) for r in (0.207067, 0.215733, 0.247884, 0.430936, 0.519016)]
    assert t.significance_level == np.float32(0.01) and t.sample_count == 100000
    assert len(t.bsdfs) == 1
    b = t.bsdfs[0]
    assert b.type == nh.BSDF_MICROFACET
    assert (np.float32(b.alpha), np.float32(b.int_ior), np.float32(b.ext_ior)) == \
        (np.float32(0.1), np.float32(1.5), np.float32(1.000277))
    assert [np.float32(x) for x in b.kd] == [np.float32(x) for x in (0.1, 0.2, 0.15)]
    assert np.float32(b.ks) == np.float32(1) - np.float32(0.2)


def test_loader_chi2test(scene_dir):
    t = nh.Test(os.path.join(scene_dir, "scenes/pa3/tests/chi2test-microfacet.xml"))
    assert t.type == "chi2test"
    assert len(t.bsdfs) == 3 and t.n_scenes == 0
    assert [np.float32(b.alpha) for b in t.bsdfs] == [np.float32(a) for a in (0.1, 0.3, 0.6)]
    assert t.significance_level == np.float32(0.01) and t.sample_count == -1  # chi2test.cpp:48, :63


def test_loader_properties_are_read(scene_dir, tmp_path):
    text = open(os.path.join(scene_dir, "scenes/pa3/tests/ttest-microfacet.xml")).read()
    text = text.replace('<bsdf type="microfacet">', '<float name="significanceLevel" value="0.05"/>\n'
                        '<integer name="sampleCount" value="1234"/>\n<bsdf type="microfacet">')
    p = tmp_path / "props.xml"
    p.write_text(text)
    t = nh.Test(str(p))
    assert t.significance_level == np.float32(0.05) and t.sample_count == 1234


def test_loader_errors(scene_dir, tmp_path):
    micro = open(os.path.join(scene_dir, "scenes/pa3/tests/ttest-microfacet.xml")).read()
    furnace_path = os.path.join(scene_dir, "scenes/pa4/tests/test-furnace.xml")
    furnace = open(furnace_path).read()

    def load(text, where=tmp_path):
        p = os.path.join(str(where), "edited.xml")
        open(p, "w").write(text)
        return nh.Test(p)

    assert "       80,       85" in micro
    with pytest.raises(nh.NoriError) as e:
        load(micro.replace("       80,       85", "       80"))
    assert ANGLES_ERR in str(e.value)
    with pytest.raises(nh.NoriError) as e:
        load(micro.replace("</test>", "<scene></scene>\n</test>"))
    assert BOTH_ERR in str(e.value)
    # (the edited furnace copies sit next to the original: their scenes name meshes relative to the file)
    head = furnace.index('<string name="references"')
    tail = furnace.index("/>", head) + 2
    with pytest.raises(nh.NoriError) as e:
        load(furnace[:head] + '<string name="references" value="2, 5, 2"/>' + furnace[tail:], os.path.dirname(furnace_path))
    assert SCENES_ERR in str(e.value)
    for tag, cls in (("camera", "ECamera"), ("integrator", "EIntegrator"), ("shape", "EShape")):
        with pytest.raises(nh.NoriError) as e:
            load(furnace.replace("</test>", f'<{tag} type="x"/>\n</test>'), os.path.dirname(furnace_path))
        assert CHILD_ERR % cls in str(e.value)
    # a <scene> root is no test (the CLI tells the two apart by this status)
    h = C.c_void_p()
    cbox = os.path.join(scene_dir, "scenes/pa4/cbox/cbox_path_mis.xml")
    assert nh.lib.nh_test_load_xml(cbox.encode(), C.byref(h)) == 1  # NH_ERR_INVALID


# ---------------------------------------------------------------------------------------
def t_grid():
    """(mean, variance, reference, n, alpha, num_tests): t from 0 to far in the tail, few and many degrees of freedom,
    variances under the 1e-5 floor."""
    out = []
    for n in (2, 3, 10, 101, 4096, 100000, 1 << 24):
        for var in (1e-7, 0.04, 1.0, 37.5):
            for z in (0.0, 1e-3, 0.3, 1.0, 1.9, 2.6, 3.3, 4.2, 6.0, 12.0, 40.0):
                se = math.sqrt(max(var, 1e-5) / n)
                for alpha, k in ((0.01, 1), (0.01, 15), (0.05, 4)):
                    out.append((2.0 + z * se, var, 2.0, n, alpha, k))
    return out


def test_students_t_p_values_match_scipy():
    worst = 0.0
    for mean, var, ref, n, alpha, k in t_grid():
        ok, p = nh.students_t_test(mean, var, ref, n, alpha, k)
        t = abs(mean - ref) * math.sqrt(n / max(var, 1e-5))
        want = 2.0 * stats.t.sf(t, n - 1)
        worst = max(worst, abs(p - want))
        assert abs(p - want) <= 1e-9, (mean, var, n, p, want)
        level = 1.0 - (1.0 - alpha) ** (1.0 / k)
        if abs(want - level) > 1e-8:  # (not on the verdict's edge)
            assert ok == (not want < level), (mean, var, n, alpha, k, p, want)
    print(f"largest |p - scipy| over the grid: {worst:.3e}")


def test_students_t_verdicts_match_reference(tmp_path):
    grid = t_grid()
    theirs = reference_verdicts([("t", m, v, r, n, a, k) for m, v, r, n, a, k in grid], tmp_path)
    mine = [nh.students_t_test(*g)[0] for g in grid]
    assert any(mine) and not all(mine)
    if theirs is not None:  # (only where the reference checkout is present, as test_oracle_kat's verdict checks)
        assert mine == theirs, [g for g, a, b in zip(grid, mine, theirs) if a != b][:5]


def test_students_t_rejects_non_finite():
    for mean, var in ((float("nan"), 1.0), (float("inf"), 1.0), (2.0, float("nan"))):
        ok, p = nh.students_t_test(mean, var, 2.0, 1000, 0.01, 1)
        assert not ok, (mean, var, p)
    ok, p = nh.students_t_test(2.0, 1.0, 2.0, 1000, 0.01, 1)
    assert ok and p == 1.0
    with pytest.raises(nh.NoriError):
        nh.students_t_test(2.0, 1.0, 2.0, 1, 0.01, 1)
    with pytest.raises(nh.NoriError):
        nh.students_t_test(2.0, 1.0, 2.0, 10, 0.01, 0)


def test_symbols_exported():
    host = ("nh_test_load_xml", "nh_test_get_desc", "nh_test_free", "nh_students_t_test")
    device = ("nh_radiance_query", "nh_ttest_scene", "nh_ttest_bsdf", "nh_test_run")
    lib_dir = os.path.dirname(nh.LIB_PATH)
    host_lib = C.CDLL(os.path.join(lib_dir, "libnori_host.so"))
    for s in host:
        assert hasattr(host_lib, s), s
    for s in device:
        assert not hasattr(host_lib, s), s  # the host library needs no GPU runtime
    for s in host + device:
        assert hasattr(nh.lib, s), s
