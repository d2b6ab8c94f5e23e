"""The host side of the reference's warp test (src/utils/warptest.cpp, runTest) on the HIP path, CPU only: the exported
symbols, the slider maps (nh_warp_map_parameter, nh_warp_wi) against warp_refs bit for bit, the restatement's own
consistency (its pdfs integrate to 1 where they are densities; its vectorised pcg32 equals the oracle's), the fixture
generator, and the refusals, which every nh_warp_* entry point issues before it touches a device."""
import ctypes as C
import json
import os
import sys

import numpy as np
import pytest

import chi2_refs
import nori_hip as nh
import warp_refs as wr

F32 = np.float32
GOLDEN_DIR = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
NH_ERR_INVALID, NH_ERR_UNSUPPORTED = 1, 4


def test_symbols_exported():
    host = ("nh_warp_map_parameter", "nh_warp_wi")
    device = ("nh_warp_query", "nh_warp_histogram", "nh_warp_expected", "nh_warp_run")
    host_lib = C.CDLL(os.path.join(os.path.dirname(nh.LIB_PATH), "libnori_host.so"))
    for s in host:
        assert hasattr(host_lib, s), s
    for s in device:
        assert not hasattr(host_lib, s), s  # the host library needs no GPU runtime
    for s in host + device:
        assert hasattr(nh.lib, s), s
    assert [getattr(nh, n) for n in ("WARP_NONE", "WARP_DISK", "WARP_UNIFORM_SPHERE", "WARP_UNIFORM_SPHERE_VOL",
                                     "WARP_UNIFORM_SPHERE_CAP", "WARP_UNIFORM_HEMISPHERE", "WARP_COSINE_HEMISPHERE",
                                     "WARP_BECKMANN", "WARP_HENYEY_GREENSTEIN", "WARP_SCHLICK", "WARP_MICROFACET_BRDF",
                                     "WARP_ISO_PHASE", "WARP_ANISO_PHASE")] == list(range(13))  # WarpTest::WarpType
    assert len(nh.WARP_NAMES) == 13 and nh.WARP_SUPPORTED == wr.SUPPORTED


def sliders():
    return [0.0, 0.25, 0.5, 1.0] + [float(x) for x in np.random.default_rng(3).random(64, dtype=np.float32)]


def test_helpers_equal_restatement():
    for s in sliders():
        for t in wr.SUPPORTED:
            got, want = F32(nh.warp_map_parameter(t, s)), wr.map_parameter(t, s)
            assert got.view(np.uint32) == want.view(np.uint32), (t, s, got, want)
        np.testing.assert_array_equal(nh.warp_wi(s).view(np.uint32), wr.wi(s).view(np.uint32), err_msg=str(s))
    # the ends of the maps: alpha from 0.05 to 1, g from -1 to 1, the cap's cosThetaMax the raw slider
    assert nh.warp_map_parameter(nh.WARP_BECKMANN, 0.0) == pytest.approx(0.05, rel=1e-6)
    assert nh.warp_map_parameter(nh.WARP_MICROFACET_BRDF, 1.0) == 1.0
    assert (nh.warp_map_parameter(nh.WARP_ANISO_PHASE, 0.0), nh.warp_map_parameter(nh.WARP_HENYEY_GREENSTEIN, 1.0)) == (-1, 1)
    assert nh.warp_map_parameter(nh.WARP_UNIFORM_SPHERE_CAP, 0.25) == 0.25
    # the angle slider's ends are grazing: cos clamps at 1e-4 before the normalization
    assert 0 < nh.warp_wi(0.0)[2] < 2e-4 and nh.warp_wi(0.0)[0] < -0.99 and nh.warp_wi(0.5)[2] == 1.0


def test_vectorised_pcg_equals_the_oracle():
    for first in (0, 7, 2 ** 33 + 1):
        rng = chi2_refs.pcg_at(first)
        want = np.array([rng.next_float() for _ in range(300)], F32)
        np.testing.assert_array_equal(wr.draws(first, 300).view(np.uint32), want.view(np.uint32))
    p = wr.points(5, 4, rtl=True)
    np.testing.assert_array_equal(p[:, ::-1], wr.points(5, 4, rtl=False))
    np.testing.assert_array_equal(p[1], wr.draws(8, 3)[::-1])


def midpoint_integral(t, par, w, n=400):
    """The integral of the restatement's pdf over its domain by a plain midpoint rule on runTest's parametrisation."""
    u = (np.arange(n) + 0.5) / n
    if t in (wr.NONE, wr.DISK):
        x, y = np.meshgrid(u, u)
        if t == wr.DISK:
            x, y = 2 * x - 1, 2 * y - 1
        v = np.stack([x.ravel(), y.ravel(), np.zeros(n * n)], -1).astype(F32)
        area = 1.0 if t == wr.NONE else 4.0
    else:
        phi, z = np.meshgrid(2 * np.pi * (np.arange(2 * n) + 0.5) / (2 * n), 2 * u - 1)
        s = np.sqrt(1 - z * z)
        v = np.stack([(s * np.cos(phi)).ravel(), (s * np.sin(phi)).ravel(), z.ravel()], -1).astype(F32)
        area = 4 * np.pi
    return float(wr.pdf(t, par, v, np.float64, w).mean() * area)


def test_restated_pdfs_integrate_to_one():
    w = wr.wi(0.7)
    cases = [(wr.NONE, 0.5), (wr.DISK, 0.5), (wr.UNIFORM_SPHERE, 0.5), (wr.UNIFORM_HEMISPHERE, 0.5),
             (wr.COSINE_HEMISPHERE, 0.5), (wr.BECKMANN, 0.3), (wr.BECKMANN, 1.0), (wr.HENYEY_GREENSTEIN, 0.3),
             (wr.HENYEY_GREENSTEIN, -0.6), (wr.ISO_PHASE, 0.0), (wr.ANISO_PHASE, 0.5)]
    for t, par in cases:
        got = midpoint_integral(t, par, w)
        print(f"type {t}, parameter {par}: {got:.6f}")
        assert abs(got - 1) < 1e-3, (t, par, got)
    # the BRDF's pdf loses what reflects below the horizon: at normal incidence and alpha = 0.3 that is the Beckmann
    # mass beyond 45 degrees, exp(-1 / 0.09) ~ 1.5e-5
    got = midpoint_integral(wr.MICROFACET_BRDF, 0.3, wr.wi(0.5))
    print(f"microfacet BRDF, alpha 0.3, normal incidence: {got:.6f}")
    assert abs(got - 1) < 1e-3, got
    # The sphere volume's pdf is no density over the sphere's surface, where runTest integrates it: the constant
    # 4/3 pi as written (warp.cpp:94-97) gives (4/3 pi) (4 pi), not 1 -- and its points lie inside the ball, not on it.
    vol = midpoint_integral(wr.UNIFORM_SPHERE_VOL, 0.5, w)
    assert abs(vol - (4 / 3 * np.pi) * 4 * np.pi) < 1e-3 and abs(vol - 1) > 1
    # The sphere cap's pdf as written (warp.cpp:68-72) is 0 on the unit sphere at or below the rim and the cap's uniform
    # density everywhere else -- off the sphere included. Over runTest's unit vectors that is the cap's density: it
    # integrates to 1 here; what it is not is a density over R^3.
    cap = midpoint_integral(wr.UNIFORM_SPHERE_CAP, 0.5, w)
    print(f"sphere cap, cosThetaMax 0.5: {cap:.6f}")
    assert abs(cap - 1) < 1e-3
    off = wr.pdf(wr.UNIFORM_SPHERE_CAP, 0.5, np.array([[0.0, 0.0, -2.0]], F32), F32)[0]
    assert off == wr.pdf(wr.UNIFORM_SPHERE_CAP, 0.5, np.array([[0.0, 0.0, 1.0]], F32), F32)[0] > 0


def test_generator_reproduces_itself(tmp_path):
    sys.path.insert(0, GOLDEN_DIR)
    try:
        import make_warp_fixture as gen
    finally:
        sys.path.remove(GOLDEN_DIR)
    a, b = gen.build(yres=4, xres=8), gen.build(yres=4, xres=8)
    assert json.dumps(a, sort_keys=True) == json.dumps(b, sort_keys=True)
    assert sorted(a["runs"]) == sorted(nh.WARP_NAMES[t] for t in wr.SUPPORTED)
    for name, r in a["runs"].items():
        assert r["obs_sum"] + r["skipped"] == r["sample_count"] == 1000 * 32 and r["nan_points"] == 0, name
    with open(os.path.join(GOLDEN_DIR, "warp_runs.json")) as f:
        committed = json.load(f)
    assert sorted(committed["runs"]) == sorted(a["runs"])
    for name, r in committed["runs"].items():  # the committed fixture is at the reference's own table
        t = nh.WARP_NAMES.index(name)
        assert (r["yres"], r["xres"], r["sample_count"]) == wr.default_table(t), name
        assert r["nan_points"] == 0 and len(r["cells"]) == 16, name
        assert F32(float.fromhex(r["parameter"])) == wr.map_parameter(t, r["parameter_slider"]), name


def refused(call, code, text):
    assert call() == code
    assert text in nh.lib.nh_host_last_error().decode(), nh.lib.nh_host_last_error()


def test_refusals():
    """Every check comes before the context is used, so a null context shows them."""
    obs, exp = (C.c_double * 16)(), (C.c_double * 16)()
    buf, nan = (C.c_float * 16)(), C.c_uint32(0)
    lib = nh.lib

    def hist(t, par=0.5, n=10, xres=2, yres=2):
        return lambda: lib.nh_warp_histogram(None, t, par, None, 0, nh.LENS_DRAWS_RTL, n, xres, yres, obs, C.byref(nan))

    def expd(t, par=0.5, xres=2, yres=2):
        return lambda: lib.nh_warp_expected(None, t, par, None, xres, yres, 100, exp, None)

    def query(t, par=0.5):
        return lambda: lib.nh_warp_query(None, t, par, None, nh.WARP_QUERY_SAMPLE, 1, buf, buf)

    for t in (-1, 13):
        for call in (hist(t), expd(t), query(t)):
            refused(call, NH_ERR_INVALID, "unknown warp type")
        v = C.c_float(0)
        refused(lambda: lib.nh_warp_map_parameter(t, 0.5, C.byref(v)), NH_ERR_INVALID, "unknown warp type")
    for call in (hist(nh.WARP_SCHLICK), expd(nh.WARP_SCHLICK), query(nh.WARP_SCHLICK)):
        refused(call, NH_ERR_UNSUPPORTED, "NH_WARP_SCHLICK")
    for bad in (float("nan"), float("inf"), -float("inf")):
        for call in (hist(nh.WARP_BECKMANN, bad), expd(nh.WARP_BECKMANN, bad), query(nh.WARP_BECKMANN, bad)):
            refused(call, NH_ERR_INVALID, "finite")
    for xres, yres in ((0, 4), (4, 0), (-1, -1), (64, 129), (8193, 1)):
        refused(hist(nh.WARP_DISK, xres=xres, yres=yres), NH_ERR_UNSUPPORTED, "at most 8192 cells")
        refused(expd(nh.WARP_DISK, xres=xres, yres=yres), NH_ERR_UNSUPPORTED, "at most 8192 cells")
    for n in (0, -3):
        refused(hist(nh.WARP_DISK, n=n), NH_ERR_INVALID, "n >= 1")
    refused(query(nh.WARP_MICROFACET_BRDF), NH_ERR_INVALID, "needs wi")
    # valid arguments reach the context check
    refused(hist(nh.WARP_DISK), NH_ERR_INVALID, "null context")
    # the runner refuses before it creates a context
    with pytest.raises(nh.NoriError, match="NH_WARP_SCHLICK"):
        nh.run_warp_test(nh.WARP_SCHLICK)
    with pytest.raises(nh.NoriError, match="unknown warp type"):
        nh.run_warp_test(13)
    with pytest.raises(nh.NoriError, match="at most 8192 cells"):
        nh.run_warp_test(nh.WARP_DISK, xres=0, yres=4, sample_count=100)
    with pytest.raises(nh.NoriError, match="at most 8192 cells"):
        nh.run_warp_test(nh.WARP_DISK, xres=128, yres=128, sample_count=100)
    with pytest.raises(nh.NoriError, match="finite"):
        nh.run_warp_test(nh.WARP_BECKMANN, parameter_slider=float("nan"))
    with pytest.raises(nh.NoriError, match="sample_count >= 1"):
        nh.run_warp_test(nh.WARP_DISK, xres=4, yres=4, sample_count=0)
