"""ChiSquareTest::execute restated on the oracle, for tests/test_chi2_host.py, tests/test_gpu_chi2.py and
tests/golden/make_chi2_fixture.py, in the manner of av_refs.py: the reference's operation order and number types, the
BSDF itself left to the oracle (no.chi2_histogram, no.bsdf_pdf) -- but for the Disney BSDF, which the oracle does not
have: its sample() and pdf() are the diffuse BSDF's (histogram, below).

Restated from:
  test_wi                src/utils/chi2test.cpp:151-155 (cosTheta and phi from the test's first two draws, fp32; sin and
                         cos of phi evaluated in fp64 and rounded, as nh_ttest_bsdf forms its wi)
  adaptive_simpson(_2d)  ext/hypothesis/hypothesis.h:62-102, the recursion as it is; counts the integrand's evaluations
  expected_frequencies   chi2test.cpp:186-214: the cell bounds (phi in fp32: nori's M_PI is a float, common.h:61), the
                         integrand (sin / cos in fp64, the three products rounded to fp32, the pdf widened)
  chi2_statistic         hypothesis.h:140-235 with scipy.stats.chi2 for the distribution; cells of equal expected
                         frequency in cell order (a stable sort)
  execute                chi2test.cpp:131-234: one default-state pcg32 through the whole file
  materialize            writes the small Disney and mixed (diffuse, mirror, dielectric) chi2test files
"""
from __future__ import annotations

import ctypes as C
import math
import os

import numpy as np
from scipy import stats

import nori_hip as nh
import nori_oracle as no

F32 = np.float32
M_PI_F = F32(3.14159265358979323846)
KINDS = ("accepted", "p-value", "expected frequency 0", "degrees of freedom")  # nori_hip.CHI2_*

DISNEY_XML = "chi2/chi2test-disney.xml"
MIXED_XML = "chi2/chi2test-mixed.xml"
SMALL_XML = "chi2/chi2test-microfacet-small.xml"
_HEAD = ('<?xml version="1.0" encoding="utf-8"?>\n<test type="chi2test">\n<integer name="resolution" value="3"/>\n'
         '<integer name="sampleCount" value="20000"/>\n<integer name="testCount" value="2"/>\n')
FILES = {
    DISNEY_XML: _HEAD + ('<bsdf type="disney"><float name="roughness" value="0.7"/><float name="metallic" value="0.2"/>'
                         '<color name="albedo" value="0.6, 0.4, 0.3"/></bsdf>\n'
                         '<bsdf type="disney"><float name="roughness" value="0.3"/><float name="clearcoat" value="1.0"/>'
                         '<float name="clearcoatGloss" value="0.6"/><color name="albedo" value="0.2, 0.5, 0.7"/></bsdf>\n'
                         "</test>\n"),
    MIXED_XML: _HEAD + ('<bsdf type="diffuse"><color name="albedo" value="0.5, 0.6, 0.7"/></bsdf>\n'
                        '<bsdf type="mirror"/>\n<bsdf type="dielectric"/>\n</test>\n'),
}


def materialize(out_dir: str, reference_xml: str | None = None) -> str:
    """Write the small chi2test files under out_dir; returns out_dir. reference_xml: the path of
    chi2test-microfacet.xml; its three BSDFs at resolution 3, 20000 samples and 2 tests each become SMALL_XML."""
    files = dict(FILES)
    if reference_xml:
        text = open(reference_xml).read()
        assert text.count('<test type="chi2test">') == 1
        head = _HEAD[_HEAD.index("<test"):]
        files[SMALL_XML] = text.replace('<test type="chi2test">', head)
    for rel, text in files.items():
        p = os.path.join(out_dir, rel)
        os.makedirs(os.path.dirname(p), exist_ok=True)
        with open(p, "w") as f:
            f.write(text)
    return out_dir


def test_wi(rng: "no.Pcg32") -> np.ndarray:
    cos_theta = F32(rng.next_float())
    sin_theta = F32(math.sqrt(max(F32(0), F32(1) - cos_theta * cos_theta)))  # (sqrt of an fp32: rounds once)
    phi = F32(2.0) * M_PI_F * F32(rng.next_float())
    sin_phi, cos_phi = F32(math.sin(float(phi))), F32(math.cos(float(phi)))
    return np.array([cos_phi * sin_theta, sin_phi * sin_theta, cos_theta], F32)


test_wi.__test__ = False  # (not a pytest function)


def pcg_at(draw: int) -> "no.Pcg32":
    """The default-state pcg32 after `draw` draws (pcg32::advance, ext/pcg32/pcg32.h:131-150)."""
    m = (1 << 64) - 1
    rng = no.Pcg32()
    cur_mult, cur_plus, acc_mult, acc_plus = 0x5851F42D4C957F2D, int(rng.inc.value), 1, 0
    while draw > 0:
        if draw & 1:
            acc_mult = (acc_mult * cur_mult) & m
            acc_plus = (acc_plus * cur_mult + cur_plus) & m
        cur_plus = ((cur_mult + 1) * cur_plus) & m
        cur_mult = (cur_mult * cur_mult) & m
        draw >>= 1
    return no.Pcg32((acc_mult * int(rng.state.value) + acc_plus) & m, int(rng.inc.value))


def _diffuse_stand_in() -> "nh.nh_bsdf":
    d = nh.nh_bsdf()
    d.type = nh.BSDF_DIFFUSE
    for k in range(3):
        d.albedo[k] = 1.0
    return d


def histogram(bsdf, wi, rng: "no.Pcg32", n: int, res_theta: int, res_phi: int) -> np.ndarray:
    """chi2test.cpp:163-181. The oracle's loop (no.chi2_histogram) for the BSDFs it has. It has no Disney BSDF; that
    one is restated here from disney.cpp:176-205: sample() takes the diffuse BSDF's direction (squareToCosineHemisphere)
    and pdf() its density, and returns eval() itself -- zero, so the sample skipped, where wi.z <= 0 or pdf < Epsilon.
    eval() is not restated: with a positive albedo and metallic < 1 its diffuse lobe is positive wherever pdf is."""
    if bsdf.type != nh.BSDF_DISNEY:
        return no.chi2_histogram(bsdf, wi, rng, n, res_theta, res_phi)
    assert min(bsdf.albedo[:]) > 0 and bsdf.metallic < 1
    wi = np.ascontiguousarray(wi, F32)
    d = _diffuse_stand_in()
    wo = np.zeros((n, 3), F32)
    keep = np.zeros(n, bool)
    for k in range(n):
        sx = rng.next_float()
        sy = rng.next_float()
        if wi[2] <= 0:
            continue
        wo[k], _, pdf, _ = no.bsdf_sample(d, wi, (sx, sy))
        keep[k] = not F32(pdf) < F32(1e-4)
    wo = wo[keep]
    ct = np.floor((wo[:, 2] * F32(0.5) + F32(0.5)) * F32(res_theta)).astype(np.int64)
    scaled = np.arctan2(wo[:, 1].astype(np.float64), wo[:, 0].astype(np.float64)).astype(F32) * F32(0.15915494309189533577)
    scaled = np.where(scaled < 0, scaled + F32(1), scaled).astype(F32)
    pb = np.floor(scaled * F32(res_phi)).astype(np.int64)
    cell = np.clip(ct, 0, res_theta - 1) * res_phi + np.clip(pb, 0, res_phi - 1)
    return np.bincount(cell, minlength=res_theta * res_phi).astype(np.float64)


def adaptive_simpson(f, x0, x1, eps=1e-6, depth=6):
    def integrate(a, b, c, fa, fb, fc, I, eps, depth):
        d, e = 0.5 * (a + b), 0.5 * (b + c)
        fd = f(d)
        fe = f(e)
        h = c - a
        I0 = (1.0 / 12.0) * h * (fa + 4.0 * fd + fb)
        I1 = (1.0 / 12.0) * h * (fb + 4.0 * fe + fc)
        Ip = I0 + I1
        if depth <= 0 or abs(Ip - I) < 15.0 * eps:
            return Ip + (1.0 / 15.0) * (Ip - I)
        left = integrate(a, d, b, fa, fd, fb, I0, 0.5 * eps, depth - 1)
        return left + integrate(b, e, c, fb, fe, fc, I1, 0.5 * eps, depth - 1)

    a, b, c = x0, 0.5 * (x0 + x1), x1
    fa = f(a)
    fb = f(b)
    fc = f(c)
    I = (c - a) * (1.0 / 6.0) * (fa + 4.0 * fb + fc)
    return integrate(a, b, c, fa, fb, fc, I, eps, depth)


def adaptive_simpson_2d(f, x0, y0, x1, y1, eps=1e-6, depth=6):
    return adaptive_simpson(lambda y: adaptive_simpson(lambda x: f(x, y), x0, x1, eps, depth), y0, y1, eps, depth)


def expected_frequencies(bsdf, wi, res_theta: int, res_phi: int, sample_count: int):
    """(exp, evals): the expected frequency of every cell (float64) and the pdf evaluations it took (uint32)."""
    if bsdf.type == nh.BSDF_DISNEY:  # disney.cpp:198-205: the diffuse BSDF's pdf (the oracle has no Disney BSDF)
        bsdf = _diffuse_stand_in()
    wi = np.ascontiguousarray(wi, F32)
    wo = np.zeros(3, F32)
    fp = C.POINTER(C.c_float)
    wi_p, wo_p, b_p = wi.ctypes.data_as(fp), wo.ctypes.data_as(fp), C.byref(bsdf)
    pdf = no._lib.no_bsdf_pdf
    count = [0]

    def integrand(cos_theta, phi):
        with np.errstate(invalid="ignore"):
            sin_theta = float(np.sqrt(np.float64(1 - cos_theta * cos_theta)))  # (NaN, not an exception, below zero)
        wo[0] = sin_theta * math.cos(phi)
        wo[1] = sin_theta * math.sin(phi)
        wo[2] = cos_theta
        count[0] += 1
        return float(pdf(b_p, wi_p, wo_p))

    exp = np.zeros(res_theta * res_phi, np.float64)
    evals = np.zeros(res_theta * res_phi, np.uint32)
    for i in range(res_theta):
        cos_start, cos_end = -1.0 + i * 2.0 / res_theta, -1.0 + (i + 1) * 2.0 / res_theta
        for j in range(res_phi):
            phi_start = float(F32(j * 2) * M_PI_F / F32(res_phi))
            phi_end = float(F32((j + 1) * 2) * M_PI_F / F32(res_phi))
            count[0] = 0
            integral = adaptive_simpson_2d(integrand, cos_start, phi_start, cos_end, phi_end)
            exp[i * res_phi + j] = integral * float(sample_count)
            evals[i * res_phi + j] = count[0]
    return exp, evals


def sidak(alpha: float, num_tests: int) -> float:
    return 1.0 - (1.0 - alpha) ** (1.0 / num_tests)


def chi2_statistic(obs, exp, sample_count: int, min_exp_frequency: float, alpha: float, num_tests: int) -> dict:
    """accepted, kind (an index into KINDS), p_value, statistic, dof, pooled_cells, as nh.chi2_test reports them."""
    obs, exp = np.asarray(obs, np.float64), np.asarray(exp, np.float64)
    order = np.argsort(exp, kind="stable")  # NaN last, equal values in cell order
    pooled_o = pooled_e = chsq = 0.0
    pooled = dof = 0
    nan = float("nan")
    for i in order:
        o, e = float(obs[i]), float(exp[i])
        if e == 0:
            if o > sample_count * 1e-5:
                return {"accepted": False, "kind": 2, "p_value": nan, "statistic": o, "dof": 0, "pooled_cells": pooled}
        elif e < min_exp_frequency or (pooled_e > 0 and pooled_e < min_exp_frequency):
            pooled_o += o
            pooled_e += e
            pooled += 1
        else:
            chsq += (o - e) * (o - e) / e
            dof += 1
    if pooled_e > 0 or pooled_o > 0:
        diff = pooled_o - pooled_e
        chsq += float(np.float64(diff * diff) / np.float64(pooled_e))
        dof += 1
    dof -= 1
    if dof <= 0:
        return {"accepted": False, "kind": 3, "p_value": nan, "statistic": chsq, "dof": dof, "pooled_cells": pooled}
    if math.isnan(chsq):
        pval = nan
    else:
        cdf = 0.0 if chsq < 0 else (1.0 - math.exp(-0.5 * chsq) if dof == 2 else float(stats.chi2.cdf(chsq, dof)))
        pval = 1 - cdf
    rejected = pval < sidak(alpha, num_tests) or not math.isfinite(pval)
    return {"accepted": not rejected, "kind": 1 if rejected else 0, "p_value": pval, "statistic": chsq, "dof": dof,
            "pooled_cells": pooled}


def execute(path: str) -> list:
    """One dict per test of the chi2test file: wi, obs, exp, evals and chi2_statistic's entries."""
    t = nh.Test(path)
    assert t.type == "chi2test"
    res_theta, res_phi, n = t.resolution, 2 * t.resolution, t.chi2_sample_count
    num_tests = t.test_count * len(t.bsdfs)
    rng = no.Pcg32()
    out = []
    for b in t.bsdfs:
        for _ in range(t.test_count):
            wi = test_wi(rng)
            obs = histogram(b, wi, rng, n, res_theta, res_phi)
            exp, evals = expected_frequencies(b, wi, res_theta, res_phi, n)
            r = chi2_statistic(obs, exp, n, float(t.min_exp_frequency), float(t.significance_level), num_tests)
            r.update(wi=wi, obs=obs, exp=exp, evals=evals, level=sidak(float(t.significance_level), num_tests),
                     sample_count=n)
            out.append(r)
    return out
