"""WarpTest::runTest restated in numpy, for tests/test_warp_host.py, tests/test_gpu_warp.py and
tests/golden/make_warp_fixture.py, in the manner of emitter_refs.py / volume_refs.py / chi2_refs.py: every warp and pdf
takes the float type T its arithmetic runs in -- F32 is the reference's precision, with transcendentals evaluated in
fp64 and rounded once, F64 the reference value -- and keeps the reference's operation order. Inputs are float32 values
in both runs; M_PI, INV_PI, INV_TWOPI and Epsilon are Nori's float constants.

Restated from:
  map_parameter, wi          src/utils/warptest.cpp:88-100, :183-184
  sample (warpPoint)         warptest.cpp:102-131 over src/utils/warp.cpp:41-205, src/bsdf/microfacet.cpp:60-148,
                             src/utils/common.cpp:308-337 (fresnel), include/nori/frame.h:82-87 (tanTheta),
                             src/bsdf/isophase.cpp, anisophase.cpp
  pdf                        the *Pdf functions of warp.cpp, Microfacet::pdf, the phases' pdf
  draws, points              ext/pcg32/pcg32.h (nextUInt, nextFloat, advance), vectorised: the state after k draws is an
                             affine map of the state, so a block of states doubles in one multiply-add;
                             warptest.cpp:152 with the argument order of g++ (rtl) or clang
  cells, histogram           warptest.cpp:457-479
  expected                   warptest.cpp:481-551 with chi2_refs.adaptive_simpson_2d (hypothesis.h:62-102)
  execute                    warptest.cpp:439-562 with chi2_refs.chi2_statistic (hypothesis.h:140-235)

A point with a NaN coordinate is not binned (the reference's (int) cast of a NaN is undefined) but counted apart, as
nh_warp_histogram does. Schlick is not restated: the HIP path refuses it.
"""
from __future__ import annotations

import hashlib
import math

import numpy as np

import chi2_refs
from emitter_refs import F32, F64, _fn, dot, eps, normalized, pi, uniform_sphere
from volume_refs import hg_pdf, hg_sample

(NONE, DISK, UNIFORM_SPHERE, UNIFORM_SPHERE_VOL, UNIFORM_SPHERE_CAP, UNIFORM_HEMISPHERE, COSINE_HEMISPHERE, BECKMANN,
 HENYEY_GREENSTEIN, SCHLICK, MICROFACET_BRDF, ISO_PHASE, ANISO_PHASE) = range(13)  # nori_hip.WARP_*
SUPPORTED = tuple(t for t in range(13) if t != SCHLICK)
HAS_WI = (MICROFACET_BRDF, ISO_PHASE, ANISO_PHASE)
INT_IOR, EXT_IOR = 1.5046, 1.000277  # microfacet.cpp:38-41


def inv_pi(T):
    return T(F32(0.31830988618379067154))


# ---- the sliders ------------------------------------------------------------------------------------------------------
def map_parameter(type: int, slider) -> np.float32:
    v = F32(slider)
    if type in (BECKMANN, MICROFACET_BRDF):
        e = F32(math.log(float(F32(0.05)))) * (F32(1) - v) + F32(math.log(1.0)) * v
        return F32(math.exp(float(e)))
    if type in (HENYEY_GREENSTEIN, ANISO_PHASE):
        return F32(2) * v - F32(1)
    return v


def wi(angle_slider) -> np.ndarray:
    angle = pi(F32) * (F32(angle_slider) - F32(0.5))
    v = np.array([F32(math.sin(float(angle))), F32(0), max(F32(math.cos(float(angle))), F32(1e-4))], F32)
    n = v[0] * v[0] + (v[1] * v[1] + v[2] * v[2])
    return (v / np.sqrt(n)).astype(F32) if n > 0 else v


def default_table(type: int):
    """(yres, xres, sample_count) of runTest itself."""
    yres, xres = 51, 51 if type in (NONE, DISK) else 102
    return yres, xres, 1000 * yres * xres


# ---- pcg32, vectorised ------------------------------------------------------------------------------------------------
_M64 = (1 << 64) - 1
_MULT, _STATE0, _INC = 0x5851F42D4C957F2D, 0x853C49E6748FEA9B, 0xDA3E39CB94B95BDB


def _advance(delta: int):
    """pcg32::advance as an affine map: (mult, plus) with state' = mult * state + plus."""
    cur_mult, cur_plus, acc_mult, acc_plus = _MULT, _INC, 1, 0
    while delta > 0:
        if delta & 1:
            acc_mult = (acc_mult * cur_mult) & _M64
            acc_plus = (acc_plus * cur_mult + cur_plus) & _M64
        cur_plus = ((cur_mult + 1) * cur_plus) & _M64
        cur_mult = (cur_mult * cur_mult) & _M64
        delta >>= 1
    return acc_mult, acc_plus


def draws(first: int, count: int) -> np.ndarray:
    """nextFloat() number first .. first + count - 1 of the default-state pcg32, float32."""
    m, p = _advance(first)
    st = np.empty(count, np.uint64)
    if count == 0:
        return st.astype(F32)
    st[0] = (m * _STATE0 + p) & _M64
    filled = 1
    while filled < count:
        k = min(filled, count - filled)
        am, ap = _advance(filled)
        st[filled:filled + k] = st[:k] * np.uint64(am) + np.uint64(ap)  # (wraps modulo 2^64)
        filled += k
    xs = (((st >> np.uint64(18)) ^ st) >> np.uint64(27)).astype(np.uint32)
    rot = (st >> np.uint64(59)).astype(np.uint32)
    u = (xs >> rot) | (xs << ((~rot + np.uint32(1)) & np.uint32(31)))
    return ((u >> np.uint32(9)) | np.uint32(0x3F800000)).view(F32) - F32(1)


def points(first_draw: int, n: int, rtl: bool = True) -> np.ndarray:
    """The n samples Point3f(nextFloat(), nextFloat(), nextFloat()) from draw first_draw, (n, 3) float32."""
    d = draws(first_draw, 3 * n).reshape(n, 3)
    return np.ascontiguousarray(d[:, ::-1]) if rtl else d


# ---- the warps --------------------------------------------------------------------------------------------------------
def _disk(s, T):
    rho = np.sqrt(s[:, 0])
    theta = s[:, 1] * T(2) * pi(T)
    return rho * _fn(np.cos, T, theta), rho * _fn(np.sin, T, theta)


def _cosine_hemisphere(s, T):
    x, y = _disk(s, T)
    with np.errstate(invalid="ignore"):
        return np.stack([x, y, np.sqrt(T(1) - (x * x + y * y))], -1)


def _beckmann(s, alpha, T):
    with np.errstate(divide="ignore"):
        ls = _fn(np.log, T, T(1) - s[:, 0])
    ls = np.where(np.isinf(ls), T(0), ls)
    tan2 = -alpha * alpha * ls
    phi = s[:, 1] * T(2) * pi(T)
    ct = T(1) / np.sqrt(T(1) + tan2)
    with np.errstate(invalid="ignore"):
        st = np.sqrt(T(1) - ct * ct)
    r = np.stack([st * _fn(np.cos, T, phi), st * _fn(np.sin, T, phi), ct], -1)
    return np.where((r[:, 2] < 0)[:, None], -r, r)


def _tan_theta(v, T):
    temp = T(1) - v[:, 2] * v[:, 2]
    with np.errstate(invalid="ignore", divide="ignore"):
        return np.where(temp <= 0, T(0), np.sqrt(np.abs(temp)) / v[:, 2])


def _beckmann_d(m, alpha, T):
    temp, ct2 = _tan_theta(m, T) / alpha, m[:, 2] * m[:, 2]
    with np.errstate(invalid="ignore", divide="ignore", over="ignore", under="ignore"):
        return _fn(np.exp, T, -temp * temp) / (pi(T) * alpha * alpha * ct2 * ct2)


def _smith_g1(v, m, alpha, T):
    tt = _tan_theta(v, T)
    with np.errstate(invalid="ignore", divide="ignore", over="ignore"):
        a = T(1) / (alpha * tt)
        a2 = a * a
        r = (T(F32(3.535)) * a + T(F32(2.181)) * a2) / (T(1) + T(F32(2.276)) * a + T(F32(2.577)) * a2)
    return np.where(tt == 0, T(1), np.where(dot(m, v) * v[:, 2] <= 0, T(0), np.where(a >= T(F32(1.6)), T(1), r)))


def _fresnel(cos_i, ext_ior, int_ior, T):
    eta_i, eta_t = np.full(cos_i.shape, ext_ior, T), np.full(cos_i.shape, int_ior, T)
    swap = cos_i < 0
    eta_i, eta_t = np.where(swap, eta_t, eta_i), np.where(swap, eta_i, eta_t)
    cos_i = np.where(swap, -cos_i, cos_i)
    eta = eta_i / eta_t
    sin_t2 = eta * eta * (T(1) - cos_i * cos_i)
    with np.errstate(invalid="ignore", divide="ignore"):
        cos_t = np.sqrt(np.abs(T(1) - sin_t2))
        rs = (eta_i * cos_i - eta_t * cos_t) / (eta_i * cos_i + eta_t * cos_t)
        rp = (eta_t * cos_i - eta_i * cos_t) / (eta_t * cos_i + eta_i * cos_t)
        f = (rs * rs + rp * rp) / T(2)
    return np.where(sin_t2 > 1, T(1), f) if ext_ior != int_ior else np.zeros(cos_i.shape, T)


def _mf_eval(wi_, wo, alpha, T):
    """Microfacet::eval's first channel with kd = 0, ks = 1 (microfacet.cpp:92-105)."""
    ks = T(1)
    with np.errstate(invalid="ignore", divide="ignore", over="ignore", under="ignore"):
        wh = normalized(wi_ + wo)
        den = ks * _beckmann_d(wh, alpha, T) * _fresnel(dot(wh, wi_), T(F32(EXT_IOR)), T(F32(INT_IOR)), T) * \
            _smith_g1(wi_, wh, alpha, T) * _smith_g1(wo, wh, alpha, T)
        num = T(4) * wi_[:, 2] * wo[:, 2]
        return np.where(wo[:, 2] < 0, T(0), T(0) * inv_pi(T) + den / num)


def _mf_pdf(wi_, wo, alpha, T):
    """Microfacet::pdf with ks = 1 (microfacet.cpp:108-119)."""
    ks = T(1)
    with np.errstate(invalid="ignore", divide="ignore", over="ignore", under="ignore"):
        wh = normalized(wo + wi_)
        p1 = ks * _beckmann_d(wh, alpha, T) * wh[:, 2] / (T(4) * dot(wo, wh))
        p2 = (T(1) - ks) * wo[:, 2] * inv_pi(T)
        return np.where(wo[:, 2] <= 0, T(0), p1 + p2)


def _wi_rows(wi_, n, T):
    return np.broadcast_to(np.asarray(wi_, F32).astype(T).reshape(1, 3), (n, 3))


def sample(type: int, parameter, s3, T, wi_=None):
    """warpPoint: (points (n, 3), weights (n,)) of the samples s3 (n, 3); only the sphere volume reads s3[:, 2]."""
    s = np.asarray(s3, F32).astype(T).reshape(-1, 3)
    par = T(F32(parameter))
    n = len(s)
    one = np.ones(n, T)
    if type == NONE:
        return np.stack([s[:, 0], s[:, 1], np.zeros(n, T)], -1), one
    if type == DISK:
        x, y = _disk(s, T)
        return np.stack([x, y, np.zeros(n, T)], -1), one
    if type in (UNIFORM_SPHERE, ISO_PHASE):
        return uniform_sphere(s[:, :2].astype(F32), T), one
    if type == UNIFORM_SPHERE_VOL:
        return _fn(np.cbrt, T, s[:, 2])[:, None] * uniform_sphere(s[:, :2].astype(F32), T), one
    if type == UNIFORM_SPHERE_CAP:
        z = s[:, 0] * (T(1) - par) + par
        with np.errstate(invalid="ignore"):
            r = np.sqrt(T(1) - z * z)
        theta = s[:, 1] * T(2) * pi(T)
        return np.stack([r * _fn(np.cos, T, theta), r * _fn(np.sin, T, theta), z], -1), one
    if type == UNIFORM_HEMISPHERE:
        w = uniform_sphere(s[:, :2].astype(F32), T)
        return np.stack([w[:, 0], w[:, 1], np.abs(w[:, 2])], -1), one
    if type == COSINE_HEMISPHERE:
        return _cosine_hemisphere(s, T), one
    if type == BECKMANN:
        return _beckmann(s, par, T), one
    if type in (HENYEY_GREENSTEIN, ANISO_PHASE):
        return hg_sample(s[:, :2].astype(F32), parameter, T), one
    if type == MICROFACET_BRDF:  # Microfacet::sample with ks = 1: sample.y / ks, always the Beckmann branch
        w = _wi_rows(wi_, n, T)
        if w[0, 2] < 0:
            return np.zeros((n, 3), T), np.zeros(n, T)
        wh = _beckmann(np.stack([s[:, 0], s[:, 1] / T(1)], -1), par, T)
        wo = T(2) * (dot(w, wh)[:, None] * wh) - w
        with np.errstate(invalid="ignore", divide="ignore", over="ignore", under="ignore"):
            e = _mf_eval(w, wo, par, T)
            c = np.where(wo[:, 2] <= 0, T(0), e / _mf_pdf(w, wo, par, T) * wo[:, 2])
            lum = c * T(F32(0.212671)) + c * T(F32(0.715160)) + c * T(F32(0.072169))
        return wo, np.where(lum == 0, T(0), e)
    raise ValueError(f"warp type {type} is not restated")


def pdf(type: int, parameter, v, T, wi_=None):
    """The matching *Pdf of the points v (n, 3); None and Disk read x, y only."""
    v = np.asarray(v, F32).astype(T).reshape(-1, 3)
    par = T(F32(parameter))
    n = len(v)
    x, y, z = v[:, 0], v[:, 1], v[:, 2]
    with np.errstate(invalid="ignore", divide="ignore", over="ignore", under="ignore"):
        if type == NONE:
            return np.where((x >= 0) & (y >= 0) & (x <= 1) & (y <= 1), T(1), T(0))
        if type == DISK:
            return np.where(x * x + y * y <= 1, T(1) / pi(T), T(0))
        on_sphere = np.abs(dot(v, v) - T(1)) < eps(T)
        sphere = np.where(on_sphere, T(0.25) / pi(T), T(0))
        if type == UNIFORM_SPHERE:
            return sphere
        if type == UNIFORM_SPHERE_VOL:  # as written: not a density
            return np.full(n, T(4) / T(3) * pi(T), T)
        if type == UNIFORM_SPHERE_CAP:  # as written: zero ON the complement of the cap
            return np.where(on_sphere & (z <= par), T(0), np.full(n, T(1) / (T(2) * pi(T) * (T(1) - par)), T))
        if type == UNIFORM_HEMISPHERE:
            return np.where(on_sphere & (z > 0), T(2) * sphere, T(0))
        if type == COSINE_HEMISPHERE:
            return np.where(on_sphere & (z > 0), z / pi(T), T(0))
        if type == BECKMANN:
            r = np.sqrt(x * x + y * y)
            tan = r / z
            val = _fn(np.exp, T, -tan * tan / par / par) / (pi(T) * par * par * z * z * z)
            return np.where((np.abs(dot(v, v) - T(1)) > eps(T)) | (z < 0), T(0), val)
        if type in (HENYEY_GREENSTEIN, ANISO_PHASE):
            return hg_pdf(v.astype(F32), parameter, T)
        if type == ISO_PHASE:
            return np.full(n, T(0.25) / pi(T), T)
        if type == MICROFACET_BRDF:
            return _mf_pdf(_wi_rows(wi_, n, T), v, par, T)
    raise ValueError(f"warp type {type} is not restated")


# ---- the two tables ---------------------------------------------------------------------------------------------------
def cells(type: int, p, xres: int, yres: int):
    """(cell, nan): the cell ybin * xres + xbin of every point p (n, 3) float32, binned in fp32 as written; nan marks
    the points with a NaN coordinate, whose cell is meaningless."""
    p = np.asarray(p, F32).reshape(-1, 3)
    half = F32(0.5)
    if type == NONE:
        x, y = p[:, 0], p[:, 1]
    elif type == DISK:
        x, y = p[:, 0] * half + half, p[:, 1] * half + half
    else:
        x = np.arctan2(p[:, 1].astype(F64), p[:, 0].astype(F64)).astype(F32) * F32(0.15915494309189533577)
        with np.errstate(invalid="ignore"):
            x = np.where(x < 0, x + F32(1), x).astype(F32)
        y = p[:, 2] * half + half
    nan = np.isnan(x) | np.isnan(y)
    with np.errstate(invalid="ignore"):
        xb = np.clip(np.floor(np.where(nan, F32(0), x) * F32(xres)).astype(np.int64), 0, xres - 1)
        yb = np.clip(np.floor(np.where(nan, F32(0), y) * F32(yres)).astype(np.int64), 0, yres - 1)
    return yb * xres + xb, nan


def histogram(type: int, parameter, n: int, xres: int, yres: int, first_draw: int = 0, rtl: bool = True, wi_=None,
              chunk: int = 1 << 20):
    """(obs, nan_points, skipped): runTest's table of n points from draw first_draw (float64 whole counts), the points
    left out for a NaN coordinate, and the points of weight 0."""
    obs = np.zeros(xres * yres, np.int64)
    nan_points = skipped = 0
    for begin in range(0, n, chunk):
        m = min(chunk, n - begin)
        p, w = sample(type, parameter, points(first_draw + 3 * begin, m, rtl), F32, wi_)
        keep = ~(w == 0)
        skipped += int(m - keep.sum())
        cell, nan = cells(type, p[keep], xres, yres)
        nan_points += int(nan.sum())
        obs += np.bincount(cell[~nan], minlength=xres * yres)
    return obs.astype(np.float64), nan_points, skipped


def expected(type: int, parameter, xres: int, yres: int, sample_count: int, wi_=None):
    """(exp, evals): the expected frequency of every cell (float64) and the pdf evaluations it took (uint32)."""
    two_pi = float(F32(2) * pi(F32))
    v = np.zeros((1, 3), F32)
    count = [0]

    def integrand(y, x):
        count[0] += 1
        if type == NONE:
            v[0] = (x, y, 0.0)
        elif type == DISK:
            v[0] = (x * 2 - 1, y * 2 - 1, 0.0)
        else:
            x *= two_pi
            y = y * 2 - 1
            with np.errstate(invalid="ignore"):
                sin_theta = float(np.sqrt(np.float64(1 - y * y)))
            v[0] = (sin_theta * math.cos(x), sin_theta * math.sin(x), y)
        return float(pdf(type, parameter, v, F32, wi_)[0])

    scale = float(sample_count)
    if type == DISK:
        scale *= 4
    elif type != NONE:
        scale *= float(F32(4) * pi(F32))
    exp = np.zeros(xres * yres, np.float64)
    evals = np.zeros(xres * yres, np.uint32)
    e = F32(1e-4)
    for y in range(yres):
        y0, y1 = y / float(yres), float(F32(y + 1) - e) / float(yres)
        for x in range(xres):
            x0, x1 = x / float(xres), float(F32(x + 1) - e) / float(xres)
            count[0] = 0
            exp[y * xres + x] = chi2_refs.adaptive_simpson_2d(integrand, y0, x0, y1, x1) * scale
            evals[y * xres + x] = count[0]
    if (exp < 0).any():
        raise ValueError("The Pdf() function returned negative values!")
    return exp, evals


def execute(type: int, parameter_slider=0.5, angle_slider=0.5, rtl: bool = True, xres: int = 0, yres: int = 0,
            sample_count: int = 0) -> dict:
    """runTest: chi2_refs.chi2_statistic's entries with parameter, wi, obs, exp, evals, nan_points, skipped, obs_sum,
    exp_sum, level, sample_count, xres, yres."""
    if xres == 0 and yres == 0 and sample_count == 0:
        yres, xres, sample_count = default_table(type)
    par = map_parameter(type, parameter_slider)
    w = wi(angle_slider) if type in HAS_WI else np.zeros(3, F32)
    obs, nan_points, skipped = histogram(type, par, sample_count, xres, yres, 0, rtl, w)
    exp, evals = expected(type, par, xres, yres, sample_count, w)
    alpha = float(F32(0.01))
    r = chi2_refs.chi2_statistic(obs, exp, sample_count, 5.0, alpha, 1)
    r.update(parameter=par, wi=w, obs=obs, exp=exp, evals=evals, nan_points=nan_points, skipped=skipped,
             obs_sum=float(obs.sum()), exp_sum=float(sum(exp.tolist())), level=chi2_refs.sidak(alpha, 1),
             sample_count=sample_count, xres=xres, yres=yres)
    return r


def digest(obs) -> str:
    """SHA-256 of the counts as little-endian uint32."""
    return hashlib.sha256(np.asarray(obs).astype("<u4").tobytes()).hexdigest()
