"""Test support for the participating media (tests/test_volume_host.py, tests/test_gpu_volume.py).

Part 1: numpy restatements of the media functions. Every function takes the float type T the arithmetic runs in, as
emitter_refs does: F32 is the device's precision (transcendentals evaluated in fp64 and rounded once), F64 the reference
value. Inputs are float32 values in both runs. M_PI and Epsilon are Nori's float constants.

  fold_medium      Medium::updateDerivedProperties (src/media/medium.cpp:112-117) and
                   HomogeneousMedium::updateDerivedProperties (src/media/homogmedium.cpp:48-54)
  free_path        HomogeneousMedium::sampleFreePath (homogmedium.cpp:61-67)
  transmittance    HomogeneousMedium::getTransmittance (homogmedium.cpp:69-73)
  iso_sample/pdf   IsoPhase (src/bsdf/isophase.cpp:20-28), Warp::squareToUniformSphere (src/utils/warp.cpp:74-82)
  hg_sample/pdf    AnisoPhase (src/bsdf/anisophase.cpp:24-33), Warp::squareToHenyeyGreenstein{,Pdf} (warp.cpp:168-205)

Part 2: an fp64 Monte-Carlo restatement of PathVolMATSIntegrator::Li (src/integrators/path_vol_mats.cpp:20-122) and
PathVolMISIntegrator::Li with traceShadowray and sampleEmitter (path_vol_mis.cpp:26-243) on scenes made of spheres
only: analytic ray-sphere intersection (src/shapes/sphere.cpp:67-124), numpy's own generator, every path of a batch
advanced together. Written from those files, quirks included; `quirks=False` turns two of them off -- the throughput is
then divided by the free-path density of the sampled event and takes the scattering coefficient at a medium
interaction, which is the textbook estimator -- so that a test can show it would tell the two apart.

Part 3: the reference's t-test (ext/hypothesis/hypothesis.h students_t_test, src/utils/ttest.cpp:191-240) for two
estimates that each come with a standard error, and the XML of the sphere scenes.
"""
from __future__ import annotations

import math
import os

import numpy as np

from emitter_refs import F32, F64, _fn, dot, eps, luminance, normalized, pi, uniform_sphere

# ---------------------------------------------------------------------------------------------------------------
# Part 1: the media functions
# ---------------------------------------------------------------------------------------------------------------


def fold_medium(sigma_a=(0.5, 0.5, 0.5), sigma_s=(0.0, 0.0, 0.0), sigma_a_intensity=1.0, sigma_s_intensity=1.0,
                density=1.0) -> dict:
    """The derived coefficients, each one fp32 product or sum, in the reference's order."""
    sa = np.asarray(sigma_a, F32) * F32(sigma_a_intensity)
    ss = np.asarray(sigma_s, F32) * F32(sigma_s_intensity)
    mu_a, mu_s = F32(density) * sa, F32(density) * ss
    return {"mu_a": mu_a, "mu_s": mu_s, "mu_t": mu_a + mu_s, "density": F32(density)}


def free_path(mu_t, u, T):
    """u: (n, 2) uniforms in draw order -> (t, draws): the channel (int)(3 u0); t = -log(u1) / mu_t[channel], or inf
    after one draw when that channel's mu_t < Epsilon."""
    u = np.asarray(u, F32).astype(T).reshape(-1, 2)
    mu_t = np.asarray(mu_t, F32).astype(T)
    ch = np.clip((T(3) * u[:, 0]).astype(np.int32), 0, 2)
    mu = mu_t[ch]
    thin = mu < eps(T)
    with np.errstate(divide="ignore", invalid="ignore"):
        t = -_fn(np.log, T, u[:, 1]) / mu
    return np.where(thin, T(np.inf), t), np.where(thin, 1, 2)


def transmittance(mu_t, a, b, T):
    """(-mu_t * |a - b|).exp() per channel; a, b: (n, 3)."""
    a, b = np.asarray(a, F32).astype(T).reshape(-1, 3), np.asarray(b, F32).astype(T).reshape(-1, 3)
    d = a - b
    with np.errstate(over="ignore"):
        length = np.sqrt(dot(d, d))
        return _fn(np.exp, T, -np.asarray(mu_t, F32).astype(T)[None, :] * length[:, None])


def iso_sample(sample, T):
    return uniform_sphere(np.asarray(sample, F32).reshape(-1, 2), T)


def iso_pdf(wo, T):
    return np.full(len(np.asarray(wo).reshape(-1, 3)), T(0.25) / pi(T), T)


def hg_sample(sample, g, T):
    """NaN where 1 - cos^2 rounds below zero, as the reference's std::sqrt returns it."""
    s = np.asarray(sample, F32).astype(T).reshape(-1, 2)
    g = T(F32(g))
    if abs(g) < eps(T):
        ct = T(1) - T(2) * s[:, 0]
    else:
        factor = (T(1) - g * g) / (T(1) - g + T(2) * g * s[:, 0])
        ct = (T(1) + g * g - factor * factor) / (T(2) * g)
    phi = T(2) * pi(T) * s[:, 1]
    with np.errstate(invalid="ignore"):
        st = np.sqrt(T(1) - ct * ct)
    return np.stack([st * _fn(np.cos, T, phi), st * _fn(np.sin, T, phi), ct], -1)


def hg_pdf(wo, g, T):
    wo = np.asarray(wo, F32).astype(T).reshape(-1, 3)
    g = T(F32(g))
    g2 = g * g
    with np.errstate(invalid="ignore", divide="ignore"):
        return T(0.25) / pi(T) * (T(1) - g2) / _fn(np.power, T, T(1) + g2 - T(2) * g * wo[:, 2], 1.5)


# ---------------------------------------------------------------------------------------------------------------
# Part 2: the two integrators on sphere-only scenes, fp64
# ---------------------------------------------------------------------------------------------------------------
_EPS = float(F32(1e-4))
VARIANCE_FLOOR = 1e-5
_PI = float(F32(3.14159265358979323846))


def sphere(center, radius, bsdf=None, albedo=(0.5, 0.5, 0.5), int_ior=1.5046, ext_ior=1.000277, medium=None,
           radiance=None) -> dict:
    """bsdf: None, "diffuse" or "dielectric"; medium: index into the scene's media or None; radiance: an area light."""
    return {"center": tuple(float(F32(x)) for x in center), "radius": float(F32(radius)), "bsdf": bsdf,
            "albedo": tuple(float(F32(x)) for x in albedo), "int_ior": float(F32(int_ior)),
            "ext_ior": float(F32(ext_ior)), "medium": medium,
            "radiance": None if radiance is None else tuple(float(F32(x)) for x in radiance)}


def medium(kind="homog", sigma_a=(0.5, 0.5, 0.5), sigma_s=(0.0, 0.0, 0.0), density=1.0, phase="iso", g=0.0) -> dict:
    return {"kind": kind, "sigma_a": tuple(sigma_a), "sigma_s": tuple(sigma_s), "density": density, "phase": phase,
            "g": float(F32(g))}


class SphereScene:
    """spheres: sphere() records; media: medium() records; ambient: index into media or None; the camera ray is
    (origin, direction)."""

    def __init__(self, spheres, media, ambient, origin, direction):
        self.spheres, self.media_desc, self.ambient = list(spheres), list(media), -1 if ambient is None else ambient
        self.origin = np.asarray(origin, F64)
        d = np.asarray(direction, F64)
        self.direction = d / np.linalg.norm(d)
        self.c = np.array([s["center"] for s in spheres], F64)
        self.r = np.array([s["radius"] for s in spheres], F64)
        kinds = {None: -1, "diffuse": 0, "dielectric": 2}
        self.bsdf = np.array([kinds[s["bsdf"]] for s in spheres])
        self.albedo = np.array([s["albedo"] for s in spheres], F64)
        self.int_ior = np.array([s["int_ior"] for s in spheres], F64)
        self.ext_ior = np.array([s["ext_ior"] for s in spheres], F64)
        self.smed = np.array([-1 if s["medium"] is None else s["medium"] for s in spheres])
        self.lights = [i for i, s in enumerate(spheres) if s["radiance"] is not None]
        self.radiance = np.array([s["radiance"] or (0, 0, 0) for s in spheres], F64)
        self.emitter = np.array([s["radiance"] is not None for s in spheres])
        # media tables, with one more row (index -1) for the default ambient vacuum
        n = len(media) + 1
        self.homog = np.zeros(n, bool)
        self.mu_t, self.mu_s = np.zeros((n, 3)), np.zeros((n, 3))
        self.hg, self.g = np.zeros(n, bool), np.zeros(n)
        for i, m in enumerate(media):
            f = fold_medium(m["sigma_a"], m["sigma_s"], density=m["density"])
            self.homog[i] = m["kind"] == "homog"
            self.mu_t[i], self.mu_s[i] = f["mu_t"].astype(F64), f["mu_s"].astype(F64)
            self.hg[i], self.g[i] = m["phase"] == "hg", m["g"]

    def vacuum_copy(self):
        """The same geometry with every medium a vacuum."""
        media = [dict(m, kind="vacuum") for m in self.media_desc]
        return SphereScene(self.spheres, media, None if self.ambient < 0 else self.ambient, self.origin, self.direction)

    # Scene::rayIntersect over Sphere::rayIntersect (sphere.cpp:67-94) with the adaptive ray epsilon (bvh.cpp:407-410)
    def intersect(self, o, d, mint, maxt):
        mint = np.where(mint == _EPS, np.maximum(mint, mint * np.abs(o).max(-1)), mint)
        L = o[:, None, :] - self.c[None]
        a = dot(d, d)[:, None]
        b = 2.0 * dot(d[:, None, :], L)
        c = dot(L, L) - (self.r * self.r)[None]
        disc = b * b - 4.0 * a * c
        with np.errstate(invalid="ignore", divide="ignore"):
            sq = np.sqrt(disc)
            t0, t1 = (-b - sq) / 2 / a, (-b + sq) / 2 / a
        lo, hi = mint[:, None], maxt[:, None]
        ok0 = (disc >= 0) & (lo <= t0) & (hi >= t0)
        ok1 = (disc >= 0) & (lo <= t1) & (hi >= t1)
        t = np.where(ok0, t0, np.where(ok1, t1, np.inf))
        k = t.argmin(-1)
        tt = t[np.arange(len(o)), k]
        return np.isfinite(tt), tt, k

    def frame(self, p, k):  # Sphere::setHitInformation (sphere.cpp:96-124): shFrame (t, b, n); geoFrame.n = n
        n = normalized(p - self.c[k])
        t = normalized(np.cross(np.broadcast_to([0.0, 0.0, 1.0], n.shape), n))
        return t, np.cross(n, t), n


def _to_local(fr, v):
    return np.stack([dot(v, fr[0]), dot(v, fr[1]), dot(v, fr[2])], -1)


def _to_world(fr, v):
    return fr[0] * v[:, :1] + fr[1] * v[:, 1:2] + fr[2] * v[:, 2:3]


def _frame_of(n):  # Frame(n): coordinateSystem (common.cpp:292-306)
    a = np.abs(n[:, 0]) > np.abs(n[:, 1])
    with np.errstate(invalid="ignore", divide="ignore"):
        il_a = 1.0 / np.sqrt(n[:, 0] ** 2 + n[:, 2] ** 2)
        il_b = 1.0 / np.sqrt(n[:, 1] ** 2 + n[:, 2] ** 2)
    z = np.zeros(len(n))
    c = np.where(a[:, None], np.stack([n[:, 2] * il_a, z, -n[:, 0] * il_a], -1),
                 np.stack([z, n[:, 2] * il_b, -n[:, 1] * il_b], -1))
    return np.cross(c, n), c, n


def _fresnel(cos_i, ext, int_):  # common.cpp:308-338
    eta_i, eta_t = np.where(cos_i < 0, int_, ext), np.where(cos_i < 0, ext, int_)
    ci = np.abs(cos_i)
    eta = eta_i / eta_t
    s2 = eta * eta * (1 - ci * ci)
    with np.errstate(invalid="ignore"):
        ct = np.sqrt(1.0 - s2)
        rs = (eta_i * ci - eta_t * ct) / (eta_i * ci + eta_t * ct)
        rp = (eta_t * ci - eta_i * ct) / (eta_t * ci + eta_i * ct)
    return np.where(ext == int_, 0.0, np.where(s2 > 1.0, 1.0, (rs * rs + rp * rp) / 2.0))


def _phase_sample(S, med, u):
    g = S.g[med]
    x, y = u[:, 0], u[:, 1]
    with np.errstate(invalid="ignore", divide="ignore"):
        factor = (1 - g * g) / (1 - g + 2 * g * x)
        ct = np.where(np.abs(g) < _EPS, 1 - 2 * x, (1 + g * g - factor * factor) / (2 * g))
        st = np.sqrt(1 - ct * ct)
    phi = 2 * _PI * y
    hg = np.stack([st * np.cos(phi), st * np.sin(phi), ct], -1)
    z = 2 * x - 1
    r = np.sqrt(np.maximum(1 - z * z, 0))
    iso = normalized(np.stack([r * np.cos(phi), r * np.sin(phi), z], -1))
    return np.where(S.hg[med][:, None], hg, iso)


def _phase_pdf(S, med, wo):
    g = S.g[med]
    with np.errstate(invalid="ignore", divide="ignore"):
        hg = 0.25 / _PI * (1 - g * g) / np.power(1 + g * g - 2 * g * wo[:, 2], 1.5)
    return np.where(S.hg[med], hg, 0.25 / _PI)


def _tr(S, med, a, b):
    length = np.sqrt(dot(a - b, a - b))
    return np.where(S.homog[med][:, None], np.exp(-S.mu_t[med] * length[:, None]), 1.0)


def _cross_medium(S, k, w, gn, n):
    """entering the shape's medium when w points against the geometric normal and the shape has one, else ambient"""
    return np.where((dot(w, gn) < 0) & (S.smed[k] >= 0), S.smed[k], np.full(n, S.ambient))


def _shadow_walk(S, med, o, d, maxt):
    """traceShadowray (path_vol_mis.cpp:26-46) -> (occluded, transmittance)"""
    n = len(o)
    tr = np.ones((n, 3))
    occluded = np.zeros(n, bool)
    live = np.ones(n, bool)
    o, med, maxt = o.copy(), med.copy(), maxt.copy()
    mint = np.full(n, _EPS)
    for _ in range(64):
        idx = np.nonzero(live)[0]
        if len(idx) == 0:
            break
        hit, t, k = S.intersect(o[idx], d[idx], mint[idx], maxt[idx])
        live[idx[~hit]] = False
        idx, t, k = idx[hit], t[hit], k[hit]
        solid = S.bsdf[k] >= 0
        occluded[idx[solid]] = True
        live[idx[solid]] = False
        idx, t, k = idx[~solid], t[~solid], k[~solid]
        p = o[idx] + t[:, None] * d[idx]
        tr[idx] *= _tr(S, med[idx], o[idx], p)
        gn = normalized(p - S.c[k])
        med[idx] = _cross_medium(S, k, d[idx], gn, len(idx))
        o[idx] = p
        maxt[idx] -= t
    assert not live.any(), "shadow walk did not end"
    return occluded, tr


def li_batch(S: SphereScene, n: int, rng: np.random.Generator, mis: bool, quirks: bool = True) -> np.ndarray:
    """Li of n independent paths along the scene's camera ray: (n, 3)."""
    li = np.zeros((n, 3))
    thr = np.ones((n, 3))
    med = np.full(n, S.ambient)
    o = np.broadcast_to(S.origin, (n, 3)).copy()
    d = np.broadcast_to(S.direction, (n, 3)).copy()
    mint, maxt = np.full(n, _EPS), np.full(n, np.inf)
    pdf_mat = np.ones(n)
    discrete = np.ones(n, bool)  # pdf_mat_measure == EDiscrete
    alive = np.ones(n, bool)
    n_lights = float(len(S.lights))
    bounces = 0
    while alive.any():
        assert bounces < 4000, "paths did not end"
        A = np.nonzero(alive)[0]
        hit, t_hit, k = S.intersect(o[A], d[A], mint[A], maxt[A])
        alive[A[~hit]] = False  # miss: the path ends before any medium is sampled (no environment map here)
        A, t_hit, k = A[hit], t_hit[hit], k[hit]
        m = len(A)
        if m == 0:
            break
        oa, da, ma = o[A], d[A], med[A]
        p_s = oa + t_hit[:, None] * da
        fr = S.frame(p_s, k)
        # free path: a channel, then a distance only when that channel's mu_t >= Epsilon; vacuum draws nothing
        ch = np.minimum((3 * rng.random(m)).astype(int), 2)
        mu = S.mu_t[ma, ch]
        with np.errstate(divide="ignore"):
            tm = np.where(S.homog[ma] & (mu >= _EPS), -np.log(rng.random(m)) / np.where(mu > 0, mu, 1.0), np.inf)
        in_med = tm < t_hit
        with np.errstate(invalid="ignore"):  # (inf * 0 where no distance was sampled: not selected)
            p = np.where(in_med[:, None], oa + tm[:, None] * da, p_s)
        tr = _tr(S, ma, oa, p)
        if quirks:
            thr[A] *= tr
        else:  # divided by the density of the sampled event (channel-uniform), scattering coefficient at an interaction
            dens = np.where(in_med[:, None], S.mu_t[ma] * tr, tr).mean(-1)
            w = tr / dens[:, None]
            w = np.where(in_med[:, None], w * S.mu_s[ma], w)
            thr[A] *= np.where(S.homog[ma][:, None], w, 1.0)
        ta = thr[A]
        # emission at a surface hit
        em = ~in_med & S.emitter[k]
        wi_e = normalized(p_s - oa)
        front = dot(fr[2], -wi_e) >= 0
        le = np.where((em & front)[:, None], S.radiance[k], 0.0)
        if mis:
            with np.errstate(invalid="ignore", divide="ignore"):
                pdf_em = (1.0 / S.r[k]) ** 2 * (0.25 / _PI) * dot(p_s - oa, p_s - oa) / np.abs(dot(fr[2], -wi_e))
            pdf_em = np.where(front, pdf_em, 0.0) / max(n_lights, 1.0)
            pm = pdf_mat[A]
            with np.errstate(invalid="ignore", divide="ignore"):
                w_mat = np.where(discrete[A], 1.0, np.where(pm > _EPS, pm / (pm + pdf_em), 0.0))
            li[A] += w_mat[:, None] * ta * le
        else:
            li[A] += ta * le
        # Russian roulette
        has_bsdf = S.bsdf[k] >= 0
        if bounces >= 3:
            rr = in_med | has_bsdf
            succ = np.minimum(ta.max(-1), 0.99)
            u = rng.random(m)
            dead = rr & ((u > succ) | (succ < _EPS))
            ta = np.where((rr & ~dead)[:, None], ta / np.where(succ > 0, succ, 1.0)[:, None], ta)
            thr[A] = ta
            alive[A[dead]] = False
            keep = ~dead
            A, k, t_hit, in_med, p, p_s, oa, da, ma, ta, has_bsdf = (x[keep] for x in (A, k, t_hit, in_med, p, p_s, oa,
                                                                                       da, ma, ta, has_bsdf))
            fr = tuple(f[keep] for f in fr)
            m = len(A)
            if m == 0:
                bounces += 1
                continue
        # next direction
        wo = da.copy()
        col = np.ones((m, 3))
        nee = np.zeros(m, bool)
        u2 = rng.random((m, 2))
        wi_l = _to_local(fr, -da)
        wl = np.zeros((m, 3))
        measure_sa = np.zeros(m, bool)
        if in_med.any():
            wl_m = _phase_sample(S, ma, u2)
            fd = _frame_of(da)
            wo = np.where(in_med[:, None], _to_world(fd, wl_m), wo)
            pdf_mat[A] = np.where(in_med, _phase_pdf(S, ma, wl_m), pdf_mat[A])
            discrete[A] = np.where(in_med, False, discrete[A])
            nee |= in_med
        surf = ~in_med & has_bsdf
        dif = surf & (S.bsdf[k] == 0)
        if dif.any():  # Diffuse::sample (diffuse.cpp:123-140): cosine hemisphere; nothing from below
            up = wi_l[:, 2] > 0
            rho, th = np.sqrt(u2[:, 0]), 2 * _PI * u2[:, 1]
            x, y = rho * np.cos(th), rho * np.sin(th)
            w_d = np.stack([x, y, np.sqrt(np.maximum(1 - (x * x + y * y), 0))], -1)
            w_d = np.where(up[:, None], w_d, 0.0)
            wl = np.where(dif[:, None], w_d, wl)
            col = np.where(dif[:, None], np.where(up[:, None], S.albedo[k], 0.0), col)
            measure_sa |= dif & up
            pdf_d = np.where(up & (w_d[:, 2] > 0), w_d[:, 2] / _PI, 0.0)  # (an unknown measure: pdf 0)
            pdf_mat[A] = np.where(dif, pdf_d, pdf_mat[A])
            discrete[A] = np.where(dif, False, discrete[A])
        die = surf & (S.bsdf[k] == 2)
        if die.any():  # Dielectric::sample (dielectric.cpp:51-102)
            ci = wi_l[:, 2]
            F = _fresnel(ci, S.ext_ior[k], S.int_ior[k])
            refl = u2[:, 0] < F
            nz = np.where(ci < 0, -1.0, 1.0)
            eta = np.where(ci < 0, S.int_ior[k] / S.ext_ior[k], S.ext_ior[k] / S.int_ior[k])
            dn = ci * nz
            nvec = np.stack([np.zeros(m), np.zeros(m), nz], -1)
            with np.errstate(invalid="ignore"):
                wt = -eta[:, None] * (wi_l - dn[:, None] * nvec) - np.sqrt(1 - eta * eta * (1 - dn * dn))[:, None] * nvec
            w_r = np.stack([-wi_l[:, 0], -wi_l[:, 1], wi_l[:, 2]], -1)
            w_x = np.where(refl[:, None], w_r, wt)
            wl = np.where(die[:, None], w_x, wl)
            col = np.where(die[:, None], np.where(refl, 1.0, 1 / eta / eta)[:, None], col)
            pdf_mat[A] = np.where(die, 0.0, pdf_mat[A])  # Dielectric::pdf is 0
            discrete[A] = np.where(die, True, discrete[A])
        wo = np.where(surf[:, None], _to_world(fr, wl), wo)
        nee |= surf & measure_sa
        if mis and nee.any():
            # sampleEmitter (path_vol_mis.cpp:53-105), reference point its.p -- the surface point -- in both cases
            N = np.nonzero(nee)[0]
            q = len(N)
            lk = np.asarray(S.lights)[np.minimum((rng.random(q) * n_lights).astype(int), len(S.lights) - 1)]
            us = rng.random((q, 2))
            z = 2 * us[:, 0] - 1
            r = np.sqrt(np.maximum(1 - z * z, 0))
            ph = 2 * _PI * us[:, 1]
            qd = normalized(np.stack([r * np.cos(ph), r * np.sin(ph), z], -1))
            pl = S.c[lk] + S.r[lk][:, None] * qd
            ref = p_s[N]
            to = pl - ref
            dist = np.sqrt(dot(to, to))
            wi = to / dist[:, None]
            cosl = dot(qd, -wi)
            with np.errstate(invalid="ignore", divide="ignore"):
                pdf_l = np.where(cosl >= 0, (1.0 / S.r[lk]) ** 2 * (0.25 / _PI) * dot(to, to) / np.abs(cosl), 0.0)
                Le = np.where(((np.abs(pdf_l) >= _EPS) & (cosl >= 0))[:, None], S.radiance[lk] / pdf_l[:, None], 0.0)
            Le = Le * n_lights
            pdf_em = pdf_l / n_lights
            sd = -wi  # the shadow ray runs from the light to the reference point
            frN = tuple(f[N] for f in fr)
            smed = np.where(dot(da[N], sd) > 0, _cross_medium(S, k[N], sd, frN[2], q), ma[N])
            occ, str_ = _shadow_walk(S, smed, pl, sd, dist - _EPS)
            is_med = in_med[N]
            pdf_ph = _phase_pdf(S, ma[N], _to_local(frN, sd))
            we = _to_local(frN, wi)
            wil = wi_l[N]
            both_up = (wil[:, 2] > 0) & (we[:, 2] > 0)
            pdf_bs = np.where(both_up, we[:, 2] / _PI, 0.0)
            pdf_other = np.where(is_med, pdf_ph, pdf_bs)
            with np.errstate(invalid="ignore", divide="ignore"):
                w_em = np.where(pdf_em > _EPS, pdf_em / (pdf_em + pdf_other), 0.0)
            f_bs = np.where(both_up[:, None], S.albedo[k[N]] / _PI, 0.0) * np.abs(dot(wi, frN[2]))[:, None]
            x = np.where(is_med[:, None], np.abs(dot(wi, sd))[:, None], f_bs)
            add = str_ * w_em[:, None] * ta[N] * Le * x
            ok = ~occ & (w_em > _EPS)
            li[A[N]] += np.where(ok[:, None], add, 0.0)
        ta = np.where(surf[:, None], ta * col, ta)
        if not quirks:
            pass  # (the scattering coefficient was applied with the free-path weight above)
        thr[A] = ta
        # entering or leaving the hit shape: at a surface, when the ray goes on through it
        sw = ~in_med & (dot(da, wo) > 0)
        med[A] = np.where(sw, _cross_medium(S, k, wo, fr[2], m), ma)
        o[A], d[A] = p, wo
        mint[A], maxt[A] = _EPS, np.inf
        zero = (wo == 0).all(-1)
        alive[A[zero]] = False  # a zero direction misses everything
        bounces += 1
    return li


def estimate(S: SphereScene, n: int, seed: int, mis: bool, quirks: bool = True, batch: int = 1 << 18) -> dict:
    """Mean luminance of Li over n paths and its standard error, with the variance floor of the reference's t-test
    (hypothesis.h:319: max(variance, 1e-5))."""
    rng = np.random.default_rng(seed)
    s1 = s2 = 0.0
    done = 0
    while done < n:
        b = min(batch, n - done)
        lum = luminance(li_batch(S, b, rng, mis, quirks), F64)
        s1 += float(lum.sum())
        s2 += float((lum * lum).sum())
        done += b
    mean = s1 / n
    var = max(s2 / n - mean * mean, 0.0) * n / (n - 1)
    return {"seed": seed, "n": n, "mean": mean, "stderr": math.sqrt(max(var, VARIANCE_FLOOR) / n)}


def render_seed(base: int, k: int) -> int:
    """The seed of the k-th of several independent renders. A path's stream is seeded from seed ^ pixel, so seeds that
    differ only in the bits a pixel index occupies give every render the same set of streams, dealt to other pixels:
    renders of a scene whose pixels all estimate one number would then agree to the last digit. These differ above
    bit 24, and two bases above bit 32."""
    return (base << 32) + ((k + 1) << 24)


def seeds_estimate(values) -> tuple:
    """(mean, standard error, degrees of freedom) of K independent estimates of one number, with the same floor."""
    v = np.asarray(values, F64)
    return float(v.mean()), math.sqrt(max(float(v.var(ddof=1)), VARIANCE_FLOOR) / len(v)), len(v) - 1


# ---------------------------------------------------------------------------------------------------------------
# Part 3: the t-test and the scenes
# ---------------------------------------------------------------------------------------------------------------
def _betacf(a, b, x):  # continued fraction of the regularized incomplete beta function (Lentz)
    tiny = 1e-300
    qab, qap, qam = a + b, a + 1.0, a - 1.0
    c, d = 1.0, 1.0 - qab * x / qap
    d = 1.0 / (d if abs(d) > tiny else tiny)
    h = d
    for m in range(1, 400):
        m2 = 2 * m
        aa = m * (b - m) * x / ((qam + m2) * (a + m2))
        d = 1.0 + aa * d
        d = 1.0 / (d if abs(d) > tiny else tiny)
        c = 1.0 + aa / c
        c = c if abs(c) > tiny else tiny
        h *= d * c
        aa = -(a + m) * (qab + m) * x / ((a + m2) * (qap + m2))
        d = 1.0 + aa * d
        d = 1.0 / (d if abs(d) > tiny else tiny)
        c = 1.0 + aa / c
        c = c if abs(c) > tiny else tiny
        delta = d * c
        h *= delta
        if abs(delta - 1.0) < 1e-15:
            break
    return h


def _betai(a, b, x):
    if x <= 0.0:
        return 0.0
    if x >= 1.0:
        return 1.0
    bt = math.exp(math.lgamma(a + b) - math.lgamma(a) - math.lgamma(b) + a * math.log(x) + b * math.log(1.0 - x))
    if x < (a + 1.0) / (a + b + 2.0):
        return bt * _betacf(a, b, x) / a
    return 1.0 - bt * _betacf(b, a, 1.0 - x) / b


def students_t_cdf(t: float, dof: float) -> float:
    x = dof / (dof + t * t)
    tail = 0.5 * _betai(0.5 * dof, 0.5, x)
    return 1.0 - tail if t >= 0 else tail


def t_test(mean_a, se_a, dof_a, mean_b, se_b, n_tests, alpha=0.01) -> dict:
    """students_t_test (hypothesis.h:314-346) for two estimates with standard errors: t = |a - b| / sqrt(se_a^2 +
    se_b^2), the degrees of freedom of the estimate with few samples (the other's are in the hundreds of thousands),
    two-sided p-value, Sidak-corrected significance 1 - (1 - alpha)^(1 / n_tests). pass: the null hypothesis stands."""
    se = math.sqrt(se_a * se_a + se_b * se_b)
    t = abs(mean_a - mean_b) / max(se, 1e-300)
    pval = 2.0 * (1.0 - students_t_cdf(t, dof_a))
    level = 1.0 - (1.0 - alpha) ** (1.0 / n_tests)
    return {"t": t, "pval": pval, "level": level, "pass": bool(pval >= level and math.isfinite(pval))}


_REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_GOLDEN = os.path.join(_REPO, "tests", "golden")
VOLUME_FIXTURE = os.path.join(_GOLDEN, "volume_scenes.json.gz")
MC_FIXTURE = os.path.join(_GOLDEN, "volume_mc.json")
# the reference's homogeneous-media scenes (tests/golden/make_volume_fixture.py)
VOLUME_SCENES = ["scenes/project/volume/%s.xml" % n for n in (
    "cbox_homog", "cbox_homog_ambient", "cbox_homog_aniso", "cbox_homog_caustic", "cbox_homog_dielectric_medium",
    "cbox_val_mats", "cbox_val_mis", "homog_test")] + [
    "scenes/pa4/cbox/cbox_path_vol_mats.xml", "scenes/pa4/cbox/cbox_path_vol_mis.xml",
    "scenes/project/optix/sphere-analytic.xml"]
EMISSION_SCENE = "scenes/project/volume-emission/volumelight-test-mats.xml"
# meshes those scenes name that an older bundle already carries, by path
SHARED_MESHES = {
    "scenes/project/meshes/cube.obj": "normalmap_scenes.json.gz",
    "scenes/project/meshes/plane.obj": "normalmap_scenes.json.gz",
}


def materialize(out_dir: str) -> str:
    """Write the volume scene bundle, the shared meshes and the older reference scenes (the pa4 Cornell box meshes)
    under out_dir; returns out_dir."""
    import gzip
    import json
    with open(os.path.join(_GOLDEN, "reference_scenes.json")) as f:
        files = json.load(f)
    with gzip.open(VOLUME_FIXTURE, "rt") as f:
        files.update(json.load(f))
    bundles = {}
    for rel, name in SHARED_MESHES.items():
        if name not in bundles:
            with gzip.open(os.path.join(_GOLDEN, name), "rt") as f:
                bundles[name] = json.load(f)
        files[rel] = bundles[name][rel]
    for rel, text in files.items():
        p = os.path.join(out_dir, rel)
        os.makedirs(os.path.dirname(p), exist_ok=True)
        with open(p, "w") as g:
            g.write(text)
    return out_dir


def _t(c):
    return ", ".join(repr(float(F32(x))) for x in c)


def medium_xml(m: dict, vacuum: bool = False) -> str:
    if vacuum or m["kind"] == "vacuum":
        return '<medium type="vacuum"/>'
    ph = f'<phase type="anisophase"><float name="g" value="{m["g"]!r}"/></phase>' if m["phase"] == "hg" else ""
    return (f'<medium type="homog"><color name="sigma_a" value="{_t(m["sigma_a"])}"/>'
            f'<color name="sigma_s" value="{_t(m["sigma_s"])}"/><float name="density" value="{float(m["density"])!r}"/>'
            f'{ph}</medium>')


def scene_xml(S: SphereScene, integrator: str, size: int = 32, spp: int = 16, vacuum: bool = False) -> str:
    """The scene as Nori XML: a near-zero field of view along the camera ray (as scenes/pa1/test-direct.xml), so every
    pixel sample estimates the same radiance."""
    o, t = S.origin, S.origin + S.direction
    up = (0, 1, 0) if abs(S.direction[1]) < 0.9 else (1, 0, 0)
    out = [f'<scene><integrator type="{integrator}"/>',
           f'<sampler type="independent"><integer name="sampleCount" value="{spp}"/></sampler>',
           f'<camera type="perspective"><transform name="toWorld"><lookat target="{_t(t)}" origin="{_t(o)}" '
           f'up="{_t(up)}"/></transform><float name="fov" value="1e-4"/><integer name="width" value="{size}"/>'
           f'<integer name="height" value="{size}"/><rfilter type="box"/></camera>']
    if S.ambient >= 0:
        out.append(medium_xml(S.media_desc[S.ambient], vacuum))
    for s in S.spheres:
        x = [f'<shape type="sphere"><point name="center" value="{_t(s["center"])}"/>'
             f'<float name="radius" value="{s["radius"]!r}"/>']
        if s["bsdf"] == "diffuse":
            x.append(f'<bsdf type="diffuse"><color name="albedo" value="{_t(s["albedo"])}"/></bsdf>')
        elif s["bsdf"] == "dielectric":
            x.append(f'<bsdf type="dielectric"><float name="intIOR" value="{s["int_ior"]!r}"/>'
                     f'<float name="extIOR" value="{s["ext_ior"]!r}"/></bsdf>')
        if s["medium"] is not None:
            x.append(medium_xml(S.media_desc[s["medium"]], vacuum))
        if s["radiance"] is not None:
            x.append(f'<emitter type="area"><color name="radiance" value="{_t(s["radiance"])}"/></emitter>')
        x.append("</shape>")
        out.append("".join(x))
    out.append("</scene>")
    return "\n".join(out)


# The Monte-Carlo scenes of tests/golden/volume_mc.json: the camera at (0.15, 0.1, -5) looks along +z through a sphere
# of radius 1 at the origin towards a sphere light behind it, all inside a diffuse sphere of radius 20 (seen from
# inside, so it reflects nothing: it gives every ray a surface to end on, without which a medium never acts).
_ORIGIN, _DIR = (0.15, 0.1, -5.0), (0.0, 0.0, 1.0)
_LIGHT = dict(center=(0.3, 0.2, 3.0), radius=0.75, bsdf="diffuse", albedo=(0.0, 0.0, 0.0), radiance=(8.0, 8.0, 8.0))
_SHELL = dict(center=(0.0, 0.0, 0.0), radius=20.0, bsdf="diffuse", albedo=(0.5, 0.5, 0.5))
_SA, _SS = (0.1, 0.2, 0.4), (0.9, 0.6, 0.3)


def floor_scene(blocker) -> SphereScene:
    """A diffuse ball as the floor under a sphere light, seen from the side; blocker: the medium record of a BSDF-less
    sphere between the light and the floor point the camera looks at, or None for no such sphere.

    The sphere is small and sits just above that point (every shadow ray and every BSDF ray towards the light crosses
    it) for a reason: after a ray has crossed a BSDF-less boundary, path_vol_mis weights the light it then hits with
    the light's density measured from the boundary (EmitterQueryRecord{ray.o, ..}, path_vol_mis.cpp:162-170), not from
    the point that scattered the ray. That is a bias of the reference which grows with the distance between the two
    points: with a sphere of radius 0.8 half way up to the light the restatement gives 0.459 against 0.284 without it.
    Here the boundary lies within 0.05 of the scattering point, 3 from the light: the density moves by under 3.5 %, the
    image by about 0.3 %, below what 8 renders of 64 spp resolve (0.4 %)."""
    media = [] if blocker is None else [blocker]
    spheres = [sphere((0, -50, 0), 50.0, bsdf="diffuse", albedo=(0.6, 0.5, 0.4)),
               sphere((0.2, 3.0, 0.1), 0.5, bsdf="diffuse", albedo=(0, 0, 0), radiance=(20, 20, 20))]
    if blocker is not None:
        spheres.append(sphere((0.0, 0.03, 0.0), 0.02, medium=0))
    return SphereScene(spheres, media, None, (3.0, 2.0, -4.0), (-3.0, -2.0, 4.0))


def mc_scenes() -> dict:
    """name -> SphereScene: (a) a BSDF-less medium sphere, (b) the same inside a dielectric boundary, (c) an ambient
    medium filling the enclosure; each with an isotropic phase function and with Henyey-Greenstein g = 0.6."""
    out = {}
    for tag, phase, g in (("iso", "iso", 0.0), ("hg", "hg", 0.6)):
        dense = medium(sigma_a=_SA, sigma_s=_SS, density=1.5, phase=phase, g=g)
        thin = medium(sigma_a=_SA, sigma_s=_SS, density=0.15, phase=phase, g=g)
        out[f"a_{tag}"] = SphereScene([sphere((0, 0, 0), 1.0, medium=0), sphere(**_LIGHT), sphere(**_SHELL)], [dense],
                                      None, _ORIGIN, _DIR)
        out[f"b_{tag}"] = SphereScene([sphere((0, 0, 0), 1.0, bsdf="dielectric", medium=0), sphere(**_LIGHT),
                                       sphere(**_SHELL)], [dense], None, _ORIGIN, _DIR)
        out[f"c_{tag}"] = SphereScene([sphere(**_LIGHT), sphere(**_SHELL)], [thin], 0, _ORIGIN, _DIR)
    return out
