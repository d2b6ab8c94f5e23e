"""numpy restatements of the reference's photon mapper pieces, for tests/test_photon_host.py and
tests/test_gpu_photon.py, in the style of emitter_refs.py: every function takes the float type T its arithmetic runs in
(F32: the device's precision; F64: the reference value), on float32 inputs.

Restated from:
  tables                src/utils/photon.cpp:30-41 (PhotonData::initialize), transcendentals in fp64 rounded once
  encode / decode       src/utils/photon.cpp:43-74, include/nori/photon.h:44-55 (float32 only: the codec is integer-valued)
  auto_radius           src/integrators/photonmapper.cpp:75-76
  cosine_hemisphere     src/utils/warp.cpp:48-52, :111-122
  frame_of              src/utils/common.cpp:292-306 (coordinateSystem), include/nori/frame.h
  sample_photon         src/emitters/arealight.cpp:127-144 on emitter_refs.mesh_sample / sphere_sample, with the
                        photon pass's `* scene->getLights().size()` (photonmapper.cpp:91)
  in_radius / gather    the acceptance test of PointKDTree::search as PhotonMapper::Li uses it: (photon.p -
                        p).squaredNorm() < r * r, strict, Eigen's grouping; brute force over the whole map
  photon_mc             src/integrators/photonmapper.cpp:61-270 as an fp64 Monte-Carlo estimator on sphere scenes
                        (second part of this file), the source of tests/golden/photon_mc.json
  materialize           writes the reference's own photon mapper scenes from tests/golden
"""
from __future__ import annotations

import os

import numpy as np

import emitter_refs as er
from emitter_refs import F32, F64, dot, normalized, pi

INT_MIN = -(1 << 31)


def tables() -> dict:
    """PhotonData's tables with cos / sin evaluated in fp64 on the float32 arguments and rounded once."""
    i = np.arange(256)
    angle = i.astype(F32) * (pi(F32) / F32(256))
    two = F32(2) * angle
    t = {"cos_phi": np.cos(two.astype(F64)).astype(F32), "sin_phi": np.sin(two.astype(F64)).astype(F32),
         "cos_theta": np.cos(angle.astype(F64)).astype(F32), "sin_theta": np.sin(angle.astype(F64)).astype(F32),
         "exp": np.ldexp(F32(1), i - (128 + 8)).astype(F32)}
    t["exp"][0] = 0
    return t


def f2i(x):
    """int(float) / the first step of uint8_t(float) as x86-64 executes them (cvttss2si to 32 bits): truncation,
    INT_MIN out of range or for NaN"""
    x = np.asarray(x, F64)
    ok = np.isfinite(x) & (np.abs(x) < 2.0 ** 31)
    return np.where(ok, np.trunc(np.where(ok, x, 0.0)), float(INT_MIN)).astype(np.int64)


def encode(direction, power) -> np.ndarray:
    """PhotonData's constructor in float32: (n, 6) uint8 = theta, phi, rgbe[0..3]"""
    d, w = np.asarray(direction, F32).reshape(-1, 3), np.asarray(power, F32).reshape(-1, 3)
    with np.errstate(invalid="ignore", divide="ignore", over="ignore"):
        acos = np.arccos(d[:, 2].astype(F64)).astype(F32)
        theta = np.minimum(255, f2i(acos * (F32(256) / pi(F32)))) & 0xFF
        atan = np.arctan2(d[:, 1].astype(F64), d[:, 0].astype(F64)).astype(F32)
        tmp = np.minimum(255, f2i(atan * (F32(256) / (F32(2) * pi(F32)))))
        phi = np.where(tmp < 0, tmp + 256, tmp) & 0xFF
        mx = np.maximum(w[:, 0], np.maximum(w[:, 1], w[:, 2]))
        zero = mx.astype(F64) < 1e-32
        m, e = np.frexp(mx)
        scale = (m.astype(F32) * F32(256) / mx).astype(F32)
        rgb = [f2i((w[:, k] * scale).astype(F32)) & 0xFF for k in range(3)]
        ex = (e.astype(np.int64) + 128) & 0xFF
    out = np.stack([theta, phi, rgb[0], rgb[1], rgb[2], ex], -1)
    out[zero, 2:] = 0
    return out.astype(np.uint8)


def decode(bytes6, tab: dict) -> tuple:
    """getDirection / getPower of (n, 6) bytes through the tables `tab` (float32): (direction, power)"""
    b = np.asarray(bytes6, np.uint8).reshape(-1, 6).astype(np.int64)
    th, ph = b[:, 0], b[:, 1]
    d = np.stack([tab["cos_phi"][ph] * tab["sin_theta"][th], tab["sin_phi"][ph] * tab["sin_theta"][th],
                  tab["cos_theta"][th]], -1).astype(F32)
    w = (b[:, 2:5].astype(F32) * tab["exp"][b[:, 5]][:, None]).astype(F32)
    return d, w


def auto_radius(bbox_min, bbox_max) -> np.float32:
    e = np.asarray(bbox_max, F32) - np.asarray(bbox_min, F32)
    return F32(np.sqrt(F32(e[0] * e[0] + F32(e[1] * e[1] + e[2] * e[2]))) / F32(500))


def cosine_hemisphere(sample, T):
    s = np.asarray(sample, F32).astype(T)
    rho = np.sqrt(s[:, 0])
    theta = s[:, 1] * T(2) * pi(T)
    x, y = rho * er._fn(np.cos, T, theta), rho * er._fn(np.sin, T, theta)
    return np.stack([x, y, np.sqrt(T(1) - (x * x + y * y))], -1)


def frame_of(n, T):
    """Frame(n) = (s, t, n) by coordinateSystem"""
    a = np.abs(n[:, 0]) > np.abs(n[:, 1])
    with np.errstate(invalid="ignore", divide="ignore"):
        il_a = T(1) / np.sqrt(n[:, 0] * n[:, 0] + n[:, 2] * n[:, 2])
        il_b = T(1) / np.sqrt(n[:, 1] * n[:, 1] + n[:, 2] * n[:, 2])
    z = np.zeros(len(n), T)
    c = np.where(a[:, None], np.stack([n[:, 2] * il_a, z, -n[:, 0] * il_a], -1),
                 np.stack([z, n[:, 2] * il_b, -n[:, 1] * il_b], -1))
    return np.cross(c, n), c, n


def to_world(fr, v):
    return (v[:, :1] * fr[0] + v[:, 1:2] * fr[1]) + v[:, 2:3] * fr[2]


def _photon(p, n, pdf, radiance, sample2, n_lights, T):
    d = to_world(frame_of(n, T), cosine_hemisphere(sample2, T))
    W = (pi(T) / pdf) * np.asarray(radiance, F32).astype(T) * T(n_lights)
    return {"o": p, "d": d, "W": np.broadcast_to(W, p.shape).copy(), "pdf": np.full(len(p), pdf, T), "n": n}


def sample_photon_mesh(V, N, faces, cdf, pdf_norm, radiance, sample, n_lights, T):
    """samplePhoton of a mesh light; sample (n, 4) = (sample1, sample2)"""
    s = np.asarray(sample, F32).reshape(-1, 4)
    r = er.mesh_sample(V, N, faces, cdf, pdf_norm, radiance, np.zeros((len(s), 3), F32), s[:, :2], T)
    out = _photon(r["o"], r["n"], T(F32(pdf_norm)), radiance, s[:, 2:], n_lights, T)
    out["face"] = r["face"]
    return out


def sample_photon_sphere(center, radius, radiance, sample, n_lights, T):
    s = np.asarray(sample, F32).reshape(-1, 4)
    r = er.sphere_sample(center, radius, radiance, np.zeros((len(s), 3), F32), s[:, :2], T)
    rr = T(F32(radius))
    pdf = T(F64(T(1) / rr) ** 2 * F64(T(0.25) / pi(T)))
    return _photon(r["o"], r["n"], pdf, radiance, s[:, 2:], n_lights, T)


def in_radius(positions, q, radius, T):
    """mask of the photons the gather accepts at point q"""
    dv = np.asarray(positions, F32).astype(T) - np.asarray(q, F32).astype(T)
    r = T(F32(radius))
    return dot(dv, dv) < r * r


def gather(positions, power, points, radius) -> tuple:
    """per point: the float32 count, and the fp64 sum of the (decoded, float32) powers of the photons the fp64 test
    accepts together with the count of that test: (count32, count64, sum64)"""
    c32, c64, s64 = [], [], []
    w = np.asarray(power, F32).astype(F64)
    for q in np.asarray(points, F32).reshape(-1, 3):
        m32 = in_radius(positions, q, radius, F32)
        m64 = in_radius(positions, q, radius, F64)
        c32.append(int(m32.sum()))
        c64.append(int(m64.sum()))
        s64.append(w[m32].sum(0))
    return np.array(c32), np.array(c64), np.array(s64)


# ---------------------------------------------------------------------------------------------------------------------
# PhotonMapper::preprocess + Li on sphere-only scenes, fp64 Monte Carlo (tests/golden/make_photon_fixture.py)
# ---------------------------------------------------------------------------------------------------------------------
# Written from src/integrators/photonmapper.cpp:61-270, src/emitters/arealight.cpp:127-144, src/shapes/sphere.cpp,
# src/bsdf/diffuse.cpp and dielectric.cpp, on volume_refs.SphereScene (its intersect and frame are the sphere's
# rayIntersect and setHitInformation). One sample = one photon map and one camera path along the scene's camera ray,
# as one render of one pixel sample is. quirks=False replaces the photon pass's `* lights.size()` by the reciprocal of
# the probability the light was chosen with; with equal light weights the two agree.
import volume_refs as vr  # noqa: E402

_PI = vr._PI
_EPS = vr._EPS


def _bsdf_sample(S, k, wi_l, u2):
    """Diffuse::sample / Dielectric::sample for hit shapes k: (wo local, weight (m, 3))"""
    m = len(k)
    wl, col = np.zeros((m, 3)), np.zeros((m, 3))
    dif = S.bsdf[k] == 0
    up = wi_l[:, 2] > 0
    rho, th = np.sqrt(u2[:, 0]), 2 * _PI * u2[:, 1]
    x, y = rho * np.cos(th), rho * np.sin(th)
    w_d = np.stack([x, y, np.sqrt(np.maximum(1 - (x * x + y * y), 0))], -1)
    wl = np.where((dif & up)[:, None], w_d, wl)
    col = np.where((dif & up)[:, None], S.albedo[k], col)
    die = S.bsdf[k] == 2
    if die.any():
        ci = wi_l[:, 2]
        F = vr._fresnel(ci, S.ext_ior[k], S.int_ior[k])
        refl = u2[:, 0] < F
        nz = np.where(ci < 0, -1.0, 1.0)
        eta = np.where(ci < 0, S.int_ior[k] / S.ext_ior[k], S.ext_ior[k] / S.int_ior[k])
        dn = ci * nz
        nvec = np.stack([np.zeros(m), np.zeros(m), nz], -1)
        with np.errstate(invalid="ignore"):
            wt = -eta[:, None] * (wi_l - dn[:, None] * nvec) - np.sqrt(1 - eta * eta * (1 - dn * dn))[:, None] * nvec
        w_r = np.stack([-wi_l[:, 0], -wi_l[:, 1], wi_l[:, 2]], -1)
        wl = np.where(die[:, None], np.where(refl[:, None], w_r, wt), wl)
        col = np.where(die[:, None], np.where(refl, 1.0, 1 / eta / eta)[:, None], col)
    return wl, col


def _photon_batch(S, weights, n, rng, quirks):
    """n photon paths (photonmapper.cpp:88-148): every deposit as (path, bounce, position, -d, W)"""
    lights = np.asarray(S.lights)
    p_sel = np.asarray(weights, F64) / np.sum(weights)
    li = rng.choice(len(lights), n, p=p_sel)
    lk = lights[li]
    u = rng.random((n, 4))
    z = 2 * u[:, 0] - 1
    r = np.sqrt(np.maximum(1 - z * z, 0))
    q = normalized(np.stack([r * np.cos(2 * _PI * u[:, 1]), r * np.sin(2 * _PI * u[:, 1]), z], -1))
    o = S.c[lk] + S.r[lk][:, None] * q
    rho, th = np.sqrt(u[:, 2]), 2 * _PI * u[:, 3]
    x, y = rho * np.cos(th), rho * np.sin(th)
    d = vr._to_world(vr._frame_of(q), np.stack([x, y, np.sqrt(np.maximum(1 - (x * x + y * y), 0))], -1))
    pdf = (1.0 / S.r[lk]) ** 2 * (0.25 / _PI)
    factor = np.full(n, float(len(lights))) if quirks else 1.0 / p_sel[li]
    W = (_PI / pdf)[:, None] * S.radiance[lk] * factor[:, None]
    ids = np.arange(n)
    out = []
    bounce = 0
    while len(ids):
        assert bounce < 4000
        hit, t, k = S.intersect(o, d, np.full(len(ids), _EPS), np.full(len(ids), np.inf))
        ids, o, d, W, t, k = (a[hit] for a in (ids, o, d, W, t, k))
        if not len(ids):
            break
        p = o + t[:, None] * d
        fr = S.frame(p, k)
        dif = S.bsdf[k] == 0
        out.append((ids[dif], np.full(dif.sum(), bounce), p[dif], -d[dif], W[dif]))
        if bounce >= 3:
            succ = np.minimum(W.max(-1), 0.99)
            keep = ~(rng.random(len(ids)) > succ)
            W = W / succ[:, None]
            ids, o, d, W, p, k = (a[keep] for a in (ids, o, d, W, p, k))
            fr = tuple(f[keep] for f in fr)
        wl, col = _bsdf_sample(S, k, vr._to_local(fr, -d), rng.random((len(ids), 2)))
        keep = ~np.all(np.abs(col) <= _EPS, -1)
        nd = vr._to_world(fr, wl)
        ids, o, d, W = ids[keep], p[keep], nd[keep], (W * col)[keep]
        bounce += 1
    return [np.concatenate([b[j] for b in out]) for j in range(5)]


def photon_mc_sample(S, weights, n_photons, radius, rng, quirks=True, batch=2048) -> tuple:
    """One sample of the estimator: (Li (3,), photons inside the gather ball or -1 if the camera path gathered nothing)"""
    # ---- the camera path (photonmapper.cpp:173-267) up to its first diffuse hit ----
    li, thr = np.zeros(3), np.ones(3)
    o, d = S.origin[None].copy(), S.direction[None].copy()
    x = None
    for bounce in range(4000):
        hit, t, k = S.intersect(o, d, np.full(1, _EPS), np.full(1, np.inf))
        if not hit[0]:
            return li, -1
        p = o + t[:, None] * d
        fr = S.frame(p, k)
        if S.emitter[k[0]] and dot(fr[2], -normalized(p - o))[0] >= 0:
            li = li + thr * S.radiance[k[0]]
        wi_l = vr._to_local(fr, -d)
        if S.bsdf[k[0]] == 0:
            x = (p[0], tuple(f[0] for f in fr), wi_l[0], S.albedo[k[0]])
            break
        if bounce >= 3:
            succ = min(thr.max(), 0.99)
            if rng.random() > succ:
                return li, -1
            thr = thr / succ
        wl, col = _bsdf_sample(S, k, wi_l, rng.random((1, 2)))
        if np.all(np.abs(col[0]) <= _EPS):
            return li, -1
        thr = thr * col[0]
        o, d = p, vr._to_world(fr, wl)
    # ---- the photon pass, until the map is full; E counts the path that fills it ----
    deps, total, k0 = [], 0, 0
    while total < n_photons:
        b = _photon_batch(S, weights, batch, rng, quirks)
        b[0] = b[0] + k0
        deps.append(b)
        total += len(b[0])
        k0 += batch
    path, bnc, pos, pdir, W = (np.concatenate([b[j] for b in deps]) for j in range(5))
    order = np.lexsort((bnc, path))[:n_photons]
    emitted = int(path[order[-1]]) + 1
    pos, pdir, W = pos[order], pdir[order], W[order]
    # ---- the gather (photonmapper.cpp:204-236), through PhotonData's bytes ----
    px, frx, wix, alb = x
    dv = pos - px
    near = dot(dv, dv) < float(F32(radius)) ** 2
    if not near.any():
        return li, 0
    dd, ww = decode(encode(pdir[near], W[near]), tables())
    wo_z = dd.astype(F64) @ frx[2]
    ok = (wo_z > 0) & (wix[2] > 0)
    pc = (ww.astype(F64)[ok] * (alb / _PI)).sum(0) / (_PI * float(F32(radius)) ** 2)
    return li + thr * pc / emitted, int(near.sum())


def photon_mc(S, weights, n_photons, radius, n_samples, seed, quirks=True) -> dict:
    rng = np.random.default_rng(seed)
    v = [photon_mc_sample(S, weights, n_photons, radius, rng, quirks) for _ in range(n_samples)]
    return {"luminance": [float(er.luminance(np.asarray(a, F64), F64)) for a, _ in v],
            "mean_photons_in_ball": float(np.mean([c for _, c in v if c >= 0]))}


def photon_scene_xml(S, weights, n_photons, radius, size=8) -> str:
    """volume_refs.scene_xml with the photon mapper and the lights' lightWeight"""
    text = vr.scene_xml(S, "photonmapper", size=size, spp=1)
    text = text.replace('<integrator type="photonmapper"/>',
                        f'<integrator type="photonmapper"><integer name="photonCount" value="{int(n_photons)}"/>'
                        f'<float name="photonRadius" value="{float(F32(radius))!r}"/></integrator>')
    parts = text.split("<emitter type=\"area\">")
    assert len(parts) == len(weights) + 1
    out = parts[0]
    for w, rest in zip(weights, parts[1:]):
        out += f'<emitter type="area"><float name="lightWeight" value="{float(w)!r}"/>' + rest
    return out


PHOTON_MC_FIXTURE = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tests", "golden",
                                 "photon_mc.json")
MC_PHOTONS, MC_RADIUS = 4000, 1.0


def mc_scenes() -> dict:
    """name -> (SphereScene, light weights): a diffuse ball as the floor seen from the side, under (one) one sphere
    light, (two) two sphere lights with lightWeight 1 and 3, the point the camera looks at lit mostly by the first,
    (glass) one light, the floor point seen through a dielectric sphere in front of the camera"""
    floor = vr.sphere((0, -50, 0), 50.0, bsdf="diffuse", albedo=(0.6, 0.5, 0.4))
    a = vr.sphere((0.2, 3.0, 0.1), 0.5, bsdf="diffuse", albedo=(0, 0, 0), radiance=(20, 20, 20))
    b = vr.sphere((14.0, 3.0, 0.0), 0.5, bsdf="diffuse", albedo=(0, 0, 0), radiance=(20, 20, 20))
    glass = vr.sphere((1.5, 1.0, -2.0), 0.4, bsdf="dielectric")
    cam = ((3.0, 2.0, -4.0), (-3.0, -2.0, 4.0))
    return {"one": (vr.SphereScene([floor, a], [], None, *cam), [1.0]),
            "two": (vr.SphereScene([floor, a, b], [], None, *cam), [1.0, 3.0]),
            "glass": (vr.SphereScene([floor, a, glass], [], None, *cam), [1.0])}


# ---------------------------------------------------------------------------------------------------------------------
# the reference's own photon mapper scenes (fixtures)
# ---------------------------------------------------------------------------------------------------------------------
_GOLDEN = os.path.dirname(PHOTON_MC_FIXTURE)
CBOX_PMAP, TABLE_PMAP = "scenes/pa4/cbox/cbox_pmap.xml", "scenes/pa4/table/table_pmap.xml"


def materialize(out_dir: str) -> str:
    """scenes/pa4/cbox/cbox_pmap.xml (photon_scenes.json; its meshes are those of reference_scenes.json, which
    scenegen.materialize writes) and scenes/pa4/table/table_pmap.xml with its meshes (photon_table.json.gz) under
    out_dir; files already there are left alone. Returns out_dir."""
    import gzip
    import json
    import scenegen
    if not os.path.exists(os.path.join(out_dir, "scenes/pa4/cbox/meshes/walls.obj")):
        scenegen.materialize(out_dir)
    with open(os.path.join(_GOLDEN, "photon_scenes.json")) as f:
        files = json.load(f)
    with gzip.open(os.path.join(_GOLDEN, "photon_table.json.gz"), "rt") as f:
        files.update(json.load(f))
    for rel, text in files.items():
        p = os.path.join(out_dir, rel)
        if not os.path.exists(p):
            os.makedirs(os.path.dirname(p), exist_ok=True)
            with open(p, "w") as g:
                g.write(text)
    return out_dir
