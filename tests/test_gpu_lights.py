"""Spot and directional lights on the HIP path (spotlight.cpp, directionalLight.cpp, warp.cpp:58-72), and nh_emitter_query.

1. nh_emitter_query -- the emitter_sample / emitter_eval / emitter_pdf device functions the integrators call -- against
   an fp64 numpy restatement of the reference's formulas, for all emitter types the tests can build without the oracle:
   spot, directional, point and area (a mesh).
2. A spot with totalwidth = 360, falloffstart = 180 is a point light of the same power: the GPU render of the Cornell
   box with that spot against the oracle's render of the box with the point light, per pixel, four integrators.
3. Exact structure: pixels outside the cone or in the umbra are exactly 0, lit ones > 0, for a spot and for an oblique
   directional light (whose umbra lies on the side the light travels towards).
4. Closed forms under direct_ems with a box filter: a directional light straight down on a diffuse floor gives
   albedo * L * sin^2(angle); a spot with its smooth falloff active gives the restatement's average over the pixel.
5. Plumbing on the reference's own spot.xml and the cut-down validation scenes, and the kernel choice: a scene that
   would take the diffuse area-light bounce kernels but for one spot takes the general ones.
"""
import os

import numpy as np
import pytest

import light_scenes
import nori_hip as nh
import scenegen

F32, F64 = np.float32, np.float64
EPS = 1e-4  # Nori's Epsilon
EPS32 = float(np.finfo(np.float32).eps)


# ---------------------------------------------------------------------------------------------------------------------
# The restatement. Every function takes the float type T the arithmetic runs in: F64 is the reference value, F32 the
# same formulas at the device's precision (the gap between the two is the float evaluation error the bounds allow for).
# Inputs (scene properties, ref points, samples) are float32 values in both runs. M_PI is Nori's float constant.
# ---------------------------------------------------------------------------------------------------------------------
def _pi(T):
    return T(F32(3.14159265358979323846))


def _cos(x, T):
    return np.cos(np.asarray(x, F64)).astype(T)


def _sin(x, T):
    return np.sin(np.asarray(x, F64)).astype(T)


def _deg_to_rad(v, T):  # common.h:218
    return T(v) * (_pi(T) / T(180.0))


def _dot(a, b):  # Eigen's grouping of a 3-vector dot product
    return a[..., 0] * b[..., 0] + (a[..., 1] * b[..., 1] + a[..., 2] * b[..., 2])


def _normalized(v):
    n = _dot(v, v)
    return v / np.sqrt(n)[..., None]


def _frame(n, T):  # Frame(n): coordinateSystem (common.cpp:292-306) -> s, t
    if abs(n[0]) > abs(n[1]):
        inv = T(1) / np.sqrt(n[0] * n[0] + n[2] * n[2])
        t = np.array([n[2] * inv, T(0), -n[0] * inv], T)
    else:
        inv = T(1) / np.sqrt(n[1] * n[1] + n[2] * n[2])
        t = np.array([T(0), n[2] * inv, -n[1] * inv], T)
    s = np.array([t[1] * n[2] - t[2] * n[1], t[2] * n[0] - t[0] * n[2], t[0] * n[1] - t[1] * n[0]], T)
    return s, t


def _to_local(s, t, n, v):
    return np.stack([_dot(v, s), _dot(v, t), _dot(v, n)], -1)


class SpotRef:
    """SpotLight (spotlight.cpp:14-23, :50, :53-77, :184-203)"""

    def __init__(self, position, direction, power, falloffstart, totalwidth, T):
        self.T = T
        self.pos = np.asarray(position, F32).astype(T)
        d = _normalized(np.asarray(direction, F32).astype(T))
        self.n = _normalized(d)  # m_coord = Frame(m_direction.normalized())
        self.s, self.t = _frame(self.n, T)
        self.cos_fs = _cos(_deg_to_rad(F32(falloffstart), T), T)
        self.cos_tw = _cos(_deg_to_rad(T(F32(totalwidth)) / T(2), T), T)
        rad = np.asarray(power, F32).astype(T) / T(2) / _pi(T)
        self.i = rad / (T(1) - T(0.5) * (self.cos_tw + self.cos_fs))

    def cos_theta(self, w):
        return _normalized(_to_local(self.s, self.t, self.n, w))[..., 2]

    def falloff(self, w):
        T = self.T
        c = self.cos_theta(w)
        with np.errstate(divide="ignore", invalid="ignore"):
            delta = (c - self.cos_tw) / (self.cos_fs - self.cos_tw)
        smooth = (delta.astype(F64) ** 4).astype(T)  # std::pow(float, int): the double pow
        return np.where(c < self.cos_tw, T(0), np.where(c >= self.cos_fs, T(1), smooth))

    def eval(self, ref, wi):
        dd = ref - self.pos
        return self.i[None, :] * self.falloff(-wi)[:, None] / _dot(dd, dd)[:, None]

    def sample(self, ref):
        T = self.T
        ref = np.asarray(ref, F32).astype(T)
        pr = self.pos - ref
        wi = _normalized(pr)
        return {"value": self.eval(ref, wi), "wi": wi, "pdf": np.ones(len(ref), T), "o": np.broadcast_to(self.pos, ref.shape),
                "d": -wi, "maxt": np.sqrt(_dot(pr, pr)) - T(F32(EPS))}


class DirectionalRef:
    """DirectionalLight (directionalLight.cpp:32-39, :90-138) with Warp::squareToUniformSphereCap(Pdf) (warp.cpp:58-72)"""

    def __init__(self, direction, radiance, angle, T):
        self.T = T
        self.n = _normalized(np.asarray(direction, F32).astype(T))
        self.s, self.t = _frame(self.n, T)
        self.rad = np.asarray(radiance, F32).astype(T)
        self.cos_max = _cos(_deg_to_rad(F32(angle), T), T)

    def pdf(self, wi):
        """-> (pdf, margin): margin = local z - cosThetaMax, whose sign picks the zero branch"""
        T = self.T
        loc = _to_local(self.s, self.t, self.n, -wi)
        with np.errstate(divide="ignore"):
            cap = T(1) / (T(2) * _pi(T) * (T(1) - self.cos_max))
        zero = (np.abs(_dot(loc, loc) - T(1)) < T(F32(EPS))) & (loc[..., 2] <= self.cos_max)
        return np.where(zero, T(0), cap), loc[..., 2] - self.cos_max

    def sample(self, ref, sample):
        T = self.T
        sx, sy = (np.asarray(sample, F32)[:, k].astype(T) for k in (0, 1))
        z = sx * (T(1) - self.cos_max) + self.cos_max
        r = np.sqrt(T(1) - z * z)
        theta = sy * T(2) * _pi(T)
        v = np.stack([r * _cos(theta, T), r * _sin(theta, T), z], -1)
        world = v[:, 0:1] * self.s + v[:, 1:2] * self.t + v[:, 2:3] * self.n
        wi = -_normalized(world)
        pdf, margin = self.pdf(wi)
        with np.errstate(divide="ignore", invalid="ignore"):
            val = np.where((pdf < T(F32(EPS)))[:, None], T(0), self.rad[None, :] / pdf[:, None])
        return {"value": val, "wi": wi, "pdf": pdf, "margin": margin}


def point_sample_ref(position, radiance, ref, T):
    """PointLight::sample (pointlight.cpp:47-78); radiance = power / (4 pi), the loader's fold"""
    pos = np.asarray(position, F32).astype(T)
    ref = np.asarray(ref, F32).astype(T)
    pr = pos - ref
    wi = _normalized(pr)
    dd = ref - pos
    return {"value": np.asarray(radiance, F32).astype(T)[None, :] / _dot(dd, dd)[:, None], "wi": wi,
            "maxt": np.sqrt(_dot(pr, pr)) - T(F32(EPS))}


def area_sample_ref(verts, faces, cdf, pdf_norm, radiance, ref, sample, T):
    """AreaEmitter::sample on a mesh without normals (arealight.cpp:58-125, mesh.cpp:50-71, warp.cpp:162-166,
    dpdf.h). cdf / pdf_norm: the mesh's area DiscretePDF as loaded (float32 data)."""
    V = np.asarray(verts, F32).astype(T)
    ref = np.asarray(ref, F32).astype(T)
    cdf = np.asarray(cdf, F32)
    s = np.asarray(sample, F32)
    idx = np.clip(np.searchsorted(cdf, s[:, 0], side="left") - 1, 0, len(cdf) - 2)  # std::lower_bound - 1, clamped
    c = cdf.astype(T)
    sx = (s[:, 0].astype(T) - c[idx]) / (c[idx + 1] - c[idx])
    su1 = np.sqrt(sx)
    bu, bv = T(1) - su1, s[:, 1].astype(T) * su1
    bw = T(1) - bu - bv
    p0, p1, p2 = (V[np.asarray(faces)[idx, k]] for k in range(3))
    p = bu[:, None] * p0 + bv[:, None] * p1 + bw[:, None] * p2
    n = _normalized(np.cross(p1 - p0, p2 - p0))
    pr = p - ref
    wi = _normalized(pr)
    cosl = _dot(n, -wi)
    pdf = T(F32(pdf_norm)) * _dot(pr, pr) / np.abs(cosl)
    pdf = np.where(cosl < 0, T(0), pdf)
    rad = np.asarray(radiance, F32).astype(T)
    with np.errstate(divide="ignore", invalid="ignore"):
        val = np.where((cosl < 0)[:, None] | (np.abs(pdf) < T(F32(EPS)))[:, None], T(0), rad[None, :] / pdf[:, None])
    return {"value": val, "wi": wi, "pdf": pdf, "p": p, "n": n, "maxt": np.sqrt(_dot(pr, pr)) - T(F32(EPS)), "cosl": cosl}


def rel_gap(a, b):
    """max |a - b| / |b| over the entries where b != 0 (b: the fp64 value)"""
    a, b = np.asarray(a, F64), np.asarray(b, F64)
    m = b != 0
    return float(np.max(np.abs(a[m] - b[m]) / np.abs(b[m]))) if m.any() else 0.0


def abs_gap(a, b):
    return float(np.max(np.abs(np.asarray(a, F64) - np.asarray(b, F64))))


def bound(gap):
    """4 x the restatement's own fp32-vs-fp64 gap on the same inputs, and never below 4 float epsilons: the device
    runs the same formulas in fp32, so its distance to the fp64 value is of the order of that gap."""
    return 4.0 * max(gap, EPS32)


# ---------------------------------------------------------------------------------------------------------------------
# helpers
# ---------------------------------------------------------------------------------------------------------------------
def upload(xml, integrator=None, res=None, spp=None):
    s = nh.Scene(xml)
    if integrator is not None:
        s.set_integrator(integrator)
    if res is not None:
        s.set_resolution(*res)
    if spp is not None:
        s.set_sample_count(spp)
    b = nh.Bvh(s)
    c = nh.Context(0)
    c.upload(s, b)
    return c, s, b


def render_rgb(c, s, s0, s1, seed, mode=nh.MODE_MEGAKERNEL, clear=True, stats=False):
    c.render(s0, s1, seed=seed, clear=clear, mode=mode, traversal=nh.TRAVERSAL_ORDERED, stats=stats)
    fb = c.framebuffer()
    return fb, nh.to_rgb(fb, s.border)


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def cone_points(pos, direction, theta_deg, phi, dist):
    """float32 points at angle theta from the light's axis, at distance dist from pos"""
    n = _normalized(np.asarray(direction, F64))
    s, t = _frame(n, F64)
    th = np.radians(np.asarray(theta_deg, F64))
    w = (np.cos(th)[:, None] * n + np.sin(th)[:, None] * (np.cos(phi)[:, None] * s + np.sin(phi)[:, None] * t))
    return (np.asarray(pos, F64) + np.asarray(dist, F64)[:, None] * w).astype(F32)


SPOT_POS, SPOT_DIR, SPOT_POWER = (-1.5, 4.0, 0.75), (1.0, -2.0, 0.5), (30.0, 20.0, 10.0)


# ---------------------------------------------------------------------------------------------------------------------
# 1. the query against the restatement
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("falloffstart,totalwidth", [(10.0, 60.0), (40.0, 60.0)], ids=["smooth", "hard-edged"])
def test_query_spot(gpu, tmp_path, falloffstart, totalwidth):
    """emitter_sample / emitter_eval / emitter_pdf of a spot light. falloffstart below totalwidth / 2 (10 < 30) reaches
    all three branches of falloff(); above it (40 > 30) the cone is hard-edged like the reference's own scenes.
    Queries keep 1 degree from the branch boundaries, so both precisions take the same branch. Exact: zeros outside
    the cone, pdf == 1, shadow origin == position, direction == -wi, mint == 1e-4f. The rest within bound(gap); on
    these queries the restatement's fp32-vs-fp64 gap is 1.7e-5 (value, smooth: the delta^4 term amplifies the cosine's
    rounding near the rim), 3.5e-7 (value, inside falloffstart), 1.3e-7 (wi, absolute) and 1.4e-7 (maxt)."""
    xml = light_scenes.floor_scene_xml(str(tmp_path / "q.xml"), light_scenes.spot_xml(
        SPOT_POS, SPOT_DIR, SPOT_POWER, falloffstart=falloffstart, totalwidth=totalwidth))
    c, s, b = upload(xml)
    rng = np.random.default_rng(5)
    half = totalwidth / 2
    inner_hi = min(falloffstart, half) - 1.0
    sets = {"inner": rng.uniform(0.0, inner_hi, 96), "outside": rng.uniform(half + 1.0, 179.0, 96)}
    if falloffstart < half:
        sets["smooth"] = rng.uniform(falloffstart + 1.0, half - 1.0, 96)
    for name, theta in sets.items():
        m = len(theta)
        ref = cone_points(SPOT_POS, SPOT_DIR, theta, rng.uniform(0, 2 * np.pi, m), rng.uniform(0.5, 8.0, m))
        r64 = SpotRef(SPOT_POS, SPOT_DIR, SPOT_POWER, falloffstart, totalwidth, F64).sample(ref)
        r32 = SpotRef(SPOT_POS, SPOT_DIR, SPOT_POWER, falloffstart, totalwidth, F32).sample(ref)
        g = c.emitter_query(0, ref, sample=rng.uniform(0, 1, (m, 2)).astype(F32))
        assert np.all(g["pdf"] == 1.0) and np.all(g["mint"] == F32(EPS))
        assert np.array_equal(g["o"], np.broadcast_to(np.asarray(SPOT_POS, F32), (m, 3)))
        assert np.array_equal(bits(g["d"]), bits(-g["wi"]))
        gaps = {k: (abs_gap if k == "wi" else rel_gap)(r32[k], r64[k]) for k in ("value", "wi", "maxt")}
        errs = {k: (abs_gap if k == "wi" else rel_gap)(g[k], r64[k]) for k in ("value", "wi", "maxt")}
        print(f"spot {falloffstart}/{totalwidth} {name}: fp32 gap {gaps}, device {errs}")
        if name == "outside":
            assert np.all(r64["value"] == 0) and np.all(g["value"] == 0)
        else:
            assert np.all(r64["value"][:, 0] > 0)
            if name == "smooth":  # strictly between the two other branches
                f = SpotRef(SPOT_POS, SPOT_DIR, SPOT_POWER, falloffstart, totalwidth, F64).falloff(-r64["wi"])
                assert np.all((f > 0) & (f < 1))
        for k in gaps:
            assert errs[k] <= bound(gaps[k]), (name, k, errs[k], gaps[k])
        # eval and pdf with the sampled wi: the same value (one function), pdf 1
        e = c.emitter_query(0, ref, wi=g["wi"])
        assert np.array_equal(bits(e["value"]), bits(g["value"])) and np.all(e["pdf"] == 1.0)


DIR_DIRECTION, DIR_RADIANCE = (1.0, -2.0, 0.5), (3.0, 2.0, 1.0)


def _directional_samples():
    rng = np.random.default_rng(9)
    top = np.nextafter(F32(1), F32(0))
    corners = np.array([[0, 0], [0, top], [top, 0], [top, top]], F32)
    inner = np.stack([rng.uniform(0.02, 1.0, 124), rng.uniform(0, 1, 124)], -1).astype(F32)
    return np.concatenate([corners, np.minimum(inner, top)])


@pytest.mark.gpu
@pytest.mark.parametrize("angle", [1.0, 2.0, 45.0])
def test_query_directional(gpu, tmp_path, angle):
    """emitter_sample / emitter_eval / emitter_pdf of a directional light, sample corners 0 and 1 - ulp included.
    Exact: shadow origin == ref, direction == +wi, mint == 1e-4f, maxt == inf, eval == radiance for any direction.
    pdf is either 0 (a unit vector with local z <= cosThetaMax, warp.cpp:69) or the cap's constant: where the fp64
    margin z - cosThetaMax is within 8 float epsilons (the sample corner sx = 0, which lands on the rim) either
    branch is right and the device must give one of the two exactly as a pair (pdf, value); elsewhere the fp64 branch.
    The rest within bound(gap): the restatement's fp32-vs-fp64 gap here is, for angle = 1 / 2 / 45 degrees,
    9.8e-5 / 2.2e-5 / 1.1e-7 on pdf and value (1 - cosThetaMax cancels: 1.5e-4 for one degree, against a float's 6e-8)
    and 1.8e-5 / 7.7e-6 / 1.7e-4 on wi (absolute; sqrt(1 - z^2) cancels the same way, worst at the sx = 1 - ulp
    corner, where z is one ulp from 1)."""
    xml = light_scenes.floor_scene_xml(str(tmp_path / "q.xml"), light_scenes.directional_xml(
        DIR_DIRECTION, DIR_RADIANCE, angle))
    c, s, b = upload(xml)
    smp = _directional_samples()
    m = len(smp)
    ref = np.random.default_rng(2).uniform(-3, 3, (m, 3)).astype(F32)
    r64 = DirectionalRef(DIR_DIRECTION, DIR_RADIANCE, angle, F64).sample(ref, smp)
    r32 = DirectionalRef(DIR_DIRECTION, DIR_RADIANCE, angle, F32).sample(ref, smp)
    g = c.emitter_query(0, ref, sample=smp)
    assert np.array_equal(bits(g["o"]), bits(ref)) and np.array_equal(bits(g["d"]), bits(g["wi"]))
    assert np.all(g["mint"] == F32(EPS)) and np.all(np.isposinf(g["maxt"]))
    assert np.all(np.isfinite(g["value"])) and np.all(np.isfinite(g["pdf"])) and np.all(np.isfinite(g["wi"]))
    rim = np.abs(r64["margin"]) < 8 * EPS32
    assert rim[:2].all() and not rim[2:].any()  # exactly the two sx = 0 corners
    cap = float(r64["pdf"].max())
    clear = ~rim
    assert np.all(r64["pdf"][clear] == cap) and np.all(r32["pdf"][clear] > 0)
    gaps = {"pdf": rel_gap(r32["pdf"][clear], r64["pdf"][clear]), "value": rel_gap(r32["value"][clear], r64["value"][clear]),
            "wi": abs_gap(r32["wi"], r64["wi"])}
    errs = {"pdf": rel_gap(g["pdf"][clear], r64["pdf"][clear]), "value": rel_gap(g["value"][clear], r64["value"][clear]),
            "wi": abs_gap(g["wi"], r64["wi"])}
    print(f"directional {angle}: fp32 gap {gaps}, device {errs}")
    for k in gaps:
        assert errs[k] <= bound(gaps[k]), (k, errs[k], gaps[k])
    for i in np.nonzero(rim)[0]:  # on the rim: (0, 0) or (cap, radiance / cap), nothing in between
        if g["pdf"][i] == 0:
            assert np.all(g["value"][i] == 0)
        else:
            assert abs(g["pdf"][i] / cap - 1) <= bound(gaps["pdf"])
            assert rel_gap(g["value"][i], np.asarray(DIR_RADIANCE, F64) / cap) <= bound(gaps["value"])
    # pdf of the sampled wi through emitter_pdf: the sample's own pdf; eval: the radiance, for any direction
    e = c.emitter_query(0, ref, wi=g["wi"])
    assert np.array_equal(bits(e["pdf"]), bits(g["pdf"]))
    anyw = _normalized(np.random.default_rng(4).normal(size=(m, 3))).astype(F32)
    assert np.array_equal(c.emitter_query(0, ref, wi=anyw, mode=nh.EMITTER_QUERY_EVAL)["value"],
                          np.broadcast_to(np.asarray(DIR_RADIANCE, F32), (m, 3)))


@pytest.mark.gpu
@pytest.mark.parametrize("direction", [(0.0, 0.0, -1.0), DIR_DIRECTION], ids=["axis", "oblique"])
def test_query_directional_angle_zero_contributes_nothing(gpu, tmp_path, direction):
    """angle = 0: 1 - cosThetaMax is 0 and the sampled direction is the axis itself. Along a coordinate axis the local z
    is exactly 1 <= cosThetaMax, so pdf == 0 and the sample is 0 (directionalLight.cpp:99-102). For an oblique
    direction n . n may round above 1, and then the reference divides the radiance by 1 / 0 = inf: also exactly 0.
    Either way no NaN and no light."""
    xml = light_scenes.floor_scene_xml(str(tmp_path / "q.xml"), light_scenes.directional_xml(direction, DIR_RADIANCE, 0.0))
    c, s, b = upload(xml)
    smp = _directional_samples()
    ref = np.random.default_rng(3).uniform(-3, 3, (len(smp), 3)).astype(F32)
    g = c.emitter_query(0, ref, sample=smp)
    assert np.all(g["value"] == 0) and not np.isnan(g["pdf"]).any() and not np.isnan(g["wi"]).any()
    assert np.all((g["pdf"] == 0) | np.isposinf(g["pdf"]))
    if direction == (0.0, 0.0, -1.0):
        assert np.all(g["pdf"] == 0)
        np.testing.assert_array_equal(g["wi"], np.broadcast_to(np.array([0, 0, 1], F32), g["wi"].shape))
    assert np.all(np.isposinf(g["maxt"])) and np.array_equal(bits(g["o"]), bits(ref))
    _, rgb = render_rgb(c, s, 0, 4, 1)
    assert np.all(rgb == 0)


AREA_QUAD = [(-0.5, 3.0, -0.25), (-0.5, 3.0, 0.75), (1.0, 3.0, 0.75), (1.0, 3.0, -0.25)]  # faces down (normal -y)


def _area_scene(path):
    d = os.path.dirname(path)
    light_scenes.quad_obj(os.path.join(d, "area_light.obj"), AREA_QUAD[::-1])
    em = ('<shape type="obj"><string name="filename" value="area_light.obj"/>'
          '<emitter type="area"><color name="radiance" value="5, 4, 3"/></emitter></shape>'
          + light_scenes.point_xml((1.0, 2.0, -0.5), (7.0, 8.0, 9.0)))
    return light_scenes.floor_scene_xml(path, em)


@pytest.mark.gpu
def test_query_point_and_area(gpu, tmp_path):
    """The query on the two older analytic / sampled emitters, pinned to the same kind of restatement, so that it
    stands for the shared emitter functions. Point: value = power / (4 pi) / d^2, pdf 1, shadow ray from the light.
    Area (a two-triangle mesh): face by the area CDF, squareToUniformTriangle, pdf = pdfSurface d^2 / |cos|, zero from
    behind. fp32-vs-fp64 gap of the restatement: 3.1e-7 (point value), 3.1e-7 / 2.8e-7 (area value / pdf), 1.1e-7 (wi),
    1.4e-7 (maxt)."""
    c, s, b = upload(_area_scene(str(tmp_path / "a.xml")))
    d = s.desc
    assert [d.emitters[i].type for i in range(2)] == [nh.EMITTER_AREA, nh.EMITTER_POINT]
    rng = np.random.default_rng(8)
    m = 128
    ref = rng.uniform(-3, 3, (m, 3))
    ref[:, 1] = np.concatenate([rng.uniform(-3, 2, m - 16), rng.uniform(4, 9, 16)])  # below the area light / above it
    ref = ref.astype(F32)
    smp = rng.uniform(0, 1, (m, 2)).astype(F32)
    # point
    g = c.emitter_query(1, ref, sample=smp)
    rad = [d.emitters[1].radiance[k] for k in range(3)]
    r64, r32 = (point_sample_ref((1.0, 2.0, -0.5), rad, ref, T) for T in (F64, F32))
    assert np.all(g["pdf"] == 1.0) and np.all(g["mint"] == F32(EPS))
    assert np.array_equal(g["o"], np.broadcast_to(np.array([1.0, 2.0, -0.5], F32), (m, 3)))
    assert np.array_equal(bits(g["d"]), bits(-g["wi"]))
    for k, fn in (("value", rel_gap), ("wi", abs_gap), ("maxt", rel_gap)):
        gap, err = fn(r32[k], r64[k]), fn(g[k], r64[k])
        print(f"point {k}: fp32 gap {gap:.3g}, device {err:.3g}")
        assert err <= bound(gap), (k, err, gap)
    # area: the emitting mesh is the second shape
    sh = d.shapes[d.emitters[0].shape]
    V = np.array([[d.V[3 * (sh.v_offset + i) + k] for k in range(3)] for i in range(sh.n_vertices)], F32)
    Fc = np.array([[d.F[3 * (sh.f_offset + i) + k] for k in range(3)] for i in range(sh.n_faces)])
    cdf = np.array([d.area_cdf[sh.pdf_offset + i] for i in range(sh.n_faces + 1)], F32)
    rad = [d.emitters[0].radiance[k] for k in range(3)]
    a64, a32 = (area_sample_ref(V, Fc, cdf, sh.pdf_normalization, rad, ref, smp, T) for T in (F64, F32))
    g = c.emitter_query(0, ref, sample=smp)
    front = a64["cosl"] > 1e-3
    behind = a64["cosl"] < -1e-3
    assert front.sum() > 64 and behind.sum() >= 8 and (front | behind).all()
    assert np.all(g["value"][behind] == 0) and np.all(g["pdf"][behind] == 0)
    assert np.all(g["mint"] == F32(EPS)) and np.array_equal(bits(g["d"]), bits(-g["wi"]))
    for k, fn in (("value", rel_gap), ("pdf", rel_gap), ("wi", abs_gap), ("maxt", rel_gap)):
        sel = slice(None) if k in ("wi", "maxt") else front
        gap, err = fn(a32[k][sel], a64[k][sel]), fn(g[k][sel], a64[k][sel])
        print(f"area {k}: fp32 gap {gap:.3g}, device {err:.3g}")
        assert err <= bound(gap), (k, err, gap)
    assert abs_gap(g["o"], a64["p"]) <= bound(abs_gap(a32["p"], a64["p"]))
    # eval / pdf at the sampled point: radiance from the front, the same pdf
    e = c.emitter_query(0, ref, wi=g["wi"], p=g["o"], n=a32["n"])
    assert np.array_equal(e["value"][front], np.broadcast_to(np.asarray(rad, F32), (int(front.sum()), 3)))
    assert np.all(e["value"][behind] == 0)
    assert rel_gap(e["pdf"][front], a64["pdf"][front]) <= bound(rel_gap(a32["pdf"][front], a64["pdf"][front]))


@pytest.mark.gpu
def test_query_and_upload_refuse_bad_input(gpu, tmp_path):
    xml = light_scenes.floor_scene_xml(str(tmp_path / "q.xml"), light_scenes.directional_xml((0, -1, 0), (1, 1, 1), 5.0))
    c, s, b = upload(xml)
    ref = np.zeros((2, 3), F32)
    with pytest.raises(nh.NoriError, match="out of range"):
        c.emitter_query(1, ref, sample=np.zeros((2, 2), F32))
    with pytest.raises(nh.NoriError, match=r"outside \[0, 1\)"):
        c.emitter_query(0, ref, sample=np.ones((2, 2), F32))
    import ctypes as C
    d = s.desc
    ext = (nh.nh_emitter_ext * 1)()
    C.memmove(ext, d.emitter_ext, C.sizeof(nh.nh_emitter_ext))
    em = (nh.nh_emitter * 1)()
    C.memmove(em, d.emitters, C.sizeof(nh.nh_emitter))
    d.emitters, d.emitter_ext = em, ext
    c2 = nh.Context(0)

    def rc():
        return nh.lib.nh_upload_scene(c2._h, C.byref(d))
    assert rc() == nh.NH_OK
    d.emitter_ext = None
    assert rc() == 1 and b"emitter_ext" in nh.lib.nh_last_error(c2._h)  # NH_ERR_INVALID
    d.emitter_ext = ext
    for bad in ((0.0, 0.0, 0.0), (float("nan"), 0.0, 1.0), (float("inf"), 0.0, 0.0)):
        for k in range(3):
            ext[0].direction[k] = bad[k]
        assert rc() == 1 and b"direction" in nh.lib.nh_last_error(c2._h)
    ext[0].direction[0], ext[0].direction[1], ext[0].direction[2] = 0.0, -1.0, 0.0
    for t in (-1, 5, 99):
        em[0].type = t
        assert rc() == 1 and b"unknown emitter type" in nh.lib.nh_last_error(c2._h)
    em[0].type = nh.EMITTER_DIRECTIONAL
    assert rc() == nh.NH_OK


# ---------------------------------------------------------------------------------------------------------------------
# 2. spot == point light, against the oracle
# ---------------------------------------------------------------------------------------------------------------------
CBOX_LIGHT_POS, CBOX_LIGHT_POWER = (0.3, 1.2, 0.4), (30.0, 25.0, 20.0)


@pytest.mark.gpu
@pytest.mark.parametrize("integrator", [nh.INTEGRATOR_DIRECT, nh.INTEGRATOR_DIRECT_EMS, nh.INTEGRATOR_DIRECT_MIS,
                                        nh.INTEGRATOR_PATH_MIS], ids=["direct", "direct_ems", "direct_mis", "path_mis"])
def test_full_sphere_spot_is_the_point_light(gpu, scene_dir, integrator):
    """totalwidth = 360, falloffstart = 180: cosTotalWidth = cosFalloffStart = cos(degToRad(180.f)) = -1 exactly in
    float (tests/test_lights_host.py), so I = power / (4 pi) and falloff == 1: the point light of that power. The GPU
    renders the Cornell box (area light, mirror and dielectric spheres) with the spot; the oracle, which has no spot,
    renders it with the point light, at matched per-path seeds. Per pixel, on the normalized RGB:
    max |g - r| / max(|r|, 1e-6) < 1e-4. This ties the spot's shadow ray, the picked light's 1 / n MIS pdf and the
    Russian roulette around it to the oracle."""
    import nori_oracle as no
    spot = light_scenes.spot_xml(CBOX_LIGHT_POS, (0.2, -1.0, 0.1), CBOX_LIGHT_POWER, falloffstart=180, totalwidth=360)
    point = light_scenes.point_xml(CBOX_LIGHT_POS, CBOX_LIGHT_POWER)
    c, s, b = upload(scenegen.cbox_xml(scene_dir, "c1", 48, 48, 8, extra_shapes=spot), integrator)
    sp = nh.Scene(scenegen.cbox_xml(scene_dir, "c1", 48, 48, 8, extra_shapes=point))
    sp.set_integrator(integrator)
    ds, dp = s.desc, sp.desc
    assert ds.emitters[1].type == nh.EMITTER_SPOT and dp.emitters[1].type == nh.EMITTER_POINT
    assert list(ds.emitters[1].radiance) == list(dp.emitters[1].radiance)  # the folded intensity, bit for bit
    ref_fb = no.OracleScene(sp).render(0, 8, seed=3)
    r = nh.to_rgb(ref_fb, sp.border).astype(F64)
    for mode in (nh.MODE_MEGAKERNEL, nh.MODE_WAVEFRONT):
        _, g = render_rgb(c, s, 0, 8, 3, mode)
        err = float(np.max(np.abs(g.astype(F64) - r) / np.maximum(np.abs(r), 1e-6)))
        print(f"integrator {integrator} mode {mode}: per-pixel error {err:.3e}")
        assert err < 1e-4, (mode, err)
    # the point light does light the box: the image differs from the one without it
    s0 = nh.Scene(scenegen.cbox_xml(scene_dir, "c1", 48, 48, 8))
    s0.set_integrator(integrator)
    r0 = nh.to_rgb(no.OracleScene(s0).render(0, 8, seed=3), s0.border)
    assert float(np.mean(r)) > 1.05 * float(np.mean(r0))


# ---------------------------------------------------------------------------------------------------------------------
# camera geometry of the floor scenes (PerspectiveCamera::sampleRay, perspective.cpp:98-135, pinhole)
# ---------------------------------------------------------------------------------------------------------------------
def camera_rays(s, sub, midpoint=False):
    """Rays through a sub x sub grid of sample positions in every pixel -- spanning the cell, corners included (to
    classify a pixel), or the midpoints of sub x sub equal sub-cells (to average over it): (H, W, sub, sub, 3) origins
    and unit directions in fp64"""
    cam = s.desc.camera
    s2c = np.array(cam.sample_to_camera[:], F64).reshape(4, 4)
    c2w = np.array(cam.camera_to_world[:], F64).reshape(4, 4)
    W, H = cam.width, cam.height
    t = (np.arange(sub) + 0.5) / sub if midpoint else np.linspace(0.0, 1.0, sub)
    x = (np.arange(W)[None, :, None, None] + t[None, None, None, :]) * cam.inv_output_size[0]
    y = (np.arange(H)[:, None, None, None] + t[None, None, :, None]) * cam.inv_output_size[1]
    x, y = np.broadcast_arrays(x, y)
    q = np.stack([x, y, np.zeros_like(x), np.ones_like(x)], -1) @ s2c.T
    near = q[..., :3] / q[..., 3:4]
    d = (near / np.linalg.norm(near, axis=-1, keepdims=True)) @ c2w[:3, :3].T
    o = np.broadcast_to(c2w[:3, 3], d.shape)
    return o, d


def floor_points(s, sub, midpoint=False):
    o, d = camera_rays(s, sub, midpoint)
    t = -o[..., 1] / d[..., 1]
    return o + t[..., None] * d, o, d


def in_square(p, centre, h, grow):
    """x / z within the square of half-width h + grow about centre"""
    return (np.abs(p[..., 0] - centre[0]) <= h + grow) & (np.abs(p[..., 2] - centre[2]) <= h + grow)


def at_height(a, b, y):
    """the point of the line a -> b at height y"""
    t = (y - a[..., 1]) / (b[..., 1] - a[..., 1])
    return a + t[..., None] * (b - a)


OCC = (-1.0, 2.5, 0.0, 0.6)  # occluder: centre, half-width


# ---------------------------------------------------------------------------------------------------------------------
# 3. exact structure
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_spot_cone_and_umbra_are_exact(gpu, tmp_path):
    """A hard-edged spot (totalwidth 40, falloffstart 30) at (-3, 5, 0) aimed at (0.5, 0, 0), a square occluder between
    it and the floor, direct_ems, box filter (a pixel's footprint is its own cell). Each pixel is classified from the
    restatement on a 5 x 5 grid of sample positions spanning its cell, corners included, with geometric margins: 0.5
    degrees on the cone angle (a cell subtends about 2 degrees from the light, the grid steps 0.5) and 0.05 on the
    occluder's edges (a grid step projects to 0.03 there). Pixels whose camera rays pass near the occluder are left
    out. Dark pixels -- wholly outside the cone, or wholly in the umbra -- are exactly 0; lit ones > 0."""
    pos, target = np.array([-3.0, 5.0, 0.0]), np.array([0.5, 0.0, 0.0])
    em = light_scenes.spot_xml(pos, target - pos, (400, 400, 400), falloffstart=30, totalwidth=40)
    c, s, b = upload(light_scenes.floor_scene_xml(str(tmp_path / "s.xml"), em, spp=16, occluder=OCC))
    P, o, d = floor_points(s, 5)
    sees_occluder = in_square(at_height(o, P, OCC[1]), OCC, OCC[3], 0.1).any(axis=(2, 3))
    spot = SpotRef(pos, target - pos, (400, 400, 400), 30, 40, F64)
    theta = np.degrees(np.arccos(np.clip(spot.cos_theta(P - pos), -1, 1)))
    crossing = at_height(P, np.broadcast_to(pos, P.shape), OCC[1])
    outside = (theta > 20.5).all(axis=(2, 3))
    umbra = in_square(crossing, OCC, OCC[3], -0.05).all(axis=(2, 3)) & (theta < 19.5).all(axis=(2, 3))
    lit = (theta < 19.5).all(axis=(2, 3)) & (~in_square(crossing, OCC, OCC[3], 0.05)).all(axis=(2, 3))
    dark = (outside | umbra) & ~sees_occluder
    lit &= ~sees_occluder
    assert outside.sum() > 100 and (umbra & ~sees_occluder).sum() > 20 and lit.sum() > 100
    for mode in (nh.MODE_MEGAKERNEL, nh.MODE_WAVEFRONT):
        _, rgb = render_rgb(c, s, 0, 16, 4, mode)
        assert np.all(rgb[dark] == 0), mode
        assert np.all(rgb[lit] > 0), mode


@pytest.mark.gpu
def test_directional_umbra_lies_downstream(gpu, tmp_path):
    """A directional light of angle = 1 travelling along (1, -1, 0) over a square occluder of half-width 0.9: its
    shadow falls on the +x side, at occluder + (2.5, -2.5, 0), clear of the occluder as the camera sees it. A point is
    in the umbra when every direction of the 1-degree cap is blocked, lit when none is: the central direction's
    crossing of the occluder plane must lie inside the square shrunk, or outside the square grown, by the cap's reach
    there (3.54 tan 1 = 0.062) plus 0.038 of margin. The umbra is exactly 0 (a shadow ray
    flipped towards the floor, or clipped at a finite maxt, would light it), the rest of the floor > 0."""
    direction = np.array([1.0, -1.0, 0.0])
    OCC = (-1.0, 2.5, 0.0, 0.9)
    em = light_scenes.directional_xml(direction, (5, 5, 5), 1.0)
    c, s, b = upload(light_scenes.floor_scene_xml(str(tmp_path / "s.xml"), em, spp=16, occluder=OCC))
    P, o, d = floor_points(s, 5)
    sees_occluder = in_square(at_height(o, P, OCC[1]), OCC, OCC[3], 0.1).any(axis=(2, 3))
    crossing = at_height(P, P - direction, OCC[1])
    umbra = in_square(crossing, OCC, OCC[3], -0.1).all(axis=(2, 3)) & ~sees_occluder
    lit = (~in_square(crossing, OCC, OCC[3], 0.1)).all(axis=(2, 3)) & ~sees_occluder
    assert umbra.sum() > 10 and lit.sum() > 500
    # downstream: the umbra's pixels lie at larger x than the occluder
    assert P[umbra][..., 0].min() > OCC[0] + OCC[3]
    for mode in (nh.MODE_MEGAKERNEL, nh.MODE_WAVEFRONT):
        _, rgb = render_rgb(c, s, 0, 16, 6, mode)
        assert np.all(rgb[umbra] == 0), mode
        assert np.all(rgb[lit] > 0), mode


# ---------------------------------------------------------------------------------------------------------------------
# 4. closed forms. k = 6 standard errors: the pixel mean of 64 bounded, independent samples is close to normal with
# lighter tails, so a pixel exceeds 6 sigma with probability about 2e-9, 2e-6 over the 1024 pixels of an image. A
# float-evaluation allowance of 1e-5 of the expected value is added (the restatement's own fp32-vs-fp64 gap on these
# floor points is at most 1.8e-5 per sample, in the ramp; the smallest bound of any pixel is 2.8e-4 of its value).
# ---------------------------------------------------------------------------------------------------------------------
K_SIGMA, SPP = 6.0, 64
CF_ALBEDO, CF_ANGLE, CF_L = 0.5, 45.0, 2.0


def directional_floor_moments():
    """mean and per-sample deviation of li * cos * f for a directional light straight down on a horizontal diffuse
    floor: li = L * 2 pi (1 - c), f = albedo / pi, cos = z uniform in [c, 1] (squareToUniformSphereCap):
    mean = albedo L (1 - c^2) = albedo L sin^2(angle), sigma = 2 albedo L (1 - c) * (1 - c) / sqrt(12)"""
    cm = np.cos(np.radians(CF_ANGLE))
    return CF_ALBEDO * CF_L * (1 - cm * cm), 2 * CF_ALBEDO * CF_L * (1 - cm) * (1 - cm) / np.sqrt(12.0)


SMOOTH_SPOT = dict(position=(0.0, 9.5, 0.0), direction=(0.0, -1.0, 0.0), power=(300.0, 200.0, 100.0), falloffstart=10.0,
                   totalwidth=60.0)


def spot_floor_value(P, T=F64):
    """li * cos * f of direct_ems at floor points P (normal +y) for SMOOTH_SPOT, albedo CF_ALBEDO"""
    spot = SpotRef(SMOOTH_SPOT["position"], SMOOTH_SPOT["direction"], SMOOTH_SPOT["power"], SMOOTH_SPOT["falloffstart"],
                   SMOOTH_SPOT["totalwidth"], T)
    flat = P.reshape(-1, 3)
    r = spot.sample(flat.astype(F32))
    return (r["value"] * r["wi"][:, 1:2] * (CF_ALBEDO / np.pi)).reshape(P.shape)


def test_closed_form_bounds_hold_for_a_numpy_monte_carlo(tmp_path):
    """The bounds of the two closed-form tests, checked on the restatement alone: numpy Monte-Carlo images with the
    tests' sample count stay inside K_SIGMA * sigma / sqrt(SPP) at every pixel, for several seeds."""
    mean, sigma = directional_floor_moments()
    assert abs(mean - 0.5) < 1e-12
    cm = np.cos(np.radians(CF_ANGLE))
    for seed in range(4):
        rng = np.random.default_rng(seed)
        z = rng.uniform(0, 1, (1024, SPP)) * (1 - cm) + cm
        img = (CF_L * 2 * np.pi * (1 - cm) * z * CF_ALBEDO / np.pi).mean(axis=1)
        assert np.all(np.abs(img - mean) <= K_SIGMA * sigma / np.sqrt(SPP))
    s = nh.Scene(light_scenes.floor_scene_xml(str(tmp_path / "mc.xml"), light_scenes.spot_xml(**SMOOTH_SPOT)))
    P, _, _ = floor_points(s, 32, midpoint=True)
    v = spot_floor_value(P)[..., 0]
    H, W = v.shape[:2]
    exp, sig = v.mean(axis=(2, 3)), v.std(axis=(2, 3))
    cam = s.desc.camera
    for seed in range(4):
        rng = np.random.default_rng(100 + seed)
        img = np.zeros((H, W))
        for _ in range(SPP):  # one jittered position per pixel and round, through the same camera matrices
            j = rng.uniform(0, 1, (H, W, 2))
            img += _value_at(s, cam, j)[..., 0]
        img /= SPP
        assert np.all(np.abs(img - exp) <= K_SIGMA * sig / np.sqrt(SPP) + 1e-5 * np.abs(exp))


def _value_at(s, cam, jitter):
    s2c = np.array(cam.sample_to_camera[:], F64).reshape(4, 4)
    c2w = np.array(cam.camera_to_world[:], F64).reshape(4, 4)
    H, W = jitter.shape[:2]
    x = (np.arange(W)[None, :] + jitter[..., 0]) * cam.inv_output_size[0]
    y = (np.arange(H)[:, None] + jitter[..., 1]) * cam.inv_output_size[1]
    q = np.stack([x, y, np.zeros_like(x), np.ones_like(x)], -1) @ s2c.T
    near = q[..., :3] / q[..., 3:4]
    d = (near / np.linalg.norm(near, axis=-1, keepdims=True)) @ c2w[:3, :3].T
    o = c2w[:3, 3]
    P = o + (-o[1] / d[..., 1])[..., None] * d
    return spot_floor_value(P)


@pytest.mark.gpu
def test_directional_light_on_a_floor_closed_form(gpu, tmp_path):
    """Directional light straight down, angle 45 degrees, radiance 2, on a horizontal diffuse floor of albedo 0.5, no
    occluder, direct_ems, box filter, 64 spp: every pixel is albedo * L * sin^2(angle) = 0.5 within
    K_SIGMA * sigma / sqrt(spp) (+ 1e-5 relative), sigma the estimator's own deviation (directional_floor_moments).
    No pixel is masked. (A sample that lands on the cap's rim is zeroed by the reference's pdf; one such sample moves
    a pixel by 1 / 64 of its value, inside the bound of 7.4 %.)"""
    em = light_scenes.directional_xml((0, -1, 0), (CF_L,) * 3, CF_ANGLE)
    c, s, b = upload(light_scenes.floor_scene_xml(str(tmp_path / "f.xml"), em, spp=SPP, albedo=(CF_ALBEDO,) * 3))
    mean, sigma = directional_floor_moments()
    tol = K_SIGMA * sigma / np.sqrt(SPP) + 1e-5 * mean
    for mode in (nh.MODE_MEGAKERNEL, nh.MODE_WAVEFRONT):
        _, rgb = render_rgb(c, s, 0, SPP, 12, mode)
        dev = np.abs(rgb.astype(F64) - mean)
        print(f"mode {mode}: max |pixel - {mean}| = {dev.max():.4f} (bound {tol:.4f}), image mean {rgb.mean():.5f}")
        assert np.all(dev <= tol)
        assert abs(float(rgb.mean()) - mean) <= tol / 8  # and the image mean, 3072 times the samples, far tighter


@pytest.mark.gpu
def test_spot_smooth_falloff_on_a_floor_closed_form(gpu, tmp_path):
    """SMOOTH_SPOT straight down from height 9.5 (falloffstart 10, totalwidth 60: the delta^4 ramp spans 10..30 degrees,
    most of the view) on the floor, direct_ems, box filter, 64 spp. The light sample is deterministic, so a pixel
    varies only with the jittered position: its expected value is the restatement averaged over the pixel (midpoint rule
    on 32 x 32 sub-cells), sigma the restatement's deviation over the same grid; bound as above.
    No pixel is masked: the cone's rim (30 degrees: 5.5 from the axis) lies outside the view (corners at 5.2). A pixel
    straddling it would draw mostly zeros and a few tiny values, a skewed distribution no Gaussian k covers at 64 spp;
    the rim is part 3's business. The ramp is really exercised: most pixels lie wholly in it, the centre ones wholly
    inside falloffstart, and ignoring the ramp would miss the bound by far."""
    c, s, b = upload(light_scenes.floor_scene_xml(str(tmp_path / "f.xml"), light_scenes.spot_xml(**SMOOTH_SPOT), spp=SPP,
                                                  albedo=(CF_ALBEDO,) * 3))
    P, _, _ = floor_points(s, 32, midpoint=True)
    v = spot_floor_value(P)
    exp, sig = v.mean(axis=(2, 3)), v.std(axis=(2, 3))
    spot = SpotRef(SMOOTH_SPOT["position"], SMOOTH_SPOT["direction"], SMOOTH_SPOT["power"], 10.0, 60.0, F64)
    f = spot.falloff(P - np.asarray(SMOOTH_SPOT["position"]))
    ramp = ((f > 0) & (f < 1)).all(axis=(2, 3))
    assert ramp.sum() > 500 and (f == 1).all(axis=(2, 3)).sum() > 50 and (f > 0).all()
    tol = K_SIGMA * sig / np.sqrt(SPP) + 1e-5 * np.abs(exp)
    for mode in (nh.MODE_MEGAKERNEL, nh.MODE_WAVEFRONT):
        _, rgb = render_rgb(c, s, 0, SPP, 14, mode)
        dev = np.abs(rgb.astype(F64) - exp)
        print(f"mode {mode}: worst pixel at {float((dev / np.maximum(tol, 1e-300)).max()):.3f} of its bound")
        assert np.all(dev <= tol)
    # with the ramp ignored (falloff == 1 inside the cone) the ramp pixels would be far off: the test can fail
    hard = v / np.where(f > 0, f, 1.0)[..., None]
    low = ramp & (f.mean(axis=(2, 3)) < 0.5)
    assert low.sum() > 50 and np.all(np.abs(hard.mean(axis=(2, 3)) - exp)[low] > 4 * tol[low])


# ---------------------------------------------------------------------------------------------------------------------
# 5. plumbing on the reference's own scenes
# ---------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def light_dir(tmp_path_factory):
    return light_scenes.materialize(str(tmp_path_factory.mktemp("lights")))


def _cut(light_dir, rel):
    p = os.path.join(light_dir, rel[:-4] + "-cut.xml")
    with open(p, "w") as f:
        f.write(light_scenes.cut_shapes(open(os.path.join(light_dir, rel)).read()))
    return p


@pytest.mark.gpu
def test_spot_xml_plumbing(gpu, light_dir, monkeypatch):
    """scenes/project/spotlight/spot.xml (path_mis, a Disney camel head, one spot) at 32 x 32, 4 spp: megakernel ==
    wavefront bit for bit, two runs identical, sample ranges [0, 2) + [2, 4) == [0, 4), NH_PERSISTENT=1 and =0
    identical, never the diffuse area-light kernels, every pixel finite, and the spot lights something. (The camel's
    BVH is too deep for the RR-ahead bounce kernels, so bounce_traits is 0 here; that a small scene with a spot takes
    the general ones, bounce_traits == 1, is test_spot_beside_an_area_light_takes_the_general_kernels.)"""
    c, s, b = upload(os.path.join(light_dir, light_scenes.SPOT_XML), res=(32, 32), spp=4)
    mk, rgb = render_rgb(c, s, 0, 4, 21, nh.MODE_MEGAKERNEL)
    assert np.isfinite(mk).all() and float(rgb.max()) > 0
    c.reset_stats()
    wf, _ = render_rgb(c, s, 0, 4, 21, nh.MODE_WAVEFRONT)
    assert c.stats()["bounce_traits"] == 0  # (a deep BVH: the pipeline without the RR-ahead bounce kernel)
    assert np.array_equal(bits(mk), bits(wf))
    assert np.array_equal(bits(wf), bits(render_rgb(c, s, 0, 4, 21, nh.MODE_WAVEFRONT)[0]))
    for mode in (nh.MODE_MEGAKERNEL, nh.MODE_WAVEFRONT):
        render_rgb(c, s, 0, 2, 21, mode)
        split, _ = render_rgb(c, s, 2, 4, 21, mode, clear=False)
        assert np.array_equal(bits(split), bits(mk)), mode
    for knob in ("1", "0"):
        monkeypatch.setenv("NH_PERSISTENT", knob)
        c2, s2, b2 = upload(os.path.join(light_dir, light_scenes.SPOT_XML), res=(32, 32), spp=4)
        c2.reset_stats()
        fb, _ = render_rgb(c2, s2, 0, 4, 21, nh.MODE_WAVEFRONT)
        assert np.array_equal(bits(fb), bits(mk)), knob
        assert c2.stats()["bounce_traits"] != 2
        c2.close()


@pytest.mark.gpu
@pytest.mark.parametrize("rel", [light_scenes.SPOT_VALIDATION_XML, light_scenes.BLENDER_VALIDATION_XML],
                         ids=["spotlight-validation", "blender-validation"])
def test_validation_scenes_plumbing(gpu, light_dir, rel):
    """The two validation scenes without their heavy shapes (direct_mis with four spots + envmap over a checkerboard
    table and a dielectric disc; direct_ems with a directional light + envmap), 48 x 48, 4 spp: megakernel ==
    wavefront, runs repeat, sample ranges add up, every pixel finite, and the lights show over the envmap alone."""
    # (the direct integrators always run as the megakernel; under path_mis the wavefront kernels meet the same lights)
    cp, sp, bp = upload(_cut(light_dir, rel), nh.INTEGRATOR_PATH_MIS, res=(48, 48), spp=4)
    mkp, _ = render_rgb(cp, sp, 0, 4, 31, nh.MODE_MEGAKERNEL)
    cp.reset_stats()
    wfp, _ = render_rgb(cp, sp, 0, 4, 31, nh.MODE_WAVEFRONT)
    assert np.isfinite(mkp).all() and np.array_equal(bits(mkp), bits(wfp))
    assert cp.stats()["bounce_traits"] == 1 and cp.stats()["invalid_samples"] == 0
    cp.close()
    c, s, b = upload(_cut(light_dir, rel), res=(48, 48), spp=4)
    mk, rgb = render_rgb(c, s, 0, 4, 31, nh.MODE_MEGAKERNEL)
    assert np.isfinite(mk).all()
    wf, _ = render_rgb(c, s, 0, 4, 31, nh.MODE_WAVEFRONT)
    assert np.array_equal(bits(mk), bits(wf))
    assert np.array_equal(bits(mk), bits(render_rgb(c, s, 0, 4, 31, nh.MODE_MEGAKERNEL)[0]))
    render_rgb(c, s, 0, 2, 31, nh.MODE_MEGAKERNEL)
    split, _ = render_rgb(c, s, 2, 4, 31, nh.MODE_MEGAKERNEL, clear=False)
    assert np.array_equal(bits(split), bits(mk))
    assert c.stats()["invalid_samples"] == 0
    env = 0.1 if rel == light_scenes.SPOT_VALIDATION_XML else 0.051
    # the lights add more than the envmap's own level (blender-validation: albedo 100 sin^2(2 deg) = 0.12 on the plane)
    assert float(rgb.max()) > 2 * env


@pytest.mark.gpu
def test_spot_beside_an_area_light_takes_the_general_kernels(gpu, scene_dir):
    """The all-diffuse Cornell box renders with the diffuse area-light bounce kernels (bounce_traits == 2,
    tests/test_gpu_bounce_traits.py); one spot beside its area light and it must take the general ones
    (bounce_traits == 1), which alone know the light -- bit-identical to the megakernel, two runs identical."""
    spot = light_scenes.spot_xml(CBOX_LIGHT_POS, (0.2, -1.0, 0.1), CBOX_LIGHT_POWER, falloffstart=20, totalwidth=70)
    c, s, b = upload(scenegen.cbox_xml(scene_dir, "c2", 32, 32, 4, extra_shapes=spot))
    mk, _ = render_rgb(c, s, 0, 4, 41, nh.MODE_MEGAKERNEL)
    c.reset_stats()
    wf, _ = render_rgb(c, s, 0, 4, 41, nh.MODE_WAVEFRONT)
    assert c.stats()["bounce_traits"] == 1
    assert np.isfinite(mk).all() and np.array_equal(bits(mk), bits(wf))
    assert np.array_equal(bits(wf), bits(render_rgb(c, s, 0, 4, 41, nh.MODE_WAVEFRONT)[0]))
    c0, s0, b0 = upload(scenegen.cbox_xml(scene_dir, "c2", 32, 32, 4))
    c0.reset_stats()
    base, _ = render_rgb(c0, s0, 0, 4, 41, nh.MODE_WAVEFRONT)
    assert c0.stats()["bounce_traits"] == 2
    assert float(mk[..., :3].sum()) > float(base[..., :3].sum())
