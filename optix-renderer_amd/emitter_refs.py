"""numpy restatements of the reference's environment map, sphere light and mesh area light, and the crafted inputs the
emitter-query tests upload (tests/test_gpu_emitter_envmap.py).

Every function takes the float type T the arithmetic runs in: F64 is the reference value, F32 the same formulas at
the device's precision. Inputs (scene data, reference points, samples, directions) are float32 values in both runs.
M_PI and Epsilon are Nori's float constants. Transcendentals are the correctly rounded ones (evaluated in fp64 and
rounded to T), as in the loader and the device code.

Restated from:
  EnvRef.sample / pdf / eval    src/emitters/environmentmap.cpp:73-131 (and :154-169 for the loader's CDF, CraftedEnv)
  EnvRef.tex_coords / texel     src/textures/PNGTexture.cpp:125-160, lookup only (sRGB textures)
  dpdf_sample                   include/nori/dpdf.h DiscretePDF::sample (and normalize, in CraftedEnv)
  spherical_direction / _coordinates   src/utils/common.cpp:270-291
  uniform_sphere                src/utils/warp.cpp:74-82
  sphere_sample                 src/shapes/sphere.cpp:126-137 with src/emitters/arealight.cpp:58-125
  mesh_sample                   src/shapes/mesh.cpp:50-90 with src/emitters/arealight.cpp:58-125, warp.cpp:162-166
"""
from __future__ import annotations

import ctypes as C

import numpy as np

F32, F64 = np.float32, np.float64
EPS = 1e-4  # Nori's Epsilon
M32 = 0xFFFFFFFF
IDENTITY = (1.0, 0.0, 0.0, 0.0, 1.0, 0.0, 0.0, 0.0, 1.0)


def pi(T):
    return T(F32(3.14159265358979323846))


def eps(T):
    return T(F32(EPS))


def dot(a, b):  # Eigen's grouping of a 3-vector dot product
    return a[..., 0] * b[..., 0] + (a[..., 1] * b[..., 1] + a[..., 2] * b[..., 2])


def normalized(v):
    return v / np.sqrt(dot(v, v))[..., None]


def _fn(f, T, *x):
    with np.errstate(invalid="ignore"):
        return f(*[np.asarray(a, F64) for a in x]).astype(T)


def spherical_direction(theta, phi, T):  # common.cpp:270-281
    st, ct, sp, cp = _fn(np.sin, T, theta), _fn(np.cos, T, theta), _fn(np.sin, T, phi), _fn(np.cos, T, phi)
    return np.stack([st * cp, st * sp, ct], -1)


def spherical_coordinates(v, T):  # common.cpp:283-291 -> theta, phi
    theta = _fn(np.arccos, T, v[..., 2])
    phi = _fn(np.arctan2, T, v[..., 1], v[..., 0])
    return theta, np.where(phi < 0, phi + T(2) * pi(T), phi)


def rot3(m, w):  # Matrix3f * Vector3f, row . w in Eigen's grouping; m: 9 values, row-major
    return np.stack([m[3 * r] * w[..., 0] + (m[3 * r + 1] * w[..., 1] + m[3 * r + 2] * w[..., 2]) for r in range(3)], -1)


def uniform_sphere(sample, T):  # warp.cpp:74-82
    s = np.asarray(sample, F32).astype(T)
    z = T(2) * s[:, 0] - T(1)
    r = np.sqrt(T(1) - z * z)
    sigma = T(2) * pi(T) * s[:, 1]
    return normalized(np.stack([r * _fn(np.cos, T, sigma), r * _fn(np.sin, T, sigma), z], -1))


def luminance(c, T):  # common.cpp:265-268
    return c[..., 0] * T(F32(0.212671)) + c[..., 1] * T(F32(0.715160)) + c[..., 2] * T(F32(0.072169))


def f2u(x):
    """static_cast<unsigned int>(float) as the reference's x86-64 build executes it (cvttss2si to 64 bits, the low
    word): truncation towards zero to int64, 0 for |x| >= 2^63 or NaN, then the low 32 bits -- in exact integers"""
    x = np.asarray(x, F64)
    ok = np.isfinite(x) & (np.abs(x) < 2.0 ** 63)
    return np.trunc(np.where(ok, x, 0.0)).astype(np.int64) & M32


def texel_index(pu, pv, W, H):
    """PNGTexture.cpp:147-150 on the float products pu = u * scaleU * width, pv = v * scaleV * height, in unsigned
    32-bit arithmetic: w = (unsigned)pu, h = height - (unsigned)pv, index = (h * width + w) % (width * height)"""
    w = f2u(pu)
    h = (H - f2u(pv)) & M32
    return ((h * W + w) & M32) % (W * H)


def dpdf_sample(cdf, x):
    """DiscretePDF::sample (dpdf.h): lower_bound - 1, clamped to [0, size - 2]; float32 comparisons"""
    cdf, x = np.asarray(cdf, F32), np.asarray(x, F32)
    return np.clip(np.searchsorted(cdf, x, side="left") - 1, 0, len(cdf) - 2)


def dpdf_sample_literal(cdf, x):
    """The same for one value, with std::lower_bound written out"""
    first, count = 0, len(cdf)
    while count > 0:
        step = count // 2
        if F32(cdf[first + step]) < F32(x):
            first += step + 1
            count -= step + 1
        else:
            count = step
    return min(max(0, first - 1), len(cdf) - 2)


def guide_bits(n):
    """The uploader's choice of the CDF guide table for n texels: 2^bits brackets, about 4 texels each"""
    bits = 0
    while bits < 20 and (1 << (bits + 2)) < n:
        bits += 1
    return bits


class EnvRef:
    """EnvMap over a PNGTexture (or a 1 x 1 constant). rgba: (W * H, 4) texels, row 0 of the image first."""

    def __init__(self, W, H, rgba, radiance, T, scale=(1.0, 1.0), offset=(0.0, 0.0), spherical=False, rotation=IDENTITY,
                 constant=False, cdf=None, normalization=0.0):
        self.T, self.W, self.H = T, int(W), int(H)
        self.rgba = np.asarray(rgba, F32).reshape(-1, 4)
        self.rad = np.asarray(radiance, F32).astype(T)
        self.su, self.sv = (T(F32(s)) for s in scale)
        self.ou, self.ov = (T(F32(o)) for o in offset)
        self.spherical, self.constant = bool(spherical), bool(constant)
        self.rot = np.asarray(rotation, F32).astype(T)
        self.cdf = None if cdf is None else np.asarray(cdf, F32)
        self.norm = T(F32(normalization))

    def tex_coords(self, u, v):
        """PNGTexture::eval up to the casts: (u * scaleU * width, v * scaleV * height)"""
        T = self.T
        if self.spherical:
            wi = rot3(self.rot, spherical_direction(v * pi(T), u * T(2) * pi(T), T))
            th, ph = spherical_coordinates(wi, T)
            u, v = ph / (T(2) * pi(T)), th / pi(T)
        else:
            u, v = u + self.ou, v + self.ov
        return u * self.su * T(self.W), v * self.sv * T(self.H)

    def tex(self, u, v):
        """-> colour (n, 3) in T, texel index, the two float products"""
        u, v = np.asarray(u, self.T), np.asarray(v, self.T)
        if self.constant:
            z = np.zeros(u.shape, np.int64)
            return np.broadcast_to(self.rgba[0, :3].astype(self.T), u.shape + (3,)), z, u * 0, v * 0
        pu, pv = self.tex_coords(u, v)
        idx = texel_index(pu, pv, self.W, self.H)
        return self.rgba[idx, :3].astype(self.T), idx, pu, pv

    def eval(self, wi):
        """EnvMap::eval (environmentmap.cpp:118-132) -> value, texel index, float products"""
        T = self.T
        wi = np.asarray(wi).astype(T)  # (float32 inputs, or a direction already computed in T)
        th, ph = spherical_coordinates(wi, T)
        c, idx, pu, pv = self.tex(ph / (T(2) * pi(T)), th / pi(T))
        return c * self.rad, idx, pu, pv

    def pdf(self, wi):
        """EnvMap::pdf (environmentmap.cpp:105-117)"""
        T = self.T
        sphere_pdf = T(0.25) / pi(T)
        val = self.eval(wi)[0]
        if self.W == 1 and self.H == 1:
            return np.full(len(val), sphere_pdf, T)
        return luminance(val, T) * self.norm / sphere_pdf * T(self.H) * T(self.W)

    def element_direction(self, elem):
        """the direction EnvMap::sample gives CDF element elem (environmentmap.cpp:79-90)"""
        T = self.T
        elem = np.asarray(elem, np.int64)
        i = (elem // self.W).astype(T) / T(self.H)
        j = (elem % self.W).astype(T) / T(self.W)
        return spherical_direction(j * pi(T), i * T(2) * pi(T), T)

    def sample(self, ref, sample):
        """EnvMap::sample (environmentmap.cpp:73-104)"""
        T = self.T
        ref = np.asarray(ref, F32).astype(T)
        s = np.asarray(sample, F32)
        elem = dpdf_sample(self.cdf, s[:, 0])
        v = uniform_sphere(s, T) if self.W == 1 and self.H == 1 else self.element_direction(elem)
        p = v * T(1) / eps(T)
        pr = p - ref
        wi = normalized(pr)
        pdf = self.pdf(wi)
        val, idx, pu, pv = self.eval(wi)
        with np.errstate(divide="ignore", invalid="ignore"):
            value = np.where((pdf < eps(T))[:, None], T(0), val / pdf[:, None])
        return {"value": value, "wi": wi, "pdf": pdf, "o": p, "d": -wi, "maxt": np.sqrt(dot(pr, pr)) - eps(T),
                "elem": elem, "texel": idx, "pu": pu, "pv": pv}


def near_texel_edge(pu, pv, margin=1e-3):
    """fp64 texel coordinates within `margin` of an integer: the texel under them depends on the rounding"""
    pu, pv = np.asarray(pu, F64), np.asarray(pv, F64)
    return (np.abs(pu - np.rint(pu)) < margin) | (np.abs(pv - np.rint(pv)) < margin)


# ---------------------------------------------------------------------------------------------------------------------
# crafted environment maps
# ---------------------------------------------------------------------------------------------------------------------
class CraftedEnv:
    """Texels and the CDF the loader would build from them (EnvMap::calculateProbs, environmentmap.cpp:154-169:
    element i * W + j is the texture at (u, v) = (i / H, j / W), the (row, column) -> (u, v) swap included; float32
    running sum of |luminance|, DiscretePDF::normalize). weights: the elements' luminances given directly instead."""

    def __init__(self, W, H, rgba, radiance=(1.0, 1.0, 1.0), scale=(1.0, 1.0), offset=(0.0, 0.0), spherical=False,
                 rotation=IDENTITY, weights=None):
        self.W, self.H = int(W), int(H)
        self.rgba = np.ascontiguousarray(rgba, F32).reshape(-1, 4)
        self.kw = dict(radiance=tuple(radiance), scale=tuple(scale), offset=tuple(offset), spherical=bool(spherical),
                       rotation=tuple(float(F32(r)) for r in rotation))
        r32 = EnvRef(W, H, self.rgba, T=F32, **self.kw)
        i, j = np.divmod(np.arange(self.W * self.H), self.W)
        c, self.elem_texel, _, _ = r32.tex(i.astype(F32) / F32(self.H), j.astype(F32) / F32(self.W))
        lum = np.abs(luminance(c, F32) if weights is None else np.asarray(weights, F32)).astype(F32)
        cdf = np.concatenate([[F32(0)], np.cumsum(lum, dtype=F32)]).astype(F32)
        total = cdf[-1]
        self.normalization = F32(0)
        if total > 0:
            self.normalization = F32(1) / total
            cdf[1:] *= self.normalization
            cdf[-1] = F32(1)
        self.cdf = np.ascontiguousarray(cdf, F32)

    def ref(self, T):
        return EnvRef(self.W, self.H, self.rgba, T=T, cdf=self.cdf, normalization=self.normalization, **self.kw)

    def apply(self, desc):
        """Repoint desc.env (an nh_scene_desc of a scene with an envmap) at this map. The arrays stay owned by self."""
        fp = C.POINTER(C.c_float)
        e = desc.env
        e.width, e.height = self.W, self.H
        e.rgba, e.cdf = self.rgba.ctypes.data_as(fp), self.cdf.ctypes.data_as(fp)
        e.normalization = float(self.normalization)
        e.scale_u, e.scale_v = self.kw["scale"]
        e.offset_u, e.offset_v = self.kw["offset"]
        e.spherical, e.constant = int(self.kw["spherical"]), 0
        for k in range(9):
            e.rotation[k] = self.kw["rotation"][k]
        for k in range(3):
            e.radiance[k] = self.kw["radiance"][k]
            desc.emitters[desc.envmap].radiance[k] = self.kw["radiance"][k]
        return desc


def random_texels(W, H, seed, black=0.0):
    """every texel its own colour in [0.05, 1]; a fraction `black` of them exactly black"""
    rng = np.random.default_rng(seed)
    rgba = np.ones((W * H, 4), F32)
    rgba[:, :3] = rng.uniform(0.05, 1.0, (W * H, 3)).astype(F32)
    if black > 0:
        rgba[rng.uniform(0, 1, W * H) < black, :3] = 0
    return rgba


def cutpoints(n):
    """the guide table's cutpoints j / 2^bits, j = 0 .. 2^bits - 1, for a CDF of n elements (exact in float32)"""
    m = 1 << guide_bits(n)
    return (np.arange(m, dtype=F64) / m).astype(F32)


def runs_env(W, H, seed, **kw):
    """A map for the CDF-search test, where only the CDF matters: its element weights are set directly instead of
    through the texels (the loader's (row, column) -> (u, v) lookup reaches only a few texels of a non-square map, 4
    of a 2 x 32 one, so the structure below cannot be had through texels at every size). The first and the last
    element black, one element holding more than half of the mass (so most guide brackets are empty), and a run of
    black elements starting exactly where the first guide cutpoint's bracket begins (see runs_properties)."""
    n = W * H
    weights = np.random.default_rng(seed).uniform(0.05, 1.0, n).astype(F32)
    weights[(5 * n) // 8] = F32(2 * n)  # against less than 1 for each of the others
    weights[0] = weights[n - 1] = 0
    t = cutpoints(n)[1]
    for _ in range(8):
        env = CraftedEnv(W, H, random_texels(W, H, seed), weights=weights, **kw)
        if runs_properties(env)["run_at_cutpoint"]:
            break
        g = int(np.searchsorted(env.cdf, t, side="left"))
        weights[g:g + 3] = 0  # elements g .. g + 2: cdf[g] == .. == cdf[g + 3]
    return env


def runs_properties(env):
    """What runs_env promises, read off the CDF alone"""
    cdf, n = env.cdf, env.W * env.H
    t = cutpoints(n)
    g = np.searchsorted(cdf, t[1:], side="left")  # guide[j]: the first entry not below the cutpoint
    mass = np.diff(cdf.astype(F64))
    guide = np.searchsorted(cdf, np.append(t, F32(1)), side="left")
    return {"monotone": bool(np.all(np.diff(cdf) >= 0)), "first_black": bool(cdf[1] == 0),
            "last_black": bool(cdf[n - 1] == cdf[n]), "heavy": float(mass.max()),
            "run_at_cutpoint": bool(np.any((cdf[g - 1] < t[1:]) & (cdf[g] == cdf[np.minimum(g + 2, n)]))),
            "empty_brackets": int(np.sum(np.diff(guide) == 0)), "brackets": len(t)}


def search_samples(cdf, seed, n_random=256):
    """sample.x of the CDF-search test: 0, the largest float below 1, every CDF entry below 1 and every guide
    cutpoint with nextafter on both sides, and n_random random values -- all in [0, 1)"""
    cdf = np.asarray(cdf, F32)
    top = np.nextafter(F32(1), F32(0))
    base = np.concatenate([cdf[cdf < 1], cutpoints(len(cdf) - 1)]).astype(F32)
    x = np.concatenate([[F32(0), top], base, np.nextafter(base, F32(-1)), np.nextafter(base, F32(2)),
                        np.random.default_rng(seed).uniform(0, 1, n_random).astype(F32)]).astype(F32)
    return x[(x >= 0) & (x < 1)]


def far_points(n, seed, lo, hi):
    """n float32 points at distances uniform in [lo, hi] from the origin, in random directions"""
    rng = np.random.default_rng(seed)
    d = rng.normal(size=(n, 3))
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    return (d * rng.uniform(lo, hi, (n, 1))).astype(F32)


def unit_vectors(n, seed):
    """n float32 directions, normalized in float32 arithmetic"""
    v = np.random.default_rng(seed).normal(size=(n, 3)).astype(F32)
    return normalized(v).astype(F32)


# ---------------------------------------------------------------------------------------------------------------------
# sphere and mesh area lights
# ---------------------------------------------------------------------------------------------------------------------
def _area_record(p, n, prob, radiance, ref, T):
    """AreaEmitter::sample past sampleSurface (arealight.cpp:75-125): prob = the shape's pdfSurface"""
    pr = p - ref
    wi = normalized(pr)
    cosl = dot(n, -wi)
    with np.errstate(divide="ignore", invalid="ignore"):
        pdf = np.where(cosl < 0, T(0), prob * dot(pr, pr) / np.abs(cosl))
        rad = np.asarray(radiance, F32).astype(T)
        val = np.where(((cosl < 0) | (np.abs(pdf) < eps(T)))[:, None], T(0), rad[None, :] / pdf[:, None])
    return {"value": val, "wi": wi, "pdf": pdf, "o": p, "n": n, "d": -wi, "maxt": np.sqrt(dot(pr, pr)) - eps(T),
            "cosl": cosl}


def sphere_sample(center, radius, radiance, ref, sample, T):
    """Sphere::sampleSurface / pdfSurface (sphere.cpp:126-137): std::pow(1.f / r, 2) is the double pow, and its product
    with the float 0.25f / M_PI is rounded to float on return"""
    ref = np.asarray(ref, F32).astype(T)
    q = uniform_sphere(sample, T)
    r = T(F32(radius))
    p = np.asarray(center, F32).astype(T) + r * q
    prob = T(F64(T(1) / r) ** 2 * F64(T(0.25) / pi(T)))
    return _area_record(p, q, prob, radiance, ref, T)


def mesh_sample(V, N, faces, cdf, pdf_norm, radiance, ref, sample, T):
    """Mesh::sampleSurface (mesh.cpp:50-90: sampleReuse, squareToUniformTriangle, interpolated vertex, the interpolated
    normal when the mesh has normals (N is not None) and the face normal otherwise). cdf / pdf_norm: the mesh's area
    DiscretePDF as loaded."""
    V = np.asarray(V, F32).astype(T)
    ref = np.asarray(ref, F32).astype(T)
    cdf = np.asarray(cdf, F32)
    s = np.asarray(sample, F32)
    idx = dpdf_sample(cdf, s[:, 0])
    c = cdf.astype(T)
    sx = (s[:, 0].astype(T) - c[idx]) / (c[idx + 1] - c[idx])
    su1 = np.sqrt(sx)
    bu, bv = T(1) - su1, s[:, 1].astype(T) * su1
    bw = T(1) - bu - bv
    f = np.asarray(faces)[idx]
    p0, p1, p2 = (V[f[:, k]] for k in range(3))
    p = bu[:, None] * p0 + bv[:, None] * p1 + bw[:, None] * p2
    if N is not None:
        N = np.asarray(N, F32).astype(T)
        n = normalized(bu[:, None] * N[f[:, 0]] + bv[:, None] * N[f[:, 1]] + bw[:, None] * N[f[:, 2]])
    else:
        n = normalized(np.cross(p1 - p0, p2 - p0))
    out = _area_record(p, n, T(F32(pdf_norm)), radiance, ref, T)
    out["face"] = idx
    return out


# five triangles of clearly unequal areas (0.02 .. 2.4), each in a plane of its own, all facing down (-y) with
# different tilts: the plane a sampled point lies on names its face
FIVE_TRIANGLES = [
    [(-2.0, 3.0, -1.0), (0.4, 3.0, -1.0), (-2.0, 3.2, 1.0)],
    [(0.6, 3.5, -1.0), (1.4, 3.5, -1.0), (0.6, 3.4, -0.2)],
    [(0.8, 4.0, 0.2), (1.0, 4.0, 0.2), (0.8, 4.04, 0.4)],
    [(-0.5, 4.5, 0.3), (0.7, 4.6, 0.3), (-0.5, 4.5, 1.6)],
    [(1.6, 5.0, -0.5), (2.2, 5.0, -0.5), (1.6, 5.1, 0.4)],
]


def five_triangles_obj(path, normals=False, seed=3):
    """FIVE_TRIANGLES as an OBJ. normals: every vertex gets a normal of its own, the face normal bent by up to about
    10 degrees, so the interpolated normal differs from the face normal and across the face."""
    rng = np.random.default_rng(seed)
    lines, nrm = [], []
    for tri in FIVE_TRIANGLES:
        a, b, c = (np.asarray(p, F64) for p in tri)
        fn = np.cross(b - a, c - a)
        fn /= np.linalg.norm(fn)
        assert fn[1] < -0.9
        for p in tri:
            lines.append("v %r %r %r" % tuple(float(x) for x in p))
            m = fn + rng.uniform(-0.12, 0.12, 3)
            nrm.append(m / np.linalg.norm(m))
    if normals:
        lines += ["vn %r %r %r" % tuple(float(x) for x in m) for m in nrm]
    for k in range(len(FIVE_TRIANGLES)):
        i = 3 * k + 1
        lines.append(f"f {i}//{i} {i + 1}//{i + 1} {i + 2}//{i + 2}" if normals else f"f {i} {i + 1} {i + 2}")
    with open(path, "w") as f:
        f.write("\n".join(lines) + "\n")
    return path


def face_of_point(V, faces, p, tol=1e-3):
    """index of the face whose plane the points p lie on (-1: none or more than one within tol)"""
    V, p = np.asarray(V, F64), np.asarray(p, F64)
    dist = []
    for f in np.asarray(faces):
        a, b, c = V[f[0]], V[f[1]], V[f[2]]
        n = np.cross(b - a, c - a)
        dist.append(np.abs((p - a) @ (n / np.linalg.norm(n))))
    dist = np.stack(dist, -1)
    hit = dist < tol
    return np.where(hit.sum(-1) == 1, np.argmin(dist, -1), -1)
