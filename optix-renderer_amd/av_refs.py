"""numpy restatement of the reference's av integrator, for tests/test_av_host.py and tests/test_gpu_av.py, in the style
of photon_refs.py / emitter_refs.py: float32 arithmetic in the reference's operation order, one rounding per operation,
nothing fused. Traversal is the oracle's (OracleScene.trace); the streams are seeded by the oracle's Pcg32.per_path.

Restated from:
  camera_rays          src/cameras/perspective.cpp:97-141 (pinhole only), Transform * Point3f / Vector3f
                       (include/nori/transform.h:73-86)
  hit_points           src/shapes/mesh.cpp:141-196 (its.p, the interpolated or the geometric normal; no normal map),
                       src/shapes/sphere.cpp:96-121
  sample_hemisphere    src/utils/warp.cpp:25-39 (Warp::sampleUniformHemisphere)
  av_paths             src/integrators/av.cpp:18-43 under renderBlock's camera sample (src/utils/render.cpp:441-447)
  ttest_estimator      the scene loop of StudentsTTest (src/utils/ttest.cpp:210-230) over av_paths
  materialize          writes the reference's av files from tests/golden/av_scenes.json

Eigen 3.3.8 adds a 3-vector's products as x0*y0 + (x1*y1 + x2*y2) in dot / squaredNorm (its unrolled redux splits
3 = 1 + 2; oracle/eigen_probe.cpp pins it), coefficient-wise sums left to right.
"""
from __future__ import annotations

import ctypes as C
import json
import os

import numpy as np

F32 = np.float32
EPSILON = F32(1e-4)
_MULT = np.uint64(0x5851F42D4C957F2D)
_GOLDEN = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tests", "golden")


# ---- pcg32 streams, stepped together (ext/pcg32/pcg32.h:96-110) -------------------------------------------------
class Streams:
    """n pcg32 generators as uint64 arrays; next_float(mask) steps only the masked ones."""

    def __init__(self, state, inc):
        self.state = np.asarray(state, np.uint64).copy()
        self.inc = np.asarray(inc, np.uint64).copy()
        self.draws = np.zeros(len(self.state), np.int64)

    @classmethod
    def per_path(cls, oracle_mod, seed: int, pixels, samples):
        """path_rng(seed, pixel, sample) of every path, seeded by the oracle's Pcg32.per_path"""
        st, inc = np.empty(len(pixels), np.uint64), np.empty(len(pixels), np.uint64)
        for i, (p, s) in enumerate(zip(pixels, samples)):
            r = oracle_mod.Pcg32.per_path(int(seed), int(p), int(s))
            st[i], inc[i] = r.state.value, r.inc.value
        return cls(st, inc)

    def next_uint(self, mask=None) -> np.ndarray:
        m = np.ones(len(self.state), bool) if mask is None else mask
        old = self.state[m]
        with np.errstate(over="ignore"):
            self.state[m] = old * _MULT + self.inc[m]
        xs = (((old >> np.uint64(18)) ^ old) >> np.uint64(27)).astype(np.uint32)
        rot = (old >> np.uint64(59)).astype(np.uint32)
        self.draws[m] += 1
        return (xs >> rot) | (xs << ((~rot + np.uint32(1)) & np.uint32(31)))

    def next_float(self, mask=None) -> np.ndarray:
        u = (self.next_uint(mask) >> np.uint32(9)) | np.uint32(0x3F800000)
        return u.view(F32) - F32(1)

    def next_floats(self, k: int) -> list:
        """the next k draws of stream 0"""
        return [self.next_float()[0] for _ in range(k)]


# ---- Eigen's 3-vector arithmetic in float32 ---------------------------------------------------------------------
def dot3(a, b):
    return a[:, 0] * b[:, 0] + (a[:, 1] * b[:, 1] + a[:, 2] * b[:, 2])


def normalized3(a):
    """Vector3f::normalized(): divided by sqrt(squaredNorm) when that is > 0"""
    n = dot3(a, a)
    with np.errstate(invalid="ignore", divide="ignore"):
        s = np.sqrt(n)
        return np.where((n > 0)[:, None], a / s[:, None], a)


def cross3(a, b):
    return np.stack([a[:, 1] * b[:, 2] - a[:, 2] * b[:, 1], a[:, 2] * b[:, 0] - a[:, 0] * b[:, 2],
                     a[:, 0] * b[:, 1] - a[:, 1] * b[:, 0]], -1)


def _mat(m):
    return np.array(list(m), F32).reshape(4, 4)


def _xform_point(m, x, y, z):
    """Transform * Point3f: the 4x4 product with (x, y, z, 1) left to right, then the division by w"""
    r = [((m[i, 0] * x + m[i, 1] * y) + m[i, 2] * z) + m[i, 3] * F32(1) for i in range(4)]
    return np.stack([r[0] / r[3], r[1] / r[3], r[2] / r[3]], -1)


def camera_rays(camera, pixel_sample):
    """PerspectiveCamera::sampleRay without a lens: (o, d, mint, maxt) of the (n, 2) float32 sample positions"""
    assert not camera.lens_radius > float(EPSILON), "pinhole cameras only"
    ps = np.asarray(pixel_sample, F32).reshape(-1, 2)
    s2c, c2w = _mat(camera.sample_to_camera), _mat(camera.camera_to_world)
    inv = np.array(list(camera.inv_output_size), F32)
    zero = np.zeros(len(ps), F32)
    near_p = _xform_point(s2c, ps[:, 0] * inv[0], ps[:, 1] * inv[1], zero)
    dl = normalized3(near_p)
    o = _xform_point(c2w, zero, zero, zero)
    d = np.stack([c2w[i, 0] * dl[:, 0] + (c2w[i, 1] * dl[:, 1] + c2w[i, 2] * dl[:, 2]) for i in range(3)], -1)
    inv_z = F32(1) / dl[:, 2]
    return o, d, F32(camera.near_clip) * inv_z, F32(camera.far_clip) * inv_z


class SceneArrays:
    """The descriptor's geometry as numpy views: what setHitInformation reads"""

    def __init__(self, scene):
        d = scene.desc
        self.desc = d
        self.shapes = [d.shapes[i] for i in range(d.n_shapes)]
        nv, nf = d.n_vertices, d.n_faces
        self.V = np.ctypeslib.as_array(d.V, shape=(nv, 3)).astype(F32) if nv else np.zeros((0, 3), F32)
        self.N = np.ctypeslib.as_array(d.N, shape=(nv, 3)).astype(F32) if nv and d.N else None
        self.F = np.ctypeslib.as_array(d.F, shape=(nf, 3)).astype(np.int64) if nf else np.zeros((0, 3), np.int64)
        off = [0]
        for s in self.shapes:
            off.append(off[-1] + (s.n_faces if s.type == 0 else 1))
        self.prim_offset = np.array(off, np.int64)


def hit_points(arr: SceneArrays, o, d, hit):
    """its.p and its.shFrame.n of the oracle's closest hits (rows where hit["hit"] is set; the others are zero)"""
    n = len(o)
    p, pole = np.zeros((n, 3), F32), np.zeros((n, 3), F32)
    for si, s in enumerate(arr.shapes):
        m = (hit["hit"] != 0) & (hit["shape"] == si)
        if not m.any():
            continue
        assert not s.normal_map, "normal maps are not restated here"
        if s.type == 1:  # sphere.cpp:98-99
            pp = o[m] + hit["t"][m, None] * d[m]
            p[m] = pp
            pole[m] = normalized3(pp - np.array(list(s.center), F32)[None])
            continue
        local = hit["prim"][m].astype(np.int64) - arr.prim_offset[si]
        idx = arr.F[s.f_offset + local] + s.v_offset
        u, v = hit["u"][m], hit["v"][m]
        b = [(F32(1) - (u + v))[:, None], u[:, None], v[:, None]]
        p0, p1, p2 = arr.V[idx[:, 0]], arr.V[idx[:, 1]], arr.V[idx[:, 2]]
        p[m] = (b[0] * p0 + b[1] * p1) + b[2] * p2
        if s.has_normals:  # mesh.cpp:165-190: the same normal with and without texture coordinates
            n0, n1, n2 = arr.N[idx[:, 0]], arr.N[idx[:, 1]], arr.N[idx[:, 2]]
            pole[m] = normalized3((b[0] * n0 + b[1] * n1) + b[2] * n2)
        else:  # mesh.cpp:163
            pole[m] = normalized3(cross3(p1 - p0, p2 - p0))
    return p, pole


def sample_hemisphere(streams: Streams, pole, mask):
    """Warp::sampleUniformHemisphere for the masked streams: rejection from the cube, three draws per try"""
    n = len(pole)
    v = np.zeros((n, 3), F32)
    todo = mask.copy()
    while todo.any():
        x = F32(1) - F32(2) * streams.next_float(todo)
        y = F32(1) - F32(2) * streams.next_float(todo)
        z = F32(1) - F32(2) * streams.next_float(todo)
        c = np.stack([x, y, z], -1)
        v[todo] = c
        rej = dot3(c, c) > F32(1)
        idx = np.flatnonzero(todo)
        todo[idx[~rej]] = False
    flip = dot3(v, pole) < F32(0)
    v = np.where(flip[:, None], -v, v)
    with np.errstate(invalid="ignore", divide="ignore"):
        out = v / np.sqrt(dot3(v, v))[:, None]
    return np.where(mask[:, None], out, F32(0)).astype(F32)


def av_paths(scene, oracle, seed: int, pixels, samples, pixel_sample=None, length=None, oracle_mod=None,
             detail: bool = False):
    """AverageVisibilityIntegrator::Li of path (pixels[i], samples[i]) on its per-path stream: (n,) float32 of 0 / 1.
    oracle: the scene's OracleScene. pixel_sample: explicit (n, 2) sample positions (a function of the two jitter draws
    is also accepted: the t-test's), default pixel + jitter. length: the scene's by default."""
    if oracle_mod is None:
        import nori_oracle as oracle_mod
    pixels, samples = np.asarray(pixels, np.int64), np.asarray(samples, np.int64)
    n = len(pixels)
    cam = scene.desc.camera
    length = F32(scene.av_params() if length is None else length)
    st = Streams.per_path(oracle_mod, seed, pixels, samples)
    jx, jy = st.next_float(), st.next_float()
    st.next_float()  # the aperture sample, unused
    st.next_float()
    if pixel_sample is None:
        py = pixels // cam.width
        px = pixels - py * cam.width
        ps = np.stack([px.astype(F32) + jx, py.astype(F32) + jy], -1)
    elif callable(pixel_sample):
        ps = pixel_sample(jx, jy)
    else:
        ps = np.asarray(pixel_sample, F32).reshape(-1, 2)
    o, d, mint, maxt = camera_rays(cam, ps)
    o = np.ascontiguousarray(np.broadcast_to(o, (n, 3)), F32)
    hit = oracle.trace(o, d, mint, maxt)
    found = hit["hit"] != 0
    p, pole = hit_points(SceneArrays(scene), o, d, hit)
    dirs = sample_hemisphere(st, pole, found)
    value = np.ones(n, F32)
    if found.any():
        k = np.flatnonzero(found)
        occ = oracle.trace(np.ascontiguousarray(p[k]), np.ascontiguousarray(dirs[k]), np.full(len(k), EPSILON, F32),
                           np.full(len(k), length, F32), any_hit=True)
        value[k[occ["hit"] != 0]] = F32(0)
    if detail:
        return {"value": value, "found": found, "p": p, "pole": pole, "dir": dirs, "draws": st.draws, "shape": hit["shape"]}
    return value


def ttest_estimator(scene, oracle, seed: int, n: int, first: int = 0, oracle_mod=None) -> dict:
    """nh_ttest_scene's estimator over av_paths: sample k on the stream of (pixel 0, sample first + k) through the pixel
    sample (a W, b H) (ttest.cpp:214-215); the luminance of (v, v, v) in float32, the mean and the unbiased variance
    in fp64 (two passes). {"ones", "mean", "variance", "lum"}"""
    cam = scene.desc.camera
    w, h = F32(cam.width), F32(cam.height)
    v = av_paths(scene, oracle, seed, np.zeros(n, np.int64), first + np.arange(n, dtype=np.int64),
                 pixel_sample=lambda a, b: np.stack([a * w, b * h], -1), oracle_mod=oracle_mod)
    lum = (v * F32(0.212671) + v * F32(0.715160)) + v * F32(0.072169)  # Color3f::getLuminance
    x = lum.astype(np.float64)
    mean = float(x.sum() / n)
    return {"ones": int((v == 1).sum()), "mean": mean, "variance": float(((x - mean) ** 2).sum() / (n - 1)), "lum": lum}


def materialize(out_dir: str) -> str:
    """scenes/pa1/test-av.xml with disk.obj, ajax-av.xml and sponza-av.xml (av_scenes.json; the two renders' meshes
    are not shipped) under out_dir; files already there are left alone. Returns out_dir."""
    with open(os.path.join(_GOLDEN, "av_scenes.json")) as f:
        files = json.load(f)
    for rel, text in files.items():
        p = os.path.join(out_dir, rel)
        if not os.path.exists(p):
            os.makedirs(os.path.dirname(p), exist_ok=True)
            with open(p, "w") as g:
                g.write(text)
    return out_dir
