"""nh_emitter_query on the environment map, sphere lights and mesh lights at their CDF boundaries, against the fp64 numpy
restatement of the reference's formulas in emitter_refs.py (which lists the reference lines each function follows).

A device value may differ from the fp64 one by bound(gap) = 4 * max(gap, float epsilon), gap being the fp32
restatement's own distance to the fp64 one on the same inputs. Everything discrete is compared exactly: the CDF element
(through the shadow-ray origin), the texel (every texel has a colour of its own), mint, d == -wi, exact zeros.
Environment maps are crafted in memory: the nh_scene_desc of a small loaded scene with desc.env repointed at numpy
arrays (CraftedEnv: texels, and the CDF built from them as the loader builds it).

1. the CDF search, element exact, at every CDF entry and guide cutpoint and their float neighbours, guided == unguided
2. the full sample record at reference points far from the origin (wi well inside a texel)
3. the sample at scene-scale reference points: geometry, and self-consistency with EVAL / PDF at the returned wi
4. eval / pdf at random and hand-placed directions, texel exact; the 1 x 1 constant map
5. the sphere area light
6. a five-triangle mesh light at its area-CDF boundaries, through emit_faces, S.F / S.V and interpolated normals
The unmarked tests check the restatement itself (DiscretePDF against a literal lower_bound, the texel lookup against
the oracle) and that the GPU tests' inputs respect their exclusion caps, on the CPU.
"""
import ctypes as C
import os

import numpy as np
import pytest

import emitter_refs as er
import light_scenes
import nori_hip as nh
import scenegen
from emitter_refs import F32, F64

EPS = 1e-4  # Nori's Epsilon
EPS32 = float(np.finfo(np.float32).eps)


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


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def origin_gap(a, b):
    """shadow-ray origins v / Epsilon, relative to their length 1e4"""
    return abs_gap(a, b) / 1e4


GAPS = {"value": rel_gap, "pdf": rel_gap, "wi": abs_gap, "o": origin_gap, "maxt": rel_gap}


def compare(label, g, r32, r64, keys, sel=None, o_gap=origin_gap):
    """device within bound(gap) of the fp64 value for every quantity in keys; sel: {key: mask}; o_gap: the measure of
    the shadow-ray origin (absolute for a point on a light in the scene)"""
    sel = sel or {}
    for k in keys:
        m = sel.get(k, slice(None))
        fn = o_gap if k == "o" else GAPS[k]
        gap, err = fn(r32[k][m], r64[k][m]), fn(g[k][m], r64[k][m])
        print(f"{label} {k}: fp32 gap {gap:.3g}, device {err:.3g}")
        assert err <= bound(gap), (label, k, err, gap)


# ---------------------------------------------------------------------------------------------------------------------
# inputs, shared by the GPU tests and the CPU checks of their admissibility
# ---------------------------------------------------------------------------------------------------------------------
ENV_SIZES = [(9, 7), (8, 8), (13, 5), (2, 32), (96, 48)]  # 63: no guide table; 64: the smallest guided CDF; 65; ...
EVAL_SIZES = [(8, 8), (13, 5), (96, 48)]
EULER = (30, -45, 110)
RADIANCE = (1.5, 0.75, 2.0)
SCALE, OFFSET = (2.5, 0.75), (-0.3, 0.6)
N_QUERIES = 4096
MAX_LEFT_OUT = 0.02


def size_id(s):
    return f"{s[0]}x{s[1]}"


@pytest.fixture(scope="module")
def base(tmp_path_factory):
    """A small scene lit by an envmap, whose desc the crafted maps are put into, and the rotation matrix the loader
    makes of eulerAngles = EULER (and of none)."""
    d = str(tmp_path_factory.mktemp("envq"))
    s = nh.Scene(scenegen.envmap_xml(os.path.join(d, "plain"), 16, 16, 1, tex_size=(8, 8), area_light=False))
    sr = nh.Scene(scenegen.envmap_xml(os.path.join(d, "rot"), 16, 16, 1, tex_size=(8, 8), area_light=False, euler=EULER))
    assert s.desc.envmap >= 0
    ident, rot = (tuple(x.desc.env.rotation[k] for k in range(9)) for x in (s, sr))
    assert np.allclose(ident, er.IDENTITY) and not np.allclose(rot, er.IDENTITY)
    return {"scene": s, "configs": {
        "spherical": dict(spherical=True, rotation=ident),
        "rotated": dict(spherical=True, rotation=rot),
        "planar": dict(spherical=False, scale=SCALE, offset=OFFSET),
        "spherical-scaled": dict(spherical=True, rotation=ident, scale=SCALE)}}


SAMPLE_CONFIGS = ["spherical", "rotated", "planar"]
EVAL_CONFIGS = SAMPLE_CONFIGS + ["spherical-scaled"]


def search_env(size, texture):
    W, H = size
    if texture == "lit":
        return er.CraftedEnv(W, H, er.random_texels(W, H, 11), radiance=RADIANCE)
    return er.runs_env(W, H, 12, radiance=RADIANCE)


def speckled_env(base, size, config):
    """every texel its own colour, one in ten black (runs of equal CDF entries, and the pdf < Epsilon branch)"""
    W, H = size
    return er.CraftedEnv(W, H, er.random_texels(W, H, 21, black=0.1), radiance=RADIANCE, **base["configs"][config])


def sample_inputs(lo, hi):
    rng = np.random.default_rng(31)
    return er.far_points(N_QUERIES, 32, lo, hi), rng.uniform(0, 1, (N_QUERIES, 2)).astype(F32)


def kept(r32, r64):
    """the queries whose fp64 texel coordinates keep 1e-3 from a texel edge; asserts the cap and that both precisions
    name the same texel on them"""
    keep = ~er.near_texel_edge(r64["pu"], r64["pv"])
    assert 1.0 - keep.mean() <= MAX_LEFT_OUT, 1.0 - keep.mean()
    assert np.array_equal(r32["texel"][keep], r64["texel"][keep])
    return keep


def hand_placed(H):
    """the poles, the phi = 0 seam from both sides, and theta / pi * H < 1 (the row H - 0 that wraps to row 0)"""
    t = 0.4 * np.pi / H
    tiny = 1e-30
    return np.array([[0, 0, 1], [0, 0, -1], [1, tiny, 0], [1, -tiny, 0], [0.6, tiny, 0.8], [0.6, -tiny, 0.8],
                     [np.sin(t) * np.cos(1.0), np.sin(t) * np.sin(1.0), np.cos(t)],
                     [np.sin(t) * np.cos(4.0), np.sin(t) * np.sin(4.0), np.cos(t)]], F32)


SPHERE_CENTER, SPHERE_RADIUS, SPHERE_RADIANCE = (0.2, 1.5, -0.3), 0.35, (5.0, 4.0, 3.0)


def sphere_inputs():
    rng = np.random.default_rng(41)
    ref = (er.far_points(256, 42, 0.6, 4.0).astype(F64) + np.asarray(SPHERE_CENTER)).astype(F32)
    return ref, rng.uniform(0, 1, (256, 2)).astype(F32)


MESH_RADIANCE = (5.0, 4.0, 3.0)


def mesh_scene(d, normals):
    name = "five_n" if normals else "five"
    er.five_triangles_obj(os.path.join(d, name + ".obj"), normals=normals)
    em = (f'<shape type="obj"><string name="filename" value="{name}.obj"/><emitter type="area">'
          f'<color name="radiance" value="{MESH_RADIANCE[0]}, {MESH_RADIANCE[1]}, {MESH_RADIANCE[2]}"/></emitter></shape>')
    return nh.Scene(light_scenes.floor_scene_xml(os.path.join(d, name + ".xml"), em))


def mesh_data(s):
    d = s.desc
    assert d.n_emitters == 1 and d.emitters[0].type == nh.EMITTER_AREA
    sh = d.shapes[d.emitters[0].shape]
    V, N = (np.array([[a[3 * (sh.v_offset + i) + k] for k in range(3)] for i in range(sh.n_vertices)], F32)
            if a else None for a in (d.V, d.N if sh.has_normals else None))
    Fc = np.array([[d.F[3 * (sh.f_offset + i) + k] for k in range(3)] for i in range(sh.n_faces)])
    cdf = np.array([d.area_cdf[sh.pdf_offset + i] for i in range(sh.n_faces + 1)], F32)
    return V, N, Fc, cdf, sh.pdf_normalization


def mesh_inputs(cdf):
    """sample.x: every area-CDF entry below 1 with its two float neighbours, 0, the largest float below 1, 128 random
    values; reference points below the light (a few above it, behind its faces)"""
    rng = np.random.default_rng(51)
    top = np.nextafter(F32(1), F32(0))
    e = cdf[cdf < 1]
    x = np.concatenate([[F32(0), top], e, np.nextafter(e, F32(-1)), np.nextafter(e, F32(2)),
                        rng.uniform(0, 1, 128).astype(F32)]).astype(F32)
    x = x[(x >= 0) & (x < 1)]
    m = len(x)
    ref = rng.uniform(-3, 3, (m, 3))
    ref[:, 1] = np.where(np.arange(m) % 16 == 15, rng.uniform(7, 9, m), rng.uniform(-1, 2, m))
    return ref.astype(F32), np.stack([x, rng.uniform(0, 1, m).astype(F32)], -1)


# ---------------------------------------------------------------------------------------------------------------------
# CPU: the restatement itself, and the admissibility of the GPU tests' inputs
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("texture", ["lit", "runs"])
@pytest.mark.parametrize("size", ENV_SIZES, ids=size_id)
def test_dpdf_restatement_is_lower_bound(size, texture):
    """The vectorised DiscretePDF::sample of the restatement against std::lower_bound written out, on every sample of
    the CDF-search test; and the crafted maps are what that test needs: non-decreasing CDFs (else the uploader builds
    no guide table), for `runs` a black first and last element, a black run at a guide cutpoint, one element with more
    than half of the mass and so at least half of the brackets empty."""
    env = search_env(size, texture)
    p = er.runs_properties(env)
    assert p["monotone"] and env.cdf[0] == 0 and env.cdf[-1] == 1
    if texture == "runs":
        assert p["first_black"] and p["last_black"] and p["run_at_cutpoint"] and p["heavy"] > 0.5
        assert p["empty_brackets"] >= p["brackets"] // 2
    else:
        assert np.all(np.diff(env.cdf) > 0)
    x = er.search_samples(env.cdf, 13)
    assert x.min() == 0 and x.max() == np.nextafter(F32(1), F32(0)) and len(x) > 3 * len(np.unique(env.cdf)) + 200
    want = np.array([er.dpdf_sample_literal(env.cdf, v) for v in x])
    assert np.array_equal(er.dpdf_sample(env.cdf, x), want)
    n = size[0] * size[1]
    assert want.min() == 0 and (want.max() == n - 1 if texture == "lit" else want.max() < n - 1)  # (a black last element)


def _png_texture_scene(tmp_path, props, tex_w=37, tex_h=23):
    d = str(tmp_path)
    img = np.random.default_rng(5).integers(0, 256, size=(tex_h, tex_w, 4), dtype=np.uint8)
    img[..., 3] = 255
    png = os.path.join(d, "albedo.png")
    scenegen.write_png(png, img)
    tex = (f'<bsdf type="diffuse"><texture type="png_texture" name="albedo"><string name="filename" '
           f'value="{png}"/>{props}</texture></bsdf>')
    return nh.Scene(scenegen.cbox_xml(d, "c2", walls_bsdf=tex))


@pytest.mark.parametrize("config", EVAL_CONFIGS)
def test_texel_lookup_restatement_matches_the_oracle(tmp_path, config):
    """EnvRef's texel lookup at float32 against OracleScene.texture_eval on a 37 x 23 PNG albedo texture with the
    tests' settings, exact: random uv in [-3, 4], the corners 0 and 1, negative and huge coordinates (the 32-bit
    wrap-around and the |x| >= 2^63 -> 0 rule of the x86 conversion)."""
    import nori_oracle as no
    props = {"planar": f'<float name="scaleU" value="{SCALE[0]}"/><float name="scaleV" value="{SCALE[1]}"/>'
                       f'<float name="offsetU" value="{OFFSET[0]}"/><float name="offsetV" value="{OFFSET[1]}"/>',
             "spherical": '<boolean name="sphericalTexture" value="true"/>',
             "rotated": '<boolean name="sphericalTexture" value="true"/>'
                        f'<vector name="eulerAngles" value="{EULER[0]},{EULER[1]},{EULER[2]}"/>',
             "spherical-scaled": '<boolean name="sphericalTexture" value="true"/>'
                                 f'<float name="scaleU" value="{SCALE[0]}"/><float name="scaleV" value="{SCALE[1]}"/>'}
    s = _png_texture_scene(tmp_path, props[config])
    d = s.desc
    t = d.textures[0]
    assert d.n_textures == 1 and t.type == nh.TEXTURE_PNG and (t.width, t.height) == (37, 23)
    texels = np.ctypeslib.as_array(d.texels, shape=(d.n_texels * 4,)).reshape(-1, 4).copy()
    r = er.EnvRef(t.width, t.height, texels, (1, 1, 1), F32, scale=(t.scale_u, t.scale_v),
                  offset=(t.offset_u, t.offset_v), spherical=bool(t.spherical), rotation=[t.rotation[k] for k in range(9)])
    assert bool(t.spherical) == (config != "planar") and (t.scale_u != 1) == (config in ("planar", "spherical-scaled"))
    rng = np.random.default_rng(6)
    edge = [0.0, 1.0, -0.0, -1.0, 0.5, -1e-3, 1e-3, 1 - 1e-7]
    if config == "planar":  # (a spherical lookup maps every coordinate to [0, 1] first)
        edge += [3e9, -3e9, 5e9, 1e19, -1e19, 1e30]
    edge = np.array(edge, F32)
    u = np.concatenate([rng.uniform(-3, 4, 20000).astype(F32), np.repeat(edge, len(edge))])
    v = np.concatenate([rng.uniform(-3, 4, 20000).astype(F32), np.tile(edge, len(edge))])
    got = no.OracleScene(s).texture_eval(1, u, v)
    c, idx, _, _ = r.tex(u, v)
    np.testing.assert_array_equal(got, c)
    assert len(np.unique(idx)) > 200


@pytest.mark.parametrize("config", SAMPLE_CONFIGS)
@pytest.mark.parametrize("size", ENV_SIZES, ids=size_id)
def test_far_sample_inputs_respect_the_exclusion_cap(base, size, config):
    """Test 2's inputs on the restatement alone: at most 2 % of the queries have an fp64 texel coordinate within 1e-3
    of an integer, and on the others fp32 and fp64 name the same texel. Worst case here: 0.66 % left out (8 x 8,
    spherical)."""
    env = speckled_env(base, size, config)
    ref, smp = sample_inputs(300.0, 3000.0)
    r32, r64 = (env.ref(T).sample(ref, smp) for T in (F32, F64))
    keep = kept(r32, r64)
    print(f"{size_id(size)} {config}: {100 * (1 - keep.mean()):.2f} % left out")
    assert np.array_equal(r32["elem"], r64["elem"])
    black = r64["pdf"][keep] < EPS / 2
    assert (black | (r64["pdf"][keep] > 2 * EPS)).all() and black.sum() > 0 and (~black).sum() > N_QUERIES // 2


@pytest.mark.parametrize("config", EVAL_CONFIGS)
@pytest.mark.parametrize("size", EVAL_SIZES, ids=size_id)
def test_eval_inputs_respect_the_exclusion_cap(base, size, config):
    """Test 4's random directions on the restatement alone, as above. Worst case here: 0.51 % left out (8 x 8, rotated)."""
    env = speckled_env(base, size, config)
    wi = er.unit_vectors(N_QUERIES, 33)
    (_, i32, _, _), (_, i64, pu, pv) = (env.ref(T).eval(wi) for T in (F32, F64))
    keep = kept({"texel": i32}, {"texel": i64, "pu": pu, "pv": pv})
    print(f"{size_id(size)} {config}: {100 * (1 - keep.mean()):.2f} % left out")
    assert len(np.unique(i64)) > min(size[0] * size[1], 1500) // 4  # the directions reach the texture at large


def test_sphere_and_mesh_inputs_are_admissible(tmp_path):
    """Tests 5 and 6 on the restatement alone: enough sphere samples face the point and face away, clear of the
    horizon; fewer than 10 % of the mesh queries graze the light; every face, and both neighbours of every area-CDF
    entry, are drawn; each sampled point lies on the plane of exactly its face."""
    ref, smp = sphere_inputs()
    r = er.sphere_sample(SPHERE_CENTER, SPHERE_RADIUS, SPHERE_RADIANCE, ref, smp, F64)
    assert np.all(np.linalg.norm(ref - np.asarray(SPHERE_CENTER), axis=1) > SPHERE_RADIUS + 0.2)
    assert (r["cosl"] > 1e-3).sum() >= 64 and (r["cosl"] < -1e-3).sum() >= 32
    for normals in (False, True):
        V, N, Fc, cdf, norm = mesh_data(mesh_scene(str(tmp_path), normals))
        assert len(Fc) == 5 and (N is not None) == normals
        areas = np.diff(cdf.astype(F64))
        assert areas.max() > 50 * areas.min() and np.all(np.abs(np.diff(np.sort(areas))) > 0.01)
        ref, smp = mesh_inputs(cdf)
        m = er.mesh_sample(V, N, Fc, cdf, norm, MESH_RADIANCE, ref, smp, F64)
        assert (np.abs(m["cosl"]) <= 1e-3).mean() < 0.10 and (m["cosl"] < -1e-3).sum() >= 8
        assert set(m["face"]) == set(range(5))
        assert np.array_equal(er.face_of_point(V, Fc, m["o"]), m["face"])
        for k in range(1, 5):  # the entry itself belongs to the face before it, its upper neighbour to the next
            for x, face in ((cdf[k], k - 1), (np.nextafter(cdf[k], F32(2)), k), (np.nextafter(cdf[k], F32(-1)), k - 1)):
                at = smp[:, 0] == x
                assert at.any() and np.all(m["face"][at] == face)


# ---------------------------------------------------------------------------------------------------------------------
# GPU helpers
# ---------------------------------------------------------------------------------------------------------------------
def upload_env(base, env):
    """a context with the base scene uploaded, its envmap replaced by env -> (context, emitter index)"""
    d = env.apply(base["scene"].desc)
    c = nh.Context(0)
    c._check(nh.lib.nh_upload_scene(c._h, C.byref(d)), "upload_scene")
    return c, d.envmap


def raw_sample(c, emitter, ref, sample):
    """all 16 floats of every SAMPLE query"""
    ref, sample = np.ascontiguousarray(ref, F32), np.ascontiguousarray(sample, F32)
    out = np.zeros((len(ref), nh.EMITTER_QUERY_SAMPLE_STRIDE), F32)
    fp = C.POINTER(C.c_float)
    c._check(nh.lib.nh_emitter_query(c._h, emitter, nh.EMITTER_QUERY_SAMPLE, len(ref), ref.ctypes.data_as(fp),
                                     sample.ctypes.data_as(fp), out.ctypes.data_as(fp)), "emitter_query")
    return out


def check_shadow_ray(g):
    assert np.all(g["mint"] == F32(EPS)) and np.array_equal(bits(g["d"]), bits(-g["wi"]))
    for k in ("value", "wi", "pdf", "o", "maxt"):
        assert np.isfinite(g[k]).all(), k


# ---------------------------------------------------------------------------------------------------------------------
# 1. the CDF search
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("texture", ["lit", "runs"])
@pytest.mark.parametrize("size", ENV_SIZES, ids=size_id)
def test_envmap_cdf_search_picks_the_element(gpu, base, monkeypatch, size, texture):
    """EnvMap::sample's pick of the CDF element (dpdf_search / dpdf_sample / dpdf_sample_guided, and the guide table the
    uploader builds), with sample.x at 0, at the largest float below 1, at every CDF entry and every guide cutpoint
    j / 2^bits and their float neighbours, and at 256 random values. 63 texels get no guide table, 64 the smallest one
    (16 brackets). `lit`: a strictly increasing CDF. `runs`: element weights set directly -- black first and last
    elements, a black run where a bracket begins, one element with 80 % of the mass (12 of 16 brackets empty).
    The expected element is clip(searchsorted(cdf, x, 'left') - 1, 0, n - 1) in float32 (checked against a literal
    lower_bound by test_dpdf_restatement_is_lower_bound). The device's element is read from the shadow-ray origin
    v / Epsilon, which must match the fp64 sphericalDirection(col / W * pi, row / H * 2 pi) / Epsilon of the expected
    element within bound(gap) relative to 1e4: neighbouring elements lie a texel angle apart (asserted: over 100 bounds),
    except that column 0 of every row is the same pole, so a slip by whole rows would go unseen there and only there.
    Guided and unguided runs agree in all 16 floats of every query, bit for bit.
    Measured: fp32 gap 3.0e-7 at most (1.6e-7 .. 3.0e-7 over the sizes), device the same figures -- on these queries the
    device's origin is the fp32 restatement's to the last digit printed."""
    env = search_env(size, texture)
    n = size[0] * size[1]
    x = er.search_samples(env.cdf, 13)
    rng = np.random.default_rng(14)
    smp = np.stack([x, rng.uniform(0, 1, len(x)).astype(F32)], -1)
    ref = er.far_points(len(x), 15, 0.5, 3.0)
    elem = er.dpdf_sample(env.cdf, x)
    assert elem.min() == 0 and (elem.max() == n - 1 if texture == "lit" else elem.max() < n - 1)
    assert len(np.unique(elem)) > n // 4
    r32, r64 = env.ref(F32), env.ref(F64)
    o32, o64 = (r.element_direction(elem) * r.T(1) / er.eps(r.T) for r in (r32, r64))
    # neighbouring elements (other than across column 0, the pole of every row) lie a texel angle apart
    gap = origin_gap(o32, o64)
    if size[0] > 2:
        row = r64.element_direction(np.arange(1, size[0]))
        assert np.min(np.linalg.norm(np.diff(row, axis=0), axis=1)) > 100 * bound(gap)
    raw = {}
    for guide in ("on", "off"):
        if guide == "on":
            monkeypatch.delenv("NH_ENV_GUIDE", raising=False)
        else:
            monkeypatch.setenv("NH_ENV_GUIDE", "0")
        c, em = upload_env(base, env)
        raw[guide] = raw_sample(c, em, ref, smp)
        c.close()
        err = origin_gap(raw[guide][:, 7:10], o64)
        print(f"{size_id(size)} {texture} guide {guide}: {len(x)} queries, o: fp32 gap {gap:.3g}, device {err:.3g}")
        assert err <= bound(gap), (guide, err, gap)
    assert np.array_equal(bits(raw["on"]), bits(raw["off"]))


# ---------------------------------------------------------------------------------------------------------------------
# 2. / 3. the sample record
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("config", SAMPLE_CONFIGS)
@pytest.mark.parametrize("size", ENV_SIZES, ids=size_id)
def test_envmap_sample_far_reference_points(gpu, base, size, config):
    """The whole record of EnvMap::sample at |ref| in [300, 3000]: wi = normalize(v / Epsilon - ref) then lies up to 0.3
    radians from the element's corner direction v, well inside some texel, so value = eval(wi) / pdf(wi) and pdf can be
    compared with fp64: spherical lookup (identity rotation), rotated by eulerAngles (30, -45, 110), and planar with
    scale (2.5, 0.75) and offset (-0.3, 0.6). One texel in ten is black: there the fp64 pdf is exactly 0 and the
    device's value and pdf must be exactly 0 (every other kept query has an fp64 pdf above 2 Epsilon). Queries whose
    fp64 texel coordinate lies within 1e-3 of an integer are left out of value / pdf: at most 0.66 % of a case, cap 2 %.
    Exact: mint == Epsilon, d == -wi. Measured over all cases, fp32 gap = device: value 3.8e-7, pdf 2.9e-7,
    wi 3.7e-7 (absolute), o 3.0e-7 (of 1e4), maxt 2.2e-7."""
    env = speckled_env(base, size, config)
    ref, smp = sample_inputs(300.0, 3000.0)
    r32, r64 = (env.ref(T).sample(ref, smp) for T in (F32, F64))
    keep = kept(r32, r64)
    c, em = upload_env(base, env)
    g = c.emitter_query(em, ref, sample=smp)
    check_shadow_ray(g)
    black = keep & (r64["pdf"] < EPS / 2)
    lit = keep & (r64["pdf"] > 2 * EPS)
    assert np.array_equal(black | lit, keep) and black.sum() > 0
    assert np.all(g["value"][black] == 0) and np.all(g["pdf"][black] == 0) and np.all(r64["pdf"][black] == 0)
    compare(f"{size_id(size)} {config}", g, r32, r64, ("value", "pdf", "wi", "o", "maxt"), {"value": lit, "pdf": lit})


@pytest.mark.gpu
@pytest.mark.parametrize("config", SAMPLE_CONFIGS)
@pytest.mark.parametrize("size", ENV_SIZES, ids=size_id)
def test_envmap_sample_scene_scale_reference_points(gpu, base, size, config):
    """EnvMap::sample at |ref| in [0.5, 3], as in a render: wi is within 3e-4 radians of the element's corner direction,
    where the texel is a matter of rounding in the reference itself, so value and pdf are not compared with fp64. The
    texel-independent outputs are: o, wi, maxt within bound(gap); mint, d exactly. And the sample is consistent with
    separate EVAL / PDF queries at the returned wi: pdf bit-identical, value bit-identical to the float32 quotient
    EVAL / PDF per channel (0 where that pdf is below Epsilon) -- the build divides exactly.
    Measured over all cases, fp32 gap = device: wi 3.4e-7, o 3.0e-7, maxt 2.0e-7."""
    env = speckled_env(base, size, config)
    ref, smp = sample_inputs(0.5, 3.0)
    r32, r64 = (env.ref(T).sample(ref, smp) for T in (F32, F64))
    c, em = upload_env(base, env)
    g = c.emitter_query(em, ref, sample=smp)
    check_shadow_ray(g)
    compare(f"{size_id(size)} {config}", g, r32, r64, ("wi", "o", "maxt"))
    e = c.emitter_query(em, ref, wi=g["wi"])
    assert np.array_equal(bits(g["pdf"]), bits(e["pdf"]))
    dark = e["pdf"] < F32(EPS)
    with np.errstate(divide="ignore", invalid="ignore"):
        want = np.where(dark[:, None], F32(0), e["value"] / e["pdf"][:, None]).astype(F32)
    assert (~dark).sum() > N_QUERIES // 2
    assert np.array_equal(bits(g["value"]), bits(want))


# ---------------------------------------------------------------------------------------------------------------------
# 4. eval / pdf
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("config", EVAL_CONFIGS)
@pytest.mark.parametrize("size", EVAL_SIZES, ids=size_id)
def test_envmap_eval_and_pdf_pick_the_texel(gpu, base, size, config):
    """EnvMap::eval / pdf at 4096 random unit directions, in the three configurations above and spherical with scale
    (2.5, 0.75) (texel coordinates beyond the image: the % (W * H) wrap). The expected texel comes from exact integer
    arithmetic (emitter_refs.texel_index: truncation to int64, the low 32 bits, H - ..., h * W + w modulo 2^32, then
    % (W * H)) on the fp64 coordinates; the device's value must equal that texel's colour times the radiance bit for
    bit (one float product; all lit colours are distinct). Left out: fp64 texel coordinates within 1e-3 of an integer,
    at most 0.51 % of a case, cap 2 %. pdf within bound(gap), exactly 0 on black texels: fp32 gap = device, 2.9e-7 at
    most. Hand-placed directions -- the poles, the phi = 0 seam with y = +-1e-30 (phi = 2 pi: u == 1 spills into the
    next row), theta / pi * H < 1 (row H wraps to row 0): finite, and one of the texels the two restatements name."""
    env = speckled_env(base, size, config)
    r32, r64 = env.ref(F32), env.ref(F64)
    colour = (env.rgba[:, :3] * np.asarray(RADIANCE, F32)).astype(F32)  # texel * radiance, one float product each
    assert len(np.unique(colour[np.any(colour != 0, axis=1)], axis=0)) == np.any(colour != 0, axis=1).sum()
    wi = er.unit_vectors(N_QUERIES, 33)
    (v32, i32, _, _), (v64, i64, pu, pv) = (r.eval(wi) for r in (r32, r64))
    keep = kept({"texel": i32}, {"texel": i64, "pu": pu, "pv": pv})
    c, em = upload_env(base, env)
    g = c.emitter_query(em, np.zeros_like(wi), wi=wi)
    assert np.array_equal(bits(g["value"][keep]), bits(colour[i64[keep]]))
    p32, p64 = r32.pdf(wi), r64.pdf(wi)
    black = keep & (p64 == 0)
    assert black.sum() > 0 and np.all(g["pdf"][black] == 0)
    gap, err = rel_gap(p32[keep], p64[keep]), rel_gap(g["pdf"][keep], p64[keep])
    print(f"{size_id(size)} {config} pdf: fp32 gap {gap:.3g}, device {err:.3g}, {100 * (1 - keep.mean()):.2f} % left out")
    assert err <= bound(gap), (err, gap)
    # hand-placed directions: one of the texels the two restatements name
    hw = hand_placed(size[1])
    h = c.emitter_query(em, np.zeros_like(hw), wi=hw)
    h32, h64 = r32.eval(hw)[1], r64.eval(hw)[1]
    assert np.isfinite(h["value"]).all() and np.isfinite(h["pdf"]).all()
    for k in range(len(hw)):
        assert any(np.array_equal(bits(h["value"][k]), bits(colour[i])) for i in (h32[k], h64[k])), (k, hw[k])


@pytest.mark.gpu
def test_envmap_constant_texture(gpu, tmp_path):
    """The 1 x 1 constant map as the loader makes it: pdf == 0.25f / M_PI exactly for any direction and for the sample,
    eval == colour * radiance exactly, and the sampled direction is squareToUniformSphere(sample): o within bound(gap)
    of it / Epsilon (fp32 gap = device: 3.4e-7 of 1e4), value within bound(gap) of colour * radiance / pdf (2.4e-8)."""
    s = nh.Scene(scenegen.envmap_xml(str(tmp_path), 16, 16, 1, texture="constant", area_light=False))
    d = s.desc
    e = d.env
    assert (e.width, e.height, e.constant) == (1, 1, 1)
    col, rad = (np.array([a[k] for k in range(3)], F32) for a in (e.rgba, e.radiance))
    c = nh.Context(0)
    c._check(nh.lib.nh_upload_scene(c._h, C.byref(d)), "upload_scene")
    em = d.envmap
    wi = np.concatenate([er.unit_vectors(256, 34), hand_placed(1)])
    q = c.emitter_query(em, np.zeros_like(wi), wi=wi)
    sphere_pdf = F32(0.25) / F32(er.pi(F32))
    assert np.all(q["pdf"] == sphere_pdf) and np.array_equal(bits(q["value"]), bits(np.broadcast_to(col * rad, wi.shape)))
    ref, smp = (a[:512] for a in sample_inputs(0.5, 3.0))
    g = c.emitter_query(em, ref, sample=smp)
    check_shadow_ray(g)
    assert np.all(g["pdf"] == sphere_pdf)
    r32, r64 = ({"o": er.uniform_sphere(smp, T) * T(1) / er.eps(T),
                 "value": np.broadcast_to((col * rad).astype(T) / (T(0.25) / er.pi(T)), ref.shape)} for T in (F32, F64))
    compare("constant", g, r32, r64, ("o", "value"))


# ---------------------------------------------------------------------------------------------------------------------
# 5. the sphere area light
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_sphere_area_light(gpu, tmp_path):
    """AreaEmitter::sample on a sphere (Sphere::sampleSurface, pdfSurface with its double-precision pow) from 256 points
    outside it. Samples facing the point (fp64 cosine above 1e-3: at least 64): value, pdf, wi, o, maxt within
    bound(gap). Facing away (below -1e-3: at least 32): value and pdf exactly 0. EVAL / PDF at the sampled point:
    the radiance exactly, the same pdf. Measured, fp32 gap = device: value 5.1e-6, pdf 5.1e-6 (the cosine of a grazing
    sample cancels), wi 1.0e-7, o 1.0e-7 (absolute), maxt 1.2e-7, pdf query 5.1e-6."""
    em = (f'<shape type="sphere"><point name="center" value="{SPHERE_CENTER[0]}, {SPHERE_CENTER[1]}, {SPHERE_CENTER[2]}"/>'
          f'<float name="radius" value="{SPHERE_RADIUS}"/><emitter type="area"><color name="radiance" '
          f'value="{SPHERE_RADIANCE[0]}, {SPHERE_RADIANCE[1]}, {SPHERE_RADIANCE[2]}"/></emitter></shape>')
    s = nh.Scene(light_scenes.floor_scene_xml(str(tmp_path / "s.xml"), em))
    d = s.desc
    assert d.n_emitters == 1 and d.shapes[d.emitters[0].shape].type == nh.SHAPE_SPHERE
    c = nh.Context(0)
    c._check(nh.lib.nh_upload_scene(c._h, C.byref(d)), "upload_scene")
    ref, smp = sphere_inputs()
    r32, r64 = (er.sphere_sample(SPHERE_CENTER, SPHERE_RADIUS, SPHERE_RADIANCE, ref, smp, T) for T in (F32, F64))
    front, back = r64["cosl"] > 1e-3, r64["cosl"] < -1e-3
    assert front.sum() >= 64 and back.sum() >= 32
    g = c.emitter_query(0, ref, sample=smp)
    check_shadow_ray(g)
    assert np.all(g["value"][back] == 0) and np.all(g["pdf"][back] == 0)
    assert np.all(r64["value"][back] == 0) and np.all(r64["pdf"][back] == 0) and np.all(r64["pdf"][front] > EPS)
    compare("sphere", g, r32, r64, ("value", "pdf", "wi", "o", "maxt"), {"value": front, "pdf": front}, abs_gap)
    e = c.emitter_query(0, ref, wi=g["wi"], p=g["o"], n=r32["n"])
    rad = np.asarray(SPHERE_RADIANCE, F32)
    assert np.array_equal(e["value"][front], np.broadcast_to(rad, (int(front.sum()), 3)))
    assert np.all(e["value"][back] == 0) and np.all(e["pdf"][back] == 0)
    gap, err = rel_gap(r32["pdf"][front], r64["pdf"][front]), rel_gap(e["pdf"][front], r64["pdf"][front])
    print(f"sphere pdf query: fp32 gap {gap:.3g}, device {err:.3g}")
    assert err <= bound(gap)


# ---------------------------------------------------------------------------------------------------------------------
# 6. the mesh area light
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_mesh_area_light_cdf_boundaries_both_vertex_sources(gpu, tmp_path, monkeypatch):
    """AreaEmitter::sample on a mesh of five triangles of areas 0.02 .. 2.4, with sample.x at every area-CDF entry and
    its float neighbours, 0, 1 - ulp and 128 random values: the face pick and the sampleReuse remap
    (x - cdf[i]) / (cdf[i + 1] - cdf[i]) at its ends. Three uploads: the precomputed emit_faces records (default), the
    S.F / S.V path (NH_EMIT_FACES=0), and the same mesh with a normal per vertex (a mesh with normals has no emit_faces
    record: S.F / S.V / S.N and the interpolated normal). The face is exact, named by the plane o lies on. Queries with
    |cos| at the light above 1e-3 (over 90 %, asserted): o, wi, value, pdf, maxt within bound(gap); behind the light
    exactly 0. Measured, fp32 gap = device: o 5.4e-7 (absolute), wi 1.2e-7, value 4.2e-7 (3.2e-7 with normals), pdf
    3.9e-7 (2.9e-7), maxt 2.0e-7. The emit_faces and S.F / S.V records are bit-identical in all 16 floats (asserted
    within bound(gap) only)."""
    out = {}
    for source in ("emit_faces", "S.F", "S.F normals"):
        if source == "S.F":
            monkeypatch.setenv("NH_EMIT_FACES", "0")
        else:
            monkeypatch.delenv("NH_EMIT_FACES", raising=False)
        s = mesh_scene(str(tmp_path), normals=source == "S.F normals")
        V, N, Fc, cdf, norm = mesh_data(s)
        d = s.desc
        c = nh.Context(0)
        c._check(nh.lib.nh_upload_scene(c._h, C.byref(d)), "upload_scene")
        ref, smp = mesh_inputs(cdf)
        r32, r64 = (er.mesh_sample(V, N, Fc, cdf, norm, MESH_RADIANCE, ref, smp, T) for T in (F32, F64))
        raw = raw_sample(c, 0, ref, smp)
        c.close()
        g = {"value": raw[:, 0:3], "wi": raw[:, 3:6], "pdf": raw[:, 6], "o": raw[:, 7:10], "d": raw[:, 10:13],
             "mint": raw[:, 13], "maxt": raw[:, 14]}
        check_shadow_ray(g)
        assert np.array_equal(er.face_of_point(V, Fc, g["o"]), r64["face"]) and set(r64["face"]) == set(range(5))
        clear = np.abs(r64["cosl"]) > 1e-3
        behind = r64["cosl"] < -1e-3
        assert (~clear).mean() < 0.10 and behind.sum() >= 8
        assert np.all(g["value"][behind] == 0) and np.all(g["pdf"][behind] == 0)
        compare(f"mesh {source}", g, r32, r64, ("o", "wi", "value", "pdf", "maxt"), {"value": clear, "pdf": clear},
                abs_gap)
        out[source] = (raw, r32, r64, clear)
    (a, r32, r64, clear), (b, _, _, _) = out["emit_faces"], out["S.F"]
    same = np.array_equal(bits(a), bits(b))
    print(f"mesh: emit_faces and S.F / S.V records bit-identical: {same}")
    for k, sl in (("value", slice(0, 3)), ("wi", slice(3, 6)), ("pdf", 6), ("o", slice(7, 10)), ("maxt", 14)):
        fn = abs_gap if k in ("wi", "o") else rel_gap
        m = clear if k in ("value", "pdf") else slice(None)
        assert fn(a[:, sl][m], b[:, sl][m]) <= bound(fn(r32[k][m], r64[k][m])), k
