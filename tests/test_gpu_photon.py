"""The photon mapper on the GPU: codec, samplePhoton, the photon map, the gather and the camera pass.

Every test here fails on the commit before the photon mapper: the loader refuses the integrator there.
"""
import json
import os

import numpy as np
import pytest

import emitter_refs as er
import light_scenes
import nori_hip as nh
import nori_oracle as no
import photon_refs as pr
import volume_refs as vr

F32, F64 = np.float32, np.float64
EPS32 = float(np.finfo(F32).eps)
pytestmark = pytest.mark.gpu


def bits(a):
    return np.ascontiguousarray(a, F32).view(np.uint32)


def check(label, g, r32, r64):
    """the emitter tests' rule: bit for bit the fp32 restatement, or within 4 x the restatement's own fp32-to-fp64 gap
    (never below 4 float epsilons), both relative to max(1, |value|)"""
    g, r32, r64 = (np.asarray(x, F64) for x in (g, r32, r64))
    scale = np.maximum(1.0, np.abs(r64))
    gap = float(np.max(np.abs(r32 - r64) / scale))
    err = np.abs(g - r64) / scale
    ok = (bits(g) == bits(r32)) | (err <= 4.0 * max(gap, EPS32))
    print(f"{label}: max err {float(err.max()):.3e}, restatement gap {gap:.3e}, bit-equal {float(np.mean(bits(g) == bits(r32))):.3f}")
    assert ok.all(), (label, float(err.max()), gap)


CAMERA = ('<camera type="perspective"><transform name="toWorld"><lookat target="0,0,0" origin="0,3,6" up="0,1,0"/>'
          '</transform><integer name="width" value="16"/><integer name="height" value="16"/></camera>')


@pytest.fixture(scope="module")
def photon_dir(tmp_path_factory):
    """the reference's photon mapper scenes, in a directory of this module's own"""
    return pr.materialize(str(tmp_path_factory.mktemp("photon_scenes")))


@pytest.fixture(scope="module")
def ctx(gpu):
    c = nh.Context(gpu)
    yield c
    c.close()


# ---------------------------------------------------------------------------------------------------------------------
# 1. codec
# ---------------------------------------------------------------------------------------------------------------------
def test_codec_bin_centres(ctx):
    """directions at the centres of the 256 x 256 (theta, phi) bins, computed in fp64 (no input on a bin edge): the
    bytes name the bin, and bytes and decoded values equal the restatement bit for bit"""
    i, j = np.meshgrid(np.arange(256), np.arange(256), indexing="ij")
    theta = (i.ravel() + 0.5) * np.pi / 256
    phi = (j.ravel() + 0.5) * 2 * np.pi / 256
    d = np.stack([np.sin(theta) * np.cos(phi), np.sin(theta) * np.sin(phi), np.cos(theta)], -1).astype(F32)
    w = np.random.default_rng(1).uniform(0, 1, d.shape).astype(F32) * F32(2.0) ** np.random.default_rng(2).integers(-20, 20, (len(d), 1)).astype(F32)
    g = ctx.photon_codec(d, w)
    want = pr.encode(d, w)
    assert np.array_equal(g["bytes"], want)
    # theta names its bin. phi does for atan2 >= 0; for atan2 < 0 the constructor's int() truncates towards zero
    # before the + 256 wrap, so those bins come out one higher, and the last one as 0 (the reference's own behaviour)
    jj = j.ravel()
    assert np.array_equal(g["bytes"][:, 0], i.ravel())
    assert np.array_equal(g["bytes"][:, 1], np.where(jj < 128, jj, (jj + 1) % 256))
    dd, ww = pr.decode(want, nh.photon_tables())
    assert np.array_equal(bits(g["direction"]), bits(dd)) and np.array_equal(bits(g["power"]), bits(ww))
    # what the gather reads is a quantisation of the input: within a bin of the direction, within 1 / 128 of the power
    assert np.abs(g["direction"] - d).max() < (np.pi / 512 + 2 * np.pi / 512) * 1.01  # half a bin in each angle
    assert np.all(g["power"] <= w) and np.all(w - g["power"] <= w.max(1, keepdims=True) / 128 * 1.0001)


def test_codec_edge_cases(ctx):
    d = np.array([[0, 0, 1], [0, 0, -1], [1, 0, 0], [-1, -0.0, 0], [0, -1, 0], [0.6, -0.8, 0.0], [0, 1, 0]], F32)
    w = np.array([[1, 0.5, 0.25], [1e-33, 0, 0], [2, 2, 2], [0.75, 1e-4, 0], [3, 1, 2], [1e-32, 1e-33, 0], [4096, 1, 4095]], F32)
    g = ctx.photon_codec(d, w)
    want = pr.encode(d, w)
    assert np.array_equal(g["bytes"], want), (g["bytes"], want)
    assert list(g["bytes"][0]) == [0, 0, 128, 64, 32, 129]   # z = 1
    assert list(g["bytes"][1]) == [255, 0, 0, 0, 0, 0]       # z = -1: the 255 clamp; power below 1e-32: all zeros
    assert list(g["bytes"][2]) == [128, 0, 128, 128, 128, 130]  # maximum an exact power of two
    assert g["bytes"][3][1] == 128 and g["bytes"][4][1] == 192 and g["bytes"][5][1] > 128  # atan2 < 0: the + 256 wrap
    assert list(g["bytes"][3][2:]) == [192, 0, 0, 128]       # a component that truncates to 0
    dd, ww = pr.decode(want, nh.photon_tables())
    assert np.array_equal(bits(g["direction"]), bits(dd)) and np.array_equal(bits(g["power"]), bits(ww))
    assert np.array_equal(g["power"][1], F32([0, 0, 0]))


# ---------------------------------------------------------------------------------------------------------------------
# 2. samplePhoton
# ---------------------------------------------------------------------------------------------------------------------
RADIANCE = (5.0, 4.0, 3.0)


def mesh_light_scene(d, normals):
    name = "pm_five_n" if normals else "pm_five"
    er.five_triangles_obj(os.path.join(d, name + ".obj"), normals=normals)
    em = (f'<shape type="obj"><string name="filename" value="{name}.obj"/><emitter type="area">'
          f'<color name="radiance" value="{RADIANCE[0]}, {RADIANCE[1]}, {RADIANCE[2]}"/></emitter></shape>')
    # a second light: the `* lights.size()` factor is 2
    em += ('<shape type="sphere"><point name="center" value="3, 2, 3"/><float name="radius" value="0.25"/>'
           '<emitter type="area"><color name="radiance" value="1, 2, 3"/><float name="lightWeight" value="3"/></emitter></shape>')
    return nh.Scene(light_scenes.floor_scene_xml(os.path.join(d, name + ".xml"), em, integrator="photonmapper"))


def mesh_data(s, e=0):
    d = s.desc
    sh = d.shapes[d.emitters[e].shape]
    V, N = (np.array([[a[3 * (sh.v_offset + i) + k] for k in range(3)] for i in range(sh.n_vertices)], F32)
            if a else None for a in (d.V, d.N if sh.has_normals else None))
    Fc = np.array([[d.F[3 * (sh.f_offset + i) + k] for k in range(3)] for i in range(sh.n_faces)])
    cdf = np.array([d.area_cdf[sh.pdf_offset + i] for i in range(sh.n_faces + 1)], F32)
    return V, N, Fc, cdf, sh.pdf_normalization


def photon_samples(x, seed):
    rng = np.random.default_rng(seed)
    return np.concatenate([np.asarray(x, F32)[:, None], rng.uniform(0, 1, (len(x), 3)).astype(F32)], 1)


@pytest.mark.parametrize("normals", [False, True], ids=["face_normals", "vertex_normals"])
def test_sample_photon_mesh_light(ctx, tmp_path, normals):
    s = mesh_light_scene(str(tmp_path), normals)
    assert s.desc.n_emitters == 2
    ctx.upload(s, nh.Bvh(s), photon_map=False)
    V, N, Fc, cdf, norm = mesh_data(s)
    smp = photon_samples(er.search_samples(cdf, 7, n_random=128), 8)  # sample1.x on the CDF's edges and beside them
    g = ctx.sample_photon(0, smp)
    r32, r64 = (pr.sample_photon_mesh(V, N, Fc, cdf, norm, RADIANCE, smp, 2, T) for T in (F32, F64))
    for k in ("o", "d", "W", "pdf"):
        check(f"mesh {k}", g[k], r32[k], r64[k])
    assert np.array_equal(er.face_of_point(V, Fc, g["o"]), r64["face"])  # the CDF search picked the face
    assert np.all(np.abs(np.linalg.norm(g["d"].astype(F64), axis=1) - 1) < 1e-5)
    assert np.all(np.sum(g["d"].astype(F64) * r64["n"], 1) >= -1e-6)  # leaves on the normal's side


def test_sample_photon_sphere_light(ctx, tmp_path):
    s = mesh_light_scene(str(tmp_path), False)
    ctx.upload(s, nh.Bvh(s), photon_map=False)
    smp = np.random.default_rng(9).uniform(0, 1, (256, 4)).astype(F32)
    g = ctx.sample_photon(1, smp)
    r32, r64 = (pr.sample_photon_sphere((3, 2, 3), 0.25, (1, 2, 3), smp, 2, T) for T in (F32, F64))
    for k in ("o", "d", "W", "pdf"):
        check(f"sphere {k}", g[k], r32[k], r64[k])
    # W = pi * area * radiance * 2 lights
    assert np.allclose(g["W"][0], np.pi * 4 * np.pi * 0.25 ** 2 * np.array([1, 2, 3]) * 2, rtol=1e-5)


# ---------------------------------------------------------------------------------------------------------------------
# 3. the map
# ---------------------------------------------------------------------------------------------------------------------
MAP_SEED, MAP_N = 5, 20000


@pytest.fixture(scope="module")
def cbox(ctx, photon_dir):
    """cbox_pmap.xml cut to 32 x 32 and its map (seed MAP_SEED, MAP_N photons), shared and left unchanged"""
    s = nh.Scene(os.path.join(photon_dir, pr.CBOX_PMAP))
    s.set_resolution(32, 32)
    s.set_sample_count(2)
    s.set_photon_params(MAP_N, 0.05)
    return s, nh.Bvh(s)


@pytest.fixture(scope="module")
def cbox_map(ctx, cbox):
    s, b = cbox
    ctx.upload(s, b, photon_map=False)
    st = ctx.build_photon_map(seed=MAP_SEED)
    return st, ctx.photons()


def test_map_is_independent_of_the_launch(ctx, cbox, cbox_map):
    st, ph = cbox_map
    assert st["stored"] == MAP_N and len(ph["path"]) == MAP_N and st["radius"] == F32(0.05)
    for batch in (0, 1000, 7777):
        st2 = ctx.build_photon_map(seed=MAP_SEED, batch_paths=batch)
        ph2 = ctx.photons()
        assert st2 == st, (batch, st2, st)
        for k in ph:
            assert np.array_equal(ph[k].view(np.uint8), ph2[k].view(np.uint8)), (batch, k)
    other = ctx.build_photon_map(seed=MAP_SEED + 1)
    assert not np.array_equal(ctx.photons()["position"], ph["position"]) and other["stored"] == MAP_N
    ctx.build_photon_map(seed=MAP_SEED)  # leave the shared map in place


def test_map_order_and_emitted_count(cbox_map):
    st, ph = cbox_map
    key = ph["path"].astype(np.int64) * (1 << 20) + ph["bounce"]
    assert np.all(np.diff(key) > 0)                       # ascending in (path, bounce), no duplicates
    assert st["emitted"] == int(ph["path"][-1]) + 1       # the path that fills the map is the last one counted
    assert ph["bounce"].min() == 0 and ph["bounce"].max() >= 4  # roulette survivors deposit too
    assert 1.0 < MAP_N / st["emitted"] < 30.0             # a closed box: several deposits per path
    assert 0 < st["occupied_cells"] <= MAP_N and st["cell_size"] >= st["radius"]
    dd, ww = pr.decode(ph["bytes"], nh.photon_tables())
    assert np.array_equal(bits(dd), bits(ph["direction"])) and np.array_equal(bits(ww), bits(ph["power"]))


def test_first_bounce_photons_are_the_sampled_photons(ctx, cbox, cbox_map):
    """every bounce-0 photon of the first paths: its bytes are the codec of (-d, W) of samplePhoton fed with the path's
    own draws, and its position is where the oracle's ray from the sampled point lands, on a diffuse shape"""
    s, _ = cbox
    st, ph = cbox_map
    first = np.flatnonzero(ph["bounce"] == 0)[:300]
    smp = []
    for k in ph["path"][first]:
        rng = no.Pcg32.per_path(MAP_SEED, nh.PHOTON_STREAM, int(k))
        rng.next_float()  # the emitter choice (one emitter)
        smp.append([rng.next_float() for _ in range(4)])
    q = ctx.sample_photon(0, np.array(smp, F32))
    enc = ctx.photon_codec(-q["d"], q["W"])
    assert np.array_equal(enc["bytes"], ph["bytes"][first])
    n = len(first)
    mint, maxt = np.full(n, 1e-4, F32), np.full(n, np.inf, F32)
    hit = no.OracleScene(s).trace(q["o"], q["d"], mint, maxt)
    dev = ctx.trace(q["o"], q["d"], mint, maxt)
    assert hit["hit"].all()
    for k in ("shape", "prim", "t", "u", "v"):  # the device's traversal finds the oracle's shape and primitive
        assert np.array_equal(dev[k], hit[k]), k
    d = s.desc
    assert all(d.bsdfs[d.shapes[int(k)].bsdf].type == nh.BSDF_DIFFUSE for k in hit["shape"])
    # ... and the photon sits on that primitive, at the hit's barycentric coordinates (Mesh::setHitInformation)
    off = cbox[1].desc.shape_offset
    for i in range(n):
        sh = d.shapes[int(hit["shape"][i])]
        assert sh.type == nh.SHAPE_MESH
        f = 3 * (sh.f_offset + int(hit["prim"][i]) - off[int(hit["shape"][i])])
        v0, v1, v2 = (np.array([d.V[3 * (sh.v_offset + d.F[f + j]) + c] for c in range(3)], F32) for j in range(3))
        u, v = hit["u"][i], hit["v"][i]
        want = ((F32(1) - (u + v)) * v0 + u * v1) + v * v2
        assert np.abs(want - ph["position"][first[i]]).max() <= 1e-6, (i, want, ph["position"][first[i]])


def test_cbox_photons_avoid_the_specular_spheres(cbox, cbox_map):
    s, _ = cbox
    _, ph = cbox_map
    d = s.desc
    p = ph["position"].astype(F64)
    for i in range(d.n_shapes):
        sh = d.shapes[i]
        if sh.type == nh.SHAPE_SPHERE:  # the mirror and the dielectric sphere: nothing is stored on them
            assert d.bsdfs[sh.bsdf].type in (nh.BSDF_MIRROR, nh.BSDF_DIELECTRIC)
            dist = np.abs(np.linalg.norm(p - np.array(list(sh.center)), axis=1) - sh.radius)
            assert dist.min() > 1e-4
    lo = np.min([list(d.shapes[i].bbox_min) for i in range(d.n_shapes) if d.shapes[i].type == nh.SHAPE_MESH], 0)
    hi = np.max([list(d.shapes[i].bbox_max) for i in range(d.n_shapes) if d.shapes[i].type == nh.SHAPE_MESH], 0)
    assert np.all(p >= lo - 1e-4) and np.all(p <= hi + 1e-4)


SPECULAR_SCENE = ('<scene><integrator type="photonmapper"><integer name="photonCount" value="30000"/>'
                  '<float name="photonRadius" value="0.1"/></integrator>' + CAMERA +
                  '<shape type="sphere"><point name="center" value="0,5,0"/><float name="radius" value="0.3"/>'
                  '<emitter type="area"><color name="radiance" value="50,50,50"/></emitter></shape>'
                  '<shape type="sphere"><point name="center" value="0,-100,0"/><float name="radius" value="100"/>'
                  '<bsdf type="diffuse"><color name="albedo" value="0.5,0.5,0.5"/></bsdf></shape>'
                  '<shape type="sphere"><point name="center" value="-0.7,1.5,0"/><float name="radius" value="0.6"/>'
                  '<bsdf type="dielectric"/></shape>'
                  '<shape type="sphere"><point name="center" value="0.7,1.5,0"/><float name="radius" value="0.6"/>'
                  '<bsdf type="mirror"/></shape></scene>')


def test_photons_pass_the_specular_spheres_and_lie_on_diffuse_ones(ctx, tmp_path):
    """A dielectric and a mirror sphere between the light and the floor. Every photon lies on the floor or on the
    light (the two diffuse shapes), none on the specular spheres. The vertex before a photon is found with the oracle:
    a ray from the photon back along its stored direction (quantised to about 1.4 degrees) ends on the shape the photon
    came from. The floor and the light are convex and see each other but not themselves, so a floor photon of bounce
    >= 1 whose ray back ends on a specular sphere has passed it; through the glass takes two specular hits."""
    p = tmp_path / "specular.xml"
    p.write_text(SPECULAR_SCENE)
    s = nh.Scene(str(p))
    ctx.upload(s, nh.Bvh(s), photon_map=False)
    ctx.build_photon_map(seed=2)
    ph = ctx.photons()
    pos = ph["position"].astype(F64)
    d = s.desc
    dist = np.stack([np.abs(np.linalg.norm(pos - np.array(list(d.shapes[i].center)), axis=1) - d.shapes[i].radius)
                     for i in range(4)], -1)
    LIGHT_S, FLOOR_S, GLASS_S, MIRROR_S = 0, 1, 2, 3
    on = dist.argmin(-1)
    assert np.all(dist.min(-1) < 1e-4 * np.array([1, 100, 1, 1])[on])   # on a sphere's surface ...
    assert set(np.unique(on)) <= {LIGHT_S, FLOOR_S}                     # ... a diffuse one
    assert dist[:, GLASS_S].min() > 1e-3 and dist[:, MIRROR_S].min() > 1e-3
    later = np.flatnonzero((on == FLOOR_S) & (ph["bounce"] >= 1))
    n = len(later)
    back = no.OracleScene(s).trace(ph["position"][later], ph["direction"][later], np.full(n, 1e-4, F32),
                                   np.full(n, np.inf, F32))
    came = np.where(back["hit"] == 1, back["shape"].astype(int), -1)
    via_glass, via_mirror = later[came == GLASS_S], later[came == MIRROR_S]
    print("floor photons of bounce >= 1:", n, "from the glass", len(via_glass), "from the mirror", len(via_mirror))
    assert len(via_glass) > 50 and len(via_mirror) > 50
    # refraction through the sphere takes two specular hits, a reflection off it one
    assert np.sum(ph["bounce"][via_glass] >= 2) > 25
    # the caustic: photons through the glass gather under it, nearer its axis than its radius
    through = via_glass[ph["bounce"][via_glass] >= 2]
    assert np.median(np.hypot(pos[through, 0] + 0.7, pos[through, 2])) < 0.6


def test_all_mirror_scene_deposits_nothing(ctx, tmp_path):
    text = ('<scene><integrator type="photonmapper"/>' + CAMERA +
            '<shape type="sphere"><point name="center" value="0,3,0"/><float name="radius" value="0.5"/>'
            '<bsdf type="mirror"/><emitter type="area"><color name="radiance" value="10,10,10"/></emitter></shape>'
            '<shape type="sphere"><point name="center" value="0,-100,0"/><float name="radius" value="100"/>'
            '<bsdf type="mirror"/></shape></scene>')
    p = tmp_path / "mirrors.xml"
    p.write_text(text)
    s = nh.Scene(str(p))
    with pytest.raises(nh.NoriError, match="no photon reaches a diffuse surface"):
        ctx.upload(s, nh.Bvh(s))


# ---------------------------------------------------------------------------------------------------------------------
# 4. the gather
# ---------------------------------------------------------------------------------------------------------------------
def gather_points(ph, st, root_min, seed):
    rng = np.random.default_rng(seed)
    pos = ph["position"][rng.choice(len(ph["position"]), 64, replace=False)]
    r = F32(st["radius"])
    shifted = pos.copy()
    shifted[:, 0] = shifted[:, 0] + r  # displaced by exactly r along x: the photon itself sits on the strict bound
    cell = F32(st["cell_size"])
    origin = (np.asarray(root_min, F32) - F32(2) * cell).astype(F32)
    corners = (origin + np.floor((pos - origin) / cell).astype(F32) * cell).astype(F32)  # the photons' cell corners
    rand = rng.uniform(pos.min(0), pos.max(0), (64, 3)).astype(F32)
    return np.concatenate([pos, shifted, corners, rand])


def check_gather(ctx, ph, st, pts):
    g = ctx.photon_gather(pts)
    c32, c64, s64 = pr.gather(ph["position"], ph["power"], pts, st["radius"])
    print("gather: counts", int(g["count"].min()), "..", int(g["count"].max()), "fp32 / fp64 tests differ at",
          int(np.sum(c32 != c64)), "points")
    assert np.array_equal(g["count"], c32)
    # all terms are non-negative: a sequential fp32 sum of n terms is within n 2^-24 of the exact sum, relatively
    bound = np.maximum(c32, 1)[:, None] * 2.0 ** -24 * s64
    assert np.all(np.abs(g["power"].astype(F64) - s64) <= bound)
    return g


def test_gather_cbox(ctx, cbox):
    s, b = cbox
    c = nh.Context(0)  # a context of its own: 50 000 photons
    try:
        c.upload(s, b, photon_map=False)
        st = c.build_photon_map(seed=3, photon_count=50000)
        ph = c.photons()
        g = check_gather(c, ph, st, gather_points(ph, st, list(b.desc.bbox_min), 11))
        assert g["count"][:64].min() >= 1 and g["count"].max() > 20
    finally:
        c.close()


def test_gather_in_a_grid_of_more_than_2_32_cells(ctx, tmp_path):
    """a radius of 1 / 8000 of the floor: 8000^2 x thousands of cells, far beyond any dense array"""
    em = ('<shape type="sphere"><point name="center" value="0, 3, 0"/><float name="radius" value="0.5"/>'
          '<emitter type="area"><color name="radiance" value="10, 10, 10"/></emitter></shape>')
    s = nh.Scene(light_scenes.floor_scene_xml(str(tmp_path / "tiny.xml"), em, integrator="photonmapper"))
    s.set_photon_params(2000, 1e-3)
    b = nh.Bvh(s)
    ctx.upload(s, b, photon_map=False)
    st = ctx.build_photon_map(seed=1)
    ext = np.array(list(b.desc.bbox_max)) - np.array(list(b.desc.bbox_min))
    assert np.prod(np.floor(ext / st["cell_size"])) > 2.0 ** 32
    ph = ctx.photons()
    g = check_gather(ctx, ph, st, gather_points(ph, st, list(b.desc.bbox_min), 12))
    assert np.all(g["count"][:64] >= 1)


# ---------------------------------------------------------------------------------------------------------------------
# 5. the camera pass
# ---------------------------------------------------------------------------------------------------------------------
def test_render_needs_a_map(ctx, cbox):
    s, b = cbox
    c = nh.Context(0)
    try:
        c.upload(s, b, photon_map=False)
        with pytest.raises(nh.NoriError, match=r"needs a photon map.*rc=5"):
            c.render(0, 1, clear=True)
        with pytest.raises(nh.NoriError, match=r"needs a photon map.*rc=5"):
            c.radiance_query([0], 0)
    finally:
        c.close()


def test_render_is_finite_and_independent_of_how_it_is_split(ctx, photon_dir):
    s = nh.Scene(os.path.join(photon_dir, pr.CBOX_PMAP))
    s.set_resolution(64, 32)  # two 32 x 32 blocks
    s.set_sample_count(2)
    s.set_photon_params(MAP_N, 0.05)
    ctx.upload(s, nh.Bvh(s))  # builds the map with seed 0
    assert ctx.photon_stats()["stored"] == MAP_N
    ctx.render(0, 2, seed=4, clear=True)
    whole = ctx.framebuffer()
    assert np.isfinite(whole).all() and whole[..., :3].max() > 0
    border = s.border
    inner = whole[border:border + 32, border:border + 64]
    # the box is closed but for its front, which only the mirror sphere shows: nearly every pixel is lit
    assert np.all(inner[..., 3] > 0) and np.mean(inner[..., :3].sum(-1) > 0) > 0.9
    ctx.render(0, 1, seed=4, clear=True)
    round0 = ctx.framebuffer()
    ctx.render(1, 2, seed=4)
    assert np.array_equal(bits(ctx.framebuffer()), bits(whole))  # sample ranges [0, 1) + [1, 2)
    # blocks over two calls. A call adds the sum of its block images to the master block, so where two blocks' borders
    # overlap a split by blocks adds the same terms in another order unless the call is one round into a cleared
    # block: that is where the bit-for-bit statement holds, for every integrator
    ctx.render(0, 1, seed=4, clear=True, blocks=[0])
    ctx.render(0, 1, seed=4, blocks=[1])
    assert np.array_equal(bits(ctx.framebuffer()), bits(round0))
    ctx.render(1, 2, seed=4, clear=True)
    round1 = ctx.framebuffer()
    ctx.render(1, 2, seed=4, clear=True, blocks=[1])
    ctx.render(1, 2, seed=4, blocks=[0])
    assert np.array_equal(bits(ctx.framebuffer()), bits(round1))
    ctx.render(0, 2, seed=4, clear=True, blocks=[0])
    ctx.render(0, 2, seed=4, blocks=[1])
    np.testing.assert_allclose(ctx.framebuffer(), whole, rtol=1e-6, atol=0)  # two rounds: the same terms, regrouped
    ctx.render(0, 2, seed=4, clear=True, mode=nh.MODE_WAVEFRONT, traversal=nh.TRAVERSAL_ORDERED)
    assert np.array_equal(bits(ctx.framebuffer()), bits(whole))
    # the radiance query runs the same Li
    q = ctx.radiance_query([5 * 64 + 7, 20 * 64 + 40], [0, 1], seed=4)
    assert np.isfinite(q["rgb"]).all() and q["rgb"].sum() > 0
    # two rounds, bit for bit: blocks whose borders do not meet (128 x 32: blocks 0 and 2 are 32 pixels apart)
    s.set_resolution(128, 32)
    ctx.upload(s, nh.Bvh(s))
    ctx.render(0, 2, seed=4, clear=True, blocks=[0, 2])
    both = ctx.framebuffer()
    assert both[..., :3].max() > 0
    ctx.render(0, 2, seed=4, clear=True, blocks=[2])
    ctx.render(0, 2, seed=4, blocks=[0])
    assert np.array_equal(bits(ctx.framebuffer()), bits(both))


def test_radiance_at_a_diffuse_hit_is_the_density_estimate(ctx, tmp_path):
    """The centre ray of the floor scene's camera runs straight down onto the floor at the origin: its radiance is
    sum(power * albedo / pi) / (pi r^2) / E over the photons within r whose decoded direction lies above the floor,
    recomputed here in fp64 from nh_get_photons. About 200 photons; the device adds fp32 terms, so the relative
    difference is bounded by count * 2^-24 plus a few roundings per term: 1e-5."""
    em = ('<shape type="sphere"><point name="center" value="2.5, 3, 0"/><float name="radius" value="0.5"/>'
          '<emitter type="area"><color name="radiance" value="10, 8, 6"/></emitter></shape>')
    s = nh.Scene(light_scenes.floor_scene_xml(str(tmp_path / "est.xml"), em, integrator="photonmapper"))
    s.set_photon_params(20000, 0.5)
    ctx.upload(s, nh.Bvh(s))
    st, ph = ctx.photon_stats(), ctx.photons()
    near = pr.in_radius(ph["position"], [0, 0, 0], st["radius"], F32)
    assert ctx.photon_gather([[0, 0, 0]])["count"][0] == near.sum() > 50
    lit = near & (ph["direction"][:, 1] > 0)  # eval is zero for a direction in or below the surface
    r = float(st["radius"])
    want = ph["power"][lit].astype(F64).sum(0) * (0.5 / np.pi) / (np.pi * r * r) / st["emitted"]
    got = ctx.radiance_query([16 * 32 + 16], [0], seed=1, pixel_sample=[[16.0, 16.0]])["rgb"][0].astype(F64)
    print("density estimate:", got, want, "photons", int(lit.sum()), "of", int(near.sum()))
    np.testing.assert_allclose(got, want, rtol=1e-5, atol=0)


def test_render_agrees_with_the_path_tracer_in_the_mean(ctx, photon_dir):
    """cbox at 32 x 32: the image mean of the photon mapper (100 000 photons, r = 0.05, 16 spp) against path_mis at 64
    spp. The density estimate is biased only where the disc leaves the surface it lies on (within r = 0.05 of an edge
    of the 0.56-wide box: under a fifth of each face, where it loses at most half) and by the quantisation of the power
    (below 1 / 128); the Monte-Carlo error of both image means is well under 1 %. A wrong normalisation (pi r^2, E, the
    lights.size() factor, a missing 1 / pi) is off by a factor of 2 or more. Bound: 15 %."""
    s = nh.Scene(os.path.join(photon_dir, pr.CBOX_PMAP))
    s.set_resolution(32, 32)
    s.set_photon_params(100000, 0.05)
    b = nh.Bvh(s)
    ctx.upload(s, b)
    ctx.render(0, 16, seed=2, clear=True)
    pm = nh.to_rgb(ctx.framebuffer(), s.border).astype(F64)
    s.set_integrator(nh.INTEGRATOR_PATH_MIS)
    ctx.upload(s, b)
    ctx.render(0, 64, seed=2, clear=True)
    pt = nh.to_rgb(ctx.framebuffer(), s.border).astype(F64)
    ratio = pm.mean((0, 1)) / pt.mean((0, 1))
    print("photon mapper / path_mis image mean per channel:", ratio)
    assert np.all(np.abs(ratio - 1) < 0.15), ratio


def test_table_pmap_renders_one_sample(ctx, photon_dir):
    """scenes/pa4/table/table_pmap.xml as it is but for its size (32 x 32) and photon count (20 000 of 5 000 000)"""
    s = nh.Scene(os.path.join(photon_dir, pr.TABLE_PMAP))
    s.set_resolution(32, 32)
    s.set_photon_params(20000, 1.0)
    ctx.upload(s, nh.Bvh(s))
    st = ctx.photon_stats()
    assert st["stored"] == 20000 and st["emitted"] > 0
    ctx.render(0, 1, seed=1, clear=True)
    fb = ctx.framebuffer()
    assert np.isfinite(fb).all() and fb[..., :3].max() > 0


def test_a_pixel_that_sees_the_light_adds_its_radiance_to_the_gather(ctx, tmp_path):
    """The camera looks at the sphere light (diffuse, albedo 0.5) along the line to its centre: Li = Le, unweighted,
    plus the density estimate of the photons the floor sent back up onto the light. The estimate is recomputed in fp64
    from nh_get_photons at the hit point c - R d; GATHER there returns the same photons. Bound: as
    test_radiance_at_a_diffuse_hit_is_the_density_estimate, on the estimate's part of the value."""
    floor = vr.sphere((0, -50, 0), 50.0, bsdf="diffuse", albedo=(0.9, 0.9, 0.9))
    light = vr.sphere((0.2, 2.0, 0.1), 0.5, bsdf="diffuse", albedo=(0.5, 0.5, 0.5), radiance=(20, 16, 12))
    o, c = np.array([3.0, 1.0, -4.0]), np.array(light["center"])
    S = vr.SphereScene([floor, light], [], None, o, c - o)
    p = tmp_path / "see_light.xml"
    p.write_text(pr.photon_scene_xml(S, [1.0], 50000, 0.5))
    s = nh.Scene(str(p))
    ctx.upload(s, nh.Bvh(s))
    st, ph = ctx.photon_stats(), ctx.photons()
    x = c - 0.5 * S.direction
    near = pr.in_radius(ph["position"], x.astype(F32), st["radius"], F32)
    g = ctx.photon_gather([x])
    assert g["count"][0] == near.sum() > 20
    n = -S.direction  # the light's normal at x
    lit = near & (ph["direction"].astype(F64) @ n > 0)
    r = float(st["radius"])
    est = ph["power"][lit].astype(F64).sum(0) * (0.5 / np.pi) / (np.pi * r * r) / st["emitted"]
    got = ctx.radiance_query([4 * 8 + 4], [0], seed=1, pixel_sample=[[4.0, 4.0]])["rgb"][0].astype(F64)
    le = np.array([20.0, 16.0, 12.0])
    print("light pixel:", got, "Le", le, "estimate", est, "photons", int(lit.sum()), "of", int(near.sum()))
    assert np.all(est > 0)
    np.testing.assert_allclose(got - le, est, rtol=1e-5, atol=float(np.finfo(F32).eps) * 20.0)
    if lit.sum() == near.sum():  # every photon in the ball counts: the radiance plus the GATHER value, scaled
        np.testing.assert_allclose(got, le + g["power"][0].astype(F64) * (0.5 / np.pi) / (np.pi * r * r) / st["emitted"],
                                   rtol=1e-5)


# ---------------------------------------------------------------------------------------------------------------------
# 6. the estimator against the fp64 Monte-Carlo restatement (tests/golden/photon_mc.json)
# ---------------------------------------------------------------------------------------------------------------------
M_MAPS, N_COMPARISONS = 32, 3  # as tests/test_photon_host.py fixed them: 32 maps reject the quirks=False estimator


@pytest.mark.parametrize("name", ["one", "two", "glass"])
def test_estimator_matches_the_monte_carlo_restatement(ctx, tmp_path, name):
    """M_MAPS maps with seeds 0 .. M_MAPS - 1, the radiance of one fixed pixel sample per map (camera path m on the
    stream of sample m), against the fixture's samples of the same estimator: volume_refs' two-sample t-test at the
    reference's 0.01, Sidak-corrected over the three comparisons of this file. `two` has lightWeight 1 and 3: the
    estimator with the true selection probability lies a factor 2 away there and is rejected (test_photon_host.py)."""
    with open(pr.PHOTON_MC_FIXTURE) as f:
        fx = json.load(f)
    S, weights = pr.mc_scenes()[name]
    p = tmp_path / f"mc_{name}.xml"
    p.write_text(pr.photon_scene_xml(S, weights, fx["photon_count"], fx["radius"]))
    s = nh.Scene(str(p))
    assert s.desc.n_emitters == len(weights) and s.photon_params() == (fx["photon_count"], fx["radius"])
    ctx.upload(s, nh.Bvh(s), photon_map=False)
    lum = []
    for m in range(M_MAPS):
        ctx.build_photon_map(seed=m)
        rgb = ctx.radiance_query([4 * 8 + 4], [m], seed=m, pixel_sample=[[4.0, 4.0]])["rgb"][0].astype(F64)
        lum.append(float(er.luminance(rgb, F64)))
    ma, sa, da = vr.seeds_estimate(lum)
    mb, sb, _ = vr.seeds_estimate(fx["scenes"][name]["quirks"]["luminance"])
    r = vr.t_test(ma, sa, da, mb, sb, N_COMPARISONS)
    print(f"{name}: device {ma:.5f} +- {sa:.5f} ({M_MAPS} maps), restatement {mb:.5f} +- {sb:.5f}, {r}")
    assert r["pass"], (name, ma, mb, r)
    if name == "two":
        mq, sq, _ = vr.seeds_estimate(fx["scenes"]["two"]["no_quirks"]["luminance"])
        assert not vr.t_test(ma, sa, da, mq, sq, N_COMPARISONS)["pass"]
