// Scene and BVH upload of the C-ABI (include/nori_hip.h): nh_upload_scene turns an nh_scene_desc into the device
// records of nh_device.h, nh_upload_bvh uploads the GPU BVH that host/gpu_layout.cpp lays out and builds the LDS image
// of a small scene. The context is nh_ctx.h's.
#include <cmath>
#include <cstdlib>
#include <cstring>

#include "../host/gpu_layout.h"
#include "nh_ctx.h"

using nhd::DBsdf;
using nhd::DEmitter;
using nhd::DShape;

// the host layout code's plain structs are uploaded as the HIP vector types the kernels read
static_assert(sizeof(nh::f4) == sizeof(float4) && alignof(float4) % alignof(nh::f4) == 0, "nh::f4 is float4's layout");
static_assert(sizeof(nh::i2) == sizeof(int2) && alignof(int2) % alignof(nh::i2) == 0, "nh::i2 is int2's layout");
static_assert(sizeof(nh::u64x2) == sizeof(ulonglong2) && alignof(ulonglong2) % alignof(nh::u64x2) == 0,
              "nh::u64x2 is ulonglong2's layout");
static_assert((int)nhd::BSDF_DIELECTRIC == (int)NH_BSDF_DIELECTRIC, "the isolated-sphere marking reads NH_BSDF_*");

// The DDisney side record of a Disney nh_bsdf: its ten parameters (the loader's clamped values); the folded fields
// are written on the device (disney_upload)
nhd::DDisney disney_record(const nh_bsdf &b) {
    nhd::DDisney o;
    std::memset(&o, 0, sizeof(o));
    o.metallic = b.metallic; o.subsurface = b.subsurface; o.specular = b.specular; o.roughness = b.roughness;
    o.specular_tint = b.specular_tint; o.anisotropic = b.anisotropic; o.sheen = b.sheen; o.sheen_tint = b.sheen_tint;
    o.clearcoat = b.clearcoat; o.clearcoat_gloss = b.clearcoat_gloss;
    return o;
}
// a Disney DBsdf names its side record by address (nh_device.h DBsdf::disney_lo / disney_hi, disney_rec)
void disney_set_record(nhd::DBsdf &o, const nhd::DDisney *rec) {
    const uint64_t a = (uint64_t)reinterpret_cast<uintptr_t>(rec);
    o.disney_lo = (uint32_t)a;
    o.disney_hi = (uint32_t)(a >> 32);
}
// Uploads the side records and folds their constants on the device (nh_disney.hip disney_fold_kernel: everything of
// Disney::eval that does not depend on the directions, by the device's own float operations -- as cam_o and
// emit_faces are formed once at upload). albedo: 3 floats per record.
int disney_upload(nh_ctx *c, std::vector<void *> &owner, const std::vector<nhd::DDisney> &recs,
                  const std::vector<float> &albedo, nhd::DDisney **out) {
    const nhd::DDisney *d_recs = nullptr;
    const float *d_alb = nullptr;
    if (int rc = upload(c, owner, recs.data(), recs.size(), &d_recs)) return rc;
    if (int rc = upload(c, owner, albedo.data(), albedo.size(), &d_alb)) return rc;
    *out = const_cast<nhd::DDisney *>(d_recs);
    nh_disney::nh::launch_disney_fold(*out, d_alb, (int)recs.size(), c->stream);
    HIP_TRY(c, hipGetLastError());
    HIP_TRY(c, hipStreamSynchronize(c->stream));  // (the host vectors are the caller's locals)
    return NH_OK;
}

namespace {

// DScene::emit_faces: each emitting face's vertices and the normal Mesh::sampleSurface computes for it
// (normalized(cross(p1 - p0, p2 - p0)), mesh.cpp:64-69), by the device functions the light sample would run
__global__ void emit_face_kernel(const float *V, const uint4 *tri, int n, float4 *out) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const uint4 t = tri[i];
    const nhd::F3 p0 = nhd::ldv(V, t.x), p1 = nhd::ldv(V, t.y), p2 = nhd::ldv(V, t.z);
    const nhd::F3 nn = nhd::normalized(nhd::cross(nhd::sub(p1, p0), nhd::sub(p2, p0)));
    out[3 * i] = make_float4(p0.x, p0.y, p0.z, nn.x);
    out[3 * i + 1] = make_float4(p1.x, p1.y, p1.z, nn.y);
    out[3 * i + 2] = make_float4(p2.x, p2.y, p2.z, nn.z);
}

}  // namespace

extern "C" {

int nh_upload_scene(nh_ctx *c, const nh_scene_desc *d) {
    if (!c || !d) return NH_ERR_INVALID;
    HIP_TRY(c, hipSetDevice(c->device));
    if (int rc_ = pipeline_drain(c)) return rc_;
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    if (d->camera.width <= 0 || d->camera.height <= 0) return fail(c, "invalid camera resolution"), NH_ERR_INVALID;
    if (d->envmap >= 0) {
        const nh_envmap &e = d->env;
        if ((uint32_t)d->envmap >= d->n_emitters || d->emitters[d->envmap].type != NH_EMITTER_ENVMAP)
            return fail(c, "envmap index does not name an envmap emitter"), NH_ERR_INVALID;
        if (e.width <= 0 || e.height <= 0 || !e.rgba || !e.cdf) return fail(c, "invalid envmap texture"), NH_ERR_INVALID;
    }
    free_all(c->scene_bufs);
    free_all(c->bvh_bufs);
    c->has_scene = c->has_bvh = false;
    c->px.have_list = false;
    drop_primary_masks(c);
    c->camera = d->camera;

    std::vector<DShape> ds(d->n_shapes);
    for (uint32_t i = 0; i < d->n_shapes; ++i) {
        const nh_shape &s = d->shapes[i];
        // a shape with a medium may have no BSDF (bsdf = -1; Shape::cloneAndInit, shape.cpp:33-35): only the volumetric
        // integrators render such a scene (nh_render)
        const uint32_t sm = d->shape_medium ? d->shape_medium[i] : 0u;
        if (sm > d->n_media || (sm && !d->media)) return fail(c, "shape medium index out of range"), NH_ERR_INVALID;
        if (s.bsdf == -1 && !sm) return fail(c, "shape without a BSDF and without a medium"), NH_ERR_INVALID;
        if (s.bsdf < -1 || (s.bsdf >= 0 && (uint32_t)s.bsdf >= d->n_bsdfs))
            return fail(c, "shape without a valid BSDF"), NH_ERR_INVALID;
        const bool bsdf_tex = s.bsdf >= 0 &&
                              (d->bsdfs[s.bsdf].type == NH_BSDF_DIFFUSE || d->bsdfs[s.bsdf].type == NH_BSDF_DISNEY) &&
                              d->bsdfs[s.bsdf].albedo_texture != 0;
        DShape &o = ds[i];
        std::memset(&o, 0, sizeof(o));
        o.type = s.type;
        o.bsdf = s.bsdf;
        o.emitter = s.emitter;
        o.v_off = (int)s.v_offset;
        o.f_off = (int)s.f_offset;
        o.n_faces = (int)s.n_faces;
        o.has_n = s.has_normals;
        o.has_uv = s.has_uvs;
        o.cx = s.center[0]; o.cy = s.center[1]; o.cz = s.center[2];
        o.radius = s.radius;
        o.pdf_off = (int)s.pdf_offset;
        o.pdf_norm = s.pdf_normalization;
        if (s.normal_map > d->n_textures || (s.normal_map && !d->textures))
            return fail(c, "shape normal map index out of range"), NH_ERR_INVALID;
        // bit 0: uv read (textured albedo or normal map); bits 1+: 1 + the normal map's texture index
        o.tex_uv = ((int)s.normal_map << 1) | (bsdf_tex || s.normal_map ? 1 : 0);
        o.ef_off = -1;
    }
    // emitting meshes without vertex normals: one emit_faces record per face (vertex index triples here)
    std::vector<uint4> ef_tri;
    if (!(std::getenv("NH_EMIT_FACES") && std::getenv("NH_EMIT_FACES")[0] == '0'))
        for (uint32_t i = 0; i < d->n_shapes; ++i) {
            const nh_shape &s = d->shapes[i];
            if (s.type != NH_SHAPE_MESH || s.emitter < 0 || s.has_normals) continue;
            if ((uint64_t)s.f_offset + s.n_faces > d->n_faces) return fail(c, "shape faces out of range"), NH_ERR_INVALID;
            ds[i].ef_off = (int)ef_tri.size();
            for (uint32_t f = 0; f < s.n_faces; ++f) {
                const uint32_t *fi = &d->F[3 * ((size_t)s.f_offset + f)];
                const uint32_t i0 = s.v_offset + fi[0], i1 = s.v_offset + fi[1], i2 = s.v_offset + fi[2];
                if (i0 >= d->n_vertices || i1 >= d->n_vertices || i2 >= d->n_vertices)
                    return fail(c, "face vertex index out of range"), NH_ERR_INVALID;
                ef_tri.push_back(make_uint4(i0, i1, i2, 0u));
            }
        }
    std::vector<DBsdf> db(d->n_bsdfs);
    // Disney BSDFs: a DDisney side record each (the DBsdf holds its address), and the albedo its constants fold
    std::vector<nhd::DDisney> dz;
    std::vector<float> dz_albedo;
    std::vector<uint32_t> dz_owner;
    for (uint32_t i = 0; i < d->n_bsdfs; ++i) {
        const nh_bsdf &b = d->bsdfs[i];
        if (b.type < NH_BSDF_DIFFUSE || b.type > NH_BSDF_DISNEY) return fail(c, "unknown BSDF type"), NH_ERR_INVALID;
        if (b.type == NH_BSDF_DISNEY) {
            dz.push_back(disney_record(b));
            dz_albedo.insert(dz_albedo.end(), b.albedo, b.albedo + 3);
            dz_owner.push_back(i);
        }
        DBsdf &o = db[i];
        std::memset(&o, 0, sizeof(o));
        o.type = b.type;
        o.ar = b.albedo[0]; o.ag = b.albedo[1]; o.ab = b.albedo[2];
        o.alpha = b.alpha; o.int_ior = b.int_ior; o.ext_ior = b.ext_ior; o.ks = b.ks;
        o.kr = b.kd[0]; o.kg = b.kd[1]; o.kb = b.kd[2];
        if (b.albedo_texture > d->n_textures || (b.albedo_texture && !d->textures))
            return fail(c, "BSDF albedo texture index out of range"), NH_ERR_INVALID;
        o.tex = b.type == NH_BSDF_DIFFUSE || b.type == NH_BSDF_DISNEY ? (int)b.albedo_texture : 0;
    }
    if (!dz.empty()) {
        nhd::DDisney *recs = nullptr;
        if (int rc_ = disney_upload(c, c->scene_bufs, dz, dz_albedo, &recs)) return rc_;
        for (size_t k = 0; k < dz_owner.size(); ++k) disney_set_record(db[dz_owner[k]], recs + k);
    }
    std::vector<nhd::DTex> dt(d->n_textures);
    for (uint32_t i = 0; i < d->n_textures; ++i) {
        const nh_texture &t = d->textures[i];
        nhd::DTex &o = dt[i];
        std::memset(&o, 0, sizeof(o));
        if (t.type < NH_TEXTURE_CONSTANT || t.type > NH_TEXTURE_PNG) return fail(c, "unknown texture type"), NH_ERR_INVALID;
        if (t.type == NH_TEXTURE_PNG &&
            (t.width <= 0 || t.height <= 0 || !d->texels ||
             t.texel_offset + (uint64_t)t.width * (uint64_t)t.height > d->n_texels))
            return fail(c, "png texture outside the scene's texels"), NH_ERR_INVALID;
        o.type = t.type;
        o.w = t.width; o.h = t.height; o.spherical = t.spherical;
        o.v1r = t.value1[0]; o.v1g = t.value1[1]; o.v1b = t.value1[2];
        o.v2r = t.value2[0]; o.v2g = t.value2[1]; o.v2b = t.value2[2];
        o.dx = t.delta[0]; o.dy = t.delta[1]; o.sx = t.scale[0]; o.sy = t.scale[1];
        o.su = t.scale_u; o.sv = t.scale_v; o.ou = t.offset_u; o.ov = t.offset_v;
        o.off = (long long)t.texel_offset;
        std::memcpy(o.rot, t.rotation, sizeof(o.rot));
        o.linear = t.type == NH_TEXTURE_PNG && t.linear;
        o.intensity = t.intensity;
    }
    std::vector<DEmitter> de(d->n_emitters);
    std::vector<nhd::DEmitterExt> dx;  // spot / directional lights: n_emitters records (else empty)
    for (uint32_t i = 0; i < d->n_emitters; ++i) {
        const nh_emitter &e = d->emitters[i];
        if (e.type < NH_EMITTER_AREA || e.type > NH_EMITTER_DIRECTIONAL)
            return fail(c, "unknown emitter type"), NH_ERR_INVALID;
        if (e.type == NH_EMITTER_ENVMAP && (int32_t)i != d->envmap)
            return fail(c, "only one environment map per scene is supported"), NH_ERR_UNSUPPORTED;
        DEmitter &o = de[i];
        std::memset(&o, 0, sizeof(o));
        o.type = e.type;
        o.shape = e.shape;
        o.lr = e.radiance[0]; o.lg = e.radiance[1]; o.lb = e.radiance[2];
        o.px = e.position[0]; o.py = e.position[1]; o.pz = e.position[2];
        if (e.type == NH_EMITTER_SPOT || e.type == NH_EMITTER_DIRECTIONAL) {
            if (!d->emitter_ext) return fail(c, "spot / directional emitter without emitter_ext"), NH_ERR_INVALID;
            const nh_emitter_ext &x = d->emitter_ext[i];
            float len2 = 0.f;
            for (int k = 0; k < 3; ++k) len2 += x.direction[k] * x.direction[k];
            if (!std::isfinite(len2) || !(len2 > 0.f))
                return fail(c, "spot / directional emitter with a zero or non-finite direction"), NH_ERR_INVALID;
            static_assert(sizeof(nh_emitter_ext) == sizeof(nhd::DEmitterExt), "nh_emitter_ext is DEmitterExt's layout");
            if (dx.empty()) dx.resize(d->n_emitters);  // (zero records for the other emitters: never read)
            std::memcpy(&dx[i], &x, sizeof(x));
            o.shape = (int)i;  // the light's DScene::emitter_ext entry
        }
    }
    // participating media: the table as it stands (nh_medium is DMedium's leading part) and the per-shape side table
    std::vector<nhd::DMedium> dm(d->n_media);
    std::vector<int> shape_medium;
    if (d->n_media && !d->media) return fail(c, "media table missing"), NH_ERR_INVALID;
    if (d->ambient_medium > d->n_media) return fail(c, "ambient medium index out of range"), NH_ERR_INVALID;
    for (uint32_t i = 0; i < d->n_media; ++i) {
        const nh_medium &m = d->media[i];
        if (m.type < NH_MEDIUM_VACUUM || m.type > NH_MEDIUM_HOMOG) return fail(c, "unknown medium type"), NH_ERR_INVALID;
        if (m.phase < NH_PHASE_ISO || m.phase > NH_PHASE_HG) return fail(c, "unknown phase function type"), NH_ERR_INVALID;
        static_assert(sizeof(nh_medium) <= sizeof(nhd::DMedium), "nh_medium is DMedium's leading part");
        std::memset(&dm[i], 0, sizeof(dm[i]));
        std::memcpy(&dm[i], &m, sizeof(m));
    }
    c->bsdfless = false;
    c->has_media = false;
    for (uint32_t i = 0; i < d->n_shapes; ++i) c->bsdfless = c->bsdfless || d->shapes[i].bsdf < 0;
    for (uint32_t i = 0; i < d->n_media; ++i) c->has_media = c->has_media || d->media[i].type != NH_MEDIUM_VACUUM;
    if (d->n_media && d->shape_medium) shape_medium.assign(d->shape_medium, d->shape_medium + d->n_shapes);
    nhd::DScene &S = c->S;
    std::memset(&S, 0, sizeof(S));
    int rc;
    if (!dm.empty() && (rc = upload(c, c->scene_bufs, dm.data(), dm.size(), &S.media))) return rc;
    if (!shape_medium.empty() && (rc = upload(c, c->scene_bufs, shape_medium.data(), shape_medium.size(), &S.shape_medium)))
        return rc;
    S.ambient_medium = (int)d->ambient_medium;
    S.n_media = (int)d->n_media;
    const size_t nv = d->n_vertices;
    if ((rc = upload(c, c->scene_bufs, ds.data(), ds.size(), &S.shapes))) return rc;
    if ((rc = upload(c, c->scene_bufs, db.data(), db.size(), &S.bsdfs))) return rc;
    if ((rc = upload(c, c->scene_bufs, de.data(), de.size(), &S.emitters))) return rc;
    if ((rc = upload(c, c->scene_bufs, d->emitter_cdf, (size_t)d->n_emitters + 1, &S.emitter_cdf))) return rc;
    if (!dx.empty() && (rc = upload(c, c->scene_bufs, dx.data(), dx.size(), &S.emitter_ext))) return rc;
    if ((rc = upload(c, c->scene_bufs, d->V, 3 * nv, &S.V))) return rc;
    if ((rc = upload(c, c->scene_bufs, d->N, 3 * nv, &S.N))) return rc;
    if ((rc = upload(c, c->scene_bufs, d->UV, 2 * nv, &S.UV))) return rc;
    if ((rc = upload(c, c->scene_bufs, d->T, 3 * nv, &S.T))) return rc;
    if ((rc = upload(c, c->scene_bufs, d->BT, 3 * nv, &S.BT))) return rc;
    if ((rc = upload(c, c->scene_bufs, d->F, 3 * (size_t)d->n_faces, &S.F))) return rc;
    S.emit_faces = nullptr;
    if (!ef_tri.empty()) {
        const uint4 *tri = nullptr;
        if ((rc = upload(c, c->scene_bufs, ef_tri.data(), ef_tri.size(), &tri))) return rc;
        float4 *faces = nullptr;
        HIP_TRY(c, hipMalloc(&faces, 3 * ef_tri.size() * sizeof(float4)));
        c->scene_bufs.push_back(faces);
        const int n = (int)ef_tri.size();
        hipLaunchKernelGGL(emit_face_kernel, dim3((n + 255) / 256), dim3(256), 0, c->stream, S.V, tri, n, faces);
        HIP_TRY(c, hipGetLastError());
        S.emit_faces = faces;
    }
    if ((rc = upload(c, c->scene_bufs, d->area_cdf, (size_t)d->n_area_cdf, &S.area_cdf))) return rc;
    if (!dt.empty() && (rc = upload(c, c->scene_bufs, dt.data(), dt.size(), &S.texs))) return rc;
    if (d->n_texels) {
        const float *tx = nullptr;
        if ((rc = upload(c, c->scene_bufs, d->texels, 4 * (size_t)d->n_texels, &tx))) return rc;
        S.texels = reinterpret_cast<const float4 *>(tx);
    }
    S.envmap = d->envmap;
    if (d->envmap >= 0) {
        const nh_envmap &e = d->env;
        const size_t texels = (size_t)e.width * (size_t)e.height;
        const float *rgba = nullptr;
        if ((rc = upload(c, c->scene_bufs, e.rgba, 4 * texels, &rgba))) return rc;
        S.env_rgba = reinterpret_cast<const float4 *>(rgba);
        if ((rc = upload(c, c->scene_bufs, e.cdf, texels + 1, &S.env_cdf))) return rc;
        // guide table of the CDF search (nh_device.h dpdf_sample_guided): guide[j] = the first index i in [0, n]
        // with !(cdf[i] < j / 2^bits) (n + 1 if none), the same float comparison as the device's search; about 4
        // texels per bracket (NH_ENV_GUIDE=0: the plain search)
        S.env_guide = nullptr;
        S.env_guide_bits = 0;
        // (only for a non-decreasing CDF without NaN, where the first entry not below x is monotone in x)
        bool monotone = true;
        for (size_t i = 0; i <= texels && monotone; ++i)
            monotone = !std::isnan(e.cdf[i]) && (i == 0 || !(e.cdf[i] < e.cdf[i - 1]));
        if (monotone && texels >= 64 && !(std::getenv("NH_ENV_GUIDE") && std::getenv("NH_ENV_GUIDE")[0] == '0')) {
            int bits = 0;
            while (bits < 20 && ((size_t)1 << (bits + 2)) < texels) ++bits;
            const size_t M = (size_t)1 << bits;
            std::vector<int> guide(M + 1);
            size_t i = 0;
            for (size_t j = 0; j <= M; ++j) {
                const float t = (float)((double)j / (double)M);  // exact: j / 2^bits
                while (i <= texels && e.cdf[i] < t) ++i;
                guide[j] = (int)i;
            }
            const int *g = nullptr;
            if ((rc = upload(c, c->scene_bufs, guide.data(), guide.size(), &g))) return rc;
            HIP_TRY(c, hipStreamSynchronize(c->stream));  // (guide is a local)
            S.env_guide = g;
            S.env_guide_bits = bits;
        }
        S.env_w = e.width;
        S.env_h = e.height;
        S.env_spherical = e.spherical;
        std::memcpy(S.env_rot, e.rotation, sizeof(S.env_rot));
        S.env_constant = e.constant;
        S.env_norm = e.normalization;
        S.env_su = e.scale_u;
        S.env_sv = e.scale_v;
        S.env_ou = e.offset_u;
        S.env_ov = e.offset_v;
        S.env_r = e.radiance[0];
        S.env_g = e.radiance[1];
        S.env_b = e.radiance[2];
    }
    S.n_emitters = (int)d->n_emitters;
    S.nee_finite = nh::nee_finite(d) ? 1 : 0;
    if (d->integrator < NH_INTEGRATOR_PATH_MIS || d->integrator > NH_INTEGRATOR_ENVMAPTESTER)
        return fail(c, "unknown integrator"), NH_ERR_INVALID;
    S.integrator = d->integrator;
    S.av_length = 0.f;  // nh_set_av_params
    for (int i = 0; i < 3; ++i) S.ndir[i] = d->normals_direction[i];
    std::memcpy(S.s2c, d->camera.sample_to_camera, sizeof(S.s2c));
    std::memcpy(S.c2w, d->camera.camera_to_world, sizeof(S.c2w));
    {  // camera_ray's origin for a (0, 0, 0) local origin (nh_shade.h): the same operations in the same order
        float ow[4];
        const float z = 0.0f;
        for (int i = 0; i < 4; ++i) {
            float acc = S.c2w[4 * i] * z;
            acc = acc + S.c2w[4 * i + 1] * z;
            acc = acc + S.c2w[4 * i + 2] * z;
            acc = acc + S.c2w[4 * i + 3] * 1.0f;
            ow[i] = acc;
        }
        for (int i = 0; i < 3; ++i) S.cam_o[i] = ow[i] / ow[3];
    }
    S.inv_w = d->camera.inv_output_size[0];
    S.inv_h = d->camera.inv_output_size[1];
    S.near_clip = d->camera.near_clip;
    S.far_clip = d->camera.far_clip;
    S.width = d->camera.width;
    S.height = d->camera.height;
    // depth of field (perspective.cpp:114: lensRadius > Epsilon): each pixel's camera-ray position within a sample
    // round of the serial render order, which places its lens sample in the camera's static pcg32 stream
    // (nh_shade.h lens_uniform)
    S.dof = d->camera.lens_radius > 1e-4f ? 1 : 0;
    S.lens_radius = d->camera.lens_radius;
    S.focal_distance = d->camera.focal_distance;
    S.lens_rtl = d->camera.lens_draw_order == NH_LENS_DRAWS_RTL ? 1 : 0;
    S.lens_pix = S.lens_lo = nullptr;
    S.lens_hi = nullptr;
    if (S.dof) {
        const nh::LensTables lt = nh::lens_tables(S.width, S.height);
        const nh::u64x2 *pix = nullptr, *lo = nullptr;
        if ((rc = upload(c, c->scene_bufs, lt.pix.data(), lt.pix.size(), &pix))) return rc;
        if ((rc = upload(c, c->scene_bufs, lt.lo.data(), lt.lo.size(), &lo))) return rc;
        if ((rc = upload(c, c->scene_bufs, lt.hi.data(), lt.hi.size(), &S.lens_hi))) return rc;
        S.lens_pix = reinterpret_cast<const ulonglong2 *>(pix);
        S.lens_lo = reinterpret_cast<const ulonglong2 *>(lo);
        HIP_TRY(c, hipStreamSynchronize(c->stream));  // (the tables are locals)
    }
    S.filter_radius = d->filter.radius;
    S.lookup = d->filter.lookup_factor;
    S.border = d->filter.border;
    std::memcpy(S.table, d->filter.table, sizeof(S.table));

    c->shapes.assign(d->shapes, d->shapes + d->n_shapes);
    c->shape_bsdf_type.clear();
    c->shape_bsdf_real.clear();
    unsigned types = 0;
    for (uint32_t i = 0; i < d->n_shapes; ++i) {
        // 0..4 (checked above); a shape without a BSDF ranks with the diffuse ones (the key only orders shading work)
        const int t = d->shapes[i].bsdf < 0 ? NH_BSDF_DIFFUSE : d->bsdfs[d->shapes[i].bsdf].type;
        c->shape_bsdf_real.push_back(t);
        types |= 1u << t;
    }
    // The material key of the sorted queues is two bits of the primitive record (nh_traverse.h kPrimMatShift), four
    // classes, and only orders the shading work (which lane shades which path). The four older types keep their own
    // value; Disney takes the key of a type the scene does not use -- microfacet's, else mirror's, else dielectric's,
    // else diffuse's -- so it ranks as a class of its own in every scene but one that uses all five types, where it
    // shares diffuse's (both sample the cosine lobe). Every reader of the key only ranks by it; the isolated-sphere
    // marking reads the shape's real type (shape_bsdf_real).
    int disney_key = 0;
    for (int k : {NH_BSDF_MICROFACET, NH_BSDF_MIRROR, NH_BSDF_DIELECTRIC, NH_BSDF_DIFFUSE})
        if (!(types & (1u << k))) {
            disney_key = k;
            break;
        }
    for (int t : c->shape_bsdf_real) c->shape_bsdf_type.push_back(t == NH_BSDF_DISNEY ? disney_key : t);
    c->disney = (types & (1u << NH_BSDF_DISNEY)) != 0;
    // a spot / directional light takes the same kernel set: only it has their branches (nh_device.h kExtLights)
    c->disney = c->disney || !dx.empty();
    c->n_bsdf_types = __builtin_popcount(types);
    c->specular = (types & ((1u << NH_BSDF_MIRROR) | (1u << NH_BSDF_DIELECTRIC))) != 0;
    // any BSDF with an albedo texture or shape with a normal map (wf_bounce_rr's lean instantiation has no lookup)
    c->textured = false;
    for (uint32_t i = 0; i < d->n_bsdfs; ++i) c->textured = c->textured || d->bsdfs[i].albedo_texture != 0;
    c->normal_mapped = false;
    for (uint32_t i = 0; i < d->n_shapes; ++i) c->normal_mapped = c->normal_mapped || d->shapes[i].normal_map != 0;
    c->textured = c->textured || c->normal_mapped;
    c->diffuse_area = S.integrator == NH_INTEGRATOR_PATH_MIS && !c->textured && !S.dof && d->envmap < 0 &&
                      d->n_emitters > 0;
    for (uint32_t i = 0; i < d->n_bsdfs; ++i) c->diffuse_area = c->diffuse_area && d->bsdfs[i].type == NH_BSDF_DIFFUSE;
    for (uint32_t i = 0; i < d->n_emitters; ++i) {
        const nh_emitter &e = d->emitters[i];
        c->diffuse_area = c->diffuse_area && e.type == NH_EMITTER_AREA && e.shape >= 0 &&
                          (uint32_t)e.shape < d->n_shapes && ds[e.shape].ef_off >= 0;
    }
    // (a shape's emitter index must be one of those: shade_head reads S.emitters[shape.emitter])
    for (uint32_t i = 0; i < d->n_shapes; ++i)
        c->diffuse_area = c->diffuse_area && d->shapes[i].emitter < (int32_t)d->n_emitters;
    c->h_shapes = ds;
    c->h_bsdfs = db;
    c->h_emitters = de;
    c->h_area_cdf.assign(d->area_cdf, d->area_cdf + d->n_area_cdf);
    c->n_emit_faces = (int)ef_tri.size();
    // the emitter faces the shadow masks reason from (host/shadow_masks.cpp): kept only when every light sample
    // starts on one of them
    c->h_emit_tris = nh::shadow_emitter_faces(*d);
    if (c->h_emit_tris.size() != 9 * ef_tri.size()) c->h_emit_tris.clear();  // (NH_EMIT_FACES=0: no record to start from)
    c->small_image = c->small_image_ref = nullptr;  // (the BVH and its images went with bvh_bufs above)
    c->flat_image = nullptr;
    c->flat_any_records = 0;
    c->pair_kinds = false;
    c->V.assign(d->V, d->V + 3 * nv);
    c->F.assign(d->F, d->F + 3 * (size_t)d->n_faces);
    c->width = d->camera.width;
    c->height = d->camera.height;
    c->border = d->filter.border;
    c->filter = d->filter;
    c->n_emitters = (int)d->n_emitters;
    c->integrator = S.integrator;
    // (appended fields: a zero-filled tail is the independent sampler)
    if (d->sampler != NH_SAMPLER_INDEPENDENT && d->sampler != NH_SAMPLER_ADAPTIVE)
        return fail(c, "unknown sampler"), NH_ERR_INVALID;
    c->sampler = d->sampler;
    c->adaptive_initial_uniform = std::max(1, (int)d->adaptive_initial_uniform);
    adaptive_release(c);  // block samplers of an earlier scene
    photon_release(c);    // and its photon map
    c->av_set = false;    // and its av length

    // master ImageBlock
    (void)hipFree(c->fb);
    c->fb = nullptr;
    c->fb_floats = 4 * (size_t)(c->width + 2 * c->border) * (size_t)(c->height + 2 * c->border);
    HIP_TRY(c, hipMalloc(&c->fb, c->fb_floats * sizeof(float)));
    HIP_TRY(c, hipMemsetAsync(c->fb, 0, c->fb_floats * sizeof(float), c->stream));
    // block spiral ranks
    auto rank = nh::spiral_rank(c->width, c->height, 32, c->nbx, c->nby);
    (void)hipFree(c->block_rank);
    HIP_TRY(c, hipMalloc(&c->block_rank, rank.size() * sizeof(int)));
    HIP_TRY(c, hipMemcpyAsync(c->block_rank, rank.data(), rank.size() * sizeof(int), hipMemcpyHostToDevice, c->stream));
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    c->has_scene = true;
    return NH_OK;
}

// The LDS image of a small scene (WfLaunch::small_image), rebuilt by every BVH upload (a scene upload drops the BVH):
// nodes, primitive records and leaf table copied from the uploaded arrays, the pair records and flat-triangle frames
// computed on the device by the float operations the kernels' staging ran per workgroup before (launch_small_image),
// and -- for a scene the diffuse area-light kernels run on, within kSmallTablesBytes -- the scene tables: shapes,
// BSDFs, emitters, the emitting meshes' area CDFs packed one after the other (the image's shape records index them)
// and the emit_faces records. Frames are part of the image whenever the scene is small enough for them; a render
// that does not want them copies the image without its last region.
// The pair records follow the host's pair_layout of g's leaves and records: by kind (NH_PAIR_KINDS=0: the reference
// arrangement), and then a second image in the reference arrangement for the counting kernels (nh_ctx::small_image_ref).
static int build_small_image(nh_ctx *c, const nh::GpuBvh &g) {
    c->small_image = c->small_image_ref = nullptr;
    c->flat_image = nullptr;
    c->flat_any_records = 0;
    c->pair_kinds = false;
    for (int &v : c->small_tab) v = 0;
    const size_t scene_bytes = 16 * (size_t)(c->n_node_f4 + c->n_prim_f4) + 8 * (size_t)c->n_leaves;
    if (scene_bytes > kSmallSceneBytes) return NH_OK;
    const int n = c->n_prim_f4 / 3;
    const int leaves_f4 = (c->n_leaves + 1) / 2;
    const int pairs_off = c->n_node_f4 + c->n_prim_f4 + leaves_f4;
    const bool frames = n <= kSmallFramesMaxPrims;
    std::vector<float4> tab;
    if (c->diffuse_area) {
        std::vector<nhd::DShape> sh = c->h_shapes;
        std::vector<float> cdf;
        for (const nhd::DEmitter &e : c->h_emitters) {  // (diffuse_area: every emitter's shape is a mesh)
            nhd::DShape &s = sh[e.shape];
            if ((size_t)s.pdf_off + s.n_faces + 1 > c->h_area_cdf.size()) return fail(c, "area CDF out of range"), NH_ERR_INVALID;
            const int off = (int)cdf.size();
            cdf.insert(cdf.end(), c->h_area_cdf.begin() + s.pdf_off, c->h_area_cdf.begin() + s.pdf_off + s.n_faces + 1);
            s.pdf_off = off;
        }
        cdf.resize((cdf.size() + 3) / 4 * 4, 0.f);
        const size_t bytes = sh.size() * sizeof(nhd::DShape) + c->h_bsdfs.size() * sizeof(nhd::DBsdf) +
                             c->h_emitters.size() * sizeof(nhd::DEmitter) + cdf.size() * sizeof(float) +
                             3 * (size_t)c->n_emit_faces * sizeof(float4);
        if (bytes <= kSmallTablesBytes) {
            static_assert(sizeof(nhd::DShape) % 16 == 0 && sizeof(nhd::DBsdf) % 16 == 0 && sizeof(nhd::DEmitter) % 16 == 0,
                          "table records are whole float4s");
            c->small_tab[0] = (int)(sh.size() * sizeof(nhd::DShape) / 16);
            c->small_tab[1] = (int)(c->h_bsdfs.size() * sizeof(nhd::DBsdf) / 16);
            c->small_tab[2] = (int)(c->h_emitters.size() * sizeof(nhd::DEmitter) / 16);
            c->small_tab[3] = (int)(cdf.size() / 4);
            c->small_tab[4] = 3 * c->n_emit_faces;
            tab.resize((size_t)c->small_tab[0] + c->small_tab[1] + c->small_tab[2] + c->small_tab[3]);
            char *w = reinterpret_cast<char *>(tab.data());
            std::memcpy(w, sh.data(), sh.size() * sizeof(nhd::DShape));
            w += sh.size() * sizeof(nhd::DShape);
            std::memcpy(w, c->h_bsdfs.data(), c->h_bsdfs.size() * sizeof(nhd::DBsdf));
            w += c->h_bsdfs.size() * sizeof(nhd::DBsdf);
            std::memcpy(w, c->h_emitters.data(), c->h_emitters.size() * sizeof(nhd::DEmitter));
            w += c->h_emitters.size() * sizeof(nhd::DEmitter);
            std::memcpy(w, cdf.data(), cdf.size() * sizeof(float));
        }
    }
    const int tab_f4 = (int)tab.size() + c->small_tab[4];
    const int pleaves_off = pairs_off + nhd::kPairF4 * n, tab_off = pleaves_off + leaves_f4;
    const int frames_off = tab_off + tab_f4;
    const size_t total = (size_t)frames_off + (frames ? 3 * (size_t)n : 0);
    const auto d2d = [&](float4 *dst, const void *src, size_t bytes) {
        return bytes ? hipMemcpyAsync(dst, src, bytes, hipMemcpyDeviceToDevice, c->stream) : hipSuccess;
    };
    const char *pk = std::getenv("NH_PAIR_KINDS");
    c->pair_kinds = n > 0 && !(pk && pk[0] == '0');
    for (int pass = 0; pass < (c->pair_kinds ? 2 : 1); ++pass) {
        const bool by_kind = c->pair_kinds && pass == 0;
        const nh::PairLayout pl = nh::pair_layout(g.leaves.data(), c->n_leaves, g.prims.data(), n, by_kind);
        float4 *img = nullptr;
        HIP_TRY(c, hipMalloc(&img, std::max<size_t>(total, 1) * sizeof(float4)));
        c->bvh_bufs.push_back(img);
        HIP_TRY(c, hipMemsetAsync(img, 0, std::max<size_t>(total, 1) * sizeof(float4), c->stream));
        HIP_TRY(c, d2d(img, c->tv.nodes, 16 * (size_t)c->n_node_f4));
        HIP_TRY(c, d2d(img + c->n_node_f4, c->tv.prims, 16 * (size_t)c->n_prim_f4));
        HIP_TRY(c, d2d(img + c->n_node_f4 + c->n_prim_f4, c->tv.leaves, 8 * (size_t)c->n_leaves));
        if (n > 0) {
            const nh::i2 *slots = nullptr;
            if (int rc = upload(c, c->bvh_bufs, pl.slots.data(), pl.slots.size(), &slots)) return rc;
            nh::launch_small_image(c->tv, c->n_prim_f4, reinterpret_cast<const int2 *>(slots), pairs_off,
                                   frames ? frames_off : -1, img, c->stream);
            HIP_TRY(c, hipGetLastError());
        }
        if (c->n_leaves > 0)
            HIP_TRY(c, hipMemcpyAsync(img + pleaves_off, pl.leaves.data(), 8 * (size_t)c->n_leaves, hipMemcpyHostToDevice,
                                      c->stream));
        if (!tab.empty()) {
            float4 *t = img + tab_off;
            HIP_TRY(c, hipMemcpyAsync(t, tab.data(), tab.size() * sizeof(float4), hipMemcpyHostToDevice, c->stream));
            HIP_TRY(c, d2d(t + tab.size(), c->S.emit_faces, 16 * (size_t)c->small_tab[4]));
        }
        HIP_TRY(c, hipStreamSynchronize(c->stream));  // (pl and tab are locals)
        (pass == 0 ? c->small_image : c->small_image_ref) = img;
    }
    // The flat image (host/gpu_layout.cpp flat_image; NH_FLAT_TRACE=0: none): the tree is one leaf, or one inner node
    // whose children are leaves 0 and 1, and the pair records by kind are few enough. The non-counting RR-ahead bounce
    // kernels then take their queries from it without a tree walk (trace_flat).
    const bool one_leaf = g.root_kind == 2 && c->n_leaves == 1;
    bool two_leaves = g.root_kind == 1 && c->n_node_f4 == 4 && c->n_leaves == 2;
    if (two_leaves) {
        int refs[2];
        std::memcpy(refs, &g.nodes[3].x, sizeof(refs));
        two_leaves = refs[0] == ~0 && refs[1] == ~1;
    }
    if (c->pair_kinds && (one_leaf || two_leaves)) {
        float boxes[18];
        for (int i = 0; i < 3; ++i) {
            boxes[i] = g.root_min[i];
            boxes[3 + i] = g.root_max[i];
        }
        if (two_leaves) {
            const nh::f4 n0 = g.nodes[0], n1 = g.nodes[1], n2 = g.nodes[2];
            const float lr[12] = {n0.x, n0.y, n0.z, n0.w, n1.x, n1.y, n1.z, n1.w, n2.x, n2.y, n2.z, n2.w};
            std::memcpy(boxes + 6, lr, sizeof(lr));
        } else {
            std::memcpy(boxes + 6, boxes, 6 * sizeof(float));
            std::memcpy(boxes + 12, boxes, 6 * sizeof(float));
        }
        const nh::PairLayout pl = nh::pair_layout(g.leaves.data(), c->n_leaves, g.prims.data(), n, true);
        // the scene-wide any-hit word (host/shadow_masks.cpp; NH_ANY_LIST=0: all ones): the records it keeps get pair
        // records of their own in the image, which the light samples' any-hit queries read
        uint64_t any_word = ~(uint64_t)0;
        if (nh::any_list_knob() && n <= 64 && !c->h_emit_tris.empty())
            any_word = nh::shadow_any_word(c->camera, g.prims.data(), n, c->h_emit_tris.data(), (int)(c->h_emit_tris.size() / 9));
        const nh::FlatImage fi = nh::flat_image(boxes, g.leaves.data(), c->n_leaves, g.prims.data(), n, pl, nh::flat_trace_knob(),
                                                any_word);
        if (fi.flat && fi.any_list)
            for (int k = 0; k < n; ++k) c->flat_any_records += (int)((any_word >> k) & 1);
        if (fi.flat) {
            const nh::f4 *dev = nullptr;
            if (int rc = upload(c, c->bvh_bufs, fi.data.data(), fi.data.size(), &dev)) return rc;
            HIP_TRY(c, hipStreamSynchronize(c->stream));  // (fi is a local)
            c->flat_image = reinterpret_cast<const float4 *>(dev);
        }
    }
    return NH_OK;
}

int nh_set_av_params(nh_ctx *c, const nh_av_params *params) {
    if (!c) return NH_ERR_INVALID;
    if (!params || std::isnan(params->length)) return fail(c, "nh_set_av_params: invalid av parameters"), NH_ERR_INVALID;
    if (!c->has_scene) return fail(c, "nh_set_av_params: no scene uploaded"), NH_ERR_STATE;
    HIP_TRY(c, hipSetDevice(c->device));
    if (int rc = pipeline_drain(c)) return rc;
    HIP_TRY(c, hipStreamSynchronize(c->stream));  // kernels in flight read the device copy
    c->S.av_length = params->length;
    // the device copy exists once a BVH is uploaded (nh_upload_bvh copies the whole record)
    if (c->d_scene && c->has_bvh)
        HIP_TRY(c, hipMemcpy(reinterpret_cast<char *>(c->d_scene) + offsetof(nhd::DScene, av_length), &c->S.av_length,
                             sizeof(float), hipMemcpyHostToDevice));
    c->av_set = true;
    return NH_OK;
}

int nh_upload_bvh(nh_ctx *c, const nh_bvh_desc *b) {
    if (!c || !b) return NH_ERR_INVALID;
    if (!c->has_scene) return fail(c, "nh_upload_bvh: upload the scene first"), NH_ERR_STATE;
    HIP_TRY(c, hipSetDevice(c->device));
    if (int rc_ = pipeline_drain(c)) return rc_;
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    free_all(c->bvh_bufs);
    c->has_bvh = false;
    photon_release(c);  // a photon map belongs to the scene and BVH it was traced in
    // the wide tree of the persistent kernels: 4-wide, or 8-wide with NH_WIDE8=1 (A/B)
    c->wide_w = std::getenv("NH_WIDE8") && std::getenv("NH_WIDE8")[0] == '1' ? 8 : 4;
    // the top of the tree the persistent kernels stage in LDS (NH_TREE_TOP: its size, 0 = none): the same bytes for
    // both widths
    int top_k = nh::tree_top_nodes() * 4 / c->wide_w;
    if (const char *e = std::getenv("NH_TREE_TOP")) top_k = std::min(std::max(0, std::atoi(e)), top_k);
    nh::GpuBvh g;
    if (int rc_ = nh::build_gpu_bvh(*b, c->shapes, c->V, c->F, c->shape_bsdf_type, c->shape_bsdf_real, c->wide_w, top_k,
                                    g, c->err))
        return rc_;
    nhd::DScene &S = c->S;
    S.root_kind = g.root_kind;
    for (int i = 0; i < 3; ++i) { S.root_min[i] = g.root_min[i]; S.root_max[i] = g.root_max[i]; }
    S.iso_spheres = g.iso_spheres;
    c->tv.n_top = g.n_top;
    int rc;
    c->n_node_f4 = (int)g.nodes.size();
    c->n_leaves = (int)g.leaves.size();
    c->n_prim_f4 = (int)g.prims.size() - 3;  // (without the zero record past the end)
    // the records the camera rays' candidate masks are built from (nh_pipeline.hip ensure_primary_masks)
    drop_primary_masks(c);
    c->h_prims.clear();
    if (c->n_prim_f4 > 0 && c->n_prim_f4 / 3 <= 64)
        c->h_prims.assign(&g.prims[0].x, &g.prims[0].x + 4 * (size_t)c->n_prim_f4);
    const nh::f4 *nodes = nullptr, *prims = nullptr, *wide = nullptr;
    const nh::i2 *leaves = nullptr;
    if ((rc = upload(c, c->bvh_bufs, g.nodes.data(), g.nodes.size(), &nodes))) return rc;
    if ((rc = upload(c, c->bvh_bufs, g.leaves.data(), g.leaves.size(), &leaves))) return rc;
    if ((rc = upload(c, c->bvh_bufs, g.prims.data(), g.prims.size(), &prims))) return rc;
    if (!g.wide.empty() && (rc = upload(c, c->bvh_bufs, g.wide.data(), g.wide.size(), &wide))) return rc;
    c->tv.nodes = reinterpret_cast<const float4 *>(nodes);
    c->tv.leaves = reinterpret_cast<const int2 *>(leaves);
    c->tv.prims = reinterpret_cast<const float4 *>(prims);
    c->tv.wnodes = reinterpret_cast<const float4 *>(wide);
    c->depth_wide = g.depth_wide;
    S.nodes = c->tv.nodes;
    S.prims = c->tv.prims;
    c->bvh_indices.assign(b->indices, b->indices + b->n_indices);
    c->shape_offset = g.shape_offset;
    c->depth = (int)g.tree_depth + 2;
    if (!c->d_scene) HIP_TRY(c, hipMalloc(&c->d_scene, sizeof(nhd::DScene)));
    HIP_TRY(c, hipMemcpyAsync(c->d_scene, &c->S, sizeof(nhd::DScene), hipMemcpyHostToDevice, c->stream));
    if ((rc = build_small_image(c, g))) return rc;
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    c->has_bvh = true;
    return NH_OK;
}

}  // extern "C"
