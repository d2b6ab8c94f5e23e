// Device-side math, sampling and shading for the gfx950 path_mis pipeline.
//
// Every routine restates a reference function (file:line in the comment) with the
// reference's fp32 rounding points: no contraction (file is compiled with
// -ffp-contract=off and the pragma below), 3-vector dot products grouped
// x0*y0 + (x1*y1 + x2*y2) as the reference's Eigen 3.3.8 emits them, Eigen's
// std::min/std::max ternaries (NaN behaviour included), and transcendentals
// evaluated in fp64 and rounded once (the reference calls the float libm, which is
// correctly rounded on the reference's inputs; a 1-ulp fp32 libm would diverge paths).
#pragma once
#pragma clang fp contract(off)

#include <hip/hip_runtime.h>
#include <stddef.h>
#include <stdint.h>

#include "nh_layout.h"

namespace nhd {

constexpr float kEps = 1e-4f;
constexpr float kPi = 3.14159265358979323846f;
constexpr float kInvPi = 0.31830988618379067154f;
constexpr uint64_t kPcgMult = 0x5851f42d4c957f2dULL;

#define NHD __device__ __forceinline__

NHD float f_sin(float x) { return (float)sin((double)x); }
NHD float f_cos(float x) { return (float)cos((double)x); }

// sin and cos of one fp32 argument in [-8, 8] (every device call site passes a warp angle
// in [0, 2*pi]), evaluated in fp64 to ~1 ulp and rounded once: the fp32 results equal the
// correctly rounded sinf/cosf except on ~2^-29 of inputs. One shared reduction
// x = k*pi/2 + r (two-part Cody-Waite: k*PIO2_HI is exact for |k| < 2^20) and the classic
// degree-13 / degree-14 minimax kernels on |r| <= pi/4 (public-domain fdlibm constants).
// Much smaller than the general fp64 library routines (no large-argument path), which
// matters for the megakernel's register budget.
NHD void f_sincos(float xf, float &s_out, float &c_out) {
    const double x = (double)xf;
    const double k = __builtin_rint(x * 6.36619772367581382433e-01);  // 2/pi
    const double r = (x - k * 1.57079632673412561417e+00) - k * 6.07710050650619224932e-11;
    const double z = r * r;
    const double sp = r + r * z * (-1.66666666666666324348e-01 +
                                   z * (8.33333333332248946124e-03 +
                                        z * (-1.98412698298579493134e-04 +
                                             z * (2.75573137070700676789e-06 +
                                                  z * (-2.50507602534068634195e-08 + z * 1.58969099521155010221e-10)))));
    const double cp = 1.0 - 0.5 * z +
                      z * z * (4.16666666666666019037e-02 +
                               z * (-1.38888888888741095749e-03 +
                                    z * (2.48015872894767294178e-05 +
                                         z * (-2.75573143513906633035e-07 +
                                              z * (2.08757232129817482790e-09 + z * -1.13596475577881948265e-11)))));
    const int q = ((int)k) & 3;
    double sv, cv;
    if (q == 0) { sv = sp; cv = cp; }
    else if (q == 1) { sv = cp; cv = -sp; }
    else if (q == 2) { sv = -sp; cv = -cp; }
    else { sv = -cp; cv = sp; }
    s_out = (float)sv;
    c_out = (float)cv;
}
#ifndef NH_AB_FAST_TRANSC  // cost attribution builds only (scripts/build_variant.sh): fp32 library forms, NOT exact
NHD float f_exp(float x) { return (float)exp((double)x); }
NHD float f_log(float x) { return (float)log((double)x); }
NHD float f_acos(float x) { return (float)acos((double)x); }
NHD float f_atan2(float y, float x) { return (float)atan2((double)y, (double)x); }
#else
NHD float f_exp(float x) { return expf(x); }
NHD float f_log(float x) { return logf(x); }
NHD float f_acos(float x) { return acosf(x); }
NHD float f_atan2(float y, float x) { return atan2f(y, x); }
#endif
NHD float f_sqrt(float x) { return __builtin_sqrtf(x); }  // correctly rounded (HIP default)
NHD float e_min(float a, float b) { return (b < a) ? b : a; }  // std::min
NHD float e_max(float a, float b) { return (a < b) ? b : a; }  // std::max

struct F3 {
    float x, y, z;
};
NHD F3 f3(float x, float y, float z) { F3 r; r.x = x; r.y = y; r.z = z; return r; }
NHD F3 add(F3 a, F3 b) { return f3(a.x + b.x, a.y + b.y, a.z + b.z); }
NHD F3 sub(F3 a, F3 b) { return f3(a.x - b.x, a.y - b.y, a.z - b.z); }
NHD F3 neg(F3 a) { return f3(-a.x, -a.y, -a.z); }
NHD F3 scl(float s, F3 a) { return f3(s * a.x, s * a.y, s * a.z); }
NHD F3 mulc(F3 a, F3 b) { return f3(a.x * b.x, a.y * b.y, a.z * b.z); }
NHD F3 divs(F3 a, float s) { return f3(a.x / s, a.y / s, a.z / s); }
NHD float dot(F3 a, F3 b) { return a.x * b.x + (a.y * b.y + a.z * b.z); }
NHD F3 cross(F3 a, F3 b) { return f3(a.y * b.z - a.z * b.y, a.z * b.x - a.x * b.z, a.x * b.y - a.y * b.x); }
NHD F3 normalized(F3 a) {
    float n = dot(a, a);
    if (n > 0.0f) {
        float s = f_sqrt(n);
        return f3(a.x / s, a.y / s, a.z / s);
    }
    return a;
}
NHD float max_coeff(F3 c) { return e_max(c.x, e_max(c.y, c.z)); }
NHD bool is_zero(F3 c) { return fabsf(c.x) <= kEps && fabsf(c.y) <= kEps && fabsf(c.z) <= kEps; }
NHD bool is_valid(F3 c) {
    return !(c.x < 0 || !isfinite(c.x) || c.y < 0 || !isfinite(c.y) || c.z < 0 || !isfinite(c.z));
}

// ---- pcg32 (ext/pcg32/pcg32.h:51-110) + the per-path seeding contract ------------
struct Rng {
    uint64_t state, inc;
    NHD uint32_t next_uint() {
        uint64_t old = state;
        state = old * kPcgMult + inc;
        uint32_t xs = (uint32_t)(((old >> 18u) ^ old) >> 27u);
        uint32_t rot = (uint32_t)(old >> 59u);
        return (xs >> rot) | (xs << ((~rot + 1u) & 31u));
    }
    NHD float next1d() { return __uint_as_float((next_uint() >> 9) | 0x3f800000u) - 1.0f; }
};
// pcg32() default state and stream (pcg32.h:29-30, :40) and pcg32::advance (pcg32.h:131-150): Brown's
// arbitrary-stride jump, O(log delta)
constexpr uint64_t kPcgDefaultState = 0x853c49e6748fea9bULL, kPcgDefaultStream = 0xda3e39cb94b95bdbULL;
NHD uint64_t pcg_advance(uint64_t state, uint64_t inc, uint64_t delta) {
    uint64_t cur_mult = kPcgMult, cur_plus = inc, acc_mult = 1u, acc_plus = 0u;
    while (delta > 0) {
        if (delta & 1) {
            acc_mult *= cur_mult;
            acc_plus = acc_plus * cur_mult + cur_plus;
        }
        cur_plus = (cur_mult + 1) * cur_plus;
        cur_mult *= cur_mult;
        delta /= 2;
    }
    return acc_mult * state + acc_plus;
}
NHD uint64_t splitmix64(uint64_t x) {
    uint64_t z = x + 0x9E3779B97F4A7C15ULL;
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ULL;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBULL;
    return z ^ (z >> 31);
}
// pcg32::seed(initstate = splitmix64(seed ^ pixel), initseq = sample)
NHD Rng path_rng(uint64_t seed, uint64_t pixel, uint64_t sample) {
    Rng r;
    r.state = 0u;
    r.inc = (sample << 1u) | 1u;
    r.next_uint();
    r.state += splitmix64(seed ^ pixel);
    r.next_uint();
    return r;
}
// path_rng with its splitmix64(seed ^ pixel) already formed (the splat reuses it over a pixel's rounds)
NHD Rng path_rng_h(uint64_t h, uint64_t sample) {
    Rng r;
    r.state = 0u;
    r.inc = (sample << 1u) | 1u;
    r.next_uint();
    r.state += h;
    r.next_uint();
    return r;
}
// The pixel jitter of a sample (render.cpp:441-442: the camera sample's first next2D): recomputed by the splat from
// the sample's seed instead of stored in its record
NHD void sample_jitter_h(uint64_t h, uint64_t sample, float &jx, float &jy) {
    Rng r = path_rng_h(h, sample);
    jx = r.next1d();
    jy = r.next1d();
}

// ---- scene records -----------------------------------------------------------
enum : int { SHAPE_MESH = 0, SHAPE_SPHERE = 1 };
enum : int { BSDF_DIFFUSE = 0, BSDF_MIRROR = 1, BSDF_DIELECTRIC = 2, BSDF_MICROFACET = 3, BSDF_DISNEY = 4 };
// The Disney branch of bsdf_eval / bsdf_pdf / bsdf_sample exists only in translation units built with -DNH_DISNEY
// (the nh_disney:: copies of the render kernels, chosen at upload for scenes with a Disney BSDF, and nh_api.hip's
// BSDF query kernel): the kernels every other scene launches are compiled without it, unchanged.
#ifdef NH_DISNEY
constexpr bool kDisney = true;
#else
constexpr bool kDisney = false;
#endif
enum : int { EMITTER_AREA = 0, EMITTER_POINT = 1, EMITTER_ENVMAP = 2, EMITTER_SPOT = 3, EMITTER_DIRECTIONAL = 4 };
// The spot / directional branches of emitter_sample / emitter_eval / emitter_pdf (nh_shade.h) exist in the same
// translation units as the Disney branch -- the -DNH_DISNEY copies of the render kernels and the query kernels --
// which nh_upload_scene also chooses for a scene with one of those lights: every other scene launches kernels
// compiled without them, unchanged (inlined into the general kernels they cost wf_bounce_rr 32 B/lane of scratch,
// profiles/lights_kernel_resources.txt).
constexpr bool kExtLights = kDisney;
enum : int { M_UNKNOWN = 0, M_SOLID_ANGLE = 1, M_DISCRETE = 2 };

struct alignas(16) DShape {
    int type, bsdf, emitter, v_off;
    int f_off, n_faces, has_n, has_uv;
    float cx, cy, cz, radius;
    int pdf_off;
    float pdf_norm;
    // bit 0: Intersection::uv is read (a textured diffuse albedo, or a normal map): hit_info computes uv only then;
    // bits 1+: 1 + the DScene::texs index of the shape's normal map (shape.cpp:138-147), 0 = none
    int tex_uv;
    int ef_off;  // emitting mesh without normals: its faces' first record in DScene::emit_faces, else -1
};
struct alignas(16) DBsdf {
    int type;
    float ar, ag, ab;      // diffuse albedo
    // disney: alpha / int_ior are unused, their words hold the device address of the BSDF's DDisney side record
    union { float alpha; uint32_t disney_lo; };
    union { float int_ior; uint32_t disney_hi; };
    float ext_ior, ks;
    float kr, kg, kb;      // microfacet kd
    int tex;               // diffuse / disney: 1 + albedo texture index (DScene::texs), 0 = the constant albedo
};
// Disney (disney.cpp): the side record of a BSDF_DISNEY DBsdf, which holds its device address in the words of
// (alpha, int_ior) (disney_lo / disney_hi, disney_rec) -- DBsdf itself stays 48 bytes for the kernels that stage it to LDS. The ten clamped
// parameters, the terms of eval that depend on them alone (ax, ay: disney.cpp:152-153; GTR1's a2 - 1 and
// M_PI * log(a2) of the clearcoat lobe: :164, :311-313), and the terms that depend on the albedo (Cdlin, Cspec0,
// Csheen: :132-137) for the constant albedo -- formed once at upload by the device functions below (nh_disney.hip
// disney_fold_kernel), the same float operations in the same order as a textured albedo runs per hit.
static_assert(sizeof(DBsdf) == 48 && offsetof(DBsdf, disney_lo) == 16 && offsetof(DBsdf, disney_hi) == 20 &&
                  offsetof(DBsdf, ext_ior) == 24, "DBsdf layout (staged to LDS as three float4)");
struct alignas(16) DDisney {
    float metallic, subsurface, specular, roughness;
    float specular_tint, anisotropic, sheen, sheen_tint;
    float clearcoat, clearcoat_gloss, ax, ay;
    float cc_a2m1, cc_pilog, pad0, pad1;
    float cdlin[3], cspec0[3], csheen[3];
    float pad2[3];
};
// Texture<Color3f> albedo (nh_texture): consttexture.cpp / checkerboard.cpp / PNGTexture.cpp
enum : int { TEX_CONSTANT = 0, TEX_CHECKERBOARD = 1, TEX_PNG = 2 };
struct alignas(16) DTex {
    int type, w, h, spherical;
    float v1r, v1g, v1b, v2r;
    float v2g, v2b, dx, dy;
    float sx, sy, su, sv;
    float ou, ov;
    long long off;  // png: first texel in DScene::texels
    float rot[9];   // png spherical lookups: the eulerAngles rotation, row-major
    int linear;     // png with sRGB = false: normal-map texels, eval blends by intensity and normalizes
    float intensity;
    float pad;
};
struct alignas(16) DEmitter {
    int type, shape;  // shape: the owning shape of an area light; spot / directional: the light's DScene::emitter_ext entry
    float lr, lg, lb;
    float px, py, pz;
};
// SpotLight / DirectionalLight (spotlight.cpp, directionalLight.cpp): what they hold beyond a DEmitter, which stays 32
// bytes for the kernels that stage the emitter table to LDS. In global memory (DScene::emitter_ext), read only by the
// spot / directional branches of the emitter functions (nh_shade.h). nh_emitter_ext's layout.
struct alignas(16) DEmitterExt {
    float dx, dy, dz, cos_total;    // m_direction; spot: cos(degToRad(totalwidth / 2))
    float sx, sy, sz, cos_falloff;  // m_coord.s; spot: cos(degToRad(falloffstart))
    float tx, ty, tz, cos_max;      // m_coord.t; directional: cos(degToRad(angle))
    float nx, ny, nz, pad;          // m_coord.n
};
static_assert(sizeof(DEmitter) == 32 && sizeof(DEmitterExt) == 64, "emitter records");
// Medium (vacuum.cpp, homogmedium.cpp) with its phase function (isophase.cpp, anisophase.cpp): nh_medium's layout
enum : int { MEDIUM_VACUUM = 0, MEDIUM_HOMOG = 1 };
enum : int { PHASE_ISO = 0, PHASE_HG = 1 };
struct alignas(16) DMedium {
    int type;
    float mu_a[3], mu_s[3], mu_t[3];
    float density;
    int phase;
    float g;
    int pad[3];
};
static_assert(sizeof(DMedium) == 64, "medium record");
// The photon map as the gather reads it (nh_photon.h): the photons sorted by (grid cell key, deposit index), their
// direction and power already decoded from PhotonData's bytes, and the uniform grid the keys come from
struct DPhotonMap {
    const float4 *pos;     // (x, y, z, -)
    const float4 *dir;     // PhotonData::getDirection of the stored bytes
    const float4 *power;   // PhotonData::getPower of the stored bytes
    const uint64_t *keys;  // cell keys, ascending
    int n;                 // photons stored
    int emitted;           // m_emittedPhotons
    float radius;          // m_photonRadius
    float cell;            // cell side, >= radius
    float origin[3];       // the grid's corner
    int pad;
};

struct DScene {
    // BVH: 4 float4 per inner node, 3 float4 per primitive in leaf order
    const float4 *nodes;
    const float4 *prims;
    float root_min[3], root_max[3];
    int root_kind;  // 0 = empty scene, 1 = root inner node 0, 2 = root is a leaf
    int root_start, root_count;
    // geometry / materials
    const DShape *shapes;
    const DBsdf *bsdfs;
    const DEmitter *emitters;
    const float *emitter_cdf;
    int n_emitters;
    int integrator;  // NH_INTEGRATOR_*
    float ndir[3];   // normals: its `direction`
    const float *V, *N, *UV, *T, *BT;
    const uint32_t *F;
    const float *area_cdf;
    // emitting meshes without vertex normals, per face: (p0, n.x) (p1, n.y) (p2, n.z) with the face normal
    // normalized(cross(p1 - p0, p2 - p0)) of Mesh::sampleSurface (mesh.cpp:64-69), computed once at upload by the
    // same device arithmetic (nh_upload.hip emit_face_kernel) instead of per light sample
    const float4 *emit_faces;
    // camera (perspective.cpp) and filter table (block.cpp)
    float s2c[16], c2w[16];
    // the pinhole ray origin (camera_ray with a (0, 0, 0) local origin: c2w * (0, 0, 0, 1), divided by its w), formed
    // once at upload by the same float operations in the same order
    float cam_o[3];
    float inv_w, inv_h, near_clip, far_clip;
    int width, height;
    // depth of field (perspective.cpp:114-130), on when lensRadius > Epsilon. The lens stream's state at a camera
    // ray's first draw (nh_shade.h lens_uniform): lens_pix[pixel] = advance by 2 x (the pixel's position within one
    // sample round of the serial render order: spiral blocks, x-major pixels) as (a, c); lens_lo[l] = advance by
    // 2 l W H; lens_hi[h] = the state at draw 2 * 256 h * W * H. lens_rtl: x = the second draw (g++'s order)
    int dof, lens_rtl;
    float lens_radius, focal_distance;
    const ulonglong2 *lens_pix, *lens_lo;
    const uint64_t *lens_hi;
    float filter_radius, lookup;
    int border;
    float table[33];
    // EnvMap (environmentmap.cpp) and its albedo texture (PNGTexture.cpp / ConstantTexture)
    int envmap;  // emitter index, or -1
    const float4 *env_rgba;
    const float *env_cdf;  // env_w * env_h + 1 entries
    const int *env_guide;  // 2^env_guide_bits + 1 entries: dpdf_sample_guided's brackets of env_cdf (nullptr: none)
    int env_guide_bits;
    int env_w, env_h, env_spherical, env_constant;
    float env_norm, env_su, env_sv, env_ou, env_ov;
    float env_r, env_g, env_b;
    float env_rot[9];  // spherical lookups: the png_texture's eulerAngles rotation, row-major
    // BSDF albedo textures (DBsdf::tex) and the png texels they index
    const DTex *texs;
    const float4 *texels;
    // 1: a light sample is always finite and never at a discrete-BSDF shading point (host/gpu_layout.cpp nee_finite, at upload), so the
    // wavefront shade skips the light sample of a discrete BSDF sample (it provably adds +-0)
    int nee_finite;
    // isolated dielectric spheres the BVH upload marked (nh_traverse.h trace_next; 0: no ray tries the shortcut)
    int iso_spheres;
    // spot / directional lights: n_emitters records indexed by DEmitter::shape (nullptr: the scene has neither)
    const DEmitterExt *emitter_ext;
    // participating media (read by the volumetric path kernel alone, nh_volume.hip): the medium table, the per-shape
    // side table (1 + medium index, 0 = none; DShape is full at 64 B) and the ambient medium (1 + index, 0 = vacuum).
    // nullptr / 0 for a scene without media.
    const DMedium *media;
    const int *shape_medium;
    int ambient_medium;
    int n_media;
    // the photon mapper's map (nh_photon.h; read by li_photonmapper and the gather query alone): all zero until
    // nh_photon_map_build
    DPhotonMap pm;
    // the av integrator's `length`, the occlusion ray's maxt (nh_set_av_params)
    float av_length;
};

NHD F3 ldv(const float *a, uint32_t i) { return f3(a[3 * i], a[3 * i + 1], a[3 * i + 2]); }

// ---- frames (frame.h, common.cpp:292-306) ---------------------------------------
struct Frame {
    F3 s, t, n;
};
NHD Frame frame_from_n(F3 a) {
    Frame f;
    f.n = a;
    F3 c;
    if (fabsf(a.x) > fabsf(a.y)) {
        float inv_len = 1.0f / f_sqrt(a.x * a.x + a.z * a.z);
        c = f3(a.z * inv_len, 0.0f, -a.x * inv_len);
    } else {
        float inv_len = 1.0f / f_sqrt(a.y * a.y + a.z * a.z);
        c = f3(0.0f, a.z * inv_len, -a.y * inv_len);
    }
    f.t = c;
    f.s = cross(c, a);
    return f;
}
NHD F3 to_local(const Frame &f, F3 v) { return f3(dot(v, f.s), dot(v, f.t), dot(v, f.n)); }
NHD F3 to_world(const Frame &f, F3 v) { return add(add(scl(v.x, f.s), scl(v.y, f.t)), scl(v.z, f.n)); }

// fresnel (common.cpp:308-338)
NHD float fresnel(float cos_i, float ext_ior, float int_ior) {
    float eta_i = ext_ior, eta_t = int_ior;
    if (ext_ior == int_ior) return 0.0f;
    if (cos_i < 0.0f) {
        float tmp = eta_i; eta_i = eta_t; eta_t = tmp;
        cos_i = -cos_i;
    }
    float eta = eta_i / eta_t, sin_t2 = eta * eta * (1 - cos_i * cos_i);
    if (sin_t2 > 1.0f) return 1.0f;
    float cos_t = f_sqrt(1.0f - sin_t2);
    float rs = (eta_i * cos_i - eta_t * cos_t) / (eta_i * cos_i + eta_t * cos_t);
    float rp = (eta_t * cos_i - eta_i * cos_t) / (eta_t * cos_i + eta_i * cos_t);
    return (rs * rs + rp * rp) / 2.0f;
}

// ---- warps (warp.cpp) -------------------------------------------------------------
NHD F3 cosine_hemisphere(float sx, float sy) {  // warp.cpp:48-52, 111-122
    float rho = f_sqrt(sx);
    float theta = sy * 2.0f * kPi;
    float st, ct;
    f_sincos(theta, st, ct);
    float x = rho * ct, y = rho * st;
    return f3(x, y, f_sqrt(1.f - (x * x + y * y)));
}
NHD F3 beckmann(float sx, float sy, float alpha) {  // warp.cpp:131-150
    float ls = f_log(1.f - sx);
    if (isinf(ls)) ls = 0;
    float tan2 = -alpha * alpha * ls;
    float phi = sy * 2.f * kPi;
    float ct = 1.f / f_sqrt(1 + tan2);
    float st = f_sqrt(1.f - ct * ct);
    float sphi, cphi;
    f_sincos(phi, sphi, cphi);
    F3 r = f3(st * cphi, st * sphi, ct);
    if (r.z < 0) r = neg(r);
    return r;
}
NHD F3 uniform_sphere(float sx, float sy) {  // warp.cpp:74-82
    F3 w;
    w.z = 2.0f * sx - 1.0f;
    float r = f_sqrt(1.0f - w.z * w.z);
    float sigma = 2.0f * kPi * sy;
    float ss, cs;
    f_sincos(sigma, ss, cs);
    w.x = r * cs;
    w.y = r * ss;
    return normalized(w);
}
// The warps and densities below are called by the warp test alone (nh_warp.hip): the render
// kernels carry the ones they need inline in their emitter, camera and BSDF code.
NHD float uniform_square_pdf(float x, float y) {  // warp.cpp:43-46
    return (x >= 0 && y >= 0 && x <= 1 && y <= 1) ? 1.0f : 0.0f;
}
NHD void uniform_disk(float sx, float sy, float &x, float &y) {  // warp.cpp:48-52
    float rho = f_sqrt(sx);
    float theta = sy * 2.0f * kPi;
    float st, ct;
    f_sincos(theta, st, ct);
    x = rho * ct;
    y = rho * st;
}
NHD float uniform_disk_pdf(float x, float y) { return (x * x + y * y <= 1.0f) ? 1.0f / kPi : 0.0f; }  // warp.cpp:54-56
NHD F3 uniform_sphere_cap(float sx, float sy, float cos_max) {  // warp.cpp:58-66
    float z = sx * (1.0f - cos_max) + cos_max;
    float r = f_sqrt(1.0f - z * z);
    float theta = sy * 2.0f * kPi;
    float st, ct;
    f_sincos(theta, st, ct);
    return f3(r * ct, r * st, z);
}
// warp.cpp:68-72, as written: zero for a unit vector at or below the cap's rim, the cap's density everywhere else
NHD float uniform_sphere_cap_pdf(F3 v, float cos_max) {
    return (fabsf(dot(v, v) - 1.0f) < kEps && v.z <= cos_max) ? 0.0f : 1.0f / (2.0f * kPi * (1.0f - cos_max));
}
NHD float uniform_sphere_pdf(F3 v) { return (fabsf(dot(v, v) - 1.0f) < kEps) ? 0.25f / kPi : 0.0f; }  // warp.cpp:84-86
NHD float f_cbrt(float x) { return (float)cbrt((double)x); }  // std::cbrt(float): fp64, rounded once
NHD F3 uniform_sphere_volume(float sx, float sy, float sz) {  // warp.cpp:88-92
    const float r = f_cbrt(sz);
    return scl(r, uniform_sphere(sx, sy));
}
NHD float uniform_sphere_volume_pdf() { return 4.f / 3.f * kPi; }  // warp.cpp:94-97, as written (not a density)
NHD F3 uniform_hemisphere(float sx, float sy) {  // warp.cpp:99-103
    F3 w = uniform_sphere(sx, sy);
    w.z = fabsf(w.z);
    return w;
}
NHD float uniform_hemisphere_pdf(F3 v) {  // warp.cpp:105-109
    return (fabsf(dot(v, v) - 1) < kEps && v.z > 0) ? 2.0f * uniform_sphere_pdf(v) : 0.0f;
}
NHD float cosine_hemisphere_pdf(F3 v) {  // warp.cpp:124-129
    return (fabsf(dot(v, v) - 1) < kEps && v.z > 0) ? v.z / kPi : 0.0f;
}
NHD float beckmann_pdf(F3 m, float alpha) {  // warp.cpp:152-160 (the BSDF's own D is beckmann_d, microfacet.cpp)
    float c_t = m.z;
    float r = f_sqrt(m.x * m.x + m.y * m.y);
    float tantheta = r / m.z;
    if (fabsf(dot(m, m) - 1) > kEps || m.z < 0) return 0.f;
    return f_exp(-tantheta * tantheta / alpha / alpha) / (kPi * alpha * alpha * c_t * c_t * c_t);
}

// ---- BSDFs (src/bsdf) ---------------------------------------------------------------
NHD float tan_theta(F3 v) {
    float temp = 1 - v.z * v.z;
    if (temp <= 0.0f) return 0.0f;
    return f_sqrt(temp) / v.z;
}
NHD float beckmann_d(const DBsdf &b, F3 m) {  // microfacet.cpp:60-66
    float temp = tan_theta(m) / b.alpha, ct = m.z, ct2 = ct * ct;
    return f_exp(-temp * temp) / (kPi * b.alpha * b.alpha * ct2 * ct2);
}
NHD float smith_g1(const DBsdf &b, F3 v, F3 m) {  // microfacet.cpp:69-89
    float tt = tan_theta(v);
    if (tt == 0.0f) return 1.0f;
    if (dot(m, v) * v.z <= 0) return 0.0f;
    float a = 1.0f / (b.alpha * tt);
    if (a >= 1.6f) return 1.0f;
    float a2 = a * a;
    return (3.535f * a + 2.181f * a2) / (1.0f + 2.276f * a + 2.577f * a2);
}
// ---- Disney (src/bsdf/disney.cpp:111-205) ----------------------------------------------------
// Overloads. disney.cpp calls pow / log / sqrt unqualified on float arguments. common.h:39 includes ImathPlatform.h,
// which includes <math.h>; with g++ that is libstdc++'s wrapper, whose using-declarations put std::'s float overloads
// into the global namespace, so every call resolves to the float overload (without <math.h> the only global
// candidates would be glibc's double functions; a probe with both include sets shows the switch):
//   pow(vec.r(), 2.2f)  std::pow(float, float) = powf   -> f_pow: fp64 pow rounded once, as the other f_* functions
//   pow(x, 2.f)         std::pow(float, float) = powf   -> x * x (powf(x, 2) is the correctly rounded square)
//   log(a2)             std::log(float) = logf          -> f_log
//   sqrt(..)            std::sqrt(float) = sqrtf        -> f_sqrt (correctly rounded)
//   std::max(0.001f, ..) float                          -> e_max
// M_PI and INV_PI are Nori's float constants (common.h:61-62), mix<float>(1.0, ..) converts its 1.0 to float: the
// whole of eval is fp32 arithmetic. (disney.cpp calls no cos.)
NHD float f_pow(float x, float y) { return (float)pow((double)x, (double)y); }
NHD const DDisney *disney_rec(const DBsdf &b) {
    return reinterpret_cast<const DDisney *>(((uint64_t)b.disney_hi << 32) | (uint64_t)b.disney_lo);
}
NHD float nori_clamp01(float v) { return v < 0.f ? 0.f : (v > 1.f ? 1.f : v); }  // common.h clamp(v, 0, 1)
NHD float schlick_fresnel(float a) {                                             // disney.cpp:289-294
    const float m = nori_clamp01(1.f - a), m2 = m * m;
    return m2 * m2 * m;
}
NHD float mixf(float a, float b, float t) { return a + (b - a) * t; }  // disney.cpp:283-287
struct DisneyCol {
    F3 cdlin, cspec0, csheen;
};
// disney.cpp:132-137: mon2lin, Cdlum, Ctint (1 for a black albedo), Cspec0, Csheen. Out of line (as tex_eval): three
// fp64 pows that only a textured albedo and the upload-time fold run. Arguments and result by value, in registers (a
// record passed by reference would have to live in scratch memory).
__device__ __noinline__ DisneyCol disney_colors(float specular, float specular_tint, float metallic, float sheen_tint,
                                                F3 alb) {
    DisneyCol c;
    c.cdlin = f3(f_pow(alb.x, 2.2f), f_pow(alb.y, 2.2f), f_pow(alb.z, 2.2f));
    const float lum = 0.3f * c.cdlin.x + 0.6f * c.cdlin.y + 0.1f * c.cdlin.z;
    const F3 tint = lum > 0.f ? divs(c.cdlin, lum) : f3(1.f, 1.f, 1.f);
    const float s8 = specular * 0.08f;
    const F3 m = f3(mixf(1.f, tint.x, specular_tint), mixf(1.f, tint.y, specular_tint),
                    mixf(1.f, tint.z, specular_tint));
    const F3 a = scl(s8, m);
    c.cspec0 = f3(mixf(a.x, c.cdlin.x, metallic), mixf(a.y, c.cdlin.y, metallic), mixf(a.z, c.cdlin.z, metallic));
    c.csheen = f3(mixf(1.f, tint.x, sheen_tint), mixf(1.f, tint.y, sheen_tint), mixf(1.f, tint.z, sheen_tint));
    return c;
}
// the direction-independent scalars (disney.cpp:151-153, :164 with GTR1's :311-313), from the ten parameters
NHD void disney_fold_params(DDisney &p) {
    const float aspect = f_sqrt(1.f - p.anisotropic * 0.9f);
    p.ax = e_max(0.001f, p.roughness * p.roughness / aspect);
    p.ay = e_max(0.001f, p.roughness * p.roughness * aspect);
    const float a = mixf(0.1f, 0.001f, p.clearcoat_gloss), a2 = a * a;  // a < 1: GTR1's a >= 1 return never fires
    p.cc_a2m1 = a2 - 1.f;
    p.cc_pilog = kPi * f_log(a2);
}
NHD float smith_ggx_aniso(float nv, float vx, float vy, float ax, float ay) {  // disney.cpp:295-298
    return 1.f / (nv + f_sqrt(vx * ax * vx * ax + vy * ay * vy * ay + nv * nv));
}
NHD float smith_ggx(float nv, float alpha_g) {  // disney.cpp:300-305
    const float a = alpha_g * alpha_g, b = nv * nv;
    return 1.f / (nv + f_sqrt(a + b - a * b));
}
// Disney::eval (disney.cpp:111-174): L = wi, V = wo, X = (1, 0, 0), Y = (0, 1, 0) (so H.dot(X) = H.x + 0 etc.); no
// measure check. alb is read only when the albedo is textured (b.tex): else the colours folded at upload.
NHD F3 disney_eval(const DBsdf &b, F3 L, F3 V, F3 alb) {
    const float ndl = L.z, ndv = V.z;
    if (ndl < kEps || ndv < kEps) return f3(0, 0, 0);
    const DDisney p = *disney_rec(b);
    DisneyCol c;
    if (b.tex) {
        c = disney_colors(p.specular, p.specular_tint, p.metallic, p.sheen_tint, alb);
    } else {
        c.cdlin = f3(p.cdlin[0], p.cdlin[1], p.cdlin[2]);
        c.cspec0 = f3(p.cspec0[0], p.cspec0[1], p.cspec0[2]);
        c.csheen = f3(p.csheen[0], p.csheen[1], p.csheen[2]);
    }
    const F3 H = normalized(add(L, V));
    const float ndh = H.z, ldh = dot(L, H);
    // diffuse fresnel (:140-143)
    const float FL = schlick_fresnel(ndl), FV = schlick_fresnel(ndv);
    const float fd90 = 0.5f + 2.f * ldh * ldh * p.roughness;
    const float Fd = mixf(1.f, fd90, FL) * mixf(1.f, fd90, FV);
    // Hanrahan-Krueger subsurface approximation (:146-148)
    const float fss90 = ldh * ldh * p.roughness;
    const float Fss = mixf(1.f, fss90, FL) * mixf(1.f, fss90, FV);
    const float ss = 1.25f * (Fss * (1.f / (ndl + ndv) - 0.5f) + 0.5f);
    // specular (:151-158); GTR2_aniso (:315-318) with pow(x, 2.f) as x * x
    const float hx = H.x / p.ax, hy = H.y / p.ay;
    const float g = hx * hx + hy * hy + ndh * ndh;
    const float Ds = 1.f / (kPi * p.ax * p.ay * (g * g));
    const float FH = schlick_fresnel(ldh);
    const F3 Fs = f3(mixf(c.cspec0.x, 1.f, FH), mixf(c.cspec0.y, 1.f, FH), mixf(c.cspec0.z, 1.f, FH));
    float Gs = smith_ggx_aniso(ndl, L.x, L.y, p.ax, p.ay);
    Gs *= smith_ggx_aniso(ndv, V.x, V.y, p.ax, p.ay);
    // sheen (:161)
    const F3 Fsheen = scl(FH * p.sheen, c.csheen);
    // clearcoat (:164-166); GTR1 (:307-314) with its a2 - 1 and M_PI * log(a2) from the record
    const float t1 = 1.f + p.cc_a2m1 * ndh * ndh;
    const float Dr = p.cc_a2m1 / (p.cc_pilog * t1);
    const float Fr = mixf(0.04f, 1.f, FH);
    const float Gr = smith_ggx(ndl, 0.25f) * smith_ggx(ndv, 0.25f);
    // :168
    const float dm = kInvPi * mixf(Fd, ss, p.subsurface), om = 1.f - p.metallic;
    const float cc = 0.25f * p.clearcoat * Gr * Fr * Dr;
    F3 r = f3((dm * c.cdlin.x + Fsheen.x) * om + Gs * Fs.x * Ds + cc, (dm * c.cdlin.y + Fsheen.y) * om + Gs * Fs.y * Ds + cc,
              (dm * c.cdlin.z + Fsheen.z) * om + Gs * Fs.z * Ds + cc);
    // :171-172, Color3f::getLuminance (color.h)
    const float lum = r.x * 0.212671f + r.y * 0.715160f + r.z * 0.072169f;
    if (lum > 1.f) r = divs(r, lum);
    return r;
}

// alb: the diffuse albedo at the query's uv (m_albedo->eval(bRec.uv): the constant albedo, or its texture's
// value, nh_shade.h bsdf_albedo); unused by the other BSDFs
NHD F3 bsdf_eval(const DBsdf &b, F3 wi, F3 wo, int measure, F3 alb) {
    if (kDisney && b.type == BSDF_DISNEY) return disney_eval(b, wi, wo, alb);
    if (b.type == BSDF_DIFFUSE) {  // diffuse.cpp:94-103
        if (measure != M_SOLID_ANGLE || wi.z <= 0 || wo.z <= 0) return f3(0, 0, 0);
        return f3(alb.x * kInvPi, alb.y * kInvPi, alb.z * kInvPi);
    }
    if (b.type == BSDF_MICROFACET) {  // microfacet.cpp:92-105
        if (wo.z < 0.f) return f3(0, 0, 0);
        F3 wh = normalized(add(wi, wo));
        float den = b.ks * beckmann_d(b, wh) * fresnel(dot(wh, wi), b.ext_ior, b.int_ior) * smith_g1(b, wi, wh) *
                    smith_g1(b, wo, wh);
        float num = 4.f * wi.z * wo.z;
        float spec = den / num;
        return f3(b.kr * kInvPi + spec, b.kg * kInvPi + spec, b.kb * kInvPi + spec);
    }
    return f3(0, 0, 0);
}
NHD float bsdf_pdf(const DBsdf &b, F3 wi, F3 wo, int measure) {
    if (b.type == BSDF_DIFFUSE || (kDisney && b.type == BSDF_DISNEY)) {  // diffuse.cpp:106-120, disney.cpp:198-205
        if (measure != M_SOLID_ANGLE || wi.z <= 0 || wo.z <= 0) return 0.0f;
        return kInvPi * wo.z;
    }
    if (b.type == BSDF_MICROFACET) {  // microfacet.cpp:108-119
        if (wo.z <= 0) return 0.f;
        F3 wh = normalized(add(wo, wi));
        float p1 = b.ks * beckmann_d(b, wh) * wh.z / (4.f * dot(wo, wh));
        float p2 = (1.f - b.ks) * wo.z * kInvPi;
        return p1 + p2;
    }
    return 0.0f;
}
// returns the sample weight; wo/measure out (wo stays (0,0,0) on early returns, vector.h:49)
NHD F3 bsdf_sample(const DBsdf &b, F3 wi, float sx, float sy, F3 &wo, int &measure, F3 alb) {
    wo = f3(0, 0, 0);
    measure = M_UNKNOWN;
    switch (b.type) {
        case BSDF_DIFFUSE:  // diffuse.cpp:123-140
            if (wi.z <= 0) return f3(0, 0, 0);
            measure = M_SOLID_ANGLE;
            wo = cosine_hemisphere(sx, sy);
            return alb;
        case BSDF_MIRROR:  // mirror.cpp:41-57
            if (wi.z <= 0) return f3(0, 0, 0);
            wo = f3(-wi.x, -wi.y, wi.z);
            measure = M_DISCRETE;
            return f3(1, 1, 1);
        case BSDF_DIELECTRIC: {  // dielectric.cpp:51-102
            float F = fresnel(wi.z, b.ext_ior, b.int_ior);
            measure = M_DISCRETE;
            if (sx < F) {
                wo = f3(-wi.x, -wi.y, wi.z);
                return f3(1, 1, 1);
            }
            F3 nrm = f3(0.f, 0.f, 1.f);
            float eta;
            if (wi.z < 0.f) {
                nrm = neg(nrm);
                eta = b.int_ior / b.ext_ior;
            } else {
                eta = b.ext_ior / b.int_ior;
            }
            float dn = dot(wi, nrm);
            F3 wt1 = scl(-eta, sub(wi, scl(dn, nrm)));
            double p2 = (double)dn * (double)dn;  // std::pow(float, 2) in double (exact)
            double root = sqrt(1.0 - (double)(eta * eta) * (1.0 - p2));
            F3 wt2 = scl((float)(-root), nrm);
            wo = add(wt1, wt2);
            float w = 1.f / eta / eta;
            return f3(w, w, w);
        }
        case BSDF_MICROFACET: {  // microfacet.cpp:122-148
            if (wi.z < 0) return f3(0, 0, 0);
            float s1 = sy;
            if (s1 < b.ks) {
                s1 /= b.ks;
                F3 wh = beckmann(sx, s1, b.alpha);
                wo = sub(scl(2.f, scl(dot(wi, wh), wh)), wi);
            } else {
                s1 = (s1 - b.ks) / (1.f - b.ks);
                wo = cosine_hemisphere(sx, s1);
            }
            if (wo.z <= 0.f) return f3(0, 0, 0);
            F3 e = bsdf_eval(b, wi, wo, M_UNKNOWN, alb);
            float p = bsdf_pdf(b, wi, wo, M_UNKNOWN);
            return f3(e.x / p * wo.z, e.y / p * wo.z, e.z / p * wo.z);
        }
    }
    if (kDisney && b.type == BSDF_DISNEY) {  // disney.cpp:176-196: returns eval itself, not eval * cos / pdf
        if (wi.z <= 0) return f3(0, 0, 0);
        measure = M_SOLID_ANGLE;
        wo = cosine_hemisphere(sx, sy);
        const F3 col = disney_eval(b, wi, wo, alb);
        if (bsdf_pdf(b, wi, wo, measure) < kEps) return f3(0, 0, 0);
        return col;
    }
    return f3(0, 0, 0);
}

// DiscretePDF::sample (dpdf.h:124-130): lower_bound then clamp
// DiscretePDF::sample (dpdf.h): the first CDF entry not below x, minus one, clamped. [lo, hi): the search range of
// that first entry (the whole CDF, or a guide table's bracket, dpdf_sample_guided)
NHD int dpdf_search(const float *cdf, int n_entries, float x, int lo, int hi) {
    while (lo < hi) {
        int mid = (lo + hi) >> 1;
        if (cdf[mid] < x) lo = mid + 1;
        else hi = mid;
    }
    int index = lo - 1;
    if (index < 0) index = 0;
    if (index > n_entries - 1) index = n_entries - 1;
    return index;
}
NHD int dpdf_sample(const float *cdf, int n_entries, float x) { return dpdf_search(cdf, n_entries, x, 0, n_entries + 1); }
// the emitter pick of the integrators (m_emitterPDF.sample): with one emitter DiscretePDF::sample's clamp returns 0 for
// every x, so the two dependent CDF reads of the search are skipped (the caller still draws x)
NHD int emitter_pick(const DScene &S, float x) {
    return S.n_emitters == 1 ? 0 : dpdf_sample(S.emitter_cdf, S.n_emitters, x);
}

// The same search bracketed by a guide table (Chen & Asau's cutpoint method), bit-identical: guide[j] is the first
// CDF index not below j / 2^bits (nh_upload.hip env_guide), and the first index not below x is monotone in x, so for
// j = floor(x * 2^bits) -- exact, a power-of-two scaling of x in [0, 1) -- it lies in [guide[j], guide[j + 1]]:
// the binary search runs over that bracket (a few entries) instead of the whole CDF (21 dependent loads for
// C5's 1500 x 750 envmap).
NHD int dpdf_sample_guided(const float *cdf, int n_entries, float x, const int *guide, int bits) {
    const float s = x * (float)(1 << bits);
    int j = (int)s;
    if (!(s >= 0.f)) j = 0;  // (x in [0, 1) from next1d; NaN would take the full bracket below)
    if (j > (1 << bits) - 1) j = (1 << bits) - 1;
    const int lo = guide[j], hi = guide[j + 1];
    if (!(x >= 0.f && x < 1.f)) return dpdf_sample(cdf, n_entries, x);
    return dpdf_search(cdf, n_entries, x, lo, hi);
}

}  // namespace nhd
