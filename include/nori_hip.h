/*
 * nori_hip.h -- C-ABI boundary of the MI355X-native Nori `path_mis` hot path.
 *
 * Everything crossing this boundary is plain C: PODs, pointers and sizes. No
 * C++ types, no exceptions, no torch types. Every call returns an int status
 * (NH_OK == 0); the message of the last failure on a context is available via
 * nh_last_error(), and for the context-free host calls via nh_host_last_error().
 *
 * What each entry point replaces in the reference (rogerbarton/optix-renderer,
 * paths relative to the reference root):
 *
 *   nh_scene_load_xml     loadFromXML + Scene::cloneAndInit/update
 *                         (src/utils/parser.cpp:28-378, src/utils/scene.cpp:59-202)
 *   nh_bvh_build          BVH::build (src/utils/bvh.cpp:54-380)
 *   nh_create/nh_destroy  OptixState context creation (include/nori/optix/OptixState.cpp:39-74)
 *   nh_upload_scene       OptixState::preRender scene/SBT upload
 *                         (include/nori/optix/OptixState.render.cpp:19-85, OptixState.cpp:344-411)
 *   nh_upload_bvh         OptixState GAS/IAS build (include/nori/optix/OptixState.as.cpp:47-248)
 *   nh_trace_rays         BVH::rayIntersect / Scene::rayIntersect
 *                         (src/utils/bvh.cpp:402-460, include/nori/scene.h:114-137)
 *   nh_render             RenderThread::renderThreadMain sample loop + renderBlock + PathMISIntegrator::Li
 *                         (src/utils/render.cpp:281-347, :421-459; src/integrators/path_mis.cpp:16-150)
 *                         and the OptiX subframe launch (include/nori/optix/OptixState.cpp:485-510)
 *   nh_get_framebuffer    ImageBlock master (src/utils/block.cpp:38-134); toBitmap is nh_framebuffer_to_rgb
 *   nh_reduce_framebuffers  (new) RCCL sum of per-GPU RGBW framebuffers over xGMI
 *   nh_denoise            Denoiser::denoise on the master ImageBlock after the render loop
 *                         (src/utils/render.cpp:368-369): SimpleDenoiser (src/denoiser/simple.cpp:29-76,
 *                         computeVarianceFromImage src/utils/common.cpp:339-398); the GPU counterpart of
 *                         OptixState::denoise (include/nori/optix/OptixState.denoiser.cpp:123-150)
 *
 * Conventions (mirroring the reference's threading contract):
 *   - input pointers are host-owned and only read during the call;
 *   - calls on one nh_ctx are serialised by the caller; distinct contexts may be
 *     driven from distinct host threads (one per GPU).
 */
#ifndef NORI_HIP_H
#define NORI_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define NH_OK 0
#define NH_ERR_INVALID 1
#define NH_ERR_IO 2
#define NH_ERR_DEVICE 3
#define NH_ERR_UNSUPPORTED 4
#define NH_ERR_STATE 5

/* ---- scene description (flattened Nori scene graph) --------------------- */

enum { NH_SHAPE_MESH = 0, NH_SHAPE_SPHERE = 1 };
enum { NH_BSDF_DIFFUSE = 0, NH_BSDF_MIRROR = 1, NH_BSDF_DIELECTRIC = 2, NH_BSDF_MICROFACET = 3, NH_BSDF_DISNEY = 4 };
enum { NH_EMITTER_AREA = 0, NH_EMITTER_POINT = 1, NH_EMITTER_ENVMAP = 2, NH_EMITTER_SPOT = 3,
       NH_EMITTER_DIRECTIONAL = 4 };
/* path_mis (src/integrators/path_mis.cpp), path_mats (path_mats.cpp), the single-bounce
 * direct_ems / direct_mats / direct_mis (direct_ems.cpp, direct_mats.cpp, direct_mis.cpp), the
 * point-light `direct` integrator (direct.cpp, scenes/pa1) and the `normals` integrator of the normal-map scenes
 * (normals.cpp: |shFrame.toWorld(direction)|, the envmap on a miss) */
enum { NH_INTEGRATOR_PATH_MIS = 0, NH_INTEGRATOR_PATH_MATS = 1, NH_INTEGRATOR_DIRECT_EMS = 2,
       NH_INTEGRATOR_DIRECT_MATS = 3, NH_INTEGRATOR_DIRECT_MIS = 4, NH_INTEGRATOR_DIRECT = 5,
       NH_INTEGRATOR_NORMALS = 6,
       /* the volumetric path tracers (path_vol_mats.cpp, path_vol_mis.cpp): the only integrators that render a scene
          with a participating medium or a shape without a BSDF */
       NH_INTEGRATOR_PATH_VOL_MATS = 7, NH_INTEGRATOR_PATH_VOL_MIS = 8,
       /* the photon mapper (photonmapper.cpp): renders once nh_photon_map_build has built the context's photon map */
       NH_INTEGRATOR_PHOTONMAPPER = 9,
       /* ambient occlusion (av.cpp: one occlusion ray of length nh_av_params::length per camera hit; renders once
          nh_set_av_params has given the context that length) and the environment map's pdf / 100
          (EnvMapTester.cpp: needs an environment map) */
       NH_INTEGRATOR_AV = 10, NH_INTEGRATOR_ENVMAPTESTER = 11 };

/* One Nori Shape (src/shapes/mesh.cpp, src/shapes/sphere.cpp). Mesh data lives in
 * the scene-wide concatenated arrays at the given offsets. */
typedef struct nh_shape {
    int32_t type;            /* NH_SHAPE_* */
    int32_t bsdf;            /* index into nh_scene_desc.bsdfs (default diffuse 0.5); -1 = none, legal only for a shape
                                with a medium (nh_scene_desc.shape_medium; Shape::cloneAndInit, shape.cpp:33-35) */
    int32_t emitter;         /* index into nh_scene_desc.emitters, or -1 */
    uint32_t v_offset;       /* first vertex in V/N/UV/T/BT */
    uint32_t n_vertices;
    uint32_t f_offset;       /* first face in F (face indices are local to the shape) */
    uint32_t n_faces;
    int32_t has_normals;     /* N present (per vertex) */
    int32_t has_uvs;         /* UV present (per vertex); tangents T/BT present iff both */
    float center[3];         /* sphere */
    float radius;            /* sphere */
    float bbox_min[3];       /* Shape::getBoundingBox() */
    float bbox_max[3];
    uint32_t pdf_offset;     /* mesh area DiscretePDF: n_faces+1 CDF entries in area_cdf */
    float pdf_normalization; /* DiscretePDF::getNormalization() = 1/sum(area) */
    uint32_t normal_map;     /* 1 + index into nh_scene_desc.textures of the shape's <texture name="normal"> child
                                (Shape::addChild, src/shapes/shape.cpp:138-147), 0 = none. It perturbs the shading
                                frame: meshes with normals and uvs take normalize(TBN * eval(uv)) (mesh.cpp:165-185),
                                spheres re-derive their frame from shFrame.toWorld(eval(uv)) (sphere.cpp:115-121) */
} nh_shape;

/* One Nori BSDF (src/bsdf/{diffuse,mirror,dielectric,microfacet,disney}.cpp). nh_upload_scene rejects a type
 * outside NH_BSDF_DIFFUSE..NH_BSDF_DISNEY with NH_ERR_INVALID. */
typedef struct nh_bsdf {
    int32_t type;            /* NH_BSDF_* */
    float albedo[3];         /* diffuse / disney: constant albedo texture */
    float alpha;             /* microfacet: Beckmann roughness */
    float int_ior, ext_ior;  /* dielectric / microfacet */
    float kd[3];             /* microfacet diffuse base */
    float ks;                /* microfacet: 1 - max(kd) */
    uint32_t albedo_texture; /* diffuse / disney: 1 + index into nh_scene_desc.textures of its Texture<Color3f> albedo
                                child (diffuse.cpp:70-91, disney.cpp:88-109); 0 = the constant albedo above */
    /* disney (disney.cpp:32-41), each after the constructor's clamp(.., 0, 1), in this order: metallic [0],
       subsurface [0], specular [0.5], roughness [0.5], specularTint [0], anisotropic [0], sheen [0], sheenTint [0.5],
       clearcoat [0], clearcoatGloss [1]. Appended: clients that fill the fields above by name compile unchanged. */
    float metallic, subsurface, specular, roughness, specular_tint, anisotropic, sheen, sheen_tint, clearcoat,
          clearcoat_gloss;
} nh_bsdf;

/* A Texture<Color3f> child of a BSDF, evaluated at the hit's uv (Intersection::uv, BSDFQueryRecord::uv):
 *   NH_TEXTURE_CONSTANT     ConstantTexture (src/textures/consttexture.cpp): value1
 *   NH_TEXTURE_CHECKERBOARD Checkerboard<Color3f> (src/textures/checkerboard.cpp:29-47): value1 / value2 by the
 *                           parity of the cell of uv / scale - delta
 *   NH_TEXTURE_PNG          PNGTexture (src/textures/PNGTexture.cpp:125-160): nearest texel of an sRGB-decoded RGBA
 *                           image (row 0 of the PNG first) at texel_offset in nh_scene_desc.texels; with
 *                           linear = 1 (sRGB = false, the default for a texture named "normal", PNGTexture.cpp:26)
 *                           the texels hold the normal-map decode of loadFromFile (x / 255 * 2 - 1 with every third
 *                           float of the RGBA array normalized as a Vector3f, PNGTexture.cpp:85-95) and eval blends
 *                           the texel by intensity and normalizes it (:155-161) */
enum { NH_TEXTURE_CONSTANT = 0, NH_TEXTURE_CHECKERBOARD = 1, NH_TEXTURE_PNG = 2 };
typedef struct nh_texture {
    int32_t type;            /* NH_TEXTURE_* */
    float value1[3];         /* constant value / checkerboard value1 */
    float value2[3];         /* checkerboard value2 */
    float delta[2];          /* checkerboard Point2f delta */
    float scale[2];          /* checkerboard Vector2f scale */
    int32_t width, height;   /* png */
    uint64_t texel_offset;   /* png: first texel (4 floats) in nh_scene_desc.texels */
    float scale_u, scale_v;  /* png scaleU / scaleV */
    float offset_u, offset_v;/* png offsetU / offsetV (non-spherical lookups) */
    int32_t spherical;       /* png sphericalTexture */
    float rotation[9];       /* png spherical lookups: the eulerAngles rotation (PNGTexture.cpp:133-139), row-major;
                                identity for eulerAngles = 0 */
    int32_t linear;          /* png: sRGB = false (normal-map decode + eval's intensity blend and normalize) */
    float intensity;         /* png, linear: PNGTexture intensity [1] */
    int32_t pad;
} nh_texture;

/* One Nori Emitter (src/emitters/{arealight,pointlight,environmentmap,spotlight,directionalLight}.cpp).
 * nh_upload_scene rejects a type outside NH_EMITTER_AREA..NH_EMITTER_DIRECTIONAL with NH_ERR_INVALID. */
typedef struct nh_emitter {
    int32_t type;            /* NH_EMITTER_* */
    int32_t shape;           /* area light: owning shape, else -1 */
    float radiance[3];       /* area / directional: radiance; point: power / (4 pi); spot: the intensity
                                I = power / 2 / pi / (1 - 0.5 (cos_total_width + cos_falloff_start))
                                (spotlight.cpp:50, :67-69) */
    float light_prob;        /* lightWeight (emitter DiscretePDF weight) */
    float position[3];       /* point / spot light */
    float pad;
} nh_emitter;

/* What a spot / directional light holds beyond its nh_emitter, which keeps its 32 bytes: entry i of
 * nh_scene_desc.emitter_ext belongs to emitter i; the entries of other emitter types are not read. */
typedef struct nh_emitter_ext {
    float direction[3];      /* m_direction: the `direction` property, normalized (non-zero and finite) */
    float cos_total_width;   /* spot: cos(degToRad(totalwidth / 2)) (spotlight.cpp:68) */
    float frame_s[3];        /* m_coord = Frame(direction) (spot: Frame(direction.normalized()), spotlight.cpp:21) */
    float cos_falloff_start; /* spot: cos(degToRad(falloffstart)) (spotlight.cpp:67) */
    float frame_t[3];
    float cos_theta_max;     /* directional: cos(degToRad(angle)) (directionalLight.cpp:92) */
    float frame_n[3];
    float pad;
} nh_emitter_ext;

/* One Nori Medium (src/media/{vacuum,homogmedium}.cpp, medium.cpp) with its phase function (src/bsdf/isophase.cpp,
 * anisophase.cpp). nh_upload_scene rejects a type outside NH_MEDIUM_VACUUM..NH_MEDIUM_HOMOG or a phase outside
 * NH_PHASE_ISO..NH_PHASE_HG with NH_ERR_INVALID. The coefficients are the derived ones, each an fp32 product in this
 * order: sigma_x = sigma_x (normalized colour) * sigma_x_intensity, mu_a = density * sigma_a, mu_s = density * sigma_s,
 * mu_t = mu_a + mu_s (defaults: sigma_a 0.5, sigma_s 0, intensities 1, density 1). */
enum { NH_MEDIUM_VACUUM = 0, NH_MEDIUM_HOMOG = 1 };
enum { NH_PHASE_ISO = 0, NH_PHASE_HG = 1 };
typedef struct nh_medium {
    int32_t type;            /* NH_MEDIUM_* */
    float mu_a[3];           /* absorption coefficient */
    float mu_s[3];           /* scattering coefficient */
    float mu_t[3];           /* extinction coefficient */
    float density;
    int32_t phase;           /* NH_PHASE_* */
    float g;                 /* NH_PHASE_HG: Henyey-Greenstein's g (anisophase.cpp) */
} nh_medium;

/* PerspectiveCamera after update() (src/cameras/perspective.cpp:48-96). Row-major 4x4. */
typedef struct nh_camera {
    int32_t width, height;
    float sample_to_camera[16];
    float camera_to_world[16];
    float inv_output_size[2];
    float near_clip, far_clip;
    /* after cloneAndInit's fstop <-> lensRadius coupling (perspective.cpp:37-42). lens_radius > 1e-4 (Epsilon):
       thin lens (perspective.cpp:114-130); camera ray k of the serial render order (round, BlockGenerator
       spiral, x-major pixels) takes draws 2k, 2k+1 of a default-state pcg32 -- the reference's static sampler */
    float lens_radius, focal_distance;
    /* which of those two draws is the lens sample's x: Independent::next2D builds Point2f(nextFloat(), nextFloat())
       (independent.cpp:74-78), whose argument evaluation order C++ leaves unspecified. NH_LENS_DRAWS_RTL (the
       loader's default): x = draw 2k+1, y = draw 2k, as g++ compiles it (oracle/normalmap_probe.cpp "order");
       NH_LENS_DRAWS_LTR: x = draw 2k, as clang compiles it */
    int32_t lens_draw_order;
} nh_camera;
enum { NH_LENS_DRAWS_LTR = 0, NH_LENS_DRAWS_RTL = 1 };

/* Tabulated reconstruction filter as ImageBlock::init builds it (src/utils/block.cpp:54-70). */
typedef struct nh_filter {
    float radius;
    int32_t border;          /* ceil(radius - 0.5) */
    float lookup_factor;     /* NORI_FILTER_RESOLUTION / radius */
    float table[33];         /* NORI_FILTER_RESOLUTION + 1 entries, last = 0 */
} nh_filter;

/* EnvMap emitter (src/emitters/environmentmap.cpp) with its albedo texture: a png_texture
 * (src/textures/PNGTexture.cpp, sRGB-decoded RGBA floats, PNG row 0 first) or the constant 0.5
 * fallback as a 1x1 texture. */
typedef struct nh_envmap {
    int32_t width, height;        /* texture size (getWidth/getHeight); 1x1 for constant textures */
    const float *rgba;            /* width*height*4 floats (PNGTexture::data) */
    float radiance[3];            /* EnvMap radiance multiplier */
    float scale_u, scale_v;       /* PNGTexture scaleU/scaleV */
    float offset_u, offset_v;     /* PNGTexture offsetU/offsetV (non-spherical lookups) */
    int32_t spherical;            /* PNGTexture sphericalTexture */
    int32_t constant;             /* ConstantTexture: eval ignores uv */
    const float *cdf;             /* EnvMap::calculateProbs DiscretePDF: width*height+1 CDF entries */
    float normalization;          /* DiscretePDF::getNormalization() */
    float rotation[9];            /* spherical lookups: the png_texture's eulerAngles rotation (PNGTexture.cpp:133-139),
                                     row-major; identity for eulerAngles = 0 */
} nh_envmap;

/* <denoiser> of the scene (Scene::m_denoiser, src/utils/scene.cpp:242-245): SimpleDenoiser's parameters after
 * its constructor's clamps (src/denoiser/simple.cpp:15-24): sigma_d = clamp(sigma_d [0], Epsilon, 10),
 * sigma_vr = clamp(sigma_vr [0.6], Epsilon, 10), range = clamp(range [1], 0, 50), amount = clamp(amount [1], 1, 10) */
enum { NH_DENOISER_NONE = 0, NH_DENOISER_SIMPLE = 1 };
typedef struct nh_denoiser {
    int32_t type;            /* NH_DENOISER_* */
    float sigma_d;           /* spatial Gaussian sigma (pixels) */
    float sigma_vr;          /* range sigma of the variance-scaled L1 colour distance */
    int32_t range;           /* window half-size: (2 range + 1)^2 pixels */
    int32_t amount;          /* passes */
} nh_denoiser;

/* <sampler> types: independent (src/samplers/independent.cpp) and adaptive (src/samplers/adaptive.cpp). Both take
 * per-path pcg32 streams on the HIP path; an adaptive scene renders through the adaptive loop of nh_render. */
enum { NH_SAMPLER_INDEPENDENT = 0, NH_SAMPLER_ADAPTIVE = 1 };

typedef struct nh_scene_desc {
    nh_camera camera;
    nh_filter filter;
    int32_t integrator;      /* NH_INTEGRATOR_* */
    int32_t sample_count;    /* sampler sampleCount */
    uint32_t n_shapes;
    const nh_shape *shapes;
    uint32_t n_bsdfs;
    const nh_bsdf *bsdfs;
    uint32_t n_emitters;
    const nh_emitter *emitters;
    const float *emitter_cdf;     /* Scene::emitterDpdf CDF, n_emitters+1 entries */
    int32_t envmap;               /* emitter index of the environment map, or -1 */
    uint32_t n_vertices;          /* total over all meshes */
    const float *V;               /* 3 floats per vertex */
    const float *N;               /* 3 per vertex (zeros for meshes without normals) */
    const float *UV;              /* 2 per vertex */
    const float *T;               /* 3 per vertex: accumulated tangents (mesh.cpp:165-190 uses normalised) */
    const float *BT;              /* 3 per vertex */
    uint32_t n_faces;
    const uint32_t *F;            /* 3 per face, local to the owning shape */
    uint32_t n_area_cdf;
    const float *area_cdf;        /* concatenated per-mesh area CDFs */
    nh_envmap env;                /* valid when envmap >= 0 */
    nh_denoiser denoiser;         /* type NH_DENOISER_NONE when the scene has none */
    uint32_t n_textures;          /* BSDF albedo textures (nh_bsdf.albedo_texture) */
    const nh_texture *textures;
    uint64_t n_texels;            /* RGBA texels of every png texture, 4 floats each */
    const float *texels;
    float normals_direction[3];   /* NH_INTEGRATOR_NORMALS: its `direction` point [0, 0, 1] (normals.cpp:10-12) */
    /* Appended (clients that fill the fields above by name compile unchanged): n_emitters entries, or NULL when the
       scene has no spot / directional light */
    const nh_emitter_ext *emitter_ext;
    /* Appended: participating media. A zero-filled tail means "no media". */
    uint32_t n_media;
    const nh_medium *media;
    const uint32_t *shape_medium; /* n_shapes entries: 1 + index into media of the shape's <medium>, 0 = none; may be
                                     NULL (no shape has a medium) */
    uint32_t ambient_medium;      /* 1 + index into media of the scene's ambient <medium>, 0 = vacuum */
    /* Appended: the scene's <sampler>. A zero-filled tail means the independent sampler. */
    int32_t sampler;                   /* NH_SAMPLER_* */
    int32_t adaptive_initial_uniform;  /* NH_SAMPLER_ADAPTIVE: initialUniform after AdaptiveSampler's clamp to
                                          [1, sampleCount] (src/samplers/adaptive.cpp:21); below 1 counts as 1 */
} nh_scene_desc;

/* ---- BVH in the reference's own layout (include/nori/bvh.h:127-165) ---- */

/* 32-byte node: word0 = flag | (size_or_axis << 1), word1 = leaf start / right child. */
typedef struct nh_bvh_node {
    uint32_t word0;
    uint32_t word1;
    float bbox_min[3];
    float bbox_max[3];
} nh_bvh_node;

typedef struct nh_bvh_desc {
    uint32_t n_nodes;
    const nh_bvh_node *nodes;
    uint32_t n_indices;           /* == primitive count */
    const uint32_t *indices;      /* global primitive ids in leaf order */
    uint32_t n_shapes;
    const uint32_t *shape_offset; /* n_shapes+1 prefix sums of primitive counts (BVH::m_shapeOffset) */
    float bbox_min[3], bbox_max[3];
    uint32_t max_depth;           /* deepest node level (root = 0): bounds the traversal stack */
} nh_bvh_desc;

/* ---- ray batches for the traversal entry point -------------------------- */

typedef struct nh_ray_soa {
    const float *ox, *oy, *oz;
    const float *dx, *dy, *dz;
    const float *mint, *maxt;     /* Ray3f semantics: mint == 1e-4f triggers the adaptive epsilon */
} nh_ray_soa;

typedef struct nh_hit_soa {
    uint8_t *hit;                 /* 0/1 */
    float *t, *u, *v;             /* closest-hit only */
    uint32_t *prim;               /* global primitive id, closest-hit only */
    uint32_t *shape;              /* shape index, closest-hit only */
} nh_hit_soa;

/* ---- rendering ------------------------------------------------------------ */

enum { NH_MODE_MEGAKERNEL = 0, NH_MODE_WAVEFRONT = 1 };
/* Visit orders of BVH::rayIntersect (src/utils/bvh.cpp:402-460); all three return the reference's hit.
 *   REFERENCE  binary tree, left child first (the reference's order)
 *   ORDERED    binary tree, nearer child first
 *   WIDE       4-wide collapse of the same tree (same boxes), nearer child first; nh_render uses it
 *              for deep trees whenever the traversal is not REFERENCE */
enum { NH_TRAVERSAL_REFERENCE = 0, NH_TRAVERSAL_ORDERED = 1, NH_TRAVERSAL_WIDE = 2 };

typedef struct nh_render_req {
    int32_t sample_begin;         /* sample rounds [sample_begin, sample_end) */
    int32_t sample_end;
    uint64_t seed;                /* base of the per-(pixel, sample) pcg32 seeding contract */
    int32_t n_blocks;             /* number of 32x32 image blocks this context renders; 0 = all */
    const int32_t *blocks;        /* block ids (by*nbx+bx) when n_blocks > 0 */
    int32_t mode;                 /* NH_MODE_* */
    int32_t traversal;            /* NH_TRAVERSAL_* */
    int32_t clear;                /* zero the framebuffer first */
    int32_t collect_stats;        /* 1: count BVH nodes/prims visited (calibration, slower) */
} nh_render_req;

/* LDS budget (bytes) of the scene tables the diffuse area-light bounce kernels stage beside a small BVH: 64 per shape,
   48 per BSDF, 32 per emitter, the emitting meshes' area CDFs (4 per entry, rounded up to 16) and 48 per emitting
   face. A scene over it renders with the general kernels (nh_render_stats::bounce_traits = 1). */
#define NH_SMALL_TABLES_BYTES 4096

typedef struct nh_render_stats {
    double kernel_ms_path;        /* summed device time of the path-tracing kernel(s) */
    double kernel_ms_splat;       /* summed device time of the ImageBlock splat kernel */
    double kernel_ms_extend;      /* wavefront: closest-hit kernel */
    double kernel_ms_shadow;      /* wavefront: any-hit kernel */
    double kernel_ms_shade;       /* wavefront: shading kernels */
    uint64_t launches_path, launches_splat, launches_extend, launches_shadow, launches_shade;
    uint64_t samples;             /* camera samples traced */
    uint64_t ray_queries;         /* closest + any-hit queries (collect_stats) */
    uint64_t nodes_visited;       /* BVH inner-node pops (collect_stats) */
    uint64_t boxes_tested;        /* child boxes tested (collect_stats) */
    uint64_t prims_tested;        /* primitive intersection tests (collect_stats) */
    uint64_t invalid_samples;     /* ImageBlock::put drops (NaN/Inf/negative) */
    /* wavefront mode: the any-hit kernel's share of ray_queries / nodes_visited / boxes_tested /
       prims_tested (the rest is the extend kernel's) */
    uint64_t shadow_queries, shadow_nodes_visited, shadow_boxes_tested, shadow_prims_tested;
    /* wavefront mode, always counted (host side, from the queue counts): path-state bytes the
       shade kernels load + store, and the queue bytes of the extend / any-hit kernels */
    uint64_t shade_state_bytes, extend_queue_bytes, shadow_queue_bytes, paths_shaded;
    /* wavefront mode: the tail kernel that finishes the last few live paths of a chunk in place */
    double kernel_ms_tail;
    uint64_t launches_tail;
    /* bytes of one BVH node as counted in nodes_visited: 64 (binary tree) or 128 (the 4-wide
       collapse, NH_TRAVERSAL_WIDE), for the last render */
    uint64_t node_bytes;
    /* the tail kernel's share of ray_queries / nodes_visited / boxes_tested / prims_tested (closest
       + any hit), and of that its any-hit part (also counted in shadow_*), collect_stats only */
    uint64_t tail_queries, tail_nodes_visited, tail_boxes_tested, tail_prims_tested;
    uint64_t tail_shadow_queries, tail_shadow_nodes_visited, tail_shadow_boxes_tested, tail_shadow_prims_tested;
    /* 1 when the last wavefront render traversed an LDS copy of the BVH (scenes of a few KB): its node
       and primitive reads then come from LDS, not HBM */
    uint64_t lds_scene;
    /* 1 when the last wavefront render ran one fused bounce kernel per bounce (shade + any-hit +
       closest-hit, LDS-staged BVHs): its time is in kernel_ms_shade, extend/shadow times are 0 */
    uint64_t fused_bounce;
    /* RCCL communicator cliques created by nh_reduce_framebuffers with this context as root (a clique
       is reused while the same contexts reduce again) */
    uint64_t comm_inits;
    /* nh_denoise / nh_denoise_image: summed device time and kernel launches */
    double kernel_ms_denoise;
    uint64_t launches_denoise;
    /* wavefront chunks whose tail kernel ran on a tail slot's stream, decoupled from the chunk's path pool
       (RR-ahead pipeline with several pools: the pool took the next chunk meanwhile) */
    uint64_t tails_async;
    /* wavefront path pools the last render drove (NH_POOLS, else 2, or 3 for scenes with mirror / dielectric BSDFs) */
    uint64_t pools_active;
    /* 1 when the last wavefront render traced each bounce's closest-hit and any-hit queries in one persistent
       launch (deep BVHs, 4-wide tree): its time is in kernel_ms_extend, kernel_ms_shadow stays 0 */
    uint64_t trace_fused;
    /* RR-ahead tail kernel (wf_tail_rr), collect_stats only: cycles its lanes spent in the shade body, the light
       sample's any-hit query, the next closest hit and the next vertex's head (clock64, summed over lanes), the
       path-bounces it ran and its longest chain (bounces of one path) */
    uint64_t tail_cycles_body, tail_cycles_shadow, tail_cycles_closest, tail_cycles_head;
    uint64_t tail_bounces, tail_max_bounces;
    /* the same four phase sums and the path-bounce count for the bounces the tail's cooperative finish ran (a path
       carried by a 16-lane group once <= 4 remain in its wave): the latency of one bounce of the last chains */
    uint64_t tail_coop_cycles_body, tail_coop_cycles_shadow, tail_coop_cycles_closest, tail_coop_cycles_head;
    uint64_t tail_coop_bounces;
    /* RR-ahead bounce kernel (wf_bounce_rr), collect_stats only: cycles its lanes spent loading the path (state and
       the Intersection of its hit), in the body, the any-hit query, the closest hit, the head and ranking + storing
       the survivors (clock64, summed over lanes), and the path-bounces it ran */
    uint64_t bounce_cycles_load, bounce_cycles_body, bounce_cycles_shadow, bounce_cycles_closest, bounce_cycles_head;
    uint64_t bounce_cycles_store, bounce_bounces;
    /* which instantiation of the RR-ahead bounce kernel the last wavefront render ran: 0 none (another pipeline),
       1 the general kernels, 2 the diffuse area-light ones (path_mis, every BSDF diffuse with a constant albedo, every
       light an area light on a mesh, no envmap, normal map or thin lens; NH_BOUNCE_TRAITS=0 forces 1) */
    uint64_t bounce_traits;
    /* 1 when bounce 0 of the last render took its camera rays' first closest hit with the per-block candidate masks
       (nh_primary_masks): a wavefront render on the RR-ahead bounce kernels, at most 64 primitive records staged in
       LDS, a pinhole camera, no collect_stats; NH_PRIMARY_MASKS=0 forces 0. Every nh_render clears it (so it reads 0
       after a megakernel render) and a wavefront chunk sets it when it starts on a path pool, which for an
       asynchronous call can be after nh_render returns: read it after nh_synchronize. */
    uint64_t primary_masks;
    /* 1 when the last render's fused bounce / tail kernels tested pair records arranged by kind (nh_pair_layout with
       by_kind: triangles paired with triangles, spheres with spheres): a wavefront render on the LDS-staged fused
       kernels without collect_stats, the scene uploaded without NH_PAIR_KINDS=0 (read when the BVH is uploaded). 0: the
       reference arrangement, records paired in their own order. Cleared and set like primary_masks. */
    uint64_t pair_kinds;
    /* 1 when the last render's fused bounce kernels took their queries without a tree walk (nh_flat_image: the scene's
       tree is one leaf, or a root with two leaves, of at most 16 pair records): a wavefront render on the RR-ahead
       bounce kernels with pair_kinds 1, the scene uploaded without NH_FLAT_TRACE=0 (read when the BVH is uploaded).
       0: every query walks the tree. Cleared and set like primary_masks. */
    uint64_t flat_trace;
    /* which candidate masks the light samples' any-hit queries of the last render's RR-ahead bounce kernels ran with
       (nh_shadow_masks): 0 none, 2 the per-block words at bounce 0 (each holds the emitter-side word's zeros). Level 1
       -- the emitter-side word alone, at every bounce -- was measured and is not built: the field never reads 1, and
       NH_SHADOW_MASKS=1 gives 0 like NH_SHADOW_MASKS=0. 2 needs what primary_masks needs, that table, and a scene
       whose emitters are all area lights on meshes without vertex normals. Cleared and set like primary_masks. */
    uint64_t shadow_masks;
    /* how many primitive records the light samples' any-hit queries of the last render's flat bounce kernels could
       test: the records the scene-wide any-hit word keeps (nh_shadow_any_word), read from the flat image's any-hit
       section (nh_flat_image_any). 0: no section -- the scene is not flat, nothing can be left out, NH_ANY_LIST=0 (read
       when the BVH is uploaded) -- and those queries test the closest-hit pair records. Cleared and set like
       primary_masks. */
    uint64_t any_list;
} nh_render_stats;

typedef struct nh_scene nh_scene;
typedef struct nh_bvh nh_bvh;
typedef struct nh_ctx nh_ctx;

/* host-side scene ingestion */
int nh_scene_load_xml(const char *path, nh_scene **out);
/* <test> roots (src/utils/ttest.cpp) hold several <scene>s: load the index-th one */
int nh_scene_load_xml_index(const char *path, int32_t index, nh_scene **out);
int nh_scene_get_desc(const nh_scene *scene, nh_scene_desc *out);
/* overrides used by benchmarks and tests (camera resize recomputes the projection) */
int nh_scene_set_resolution(nh_scene *scene, int32_t width, int32_t height);
int nh_scene_set_sample_count(nh_scene *scene, int32_t spp);
/* the scene's sampler: NH_SAMPLER_INDEPENDENT, or NH_SAMPLER_ADAPTIVE with its initialUniform (clamped to
   [1, sampleCount] as the reference's constructor does; set the sample count first) */
int nh_scene_set_sampler(nh_scene *scene, int32_t type, int32_t initial_uniform);
int nh_scene_set_bsdf(nh_scene *scene, uint32_t shape, const nh_bsdf *bsdf);
/* append a texture to the scene's texture table (png: texels = width*height*4 floats, copied); returns its
   index + 1 for nh_bsdf.albedo_texture, or 0 on error (nh_host_last_error) */
uint32_t nh_scene_add_texture(nh_scene *scene, const nh_texture *tex, const float *texels);
/* give a shape a normal map (Shape::addChild of a <texture name="normal">, src/shapes/shape.cpp:138-147):
   texture = a value nh_scene_add_texture returned, 0 removes it */
int nh_scene_set_normal_map(nh_scene *scene, uint32_t shape, uint32_t texture);
/* the thin-lens sample's draw order (nh_camera.lens_draw_order): NH_LENS_DRAWS_RTL or NH_LENS_DRAWS_LTR */
int nh_scene_set_lens_draw_order(nh_scene *scene, int32_t order);
/* PNGTexture::loadFromFile's byte -> float loop over lodepng's RGBA8 array (PNGTexture.cpp:78-95): srgb != 0
   InverseGammaCorrect(b / 255) per byte; srgb == 0 the normal-map decode b / 255 * 2 - 1 with every third float
   of the array normalized as an Eigen Vector3f (the triples run over RGBA data, so they straddle pixels -- the
   reference's behaviour, reproduced). out: n floats. */
int nh_texture_decode(const uint8_t *rgba8, uint64_t n, int32_t srgb, float *out);
int nh_scene_set_integrator(nh_scene *scene, int32_t integrator);
/* <integrator type="photonmapper"> (src/integrators/photonmapper.cpp:36-41): photonCount [1000000] and photonRadius
 * [0 = automatic]. Kept beside nh_scene_desc, which does not grow. nh_scene_get_photon_params returns the radius
 * resolved as PhotonMapper::preprocess does (photonmapper.cpp:75-76): a radius of 0 becomes
 * scene->getBoundingBox().getExtents().norm() / 500.0f, in fp32 with Eigen's grouping, over the union of the shapes'
 * boxes (the BVH root box). nh_scene_set_photon_params overrides both (photon_count >= 1, photon_radius >= 0 and
 * finite; 0 = automatic again). On a scene with another integrator get returns the defaults. */
typedef struct nh_photon_params {
    int32_t photon_count;
    float photon_radius;
} nh_photon_params;
int nh_scene_get_photon_params(const nh_scene *scene, nh_photon_params *out);
int nh_scene_set_photon_params(nh_scene *scene, const nh_photon_params *params);
/* <integrator type="av"> (src/integrators/av.cpp:10-13): `length`, the occlusion ray's maxt. It has no default (the
 * loader refuses a scene without it). Kept beside nh_scene_desc, like nh_photon_params. On a scene with another
 * integrator get returns 0. set takes any length that is not NaN. */
typedef struct nh_av_params {
    float length;
} nh_av_params;
int nh_scene_get_av_params(const nh_scene *scene, nh_av_params *out);
int nh_scene_set_av_params(nh_scene *scene, const nh_av_params *params);
/* PhotonData::initialize (src/utils/photon.cpp:30-41): the five 256-entry decode tables, built with std::cos /
 * std::sin / std::ldexp on float as there; exp_table[0] = 0. Host only. */
int nh_photon_tables(float *cos_theta, float *sin_theta, float *cos_phi, float *sin_phi, float *exp_table);
void nh_scene_free(nh_scene *scene);
const char *nh_host_last_error(void);
/* Parity hook for the loader's transform arithmetic (the Eigen operations of parser.cpp:308-360,
 * transform.h:73-86, transform.cpp:9-10 and perspective.cpp:68-95 as the product restates them). One
 * request line in the protocol of oracle/eigen_xform_probe.cpp (floats as 8-hex-digit bit patterns:
 * "inv", "xf", "cam", "pt", "vec", "nrm"); writes the reply floats to out and returns their count, or
 * -1 (nh_host_last_error) for a malformed request or too small a cap. */
int nh_debug_transform(const char *request, float *out, int32_t cap);

int nh_bvh_build(const nh_scene_desc *scene, int32_t n_threads, nh_bvh **out);
int nh_bvh_get_desc(const nh_bvh *bvh, nh_bvh_desc *out);
void nh_bvh_free(nh_bvh *bvh);

/* Per-block candidate masks of the camera rays' first closest hit (host/primary_masks.cpp; host only). records:
 * n_records primitive records of 12 floats, as the device reads them -- a triangle (p0, .) (p1, .) (p2, bits), a sphere
 * (centre, radius) (., ., ., .) (., ., ., bits) with bit 0 of the last word's integer pattern set. blocks: n_blocks ids
 * (by * nbx + bx) of 32x32 image blocks. *built = 1 and masks[i] bit k set when a camera ray through block blocks[i],
 * grown by nh_primary_mask_pad pixels, can hit record k; *built = 0 (masks untouched) when the scene has more than 64
 * records or the camera a lens: nh_render then tests every record, as it does with NH_PRIMARY_MASKS=0. */
int nh_primary_masks(const nh_camera *camera, const float *records, int32_t n_records, const int32_t *blocks,
                     int32_t n_blocks, uint64_t *masks, int32_t *built);
int32_t nh_primary_mask_pad(int32_t width, int32_t height);

/* Candidate masks of the light sample's any-hit query (host/shadow_masks.cpp; host only). records, blocks: as for
 * nh_primary_masks. emit_faces: n_emit_faces emitter faces of 9 floats (three vertices) -- every face of every emitter
 * when all of them are area lights on meshes without vertex normals, else n_emit_faces = 0. *emitter_mask bit k clear:
 * no shadow ray (from an emitter face, leaving on its front side, no longer than the scene) can be accepted by record
 * k; all ones when nothing can be left out. *built = 1 and masks[i] bit k clear when no shadow ray ending at a first
 * hit of block blocks[i]'s camera rays can be accepted by record k (each word holds *emitter_mask's zeros as well);
 * *built = 0 (masks untouched) when nh_primary_masks builds no table. */
/* The emitter faces nh_shadow_masks takes, as nh_render forms them: *n_faces faces of 9 floats, 0 unless every emitter
 * of the scene is an area light on a mesh without vertex normals. faces has room for cap_faces of them. */
int nh_shadow_emitter_faces(const nh_scene_desc *scene, float *faces, int32_t cap_faces, int32_t *n_faces);
int nh_shadow_masks(const nh_camera *camera, const float *records, int32_t n_records, const float *emit_faces,
                    int32_t n_emit_faces, const int32_t *blocks, int32_t n_blocks, uint64_t *emitter_mask,
                    uint64_t *masks, int32_t *built);
/* The scene-wide any-hit word (host/shadow_masks.cpp; host only): *word bit k clear when no shadow ray of any bounce
 * can be accepted by record k -- *emitter_mask's zeros, and the supporting walls: triangle records with every emitter
 * vertex well in front of their plane and every hit point of the scene on that same side, which a shadow ray, ending
 * 1e-4 short of its far end, does not reach. The camera gives the longest ray that can hit a sphere. All ones when
 * nothing can be left out (as *emitter_mask). */
int nh_shadow_any_word(const nh_camera *camera, const float *records, int32_t n_records, const float *emit_faces,
                       int32_t n_emit_faces, uint64_t *word);

/* Which primitive records share a pair record of a small scene's LDS image (host/gpu_layout.cpp pair_layout; host
 * only). records: as for nh_primary_masks; leaves: n_leaves (start, count) ranges of records, disjoint. slots: 2 ints per
 * pair position, n_records positions -- (slot 0 record, slot 1 record or -1), (-1, -1) for an unused position.
 * leaf_pairs: 3 ints per leaf -- first pair position, triangle pairs, sphere pairs. by_kind != 0: a leaf's triangles
 * two by two, then its spheres two by two; 0: the reference arrangement, position p = records (p, p + 1), both counts 0. */
int nh_pair_layout(const float *records, int32_t n_records, const int32_t *leaves, int32_t n_leaves, int32_t by_kind,
                   int32_t *slots, int32_t *leaf_pairs);

/* The flat image of a scene the fused bounce kernels traverse without a tree walk (host/gpu_layout.cpp flat_image; host
 * only). records, leaves: as for nh_pair_layout, leaf 0 the root's left child and leaf 1 its right one (or the one leaf
 * of the tree). boxes: 18 floats -- the root's box (min xyz, max xyz), the left child's, the right child's. allowed: the
 * scene is staged in LDS with its pair records by kind. *n_f4 = 0: the scene is not flat (more than two leaves, more
 * than 16 pair records, allowed 0 or NH_FLAT_TRACE=0); else the image's float4 count, and image (image_cap_f4 float4s
 * of room) holds it: 6 header float4 (the three boxes, each leaf's triangle-pair and sphere-pair counts), then the pair
 * records, 6 float4 each, the left leaf's first. *box_equal: bit 0 / bit 1 -- the left / right child's box is bit-equal
 * to the root's. */
int nh_flat_image(const float *records, int32_t n_records, const int32_t *leaves, int32_t n_leaves, const float *boxes,
                  int32_t allowed, float *image, int32_t image_cap_f4, int32_t *n_f4, int32_t *box_equal);
/* nh_flat_image with the scene-wide any-hit word (nh_shadow_any_word; all ones: nh_flat_image's image). Unless every
 * record's bit is set (or NH_ANY_LIST=0) the image carries an any-hit section, which the light samples' any-hit
 * queries read instead of the pair records: bit 2 of header word [0].w is set, [3].w and [5].w hold the left and the
 * right leaf's any-hit counts (triangle pairs | sphere pairs << 16), and at float4 6 + 6 * 16 -- zeros in between --
 * follow pair records of each leaf's kept records, paired among themselves by nh_pair_layout's by-kind rules, the
 * left leaf's first. The image then has up to 6 + 6 * 32 float4. *box_equal is nh_flat_image's. */
int nh_flat_image_any(const float *records, int32_t n_records, const int32_t *leaves, int32_t n_leaves,
                      const float *boxes, int32_t allowed, uint64_t any_word, float *image, int32_t image_cap_f4,
                      int32_t *n_f4, int32_t *box_equal);

/* ImageBlock::toBitmap (src/utils/block.cpp:76-82): rgbw with border -> W*H*3 rgb */
int nh_framebuffer_to_rgb(const float *rgbw, int32_t width, int32_t height, int32_t border, float *rgb);
/* Bitmap::save equivalents: PFM (always available) and uncompressed OpenEXR */
int nh_write_pfm(const char *path, const float *rgb, int32_t width, int32_t height);
/* PNG decode as PNGTexture::loadFromFile's lodepng call (8-bit RGBA, row 0 first); rgba may be
   NULL (or cap too small) to query the size */
int nh_image_load_png(const char *path, uint8_t *rgba, size_t cap, int32_t *width, int32_t *height);
int nh_write_exr(const char *path, const float *rgb, int32_t width, int32_t height);
/* Bitmap::saveToLDR (src/utils/bitmap.cpp:122-140): sRGB gamma (GammaCorrect, :109-112), bytes
 * (uint8_t)Clamp(255 * v + 0.5, 0, 255) per channel, written as an 8-bit RGB PNG. nh_rgb_to_ldr
 * produces the bytes only (3 per pixel, row 0 first). */
int nh_rgb_to_ldr(const float *rgb, int32_t width, int32_t height, uint8_t *rgb8);
int nh_write_png(const char *path, const float *rgb, int32_t width, int32_t height);

/* device side */
int nh_get_device_count(int *n);
int nh_create(int device, nh_ctx **out);
void nh_destroy(nh_ctx *ctx);
int nh_upload_scene(nh_ctx *ctx, const nh_scene_desc *scene);
int nh_upload_bvh(nh_ctx *ctx, const nh_bvh_desc *bvh);
int nh_trace_rays(nh_ctx *ctx, const nh_ray_soa *rays, int32_t n, int32_t any_hit, int32_t traversal, nh_hit_soa *out);
/* A scene with the adaptive sampler (nh_scene_desc.sampler == NH_SAMPLER_ADAPTIVE) renders through the adaptive loop
 * (src/utils/render.cpp:323-336 in the reference's single-thread order): sample_begin..sample_end
 * count outer samples, every 4x4 block running passes of size.x * size.y paths until its variance test stops it; mode
 * and traversal change nothing visible. Refused: blocks != NULL, a range that neither starts at 0 nor continues the
 * previous call's (the blocks' index streams live across calls), a thin-lens camera, a filter wider than border 2,
 * sample_end beyond NH_ADAPTIVE_MAX_SAMPLES (the int32 path sample index (s * 1002 + pass) * 16 + i), and a render
 * whose staged block images (1 KiB per block and pass of one outer sample) exceed NH_ADAPTIVE_STAGING_BYTES
 * (NH_ADAPTIVE_STAGING_MB overrides it): the framebuffer then holds the outer samples before the refused one. */
#define NH_ADAPTIVE_MAX_SAMPLES 133948
#define NH_ADAPTIVE_STAGING_BYTES ((size_t)4 << 30)
int nh_render(nh_ctx *ctx, const nh_render_req *req);
/* Adaptive renders since the last range that started at 0 (render.cpp:373 "Total Samples Placed") */
typedef struct nh_adaptive_stats {
    uint64_t total_samples;       /* size.x * size.y per pass, summed */
    uint64_t passes;              /* passes summed over blocks and outer samples */
    uint64_t max_passes;          /* the most passes one block ran in one outer sample (at most 1001) */
    uint64_t n_blocks;            /* 4x4 blocks of the image */
} nh_adaptive_stats;
int nh_get_adaptive_stats(nh_ctx *ctx, nh_adaptive_stats *out);
/* m_oldVariance of every block at its place in the image (AdaptiveSampler::writeVarianceMatrix): width * height floats,
   row-major. The reference writes it through Color4f(v), whose weight is v itself, so its <scene>_variance.exr shows 1
   where this is non-zero. */
int nh_get_adaptive_variance(nh_ctx *ctx, float *out, size_t n_floats);
int nh_synchronize(nh_ctx *ctx);
int nh_get_framebuffer(nh_ctx *ctx, float *rgbw, size_t n_floats);
/* device pointer of the (W+2b)(H+2b)x4 fp32 framebuffer, for collectives issued by the caller;
   completes every submitted render first (the wavefront pipeline advances only inside library calls) */
int nh_framebuffer_device_ptr(nh_ctx *ctx, void **dptr, size_t *n_floats);
int nh_get_stats(nh_ctx *ctx, nh_render_stats *out);
int nh_reset_stats(nh_ctx *ctx);
/* single-process multi-GPU: RCCL sum of the framebuffers of n contexts into ctxs[root] (n = 1 included:
   a one-rank reduce). The communicator clique is created on the first call for a set of contexts and
   reused by later calls with the same contexts in the same order; it is destroyed with the contexts. */
int nh_reduce_framebuffers(nh_ctx **ctxs, int32_t n, int32_t root);
/* SimpleDenoiser::denoise (src/denoiser/simple.cpp:29-76) in place on the context's master ImageBlock (its
   interior W x H pixels; the border is left as is), after completing every submitted render. The pixels are
   updated in the row-major order of the reference's loops -- a pixel reads the already denoised values of
   the pixels before it and the previous pass's values of the others -- which is what the reference computes
   with one TBB thread (with more, its rows race). params->type must be NH_DENOISER_SIMPLE, the other fields
   within the constructor's clamps. Finite framebuffer values are assumed (ImageBlock::put drops the others). */
int nh_denoise(nh_ctx *ctx, const nh_denoiser *params);
/* the same on a caller's host ImageBlock: (width + 2 border) x (height + 2 border) x 4 floats, in place */
int nh_denoise_image(nh_ctx *ctx, float *rgbw, int32_t width, int32_t height, int32_t border,
                     const nh_denoiser *params);
/* BSDF queries on the device, by the bsdf_eval / bsdf_pdf / bsdf_sample device functions the render kernels call: the
 * GPU counterpart of the reference's chi2test / ttest BSDF hooks (src/utils/chi2test.cpp, ttest.cpp). One BSDF of
 * any NH_BSDF_* type, n queries in its local frame; `albedo` (3 floats, or NULL for bsdf->albedo) stands in for the
 * albedo texture's value at the query's uv, and bsdf->albedo_texture != 0 makes a Disney BSDF form its colour terms
 * per query from it (the textured route) instead of once (the constant-albedo route).
 *   NH_BSDF_QUERY_EVAL    in: wi, wo (3n floats each). out: value = eval(wi, wo) (3n), pdf = pdf(wi, wo) (n), both in
 *                         the solid-angle measure; wo_out / measure may be NULL
 *   NH_BSDF_QUERY_SAMPLE  in: wi (3n), sample (2n). out: wo_out (3n), value = the sample's weight (3n), measure (n:
 *                         0 unknown, 1 solid angle, 2 discrete), pdf = pdf(wi, wo_out) in that measure (n)
 * Needs no uploaded scene. */
enum { NH_BSDF_QUERY_EVAL = 0, NH_BSDF_QUERY_SAMPLE = 1 };
int nh_bsdf_query(nh_ctx *ctx, const nh_bsdf *bsdf, const float *albedo, int32_t mode, int32_t n, const float *wi,
                  const float *wo, const float *sample, float *wo_out, float *value, float *pdf, int32_t *measure);
/* Emitter queries on the device, by the emitter_sample / emitter_eval / emitter_pdf device functions the render
 * kernels call: emitter `emitter` (any NH_EMITTER_* type) of the uploaded scene, n queries, one lane each.
 *   NH_EMITTER_QUERY_SAMPLE  in: ref (3n), sample (2n floats). out: NH_EMITTER_QUERY_SAMPLE_STRIDE floats per query:
 *                            [0..2] the sample's weight (value / pdf), [3..5] wi, [6] pdf(ref, p, n, wi),
 *                            [7..9] shadow ray origin, [10..12] its direction, [13] mint, [14] maxt, [15] 0
 *   NH_EMITTER_QUERY_EVAL    in: ref (3n), sample = NH_EMITTER_QUERY_IN_STRIDE floats per query: [0..2] wi,
 *   NH_EMITTER_QUERY_PDF         [3..5] the point p on the light, [6..8] its normal n (p and n are read for area
 *                                lights only). out: 3 floats per query (eval's value), 1 float per query (pdf)
 * Needs an uploaded scene (nh_upload_scene; no BVH). */
enum { NH_EMITTER_QUERY_SAMPLE = 0, NH_EMITTER_QUERY_EVAL = 1, NH_EMITTER_QUERY_PDF = 2,
       /* Emitter::samplePhoton of an area light (arealight.cpp:127-144), by the device function the photon pass calls.
          in: sample = 4n floats (sample1.x, sample1.y, sample2.x, sample2.y); ref is not read (may be NULL). out:
          NH_EMITTER_QUERY_PHOTON_STRIDE floats per query: [0..2] the ray's origin, [3..5] its direction, [6..8] W =
          M_PI / pdf * radiance * the number of emitters (photonmapper.cpp:91), [9] the surface pdf, [10..11] 0.
          NH_ERR_UNSUPPORTED for an emitter that is not an area light. */
       NH_EMITTER_QUERY_SAMPLE_PHOTON = 3 };
#define NH_EMITTER_QUERY_SAMPLE_STRIDE 16
#define NH_EMITTER_QUERY_PHOTON_STRIDE 12
#define NH_EMITTER_QUERY_IN_STRIDE 9
int nh_emitter_query(nh_ctx *ctx, uint32_t emitter, int32_t mode, int32_t n, const float *ref, const float *sample,
                     float *out);
/* Medium queries on the device, by the device functions the volumetric path kernel calls (nh_volume.hip): medium
 * `medium` of the uploaded scene, n queries, one lane each.
 *   NH_MEDIUM_QUERY_FREE_PATH      in: 2n floats (the two uniforms sampleFreePath may draw, in draw order).
 *                                  out: 2n floats: t, and the number of draws it consumed (0, 1 or 2)
 *   NH_MEDIUM_QUERY_TRANSMITTANCE  in: 6n floats (from, to). out: 3n floats
 *   NH_MEDIUM_QUERY_PHASE_SAMPLE   in: 2n floats (the 2D sample). out: 4n floats: wo (local frame, wi = +z), pdf(wo)
 *   NH_MEDIUM_QUERY_PHASE_PDF      in: 3n floats (wo). out: n floats
 * Needs an uploaded scene (nh_upload_scene; no BVH). */
enum { NH_MEDIUM_QUERY_FREE_PATH = 0, NH_MEDIUM_QUERY_TRANSMITTANCE = 1, NH_MEDIUM_QUERY_PHASE_SAMPLE = 2,
       NH_MEDIUM_QUERY_PHASE_PDF = 3 };
int nh_medium_query(nh_ctx *ctx, uint32_t medium, int32_t mode, int32_t n, const float *in, float *out);

/* ---- the reference's t-test procedure (src/utils/ttest.cpp) and the per-path radiance query ----------------- */

/* A <test> root: StudentsTTest ("ttest") or ChiSquareTest ("chi2test"). The constructor's properties with their
 * defaults, the `angles` / `references` lists tokenised as ttest.cpp:62-79 (an absent list is the one value 0, as
 * there: toFloat reads the empty token as 0), the number of <scene> children (each
 * loads through nh_scene_load_xml_index) and the <bsdf> children. nh_test_load_xml fails (NH_ERR_IO, the reference's
 * own message in nh_host_last_error) where StudentsTTest's addChild or execute() throw, and with NH_ERR_INVALID on
 * a file whose root is not a <test>. The pointers live as long as the nh_test. */
enum { NH_TEST_TTEST = 0, NH_TEST_CHI2TEST = 1 };
typedef struct nh_test_desc {
    int32_t type;                 /* NH_TEST_* */
    float significance_level;     /* significanceLevel [0.01] */
    int32_t sample_count;         /* sampleCount [ttest: 100000; chi2test: -1] */
    uint32_t n_angles;
    const float *angles;
    uint32_t n_references;
    const float *references;
    uint32_t n_scenes;
    uint32_t n_bsdfs;
    const nh_bsdf *bsdfs;
} nh_test_desc;
typedef struct nh_test nh_test;
int nh_test_load_xml(const char *path, nh_test **out);
int nh_test_get_desc(const nh_test *test, nh_test_desc *out);
void nh_test_free(nh_test *test);

/* hypothesis::students_t_test (ext/hypothesis/hypothesis.h:314-346): t = |mean - reference| sqrt(n / max(variance,
 * 1e-5)), the two-sided p-value of Student's t with n - 1 degrees of freedom, the Sidak-corrected level
 * 1 - (1 - alpha)^(1 / num_tests); *accepted = 0 when p < level or p is not finite. p_value may be NULL.
 * NH_ERR_INVALID for n < 2 or num_tests < 1. Host only. */
int nh_students_t_test(double mean, double variance, double reference, int32_t n, double alpha, int32_t num_tests,
                       int32_t *accepted, double *p_value);

/* One path's radiance, by the device functions the render kernels call: entry i is sample sample[i] of pixel
 * pixel[i] (y * width + x) under `seed` -- the per-path stream path_rng(seed, pixel, sample), two jitter draws, the two
 * unused aperture draws, the camera ray through (x + jx, y + jy) or through (pixel_sample[2i], pixel_sample[2i + 1])
 * when pixel_sample is given (the draws are made all the same), a thin-lens camera's lens sample of (pixel, sample) as
 * in a render, then the Li of the uploaded scene's integrator. rgb (3n) is that radiance as it is: no NaN / negative
 * filtering (ImageBlock::put's job). jitter (2n, may be NULL): (jx, jy). The scene's sampler type is not read.
 * Closest hits go nearer child first. n <= 2^24; NH_ERR_INVALID for a pixel outside [0, width * height) or a negative
 * sample. Needs an uploaded scene and BVH. */
#define NH_RADIANCE_QUERY_MAX (1 << 24)
int nh_radiance_query(nh_ctx *ctx, uint64_t seed, int32_t n, const int32_t *pixel, const int32_t *sample,
                      const float *pixel_sample, float *rgb, float *jitter);
/* StudentsTTest's scene branch (ttest.cpp:210-230) over samples k = first .. first + n - 1, each on its own stream
 * path_rng(seed, 0, k): pixelSample = (a * (float)width, b * (float)height) from its first two draws, the two aperture
 * draws, Li, Color3f::getLuminance in fp32 widened to double; mean and unbiased variance (n >= 2) reduced on the
 * device in fp64, in an order that depends on n alone. luminance (n floats, may be NULL): every sample's. The
 * reference draws all samples from one sequential stream; per-sample streams are this library's contract.
 * A thin-lens camera is refused (NH_ERR_UNSUPPORTED). Needs an uploaded scene and BVH. */
int nh_ttest_scene(nh_ctx *ctx, uint64_t seed, int64_t first, int32_t n, double *mean, double *variance,
                   float *luminance);
/* StudentsTTest's BSDF branch (ttest.cpp:167-181): wi = sphericalDirection(degToRad(angle_deg), 0); sample k takes
 * draws first_draw + 2k and first_draw + 2k + 1 of the default-state pcg32 (the reference's own stream: the test's
 * j-th run of n samples starts at first_draw = 2 n j) and contributes the luminance of bsdf_sample's weight. albedo
 * (3 floats, or NULL for bsdf->albedo) as in nh_bsdf_query. Needs no uploaded scene. */
int nh_ttest_bsdf(nh_ctx *ctx, const nh_bsdf *bsdf, const float *albedo, float angle_deg, uint64_t first_draw,
                  int32_t n, double *mean, double *variance, float *luminance);
/* StudentsTTest::execute on device `device`: every <scene> of the file loaded, built, uploaded and run through
 * nh_ttest_scene with the file's sampleCount (scene tests), or every <bsdf> x angle through nh_ttest_bsdf with
 * first_draw running on across the tests (BSDF tests), then nh_students_t_test with num_tests = the number of
 * references. Writes min(*n_results, cap) results. A chi2test file returns NH_ERR_UNSUPPORTED here: nh_chi2_run
 * (below) is its entry point. Errors are reported through nh_host_last_error. */
typedef struct nh_test_result {
    double mean, variance, reference, p_value;
    int32_t accepted;
    int32_t sample_count;
    float angle;                  /* BSDF tests: the incidence angle (degrees) */
    int32_t pad;
} nh_test_result;
int nh_test_run(int device, const char *path, uint64_t seed, nh_test_result *results, int32_t cap,
                int32_t *n_results);

/* ---- the reference's chi^2 test procedure (src/utils/chi2test.cpp) --------------------- */

/* ChiSquareTest's constructor properties (chi2test.cpp:45-74), beside nh_test_desc: resolution [10] (the cos(theta)
 * cells; phi takes twice as many), minExpFrequency [5], testCount [5] and sampleCount resolved (-1, or any negative
 * value: resolution * 2 resolution * 5000; nh_test_desc keeps the file's own value). NH_ERR_INVALID for a ttest. */
typedef struct nh_chi2_params {
    int32_t resolution;
    int32_t min_exp_frequency;
    int32_t test_count;
    int32_t sample_count;
} nh_chi2_params;
int nh_test_get_chi2_params(const nh_test *test, nh_chi2_params *out);

/* largest contingency table of nh_chi2_histogram: one uint32 per cell in 32 KB of LDS */
#define NH_CHI2_MAX_CELLS 8192
/* largest n_wi * cells of one nh_chi2_expected call */
#define NH_CHI2_EXPECTED_MAX (1 << 20)
/* ChiSquareTest's sampling loop (chi2test.cpp:163-181) on the device: sample k takes draws first_draw + 2k (x) and
 * first_draw + 2k + 1 (y) of the default-state pcg32, as nh_ttest_bsdf does; a sample whose weight is all zero is
 * skipped; the others count into cell cosThetaBin * res_phi + phiBin, the bins formed in fp32 as the reference writes
 * them. obs: res_theta * res_phi doubles (the reference's obsFrequencies), whole counts, the same bits on every run
 * (integer atomics only). wi: the incident direction in the BSDF's frame; albedo as in nh_bsdf_query.
 * 1 <= n <= INT32_MAX. NH_ERR_UNSUPPORTED for a resolution below 1 or more than NH_CHI2_MAX_CELLS cells. Needs no
 * uploaded scene. */
int nh_chi2_histogram(nh_ctx *ctx, const nh_bsdf *bsdf, const float *albedo, const float *wi, uint64_t first_draw,
                      int32_t n, int32_t res_theta, int32_t res_phi, double *obs);
/* The expected frequencies (chi2test.cpp:186-214) of n_wi incident directions (wi: 3 n_wi floats) in one launch: per
 * (wi, cell) hypothesis::adaptiveSimpson2D (eps 1e-6, depth 6) of the device's bsdf_pdf in the solid-angle measure
 * over the cell's cos(theta) x phi rectangle -- the phi bounds evaluated in fp32 as the reference's float M_PI makes
 * them -- times (double)sample_count. exp: n_wi * cells doubles; evals (n_wi * cells, may be NULL): the pdf
 * evaluations each cell took. The integrator is csrc/nh_simpson.h, the recursion's own summation order. */
int nh_chi2_expected(nh_ctx *ctx, const nh_bsdf *bsdf, const float *albedo, int32_t n_wi, const float *wi,
                     int32_t res_theta, int32_t res_phi, int32_t sample_count, double *exp, uint32_t *evals);
/* hypothesis::chi2_test (ext/hypothesis/hypothesis.h:140-235): the cells sorted by expected frequency (ties by cell
 * index: a stable order, where std::sort's is unspecified), pooled as its two pooling branches say, Pearson's
 * statistic, dof - 1, p = 1 - chi2_cdf, the Sidak-corrected level; *accepted = 0 when p < level or p is not finite.
 * *kind tells the rejections apart; on NH_CHI2_REJECTED_ZERO_CELL *statistic is the observed count of the offending
 * cell and *p_value NaN, on NH_CHI2_REJECTED_DOF *p_value is NaN. Every out pointer but accepted may be NULL.
 * NH_ERR_INVALID for n_cells < 1 or num_tests < 1. Host only. */
enum { NH_CHI2_ACCEPTED = 0, NH_CHI2_REJECTED_P_VALUE = 1, NH_CHI2_REJECTED_ZERO_CELL = 2, NH_CHI2_REJECTED_DOF = 3 };
int nh_chi2_test(int32_t n_cells, const double *obs, const double *exp, int32_t sample_count,
                 double min_exp_frequency, double alpha, int32_t num_tests, int32_t *accepted, double *p_value,
                 double *statistic, int32_t *dof, int32_t *pooled_cells, int32_t *kind);
/* ChiSquareTest::execute (chi2test.cpp:131-234) on device `device`: one default-state pcg32 runs through the file;
 * test T (over <bsdf> x testCount) draws cosTheta and phi of its wi at draws T (2 + 2n), + 1 and its n samples from
 * draw T (2 + 2n) + 2 (nh_chi2_histogram); the expected frequencies of every test come from one nh_chi2_expected
 * launch per <bsdf>; nh_chi2_test with num_tests = testCount * the number of <bsdf>. Writes min(*n_results, cap)
 * results. tables (may be NULL): per written result 2 * cells doubles, the observed then the expected frequencies.
 * A ttest file returns NH_ERR_INVALID, a textured <bsdf> NH_ERR_UNSUPPORTED. Errors through nh_host_last_error. */
typedef struct nh_chi2_result {
    double statistic;             /* chi^2 (NH_CHI2_REJECTED_ZERO_CELL: the offending cell's observed count) */
    double p_value, level;        /* level: the Sidak-corrected significance level */
    double obs_sum, exp_sum;      /* sums of the two tables, in cell order */
    float wi[3];
    int32_t dof, pooled_cells;
    int32_t accepted, kind;       /* kind: NH_CHI2_* */
    int32_t sample_count;
} nh_chi2_result;
int nh_chi2_run(int device, const char *path, nh_chi2_result *results, int32_t cap, int32_t *n_results);
int nh_chi2_run_tables(int device, const char *path, nh_chi2_result *results, int32_t cap, int32_t *n_results,
                       double *tables);

/* ---- the reference's warp test (src/utils/warptest.cpp, runTest) ------------------------ */

/* WarpTest::WarpType (warptest.cpp:67-81), in its order. NH_WARP_SCHLICK exists only to be refused by name
 * (NH_ERR_UNSUPPORTED): squareToSchlick leaves [-1, 1], and the reference then bins a NaN through an (int) cast, which
 * is undefined -- the reason the loader gives for the phase function. */
enum { NH_WARP_NONE = 0, NH_WARP_DISK, NH_WARP_UNIFORM_SPHERE, NH_WARP_UNIFORM_SPHERE_VOL, NH_WARP_UNIFORM_SPHERE_CAP,
       NH_WARP_UNIFORM_HEMISPHERE, NH_WARP_COSINE_HEMISPHERE, NH_WARP_BECKMANN, NH_WARP_HENYEY_GREENSTEIN,
       NH_WARP_SCHLICK, NH_WARP_MICROFACET_BRDF, NH_WARP_ISO_PHASE, NH_WARP_ANISO_PHASE };
/* mapParameter (warptest.cpp:88-100) in fp32 as written: the parameter slider's value in [0, 1] becomes alpha =
 * exp(log(0.05) (1 - s) + log(1) s) for Beckmann and the microfacet BRDF, g = 2 s - 1 for Henyey-Greenstein and the
 * anisotropic phase function, and stays as it is for the rest (the sphere cap takes it as cosThetaMax). Host only. */
int nh_warp_map_parameter(int32_t type, float slider, float *value);
/* The incident direction of the BRDF and the phase functions from the angle slider (warptest.cpp:183-184):
 * (sin a, 0, max(cos a, 1e-4)).normalized() with a = M_PI (s - 0.5). Host only. */
int nh_warp_wi(float angle_slider, float wi[3]);
/* Every entry point below takes the type, the mapped parameter (finite) and wi (3 floats; read for
 * NH_WARP_MICROFACET_BRDF only, may be NULL otherwise). The microfacet BRDF is microfacet.cpp's with alpha =
 * parameter, kd = 0 (so ks = 1) and its default intIOR / extIOR, run through the bsdf_sample / bsdf_eval / bsdf_pdf
 * device functions; the phases through phase_sample / phase_pdf. None needs an uploaded scene.
 *
 * nh_warp_query, one lane per query:
 *   NH_WARP_QUERY_SAMPLE  in: 3n floats, the Point3f sample (only the sphere volume reads z). out: 4n floats, the
 *                         warped point and warpPoint's weight (warptest.cpp:102-131): 1, or for the microfacet BRDF
 *                         value == 0 ? 0 : eval[0]
 *   NH_WARP_QUERY_PDF     in: 3n floats, the point (None and Disk use x, y only). out: n floats, the matching *Pdf in
 *                         fp32; the BRDF's pdf in the solid-angle measure */
enum { NH_WARP_QUERY_SAMPLE = 0, NH_WARP_QUERY_PDF = 1 };
int nh_warp_query(nh_ctx *ctx, int32_t type, float parameter, const float *wi, int32_t mode, int32_t n,
                  const float *in, float *out);
/* generatePoints(Independent) and runTest's binning loop (warptest.cpp:146-168, :457-479). Point k takes three
 * consecutive draws of the default-state pcg32 from draw first_draw + 3k. Point3f(nextFloat(), nextFloat(),
 * nextFloat()) leaves the order of its arguments to the compiler: draw_order NH_LENS_DRAWS_RTL (g++: x = draw 3k + 2,
 * z = draw 3k) or NH_LENS_DRAWS_LTR (x = draw 3k). A point of weight 0 is skipped. A point with a NaN coordinate is not
 * counted either -- the reference's (int) cast is undefined there -- but tallied in *nan_points (may be NULL). The rest
 * are binned in fp32 as written: None by (x, y), Disk by 0.5 p + 0.5, everything else by atan2(y, x) * INV_TWOPI
 * wrapped into [0, 1) and 0.5 z + 0.5 of the point as it is (sphere-volume points are not normalized); every bin is
 * min(res - 1, max(0, floor(v res))). obs: yres * xres doubles, row ybin, whole counts, the same bits on every run.
 * 1 <= n <= INT32_MAX (NH_ERR_INVALID); xres, yres >= 1 and xres * yres <= NH_CHI2_MAX_CELLS (NH_ERR_UNSUPPORTED). */
int nh_warp_histogram(nh_ctx *ctx, int32_t type, float parameter, const float *wi, uint64_t first_draw,
                      int32_t draw_order, int32_t n, int32_t xres, int32_t yres, double *obs, uint32_t *nan_points);
/* runTest's expected frequencies (warptest.cpp:481-551): per cell hypothesis::adaptiveSimpson2D (eps 1e-6, depth 6;
 * csrc/nh_simpson.h) of the integrand as written -- yStart = y / (double)yres, yEnd = (y + 1 - Epsilon) / (double)yres,
 * likewise for x, the direction built in fp64 with the reference's float M_PI and narrowed to fp32, the pdf in fp32 --
 * times sample_count x 1 (None), 4 (Disk) or 4 * M_PI. exp: yres * xres doubles; evals (may be NULL): the pdf
 * evaluations each cell took. A negative cell returns NH_ERR_INVALID with the reference's message "The Pdf() function
 * returned negative values!". Resolution limits as nh_warp_histogram's. */
int nh_warp_expected(nh_ctx *ctx, int32_t type, float parameter, const float *wi, int32_t xres, int32_t yres,
                     int32_t sample_count, double *exp, uint32_t *evals);
/* runTest (warptest.cpp:439-562) on device `device`: nh_warp_map_parameter, nh_warp_wi, the two tables from draw 0,
 * then nh_chi2_test with minExpFrequency 5, significance level 0.01 and one test. xres = yres = sample_count = 0
 * selects the reference's own values: 51 x 51 cells, xres doubled except for None and Disk, 1000 samples per cell.
 * result->wi is zero where the type has no incident direction. tables (may be NULL): yres * xres observed then as
 * many expected frequencies. Errors through nh_host_last_error. */
int nh_warp_run(int device, int32_t type, float parameter_slider, float angle_slider, int32_t draw_order, int32_t xres,
                int32_t yres, int32_t sample_count, nh_chi2_result *result, double *tables);

/* ---- the photon mapper (src/integrators/photonmapper.cpp) ------------------------------- */

/* Photon path k draws from its own stream path_rng(seed, NH_PHOTON_STREAM, k): no pixel index reaches 2^32. */
#define NH_PHOTON_STREAM ((uint64_t)1 << 32)
/* paths of one launch of the photon pass when batch_paths = 0 */
#define NH_PHOTON_DEFAULT_BATCH (1 << 18)
/* PhotonMapper::preprocess on the uploaded scene and BVH: photon paths 0, 1, .. are traced (photonmapper.cpp:86-149)
 * and deposit (its.p, -d, W) at every hit of a diffuse or Disney BSDF. The map holds the first photon_count deposits
 * in (path, bounce) order; the emitted count E is the number of paths up to and including the one that fills it.
 * Neither depends on batch_paths (paths per launch, 0 = NH_PHOTON_DEFAULT_BATCH) nor on anything else about how the
 * pass is launched. params->photon_radius = 0 resolves as nh_scene_get_photon_params does, from the uploaded BVH's
 * root box. The map lives in the context until the next build or scene / BVH upload; nh_render, nh_radiance_query
 * and nh_ttest_scene of a photon-mapper scene return NH_ERR_STATE without one. NH_ERR_UNSUPPORTED: the scene's
 * integrator is not the photon mapper, an emitter is not an area light, the first 2^16 paths deposit nothing ("no
 * photon reaches a diffuse surface": the reference would loop forever), or E would pass INT32_MAX. */
int nh_photon_map_build(nh_ctx *ctx, const nh_photon_params *params, uint64_t seed, int32_t batch_paths);
typedef struct nh_photon_stats {
    int32_t stored;               /* photons in the map (= photon_count) */
    int32_t emitted;              /* E, m_emittedPhotons */
    float radius;                 /* the resolved gather radius */
    float cell_size;              /* side of a cell of the search grid (>= radius) */
    uint64_t occupied_cells;      /* grid cells that hold a photon */
} nh_photon_stats;
int nh_get_photon_stats(nh_ctx *ctx, nh_photon_stats *out);
/* Photons first .. first + n - 1 in deposit order ((path, bounce) ascending). Every output may be NULL: position (3n
 * floats), direction and power as the gather reads them, i.e. decoded from the stored bytes through PhotonData's
 * tables (3n each), bytes (6n: theta, phi, rgbe[0..3]), path index and bounce (n each). */
int nh_get_photons(nh_ctx *ctx, int32_t first, int32_t n, float *position, float *direction, float *power,
                   uint8_t *bytes, int32_t *path, int32_t *bounce);
/* Point queries by the device functions the photon pass and the gather call.
 *   NH_PHOTON_QUERY_CODEC   in: 6n floats (direction, power). bytes: 6n (theta, phi, rgbe[0..3] of PhotonData's
 *                           constructor, photon.cpp:43-74); out: 6n floats (getDirection, getPower of those bytes).
 *                           count is not written. Needs no scene.
 *   NH_PHOTON_QUERY_GATHER  in: 3n floats (points). count: n (photons with (photon.p - p).squaredNorm() < r * r in
 *                           fp32); out: 3n floats (the fp32 sum of their decoded powers, added in ascending (cell key,
 *                           deposit index) order, the order of the render's gather). bytes is not written. Needs a map. */
enum { NH_PHOTON_QUERY_CODEC = 0, NH_PHOTON_QUERY_GATHER = 1 };
int nh_photon_query(nh_ctx *ctx, int32_t mode, int32_t n, const float *in, uint8_t *bytes, int32_t *count, float *out);

/* ---- the av integrator (src/integrators/av.cpp) ------------------------------------------ */

/* The occlusion ray's length of an NH_INTEGRATOR_AV scene, which nh_scene_desc does not carry. Called after
 * nh_upload_scene (every scene upload forgets it); nh_render, nh_radiance_query and nh_ttest_scene of an av scene
 * return NH_ERR_STATE until it has been. NH_ERR_INVALID: a NaN length. */
int nh_set_av_params(nh_ctx *ctx, const nh_av_params *params);

const char *nh_last_error(const nh_ctx *ctx);

#ifdef __cplusplus
}
#endif
#endif /* NORI_HIP_H */
