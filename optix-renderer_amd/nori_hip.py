"""Python binding of the nori_hip C-ABI (include/nori_hip.h) via ctypes.

This is the host-side mirror of the reference's render entry points for tests and the
benchmark: `Scene` ~ loadFromXML + Scene::cloneAndInit/update
(src/utils/parser.cpp:28-378, src/utils/scene.cpp:59-202), `Bvh` ~ BVH::build
(src/utils/bvh.cpp:327-380), `Context.render` ~ RenderThread::renderThreadMain over a
sample range (src/utils/render.cpp:232-459), `Context.trace` ~ Scene::rayIntersect
(include/nori/scene.h:114-137).

The library is the in-tree build optix-renderer_amd/lib/libnori_hip.so. There is no
fallback: if it is missing, importing raises.
"""
from __future__ import annotations

import ctypes as C
import os

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
# NH_LIB_PATH: an alternative in-tree build, for A/B measurements in one GPU session
LIB_PATH = os.environ.get("NH_LIB_PATH") or os.path.join(_HERE, "lib", "libnori_hip.so")

from nh_env import raise_hw_queues  # noqa: E402  (nori_hip's own directory is on sys.path)

if not os.path.exists(LIB_PATH):
    raise ImportError(f"nori_hip: HIP library not built ({LIB_PATH}); run `make` or __graft_entry__.build()")
_lib = C.CDLL(LIB_PATH)

NH_OK = 0
SHAPE_MESH, SHAPE_SPHERE = 0, 1
BSDF_DIFFUSE, BSDF_MIRROR, BSDF_DIELECTRIC, BSDF_MICROFACET = 0, 1, 2, 3
BSDF_DISNEY = 4  # disney.cpp
BSDF_QUERY_EVAL, BSDF_QUERY_SAMPLE = 0, 1
EMITTER_AREA, EMITTER_POINT, EMITTER_ENVMAP = 0, 1, 2
EMITTER_SPOT, EMITTER_DIRECTIONAL = 3, 4  # spotlight.cpp, directionalLight.cpp
EMITTER_QUERY_SAMPLE, EMITTER_QUERY_EVAL, EMITTER_QUERY_PDF = 0, 1, 2
EMITTER_QUERY_SAMPLE_STRIDE, EMITTER_QUERY_IN_STRIDE = 16, 9
INTEGRATOR_PATH_MIS, INTEGRATOR_PATH_MATS, INTEGRATOR_DIRECT_EMS, INTEGRATOR_DIRECT_MATS, INTEGRATOR_DIRECT_MIS = 0, 1, 2, 3, 4
INTEGRATOR_DIRECT = 5  # the point-light `direct` integrator of scenes/pa1 (direct.cpp)
INTEGRATOR_NORMALS = 6  # the `normals` integrator of the normal-map scenes (normals.cpp)
# the volumetric path tracers (path_vol_mats.cpp, path_vol_mis.cpp): the integrators that render participating media
INTEGRATOR_PATH_VOL_MATS, INTEGRATOR_PATH_VOL_MIS = 7, 8
MEDIUM_VACUUM, MEDIUM_HOMOG = 0, 1  # vacuum.cpp, homogmedium.cpp
PHASE_ISO, PHASE_HG = 0, 1  # isophase.cpp, anisophase.cpp (Henyey-Greenstein)
MEDIUM_QUERY_FREE_PATH, MEDIUM_QUERY_TRANSMITTANCE, MEDIUM_QUERY_PHASE_SAMPLE, MEDIUM_QUERY_PHASE_PDF = 0, 1, 2, 3
MODE_MEGAKERNEL, MODE_WAVEFRONT = 0, 1
SMALL_TABLES_BYTES = 4096  # NH_SMALL_TABLES_BYTES: LDS budget of the scene tables of the diffuse area-light kernels
TRAVERSAL_REFERENCE, TRAVERSAL_ORDERED, TRAVERSAL_WIDE = 0, 1, 2
DENOISER_NONE, DENOISER_SIMPLE = 0, 1
SAMPLER_INDEPENDENT, SAMPLER_ADAPTIVE = 0, 1  # independent.cpp, adaptive.cpp
ADAPTIVE_MAX_SAMPLES = 133948  # NH_ADAPTIVE_MAX_SAMPLES
LENS_DRAWS_LTR, LENS_DRAWS_RTL = 0, 1

_f = C.c_float
_i32 = C.c_int32
_u32 = C.c_uint32
_fp = C.POINTER(C.c_float)
_u32p = C.POINTER(C.c_uint32)


class nh_shape(C.Structure):
    _fields_ = [("type", _i32), ("bsdf", _i32), ("emitter", _i32), ("v_offset", _u32), ("n_vertices", _u32),
                ("f_offset", _u32), ("n_faces", _u32), ("has_normals", _i32), ("has_uvs", _i32),
                ("center", _f * 3), ("radius", _f), ("bbox_min", _f * 3), ("bbox_max", _f * 3),
                ("pdf_offset", _u32), ("pdf_normalization", _f), ("normal_map", _u32)]


# nh_bsdf's Disney parameters in the struct's order, with the defaults of disney.cpp:32-41
DISNEY_PARAMS = ("metallic", "subsurface", "specular", "roughness", "specular_tint", "anisotropic", "sheen",
                 "sheen_tint", "clearcoat", "clearcoat_gloss")
DISNEY_DEFAULTS = dict(zip(DISNEY_PARAMS, (0.0, 0.0, 0.5, 0.5, 0.0, 0.0, 0.0, 0.5, 0.0, 1.0)))


class nh_bsdf(C.Structure):
    _fields_ = [("type", _i32), ("albedo", _f * 3), ("alpha", _f), ("int_ior", _f), ("ext_ior", _f),
                ("kd", _f * 3), ("ks", _f), ("albedo_texture", _u32)] + [(n, _f) for n in DISNEY_PARAMS]


TEXTURE_CONSTANT, TEXTURE_CHECKERBOARD, TEXTURE_PNG = 0, 1, 2


class nh_texture(C.Structure):
    _fields_ = [("type", _i32), ("value1", _f * 3), ("value2", _f * 3), ("delta", _f * 2), ("scale", _f * 2),
                ("width", _i32), ("height", _i32), ("texel_offset", C.c_uint64), ("scale_u", _f), ("scale_v", _f),
                ("offset_u", _f), ("offset_v", _f), ("spherical", _i32), ("rotation", _f * 9), ("linear", _i32),
                ("intensity", _f), ("pad", _i32)]


class nh_emitter(C.Structure):
    _fields_ = [("type", _i32), ("shape", _i32), ("radiance", _f * 3), ("light_prob", _f),
                ("position", _f * 3), ("pad", _f)]


class nh_emitter_ext(C.Structure):
    _fields_ = [("direction", _f * 3), ("cos_total_width", _f), ("frame_s", _f * 3), ("cos_falloff_start", _f),
                ("frame_t", _f * 3), ("cos_theta_max", _f), ("frame_n", _f * 3), ("pad", _f)]


class nh_medium(C.Structure):
    _fields_ = [("type", _i32), ("mu_a", _f * 3), ("mu_s", _f * 3), ("mu_t", _f * 3), ("density", _f),
                ("phase", _i32), ("g", _f)]


class nh_camera(C.Structure):
    _fields_ = [("width", _i32), ("height", _i32), ("sample_to_camera", _f * 16), ("camera_to_world", _f * 16),
                ("inv_output_size", _f * 2), ("near_clip", _f), ("far_clip", _f), ("lens_radius", _f),
                ("focal_distance", _f), ("lens_draw_order", _i32)]


class nh_filter(C.Structure):
    _fields_ = [("radius", _f), ("border", _i32), ("lookup_factor", _f), ("table", _f * 33)]


class nh_envmap(C.Structure):
    _fields_ = [("width", _i32), ("height", _i32), ("rgba", _fp), ("radiance", _f * 3), ("scale_u", _f),
                ("scale_v", _f), ("offset_u", _f), ("offset_v", _f), ("spherical", _i32), ("constant", _i32),
                ("cdf", _fp), ("normalization", _f), ("rotation", _f * 9)]


class nh_denoiser(C.Structure):
    _fields_ = [("type", _i32), ("sigma_d", _f), ("sigma_vr", _f), ("range", _i32), ("amount", _i32)]


def simple_denoiser(sigma_d: float = 0.0, sigma_vr: float = 0.6, range: int = 1, amount: int = 1) -> nh_denoiser:
    """SimpleDenoiser's parameters with its constructor's defaults and clamps (src/denoiser/simple.cpp:15-24,
    Nori's clamp and Epsilon = 1e-4f)."""
    eps = np.float32(1e-4)

    def clampf(v, lo, hi):
        v = np.float32(v)
        return float(lo if v < lo else (hi if v > hi else v))
    d = nh_denoiser()
    d.type = DENOISER_SIMPLE
    d.sigma_d = clampf(sigma_d, eps, np.float32(10))
    d.sigma_vr = clampf(sigma_vr, eps, np.float32(10))
    d.range = int(min(max(range, 0), 50))
    d.amount = int(min(max(amount, 1), 10))
    return d


class nh_scene_desc(C.Structure):
    _fields_ = [("camera", nh_camera), ("filter", nh_filter), ("integrator", _i32), ("sample_count", _i32),
                ("n_shapes", _u32), ("shapes", C.POINTER(nh_shape)), ("n_bsdfs", _u32),
                ("bsdfs", C.POINTER(nh_bsdf)), ("n_emitters", _u32), ("emitters", C.POINTER(nh_emitter)),
                ("emitter_cdf", _fp), ("envmap", _i32), ("n_vertices", _u32), ("V", _fp), ("N", _fp),
                ("UV", _fp), ("T", _fp), ("BT", _fp), ("n_faces", _u32), ("F", _u32p), ("n_area_cdf", _u32),
                ("area_cdf", _fp), ("env", nh_envmap), ("denoiser", nh_denoiser), ("n_textures", _u32),
                ("textures", C.POINTER(nh_texture)), ("n_texels", C.c_uint64), ("texels", _fp),
                ("normals_direction", _f * 3), ("emitter_ext", C.POINTER(nh_emitter_ext)),
                ("n_media", _u32), ("media", C.POINTER(nh_medium)), ("shape_medium", _u32p),
                ("ambient_medium", _u32), ("sampler", _i32), ("adaptive_initial_uniform", _i32)]


class nh_bvh_node(C.Structure):
    _fields_ = [("word0", _u32), ("word1", _u32), ("bbox_min", _f * 3), ("bbox_max", _f * 3)]


class nh_bvh_desc(C.Structure):
    _fields_ = [("n_nodes", _u32), ("nodes", C.POINTER(nh_bvh_node)), ("n_indices", _u32), ("indices", _u32p),
                ("n_shapes", _u32), ("shape_offset", _u32p), ("bbox_min", _f * 3), ("bbox_max", _f * 3),
                ("max_depth", _u32)]


class nh_ray_soa(C.Structure):
    _fields_ = [(n, _fp) for n in ("ox", "oy", "oz", "dx", "dy", "dz", "mint", "maxt")]


class nh_hit_soa(C.Structure):
    _fields_ = [("hit", C.POINTER(C.c_uint8)), ("t", _fp), ("u", _fp), ("v", _fp), ("prim", _u32p),
                ("shape", _u32p)]


class nh_render_req(C.Structure):
    _fields_ = [("sample_begin", _i32), ("sample_end", _i32), ("seed", C.c_uint64), ("n_blocks", _i32),
                ("blocks", C.POINTER(_i32)), ("mode", _i32), ("traversal", _i32), ("clear", _i32),
                ("collect_stats", _i32)]


class nh_adaptive_stats(C.Structure):
    _fields_ = [("total_samples", C.c_uint64), ("passes", C.c_uint64), ("max_passes", C.c_uint64),
                ("n_blocks", C.c_uint64)]


class nh_render_stats(C.Structure):
    _fields_ = [("kernel_ms_path", C.c_double), ("kernel_ms_splat", C.c_double), ("kernel_ms_extend", C.c_double),
                ("kernel_ms_shadow", C.c_double), ("kernel_ms_shade", C.c_double), ("launches_path", C.c_uint64),
                ("launches_splat", C.c_uint64), ("launches_extend", C.c_uint64), ("launches_shadow", C.c_uint64),
                ("launches_shade", C.c_uint64), ("samples", C.c_uint64), ("ray_queries", C.c_uint64),
                ("nodes_visited", C.c_uint64), ("boxes_tested", C.c_uint64), ("prims_tested", C.c_uint64),
                ("invalid_samples", C.c_uint64), ("shadow_queries", C.c_uint64),
                ("shadow_nodes_visited", C.c_uint64), ("shadow_boxes_tested", C.c_uint64),
                ("shadow_prims_tested", C.c_uint64), ("shade_state_bytes", C.c_uint64),
                ("extend_queue_bytes", C.c_uint64), ("shadow_queue_bytes", C.c_uint64),
                ("paths_shaded", C.c_uint64), ("kernel_ms_tail", C.c_double), ("launches_tail", C.c_uint64),
                ("node_bytes", C.c_uint64)] + [
        (n, C.c_uint64) for n in ("tail_queries", "tail_nodes_visited", "tail_boxes_tested", "tail_prims_tested",
                                  "tail_shadow_queries", "tail_shadow_nodes_visited", "tail_shadow_boxes_tested",
                                  "tail_shadow_prims_tested", "lds_scene", "fused_bounce", "comm_inits")] + [
        ("kernel_ms_denoise", C.c_double), ("launches_denoise", C.c_uint64), ("tails_async", C.c_uint64),
        ("pools_active", C.c_uint64), ("trace_fused", C.c_uint64)] + [
        (n, C.c_uint64) for n in ("tail_cycles_body", "tail_cycles_shadow", "tail_cycles_closest", "tail_cycles_head",
                                  "tail_bounces", "tail_max_bounces", "tail_coop_cycles_body",
                                  "tail_coop_cycles_shadow", "tail_coop_cycles_closest", "tail_coop_cycles_head",
                                  "tail_coop_bounces", "bounce_cycles_load", "bounce_cycles_body",
                                  "bounce_cycles_shadow", "bounce_cycles_closest", "bounce_cycles_head",
                                  "bounce_cycles_store", "bounce_bounces", "bounce_traits", "primary_masks",
                                  "pair_kinds", "flat_trace", "shadow_masks", "any_list")]


def _sig(name, res, *args):
    fn = getattr(_lib, name)
    fn.restype = res
    fn.argtypes = list(args)
    return fn


_vp = C.c_void_p
_sig("nh_scene_load_xml", _i32, C.c_char_p, C.POINTER(_vp))
_sig("nh_scene_load_xml_index", _i32, C.c_char_p, _i32, C.POINTER(_vp))
_sig("nh_scene_get_desc", _i32, _vp, C.POINTER(nh_scene_desc))
_sig("nh_scene_set_resolution", _i32, _vp, _i32, _i32)
_sig("nh_scene_set_sample_count", _i32, _vp, _i32)
_sig("nh_scene_set_sampler", _i32, _vp, _i32, _i32)
_sig("nh_scene_set_bsdf", _i32, _vp, _u32, C.POINTER(nh_bsdf))
_sig("nh_scene_set_integrator", _i32, _vp, _i32)
_sig("nh_scene_add_texture", _u32, _vp, C.POINTER(nh_texture), _fp)
_sig("nh_scene_set_normal_map", _i32, _vp, _u32, _u32)
_sig("nh_scene_set_lens_draw_order", _i32, _vp, _i32)
_sig("nh_texture_decode", _i32, C.POINTER(C.c_uint8), C.c_uint64, _i32, _fp)
_sig("nh_scene_free", None, _vp)
_sig("nh_host_last_error", C.c_char_p)
_sig("nh_debug_transform", _i32, C.c_char_p, _fp, _i32)
_sig("nh_bvh_build", _i32, C.POINTER(nh_scene_desc), _i32, C.POINTER(_vp))
_sig("nh_bvh_get_desc", _i32, _vp, C.POINTER(nh_bvh_desc))
_sig("nh_bvh_free", None, _vp)
_sig("nh_primary_masks", _i32, C.POINTER(nh_camera), _fp, _i32, C.POINTER(_i32), _i32, C.POINTER(C.c_uint64),
     C.POINTER(_i32))
_sig("nh_primary_mask_pad", _i32, _i32, _i32)
_sig("nh_shadow_emitter_faces", _i32, C.POINTER(nh_scene_desc), _fp, _i32, C.POINTER(_i32))
_sig("nh_shadow_masks", _i32, C.POINTER(nh_camera), _fp, _i32, _fp, _i32, C.POINTER(_i32), _i32, C.POINTER(C.c_uint64),
     C.POINTER(C.c_uint64), C.POINTER(_i32))
_sig("nh_pair_layout", _i32, _fp, _i32, C.POINTER(_i32), _i32, _i32, C.POINTER(_i32), C.POINTER(_i32))
_sig("nh_flat_image", _i32, _fp, _i32, C.POINTER(_i32), _i32, _fp, _i32, _fp, _i32, C.POINTER(_i32), C.POINTER(_i32))
_sig("nh_shadow_any_word", _i32, C.POINTER(nh_camera), _fp, _i32, _fp, _i32, C.POINTER(C.c_uint64))
_sig("nh_flat_image_any", _i32, _fp, _i32, C.POINTER(_i32), _i32, _fp, _i32, C.c_uint64, _fp, _i32, C.POINTER(_i32),
     C.POINTER(_i32))
_sig("nh_framebuffer_to_rgb", _i32, _fp, _i32, _i32, _i32, _fp)
_sig("nh_write_pfm", _i32, C.c_char_p, _fp, _i32, _i32)
_sig("nh_image_load_png", _i32, C.c_char_p, C.POINTER(C.c_uint8), C.c_size_t, C.POINTER(_i32), C.POINTER(_i32))
_sig("nh_write_exr", _i32, C.c_char_p, _fp, _i32, _i32)
_sig("nh_write_png", _i32, C.c_char_p, _fp, _i32, _i32)
_sig("nh_rgb_to_ldr", _i32, _fp, _i32, _i32, C.POINTER(C.c_uint8))
_sig("nh_get_device_count", _i32, C.POINTER(C.c_int))
_sig("nh_create", _i32, C.c_int, C.POINTER(_vp))
_sig("nh_destroy", None, _vp)
_sig("nh_upload_scene", _i32, _vp, C.POINTER(nh_scene_desc))
_sig("nh_upload_bvh", _i32, _vp, C.POINTER(nh_bvh_desc))
_sig("nh_trace_rays", _i32, _vp, C.POINTER(nh_ray_soa), _i32, _i32, _i32, C.POINTER(nh_hit_soa))
_sig("nh_render", _i32, _vp, C.POINTER(nh_render_req))
_sig("nh_synchronize", _i32, _vp)
_sig("nh_get_framebuffer", _i32, _vp, _fp, C.c_size_t)
_sig("nh_framebuffer_device_ptr", _i32, _vp, C.POINTER(_vp), C.POINTER(C.c_size_t))
_sig("nh_get_stats", _i32, _vp, C.POINTER(nh_render_stats))
_sig("nh_reset_stats", _i32, _vp)
_sig("nh_get_adaptive_stats", _i32, _vp, C.POINTER(nh_adaptive_stats))
_sig("nh_get_adaptive_variance", _i32, _vp, _fp, C.c_size_t)
_sig("nh_reduce_framebuffers", _i32, C.POINTER(_vp), _i32, _i32)
_sig("nh_denoise", _i32, _vp, C.POINTER(nh_denoiser))
_sig("nh_denoise_image", _i32, _vp, _fp, _i32, _i32, _i32, C.POINTER(nh_denoiser))
_sig("nh_bsdf_query", _i32, _vp, C.POINTER(nh_bsdf), _fp, _i32, _i32, _fp, _fp, _fp, _fp, _fp, _fp, C.POINTER(_i32))
_sig("nh_emitter_query", _i32, _vp, _u32, _i32, _i32, _fp, _fp, _fp)
_sig("nh_medium_query", _i32, _vp, _u32, _i32, _i32, _fp, _fp)
_sig("nh_last_error", C.c_char_p, _vp)


class nh_test_desc(C.Structure):
    _fields_ = [("type", _i32), ("significance_level", _f), ("sample_count", _i32), ("n_angles", _u32),
                ("angles", _fp), ("n_references", _u32), ("references", _fp), ("n_scenes", _u32), ("n_bsdfs", _u32),
                ("bsdfs", C.POINTER(nh_bsdf))]


class nh_test_result(C.Structure):
    _fields_ = [("mean", C.c_double), ("variance", C.c_double), ("reference", C.c_double), ("p_value", C.c_double),
                ("accepted", _i32), ("sample_count", _i32), ("angle", _f), ("pad", _i32)]


TEST_TTEST, TEST_CHI2TEST = 0, 1
RADIANCE_QUERY_MAX = 1 << 24  # NH_RADIANCE_QUERY_MAX
_dp = C.POINTER(C.c_double)
_i32p = C.POINTER(_i32)
_sig("nh_test_load_xml", _i32, C.c_char_p, C.POINTER(_vp))
_sig("nh_test_get_desc", _i32, _vp, C.POINTER(nh_test_desc))
_sig("nh_test_free", None, _vp)
_sig("nh_students_t_test", _i32, C.c_double, C.c_double, C.c_double, _i32, C.c_double, _i32, _i32p, _dp)
_sig("nh_radiance_query", _i32, _vp, C.c_uint64, _i32, _i32p, _i32p, _fp, _fp, _fp)
_sig("nh_ttest_scene", _i32, _vp, C.c_uint64, C.c_int64, _i32, _dp, _dp, _fp)
_sig("nh_ttest_bsdf", _i32, _vp, C.POINTER(nh_bsdf), _fp, _f, C.c_uint64, _i32, _dp, _dp, _fp)
_sig("nh_test_run", _i32, C.c_int, C.c_char_p, C.c_uint64, C.POINTER(nh_test_result), _i32, _i32p)


# ---- the chi^2 test (chi2test.cpp) ----
class nh_chi2_params(C.Structure):
    _fields_ = [("resolution", _i32), ("min_exp_frequency", _i32), ("test_count", _i32), ("sample_count", _i32)]


class nh_chi2_result(C.Structure):
    _fields_ = [("statistic", C.c_double), ("p_value", C.c_double), ("level", C.c_double), ("obs_sum", C.c_double),
                ("exp_sum", C.c_double), ("wi", _f * 3), ("dof", _i32), ("pooled_cells", _i32), ("accepted", _i32),
                ("kind", _i32), ("sample_count", _i32)]


CHI2_MAX_CELLS = 8192  # NH_CHI2_MAX_CELLS
CHI2_ACCEPTED, CHI2_REJECTED_P_VALUE, CHI2_REJECTED_ZERO_CELL, CHI2_REJECTED_DOF = 0, 1, 2, 3
CHI2_KINDS = ("accepted", "p-value", "expected frequency 0", "degrees of freedom")
_sig("nh_test_get_chi2_params", _i32, _vp, C.POINTER(nh_chi2_params))
_sig("nh_chi2_histogram", _i32, _vp, C.POINTER(nh_bsdf), _fp, _fp, C.c_uint64, _i32, _i32, _i32, _dp)
_sig("nh_chi2_expected", _i32, _vp, C.POINTER(nh_bsdf), _fp, _i32, _fp, _i32, _i32, _i32, _dp, _u32p)
_sig("nh_chi2_test", _i32, _i32, _dp, _dp, _i32, C.c_double, C.c_double, _i32, _i32p, _dp, _dp, _i32p, _i32p, _i32p)
_sig("nh_chi2_run", _i32, C.c_int, C.c_char_p, C.POINTER(nh_chi2_result), _i32, _i32p)
_sig("nh_chi2_run_tables", _i32, C.c_int, C.c_char_p, C.POINTER(nh_chi2_result), _i32, _i32p, _dp)

# ---- the warp test (warptest.cpp's runTest) ----
(WARP_NONE, WARP_DISK, WARP_UNIFORM_SPHERE, WARP_UNIFORM_SPHERE_VOL, WARP_UNIFORM_SPHERE_CAP, WARP_UNIFORM_HEMISPHERE,
 WARP_COSINE_HEMISPHERE, WARP_BECKMANN, WARP_HENYEY_GREENSTEIN, WARP_SCHLICK, WARP_MICROFACET_BRDF, WARP_ISO_PHASE,
 WARP_ANISO_PHASE) = range(13)
# the names the CLI's --warptest takes, by type
WARP_NAMES = ("none", "disk", "sphere", "spherevol", "spherecap", "hemisphere", "cosinehemisphere", "beckmann",
              "henyeygreenstein", "schlick", "microfacet", "isophase", "anisophase")
WARP_SUPPORTED = tuple(t for t in range(13) if t != WARP_SCHLICK)
WARP_QUERY_SAMPLE, WARP_QUERY_PDF = 0, 1
_sig("nh_warp_map_parameter", _i32, _i32, _f, _fp)
_sig("nh_warp_wi", _i32, _f, _fp)
_sig("nh_warp_query", _i32, _vp, _i32, _f, _fp, _i32, _i32, _fp, _fp)
_sig("nh_warp_histogram", _i32, _vp, _i32, _f, _fp, C.c_uint64, _i32, _i32, _i32, _i32, _dp, _u32p)
_sig("nh_warp_expected", _i32, _vp, _i32, _f, _fp, _i32, _i32, _i32, _dp, _u32p)
_sig("nh_warp_run", _i32, C.c_int, _i32, _f, _f, _i32, _i32, _i32, _i32, C.POINTER(nh_chi2_result), _dp)


# ---- the photon mapper (photonmapper.cpp) ----
INTEGRATOR_PHOTONMAPPER = 9
EMITTER_QUERY_SAMPLE_PHOTON, EMITTER_QUERY_PHOTON_STRIDE = 3, 12
PHOTON_QUERY_CODEC, PHOTON_QUERY_GATHER = 0, 1
PHOTON_STREAM = 1 << 32          # NH_PHOTON_STREAM: photon path k draws from path_rng(seed, PHOTON_STREAM, k)
PHOTON_DEFAULT_BATCH = 1 << 18   # NH_PHOTON_DEFAULT_BATCH


class nh_photon_params(C.Structure):
    _fields_ = [("photon_count", _i32), ("photon_radius", _f)]


class nh_photon_stats(C.Structure):
    _fields_ = [("stored", _i32), ("emitted", _i32), ("radius", _f), ("cell_size", _f),
                ("occupied_cells", C.c_uint64)]


_u8p = C.POINTER(C.c_uint8)
_sig("nh_scene_get_photon_params", _i32, _vp, C.POINTER(nh_photon_params))
_sig("nh_scene_set_photon_params", _i32, _vp, C.POINTER(nh_photon_params))
_sig("nh_photon_tables", _i32, _fp, _fp, _fp, _fp, _fp)
_sig("nh_photon_map_build", _i32, _vp, C.POINTER(nh_photon_params), C.c_uint64, _i32)
_sig("nh_get_photon_stats", _i32, _vp, C.POINTER(nh_photon_stats))
_sig("nh_get_photons", _i32, _vp, _i32, _i32, _fp, _fp, _fp, _u8p, _i32p, _i32p)
_sig("nh_photon_query", _i32, _vp, _i32, _i32, _fp, _u8p, _i32p, _fp)


# ---- the av and envmaptester integrators (av.cpp, EnvMapTester.cpp) ----
INTEGRATOR_AV, INTEGRATOR_ENVMAPTESTER = 10, 11


class nh_av_params(C.Structure):
    _fields_ = [("length", _f)]


_sig("nh_scene_get_av_params", _i32, _vp, C.POINTER(nh_av_params))
_sig("nh_scene_set_av_params", _i32, _vp, C.POINTER(nh_av_params))
_sig("nh_set_av_params", _i32, _vp, C.POINTER(nh_av_params))


def photon_tables() -> dict:
    """nh_photon_tables: PhotonData's five 256-entry decode tables (photon.cpp:30-41), float32."""
    t = {k: np.zeros(256, np.float32) for k in ("cos_theta", "sin_theta", "cos_phi", "sin_phi", "exp")}
    _host_check(_lib.nh_photon_tables(*[_fptr(t[k]) for k in ("cos_theta", "sin_theta", "cos_phi", "sin_phi", "exp")]),
                "photon_tables")
    return t


lib = _lib
_hip_used = False  # set by the first call that initialises the HIP runtime (device_count, Context)


def configure_runtime(min_hw_queues: int = 8) -> int:
    """Process settings the HIP runtime reads once, when it initialises: GPU_MAX_HW_QUEUES raised to min_hw_queues
    (one hardware queue per path-pool stream, nh_env.py) unless a larger value is set or NH_KEEP_HW_QUEUES keeps the
    caller's. An explicit call, not an import side effect; it must come before the first device_count() / Context().
    Returns the value the runtime will see."""
    if _hip_used:
        raise RuntimeError("configure_runtime: the HIP runtime is already initialised in this process")
    return raise_hw_queues(min_hw_queues)


class NoriError(RuntimeError):
    pass


def _fptr(a):
    return a.ctypes.data_as(_fp)


def _host_check(rc, what):
    if rc != NH_OK:
        raise NoriError(f"{what}: {_lib.nh_host_last_error().decode()}")


class Scene:
    """A loaded Nori XML scene (host-owned flattened arrays)."""

    def __init__(self, path: str, index: int = 0):
        h = _vp()
        _host_check(_lib.nh_scene_load_xml_index(path.encode(), index, C.byref(h)), f"load {path}")
        self._h = h
        self.path = path

    def __del__(self):
        if getattr(self, "_h", None):
            _lib.nh_scene_free(self._h)
            self._h = None

    @property
    def desc(self) -> nh_scene_desc:
        d = nh_scene_desc()
        _host_check(_lib.nh_scene_get_desc(self._h, C.byref(d)), "get_desc")
        return d

    def set_resolution(self, w: int, h: int):
        _host_check(_lib.nh_scene_set_resolution(self._h, w, h), "set_resolution")

    def set_sample_count(self, spp: int):
        _host_check(_lib.nh_scene_set_sample_count(self._h, spp), "set_sample_count")

    def set_sampler(self, type: int, initial_uniform: int = 2):
        """SAMPLER_INDEPENDENT, or SAMPLER_ADAPTIVE with its initialUniform (clamped to [1, sampleCount] as
        AdaptiveSampler's constructor does: set the sample count first)."""
        _host_check(_lib.nh_scene_set_sampler(self._h, type, initial_uniform), "set_sampler")

    def set_integrator(self, integ: int):
        _host_check(_lib.nh_scene_set_integrator(self._h, integ), "set_integrator")

    def photon_params(self) -> tuple:
        """nh_scene_get_photon_params: (photonCount, photonRadius) of the scene's photon mapper, the radius resolved
        (0 = automatic becomes the scene box's diagonal / 500, photonmapper.cpp:75-76)."""
        p = nh_photon_params()
        _host_check(_lib.nh_scene_get_photon_params(self._h, C.byref(p)), "get_photon_params")
        return int(p.photon_count), float(np.float32(p.photon_radius))

    def av_params(self) -> float:
        """nh_scene_get_av_params: `length` of the scene's av integrator (0 on a scene with another integrator)."""
        p = nh_av_params()
        _host_check(_lib.nh_scene_get_av_params(self._h, C.byref(p)), "get_av_params")
        return float(np.float32(p.length))

    def set_av_params(self, length: float):
        """nh_scene_set_av_params: override the av integrator's `length`."""
        p = nh_av_params(length)
        _host_check(_lib.nh_scene_set_av_params(self._h, C.byref(p)), "set_av_params")

    def set_photon_params(self, photon_count: int, photon_radius: float = 0.0):
        """nh_scene_set_photon_params: override photonCount and photonRadius (0 = automatic)."""
        p = nh_photon_params(photon_count, photon_radius)
        _host_check(_lib.nh_scene_set_photon_params(self._h, C.byref(p)), "set_photon_params")

    def set_bsdf(self, shape: int, **kw):
        b = nh_bsdf()
        b.type = kw.get("type", BSDF_DIFFUSE)
        for i, v in enumerate(kw.get("albedo", (0.5, 0.5, 0.5))):
            b.albedo[i] = v
        b.alpha = kw.get("alpha", 0.1)
        b.int_ior = kw.get("int_ior", 1.5046)
        b.ext_ior = kw.get("ext_ior", 1.000277)
        kd = kw.get("kd", (0.5, 0.5, 0.5))
        for i, v in enumerate(kd):
            b.kd[i] = v
        kdf = np.asarray(kd, dtype=np.float32)
        m = kdf[1] if not (kdf[1] < kdf[2]) else kdf[2]
        m = kdf[0] if not (kdf[0] < m) else m
        b.ks = float(np.float32(1) - np.float32(m))
        b.albedo_texture = kw.get("albedo_texture", 0)
        for n in DISNEY_PARAMS:  # as Disney's constructor: its default, clamped to [0, 1]
            setattr(b, n, min(max(float(kw.get(n, DISNEY_DEFAULTS[n])), 0.0), 1.0))
        _host_check(_lib.nh_scene_set_bsdf(self._h, shape, C.byref(b)), "set_bsdf")

    def add_texture(self, type: int, value1=(0, 0, 0), value2=(1, 1, 1), delta=(0, 0), scale=(1, 1), texels=None,
                    scale_uv=(1, 1), offset_uv=(0, 0), spherical=False, linear=False, intensity=1.0) -> int:
        """Append a texture (nh_scene_add_texture); returns the value naming it in nh_bsdf.albedo_texture or
        nh_shape.normal_map (set_normal_map). texels: (H, W, 4) float32 RGBA for TEXTURE_PNG, already decoded
        (texture_decode), row 0 first; linear: sRGB = false (normal-map texels, eval blends by intensity)."""
        t = nh_texture()
        t.type = type
        t.linear = int(linear)
        t.intensity = intensity
        for i in range(3):
            t.value1[i], t.value2[i] = value1[i], value2[i]
        t.delta[0], t.delta[1] = delta
        t.scale[0], t.scale[1] = scale
        t.scale_u, t.scale_v = scale_uv
        t.offset_u, t.offset_v = offset_uv
        t.spherical = int(spherical)
        for i in range(9):
            t.rotation[i] = 1.0 if i % 4 == 0 else 0.0
        ptr = None
        if texels is not None:
            tx = np.ascontiguousarray(texels, dtype=np.float32)
            t.height, t.width = tx.shape[0], tx.shape[1]
            ptr = _fptr(tx)
        idx = _lib.nh_scene_add_texture(self._h, C.byref(t), ptr)
        if idx == 0:
            raise NoriError(f"add_texture: {_lib.nh_host_last_error().decode()}")
        return idx

    def media(self) -> list:
        """The scene's media as dicts (type, mu_a, mu_s, mu_t, density, phase, g), in nh_scene_desc.media order."""
        d = self.desc
        return [{"type": m.type, "mu_a": np.array(m.mu_a[:], np.float32), "mu_s": np.array(m.mu_s[:], np.float32),
                 "mu_t": np.array(m.mu_t[:], np.float32), "density": np.float32(m.density), "phase": m.phase,
                 "g": np.float32(m.g)} for m in (d.media[i] for i in range(d.n_media))]

    def shape_media(self) -> list:
        """Per shape: the index of its medium in media(), or -1 (nh_scene_desc.shape_medium, minus one)."""
        d = self.desc
        return [int(d.shape_medium[i]) - 1 if d.shape_medium else -1 for i in range(d.n_shapes)]

    @property
    def ambient_medium(self) -> int:
        """The index of the scene's ambient medium in media(), or -1 for the default vacuum."""
        return int(self.desc.ambient_medium) - 1

    def set_lens_draw_order(self, order: int):
        """LENS_DRAWS_RTL (default, g++'s evaluation of Point2f(nextFloat(), nextFloat())) or LENS_DRAWS_LTR."""
        _host_check(_lib.nh_scene_set_lens_draw_order(self._h, order), "set_lens_draw_order")

    def set_normal_map(self, shape: int, texture: int):
        """Shape::addChild(<texture name="normal">): texture = an add_texture value, 0 removes the map."""
        _host_check(_lib.nh_scene_set_normal_map(self._h, shape, texture), "set_normal_map")

    @property
    def width(self):
        return self.desc.camera.width

    @property
    def height(self):
        return self.desc.camera.height

    @property
    def border(self):
        return self.desc.filter.border

    @property
    def spp(self):
        """the sampler's sampleCount"""
        return self.desc.sample_count

    def framebuffer_shape(self):
        d = self.desc
        b = d.filter.border
        return (d.camera.height + 2 * b, d.camera.width + 2 * b, 4)


class Test:
    """A loaded <test> root (nh_test_load_xml): StudentsTTest's or ChiSquareTest's properties and children. Loading
    raises NoriError with the reference's own message where StudentsTTest's addChild or execute() throw."""
    __test__ = False  # (not a pytest class)

    def __init__(self, path: str):
        h = _vp()
        _host_check(_lib.nh_test_load_xml(path.encode(), C.byref(h)), f"load {path}")
        self._h = h
        self.path = path
        d = nh_test_desc()
        _host_check(_lib.nh_test_get_desc(h, C.byref(d)), "test_get_desc")
        self.type = "chi2test" if d.type == TEST_CHI2TEST else "ttest"
        self.significance_level = np.float32(d.significance_level)
        self.sample_count = int(d.sample_count)
        self.angles = [np.float32(d.angles[i]) for i in range(d.n_angles)]
        self.references = [np.float32(d.references[i]) for i in range(d.n_references)]
        self.n_scenes = int(d.n_scenes)
        self.bsdfs = []
        for i in range(d.n_bsdfs):  # copies: the handle owns the originals
            b = nh_bsdf()
            C.memmove(C.byref(b), C.byref(d.bsdfs[i]), C.sizeof(nh_bsdf))
            self.bsdfs.append(b)
        # ChiSquareTest's own properties (nh_test_get_chi2_params; None on a ttest). sample_count stays the file's
        # value (-1: automatic); chi2_sample_count is the resolved one
        self.resolution = self.min_exp_frequency = self.test_count = self.chi2_sample_count = None
        if d.type == TEST_CHI2TEST:
            cp = nh_chi2_params()
            _host_check(_lib.nh_test_get_chi2_params(h, C.byref(cp)), "test_get_chi2_params")
            self.resolution, self.min_exp_frequency = int(cp.resolution), int(cp.min_exp_frequency)
            self.test_count, self.chi2_sample_count = int(cp.test_count), int(cp.sample_count)

    def __del__(self):
        if getattr(self, "_h", None):
            _lib.nh_test_free(self._h)
            self._h = None


def students_t_test(mean: float, variance: float, reference: float, n: int, alpha: float, num_tests: int):
    """hypothesis::students_t_test (nh_students_t_test): (accepted, two-sided p-value) at the Sidak-corrected level."""
    ok, p = _i32(0), C.c_double(0.0)
    _host_check(_lib.nh_students_t_test(mean, variance, reference, n, alpha, num_tests, C.byref(ok), C.byref(p)),
                "students_t_test")
    return bool(ok.value), p.value


def chi2_test(obs, exp, sample_count: int, min_exp_frequency: float, alpha: float, num_tests: int) -> dict:
    """hypothesis::chi2_test (nh_chi2_test): accepted, p_value, statistic, dof, pooled_cells and kind (CHI2_*) at the
    Sidak-corrected level. On CHI2_REJECTED_ZERO_CELL statistic is the offending cell's observed count."""
    obs = np.ascontiguousarray(obs, dtype=np.float64).ravel()
    exp = np.ascontiguousarray(exp, dtype=np.float64).ravel()
    if len(obs) != len(exp):
        raise ValueError("chi2_test: obs and exp differ in length")
    ok, dof, pooled, kind = _i32(0), _i32(0), _i32(0), _i32(0)
    p, stat = C.c_double(0.0), C.c_double(0.0)
    _host_check(_lib.nh_chi2_test(len(obs), obs.ctypes.data_as(_dp), exp.ctypes.data_as(_dp), sample_count,
                                  min_exp_frequency, alpha, num_tests, C.byref(ok), C.byref(p), C.byref(stat),
                                  C.byref(dof), C.byref(pooled), C.byref(kind)), "chi2_test")
    return {"accepted": bool(ok.value), "p_value": p.value, "statistic": stat.value, "dof": dof.value,
            "pooled_cells": pooled.value, "kind": kind.value}


def run_chi2_tests(path: str, device: int = 0, tables: bool = True) -> list:
    """ChiSquareTest::execute on the HIP path (nh_chi2_run): one dict per test of the file (<bsdf> x testCount) -- wi,
    statistic, dof, pooled_cells, p_value, level, accepted, kind (CHI2_*), sample_count, obs_sum, exp_sum and, with
    tables, obs and exp (cells float64 each, cell = cosThetaBin * 2 resolution + phiBin)."""
    global _hip_used
    _hip_used = True
    t = Test(path)
    if t.type != "chi2test":
        cap, cells = 1, 1  # (nh_chi2_run refuses the file itself)
    else:
        cap = max(1, len(t.bsdfs) * max(t.test_count, 0))
        cells = max(1, min(2 * t.resolution * t.resolution, CHI2_MAX_CELLS))
    n = _i32(0)
    res = (nh_chi2_result * cap)()
    tab = np.zeros((cap, 2, cells), np.float64) if tables else None
    _host_check(_lib.nh_chi2_run_tables(device, path.encode(), res, cap, C.byref(n),
                                        None if tab is None else tab.ctypes.data_as(_dp)), f"run_chi2_tests {path}")
    out = []
    for i, r in enumerate(res[:n.value]):
        d = {"wi": np.array(r.wi[:], np.float32), "statistic": r.statistic, "dof": r.dof,
             "pooled_cells": r.pooled_cells, "p_value": r.p_value, "level": r.level, "accepted": bool(r.accepted),
             "kind": r.kind, "sample_count": r.sample_count, "obs_sum": r.obs_sum, "exp_sum": r.exp_sum}
        if tables:
            d["obs"], d["exp"] = tab[i, 0].copy(), tab[i, 1].copy()
        out.append(d)
    return out


def warp_map_parameter(type: int, slider: float) -> float:
    """mapParameter (warptest.cpp:88-100, nh_warp_map_parameter): the parameter slider's value as the warp takes it."""
    v = _f(0.0)
    _host_check(_lib.nh_warp_map_parameter(type, slider, C.byref(v)), "warp_map_parameter")
    return float(v.value)


def warp_wi(angle_slider: float) -> np.ndarray:
    """The incident direction the angle slider stands for (warptest.cpp:183-184, nh_warp_wi)."""
    wi = np.zeros(3, np.float32)
    _host_check(_lib.nh_warp_wi(angle_slider, _fptr(wi)), "warp_wi")
    return wi


def warp_default_table(type: int):
    """runTest's own (yres, xres, sample_count) (warptest.cpp:440-447)."""
    yres, xres = 51, 51 if type in (WARP_NONE, WARP_DISK) else 102
    return yres, xres, 1000 * yres * xres


def run_warp_test(type: int, parameter_slider: float = 0.5, angle_slider: float = 0.5, draw_order: int = LENS_DRAWS_RTL,
                  xres: int = 0, yres: int = 0, sample_count: int = 0, device: int = 0, tables: bool = True) -> dict:
    """WarpTest::runTest on the HIP path (nh_warp_run): wi, statistic, dof, pooled_cells, p_value, level, accepted,
    kind (CHI2_*), sample_count, obs_sum, exp_sum, xres, yres and, with tables, obs and exp (yres * xres float64 each,
    cell = ybin * xres + xbin). xres = yres = sample_count = 0: the reference's own table (warp_default_table)."""
    global _hip_used
    _hip_used = True
    if xres == 0 and yres == 0 and sample_count == 0:
        ty, tx, _ = warp_default_table(type)
    else:
        ty, tx = yres, xres
    cells = max(1, min(max(tx, 0) * max(ty, 0), CHI2_MAX_CELLS))
    r = nh_chi2_result()
    tab = np.zeros((2, cells), np.float64) if tables else None
    _host_check(_lib.nh_warp_run(device, type, parameter_slider, angle_slider, draw_order, xres, yres, sample_count,
                                 C.byref(r), None if tab is None else tab.ctypes.data_as(_dp)), "run_warp_test")
    d = {"wi": np.array(r.wi[:], np.float32), "statistic": r.statistic, "dof": r.dof, "pooled_cells": r.pooled_cells,
         "p_value": r.p_value, "level": r.level, "accepted": bool(r.accepted), "kind": r.kind,
         "sample_count": r.sample_count, "obs_sum": r.obs_sum, "exp_sum": r.exp_sum, "xres": tx, "yres": ty}
    if tables:
        d["obs"], d["exp"] = tab[0].copy(), tab[1].copy()
    return d


def run_tests(path: str, seed: int = 0, device: int = 0) -> list:
    """StudentsTTest::execute on the HIP path (nh_test_run): one dict per test of the file -- mean, variance,
    reference, p_value, accepted, sample_count, angle (BSDF tests)."""
    global _hip_used
    _hip_used = True
    t = Test(path)
    cap = max(1, t.n_scenes + len(t.bsdfs) * len(t.references))
    n = _i32(0)
    res = (nh_test_result * cap)()
    _host_check(_lib.nh_test_run(device, path.encode(), seed, res, cap, C.byref(n)), f"run_tests {path}")
    return [{"mean": r.mean, "variance": r.variance, "reference": r.reference, "p_value": r.p_value,
             "accepted": bool(r.accepted), "sample_count": r.sample_count, "angle": r.angle} for r in res[:n.value]]


def texture_decode(rgba8, srgb: bool) -> np.ndarray:
    """PNGTexture::loadFromFile's byte -> float loop (nh_texture_decode): sRGB or the normal-map decode."""
    b = np.ascontiguousarray(rgba8, dtype=np.uint8).ravel()
    out = np.empty(b.size, dtype=np.float32)
    _host_check(_lib.nh_texture_decode(b.ctypes.data_as(C.POINTER(C.c_uint8)), b.size, int(srgb), _fptr(out)),
                "texture_decode")
    return out


class Bvh:
    def __init__(self, scene: Scene, n_threads: int = 0):
        self._scene = scene
        d = scene.desc
        h = _vp()
        _host_check(_lib.nh_bvh_build(C.byref(d), n_threads, C.byref(h)), "bvh_build")
        self._h = h

    def __del__(self):
        if getattr(self, "_h", None):
            _lib.nh_bvh_free(self._h)
            self._h = None

    @property
    def desc(self) -> nh_bvh_desc:
        d = nh_bvh_desc()
        _host_check(_lib.nh_bvh_get_desc(self._h, C.byref(d)), "bvh_get_desc")
        return d

    def nodes(self) -> np.ndarray:
        d = self.desc
        raw = np.ctypeslib.as_array(C.cast(d.nodes, C.POINTER(C.c_uint32)), shape=(d.n_nodes * 8,))
        return raw.reshape(d.n_nodes, 8).copy()

    def indices(self) -> np.ndarray:
        d = self.desc
        return np.ctypeslib.as_array(d.indices, shape=(d.n_indices,)).copy()


def debug_transform(request: str) -> np.ndarray:
    """The loader's transform arithmetic on one request of oracle/eigen_xform_probe.cpp's protocol
    (parity hook, include/nori_hip.h nh_debug_transform): float32 results."""
    out = np.zeros(64, np.float32)
    n = _lib.nh_debug_transform(request.encode(), _fptr(out), out.size)
    if n < 0:
        raise NoriError(f"debug_transform: {_lib.nh_host_last_error().decode()}")
    return out[:n].copy()


def device_count() -> int:
    global _hip_used
    _hip_used = True
    n = C.c_int(0)
    _lib.nh_get_device_count(C.byref(n))
    return n.value


class Context:
    """One GPU: device scene, BVH, master framebuffer (nh_ctx)."""

    def __init__(self, device: int = 0):
        global _hip_used
        _hip_used = True
        h = _vp()
        rc = _lib.nh_create(device, C.byref(h))
        if rc != NH_OK:
            raise NoriError(f"nh_create(device={device}) failed with {rc}")
        self._h = h
        self.scene = None

    def close(self):
        if getattr(self, "_h", None):
            _lib.nh_destroy(self._h)
            self._h = None

    def __del__(self):
        self.close()

    def _check(self, rc, what):
        if rc != NH_OK:
            raise NoriError(f"{what}: {_lib.nh_last_error(self._h).decode()} (rc={rc})")

    def upload(self, scene: Scene, bvh: Bvh, photon_map: bool = True, av_params: bool = True):
        """Uploads the scene and its BVH; a photon-mapper scene also builds its photon map with seed 0 (photon_map=False
        leaves that to build_photon_map), an av scene also passes its `length` (av_params=False leaves that to
        set_av_params)."""
        self.scene = scene
        d = scene.desc
        self._check(_lib.nh_upload_scene(self._h, C.byref(d)), "upload_scene")
        b = bvh.desc
        self._check(_lib.nh_upload_bvh(self._h, C.byref(b)), "upload_bvh")
        if photon_map and d.integrator == INTEGRATOR_PHOTONMAPPER:  # Integrator::preprocess, map seed 0
            self.build_photon_map(seed=0)
        if av_params and d.integrator == INTEGRATOR_AV:
            self.set_av_params()

    def set_av_params(self, length: float = None):
        """nh_set_av_params on the uploaded scene: the av integrator's occlusion-ray length, the scene's by default."""
        p = nh_av_params(self.scene.av_params() if length is None else length)
        self._check(_lib.nh_set_av_params(self._h, C.byref(p)), "set_av_params")

    def build_photon_map(self, seed: int = 0, batch_paths: int = 0, photon_count: int = None,
                         photon_radius: float = None) -> dict:
        """nh_photon_map_build on the uploaded scene: PhotonMapper::preprocess with photon path k on the stream
        (seed, PHOTON_STREAM, k). photon_count / photon_radius default to the scene's; batch_paths (paths per launch,
        0 = PHOTON_DEFAULT_BATCH) changes nothing in the result. Returns photon_stats()."""
        n, r = self.scene.photon_params()
        p = nh_photon_params(n if photon_count is None else photon_count, r if photon_radius is None else photon_radius)
        self._check(_lib.nh_photon_map_build(self._h, C.byref(p), seed, batch_paths), "photon_map_build")
        return self.photon_stats()

    def photon_stats(self) -> dict:
        """nh_get_photon_stats: stored, emitted (E), radius, cell_size, occupied_cells of the context's map."""
        s = nh_photon_stats()
        self._check(_lib.nh_get_photon_stats(self._h, C.byref(s)), "get_photon_stats")
        return {"stored": int(s.stored), "emitted": int(s.emitted), "radius": np.float32(s.radius),
                "cell_size": np.float32(s.cell_size), "occupied_cells": int(s.occupied_cells)}

    def photons(self, first: int = 0, n: int = None) -> dict:
        """nh_get_photons: photons first .. first + n - 1 in deposit order. {"position", "direction", "power": (n, 3)
        float32 (direction and power decoded from the stored bytes), "bytes": (n, 6) uint8 (theta, phi, rgbe),
        "path", "bounce": (n,) int32}."""
        if n is None:
            n = self.photon_stats()["stored"] - first
        out = {"position": np.zeros((n, 3), np.float32), "direction": np.zeros((n, 3), np.float32),
               "power": np.zeros((n, 3), np.float32), "bytes": np.zeros((n, 6), np.uint8),
               "path": np.zeros(n, np.int32), "bounce": np.zeros(n, np.int32)}
        self._check(_lib.nh_get_photons(self._h, first, n, _fptr(out["position"]), _fptr(out["direction"]),
                                        _fptr(out["power"]), out["bytes"].ctypes.data_as(_u8p),
                                        out["path"].ctypes.data_as(_i32p), out["bounce"].ctypes.data_as(_i32p)),
                    "get_photons")
        return out

    def photon_codec(self, direction: np.ndarray, power: np.ndarray) -> dict:
        """nh_photon_query, PHOTON_QUERY_CODEC: PhotonData's constructor and getters on the device. {"bytes": (n, 6)
        uint8 (theta, phi, rgbe), "direction", "power": (n, 3) float32 decoded from them}. Needs no scene."""
        inp = np.ascontiguousarray(np.concatenate([np.asarray(direction, np.float32).reshape(-1, 3),
                                                   np.asarray(power, np.float32).reshape(-1, 3)], axis=1))
        n = len(inp)
        b, o = np.zeros((n, 6), np.uint8), np.zeros((n, 6), np.float32)
        self._check(_lib.nh_photon_query(self._h, PHOTON_QUERY_CODEC, n, _fptr(inp), b.ctypes.data_as(_u8p), None,
                                         _fptr(o)), "photon_query")
        return {"bytes": b, "direction": o[:, 0:3].copy(), "power": o[:, 3:6].copy()}

    def photon_gather(self, points: np.ndarray) -> dict:
        """nh_photon_query, PHOTON_QUERY_GATHER: per point the number of photons within the map's radius (strict,
        fp32) and the fp32 sum of their decoded powers in the gather's order. {"count": (n,) int32, "power": (n, 3)}."""
        pts = np.ascontiguousarray(points, dtype=np.float32).reshape(-1, 3)
        n = len(pts)
        cnt, o = np.zeros(n, np.int32), np.zeros((n, 3), np.float32)
        self._check(_lib.nh_photon_query(self._h, PHOTON_QUERY_GATHER, n, _fptr(pts), None,
                                         cnt.ctypes.data_as(_i32p), _fptr(o)), "photon_query")
        return {"count": cnt, "power": o}

    def sample_photon(self, emitter: int, sample: np.ndarray) -> dict:
        """nh_emitter_query, EMITTER_QUERY_SAMPLE_PHOTON: samplePhoton of area light `emitter` for sample (n, 4) =
        (sample1, sample2). {"o", "d", "W": (n, 3), "pdf": (n,)}; W includes the photon pass's `* lights.size()`."""
        s = np.ascontiguousarray(sample, dtype=np.float32).reshape(-1, 4)
        o = np.zeros((len(s), EMITTER_QUERY_PHOTON_STRIDE), np.float32)
        self._check(_lib.nh_emitter_query(self._h, emitter, EMITTER_QUERY_SAMPLE_PHOTON, len(s), None, _fptr(s),
                                          _fptr(o)), "emitter_query")
        return {"o": o[:, 0:3].copy(), "d": o[:, 3:6].copy(), "W": o[:, 6:9].copy(), "pdf": o[:, 9].copy()}

    def render(self, s0: int, s1: int, seed: int = 0, blocks=None, traversal: int = TRAVERSAL_REFERENCE,
               clear: bool = False, stats: bool = False, mode: int = MODE_MEGAKERNEL):
        q = nh_render_req()
        q.sample_begin, q.sample_end, q.seed = s0, s1, seed
        keep = None
        if blocks is not None:
            keep = np.ascontiguousarray(blocks, dtype=np.int32)
            q.n_blocks = len(keep)
            q.blocks = keep.ctypes.data_as(C.POINTER(_i32))
        q.mode, q.traversal, q.clear, q.collect_stats = mode, traversal, int(clear), int(stats)
        self._check(_lib.nh_render(self._h, C.byref(q)), "render")

    def synchronize(self):
        self._check(_lib.nh_synchronize(self._h), "synchronize")

    def framebuffer(self) -> np.ndarray:
        shp = self.scene.framebuffer_shape()
        out = np.zeros(shp, dtype=np.float32)
        self._check(_lib.nh_get_framebuffer(self._h, _fptr(out), out.size), "get_framebuffer")
        return out

    def framebuffer_device_ptr(self):
        p, n = _vp(), C.c_size_t()
        self._check(_lib.nh_framebuffer_device_ptr(self._h, C.byref(p), C.byref(n)), "framebuffer_device_ptr")
        return p.value, n.value

    def stats(self) -> dict:
        s = nh_render_stats()
        self._check(_lib.nh_get_stats(self._h, C.byref(s)), "get_stats")
        return {f: getattr(s, f) for f, _ in s._fields_}

    def adaptive_stats(self) -> dict:
        """nh_get_adaptive_stats: total_samples ("Total Samples Placed"), passes, max_passes, n_blocks of the
        adaptive renders since the last range that started at 0."""
        s = nh_adaptive_stats()
        self._check(_lib.nh_get_adaptive_stats(self._h, C.byref(s)), "get_adaptive_stats")
        return {f: int(getattr(s, f)) for f, _ in s._fields_}

    def adaptive_variance(self) -> np.ndarray:
        """nh_get_adaptive_variance: every block's m_oldVariance at its place in the image, (H, W) float32."""
        out = np.zeros((self.scene.height, self.scene.width), np.float32)
        self._check(_lib.nh_get_adaptive_variance(self._h, _fptr(out), out.size), "get_adaptive_variance")
        return out

    def reset_stats(self):
        self._check(_lib.nh_reset_stats(self._h), "reset_stats")

    def denoise(self, params: nh_denoiser = None):
        """Denoiser::denoise on the master ImageBlock (src/utils/render.cpp:368-369): the scene's
        <denoiser> unless params are given."""
        if params is None:
            params = self.scene.desc.denoiser
        self._check(_lib.nh_denoise(self._h, C.byref(params)), "denoise")

    def denoise_image(self, rgbw: np.ndarray, border: int, params: nh_denoiser) -> np.ndarray:
        """SimpleDenoiser on a host (H+2b, W+2b, 4) float32 ImageBlock; returns the denoised copy."""
        out = np.array(rgbw, dtype=np.float32, order="C", copy=True)
        h, w = out.shape[0] - 2 * border, out.shape[1] - 2 * border
        self._check(_lib.nh_denoise_image(self._h, _fptr(out), w, h, border, C.byref(params)), "denoise_image")
        return out

    def bsdf_query(self, bsdf: nh_bsdf, wi: np.ndarray, wo: np.ndarray = None, sample: np.ndarray = None,
                   albedo=None) -> dict:
        """nh_bsdf_query: n BSDF queries by the render kernels' own device functions. wi: (n, 3) local directions.
        With wo (n, 3): {"value": eval (n, 3), "pdf": (n,)}, solid-angle measure. With sample (n, 2) instead:
        {"wo": (n, 3), "value": the sample's weight (n, 3), "pdf": pdf(wi, wo) (n,), "measure": (n,)}. albedo: the
        colour standing in for the albedo texture's value (default: bsdf.albedo)."""
        if (wo is None) == (sample is None):
            raise ValueError("bsdf_query: give either wo (eval) or sample (sample)")
        wi = np.ascontiguousarray(wi, dtype=np.float32).reshape(-1, 3)
        n = len(wi)
        out = {"value": np.zeros((n, 3), np.float32), "pdf": np.zeros(n, np.float32)}
        alb = None if albedo is None else np.ascontiguousarray(albedo, dtype=np.float32).reshape(3)
        if wo is not None:
            wo = np.ascontiguousarray(wo, dtype=np.float32).reshape(n, 3)
            rc = _lib.nh_bsdf_query(self._h, C.byref(bsdf), None if alb is None else _fptr(alb), BSDF_QUERY_EVAL, n,
                                    _fptr(wi), _fptr(wo), None, None, _fptr(out["value"]), _fptr(out["pdf"]), None)
        else:
            sample = np.ascontiguousarray(sample, dtype=np.float32).reshape(n, 2)
            out["wo"] = np.zeros((n, 3), np.float32)
            out["measure"] = np.zeros(n, np.int32)
            rc = _lib.nh_bsdf_query(self._h, C.byref(bsdf), None if alb is None else _fptr(alb), BSDF_QUERY_SAMPLE, n,
                                    _fptr(wi), None, _fptr(sample), _fptr(out["wo"]), _fptr(out["value"]),
                                    _fptr(out["pdf"]), out["measure"].ctypes.data_as(C.POINTER(_i32)))
        self._check(rc, "bsdf_query")
        return out

    def emitter_query(self, emitter: int, ref: np.ndarray, sample: np.ndarray = None, wi: np.ndarray = None,
                      p: np.ndarray = None, n: np.ndarray = None, mode: int = None) -> dict:
        """nh_emitter_query: queries of emitter `emitter` of the uploaded scene by the render kernels' own device
        functions. ref: (m, 3) reference points. With sample (m, 2): emitter_sample -> {"value": the sample's weight
        (m, 3), "wi": (m, 3), "pdf": (m,), "o" / "d": the shadow ray (m, 3), "mint" / "maxt": (m,)}. With wi (m, 3)
        instead (and, for area lights, the point p on the light and its normal n): {"value": eval (m, 3),
        "pdf": (m,)}; mode = EMITTER_QUERY_EVAL / EMITTER_QUERY_PDF runs only that one."""
        if (sample is None) == (wi is None):
            raise ValueError("emitter_query: give either sample (sample) or wi (eval and pdf)")
        ref = np.ascontiguousarray(ref, dtype=np.float32).reshape(-1, 3)
        m = len(ref)

        def call(md, inp, out):
            self._check(_lib.nh_emitter_query(self._h, emitter, md, m, _fptr(ref), _fptr(inp), _fptr(out)),
                        "emitter_query")
            return out
        if sample is not None:
            sample = np.ascontiguousarray(sample, dtype=np.float32).reshape(m, 2)
            o = call(EMITTER_QUERY_SAMPLE, sample, np.zeros((m, EMITTER_QUERY_SAMPLE_STRIDE), np.float32))
            return {"value": o[:, 0:3].copy(), "wi": o[:, 3:6].copy(), "pdf": o[:, 6].copy(), "o": o[:, 7:10].copy(),
                    "d": o[:, 10:13].copy(), "mint": o[:, 13].copy(), "maxt": o[:, 14].copy()}
        inp = np.zeros((m, EMITTER_QUERY_IN_STRIDE), np.float32)
        inp[:, 0:3] = np.asarray(wi, np.float32).reshape(m, 3)
        if p is not None:
            inp[:, 3:6] = np.asarray(p, np.float32).reshape(m, 3)
        if n is not None:
            inp[:, 6:9] = np.asarray(n, np.float32).reshape(m, 3)
        out = {}
        if mode in (None, EMITTER_QUERY_EVAL):
            out["value"] = call(EMITTER_QUERY_EVAL, inp, np.zeros((m, 3), np.float32))
        if mode in (None, EMITTER_QUERY_PDF):
            out["pdf"] = call(EMITTER_QUERY_PDF, inp, np.zeros(m, np.float32))
        return out

    def medium_query(self, medium: int, mode: int, inp: np.ndarray) -> np.ndarray:
        """nh_medium_query: queries of medium `medium` of the uploaded scene by the volumetric kernel's own device
        functions. MEDIUM_QUERY_FREE_PATH: inp (m, 2) uniforms -> (m, 2): t and the draws consumed;
        MEDIUM_QUERY_TRANSMITTANCE: inp (m, 6) from, to -> (m, 3); MEDIUM_QUERY_PHASE_SAMPLE: inp (m, 2) -> (m, 4): wo
        and its pdf; MEDIUM_QUERY_PHASE_PDF: inp (m, 3) wo -> (m,)."""
        n_in, n_out = {MEDIUM_QUERY_FREE_PATH: (2, 2), MEDIUM_QUERY_TRANSMITTANCE: (6, 3),
                       MEDIUM_QUERY_PHASE_SAMPLE: (2, 4), MEDIUM_QUERY_PHASE_PDF: (3, 1)}[mode]
        inp = np.ascontiguousarray(inp, dtype=np.float32).reshape(-1, n_in)
        out = np.zeros((len(inp), n_out), np.float32)
        self._check(_lib.nh_medium_query(self._h, medium, mode, len(inp), _fptr(inp), _fptr(out)), "medium_query")
        return out[:, 0] if n_out == 1 else out

    def radiance_query(self, pixel, sample, seed: int = 0, pixel_sample=None) -> dict:
        """nh_radiance_query: the radiance of sample sample[i] of pixel pixel[i] (y * width + x) of the uploaded scene
        under `seed`, by the render kernels' own integrators, unfiltered. pixel_sample (n, 2): the image-plane
        positions to shoot through instead of pixel + jitter. {"rgb": (n, 3), "jitter": (n, 2)} float32."""
        pixel = np.ascontiguousarray(pixel, dtype=np.int32).ravel()
        sample = np.ascontiguousarray(np.broadcast_to(np.asarray(sample, dtype=np.int32), pixel.shape))
        n = len(pixel)
        ps = None if pixel_sample is None else np.ascontiguousarray(pixel_sample, dtype=np.float32).reshape(n, 2)
        out = {"rgb": np.zeros((n, 3), np.float32), "jitter": np.zeros((n, 2), np.float32)}
        self._check(_lib.nh_radiance_query(self._h, seed, n, pixel.ctypes.data_as(_i32p), sample.ctypes.data_as(_i32p),
                                           None if ps is None else _fptr(ps), _fptr(out["rgb"]), _fptr(out["jitter"])),
                    "radiance_query")
        return out

    def ttest_scene(self, n: int, seed: int = 0, first: int = 0, luminance: bool = False):
        """nh_ttest_scene: StudentsTTest's scene estimator over samples first .. first + n - 1 of the uploaded scene,
        each on its own stream (seed, pixel 0, sample k). (mean, variance), and the n luminances (float32) as a third
        element with luminance=True."""
        m, v = C.c_double(0.0), C.c_double(0.0)
        lum = np.zeros(max(n, 0), np.float32) if luminance else None
        self._check(_lib.nh_ttest_scene(self._h, seed, first, n, C.byref(m), C.byref(v),
                                        None if lum is None else _fptr(lum)), "ttest_scene")
        return (m.value, v.value, lum) if luminance else (m.value, v.value)

    def ttest_bsdf(self, bsdf: nh_bsdf, angle_deg: float, n: int, first_draw: int = 0, albedo=None,
                   luminance: bool = False):
        """nh_ttest_bsdf: StudentsTTest's BSDF estimator at incidence angle angle_deg: sample k takes draws
        first_draw + 2k, + 2k + 1 of the default-state pcg32. Returns as ttest_scene."""
        m, v = C.c_double(0.0), C.c_double(0.0)
        lum = np.zeros(max(n, 0), np.float32) if luminance else None
        alb = None if albedo is None else np.ascontiguousarray(albedo, dtype=np.float32).reshape(3)
        self._check(_lib.nh_ttest_bsdf(self._h, C.byref(bsdf), None if alb is None else _fptr(alb), angle_deg, first_draw,
                                       n, C.byref(m), C.byref(v), None if lum is None else _fptr(lum)), "ttest_bsdf")
        return (m.value, v.value, lum) if luminance else (m.value, v.value)

    def chi2_histogram(self, bsdf: nh_bsdf, wi, n: int, res_theta: int, res_phi: int, first_draw: int = 0,
                       albedo=None) -> np.ndarray:
        """nh_chi2_histogram: ChiSquareTest's contingency table of n samples of bsdf_sample at incident direction wi
        (the BSDF's frame): sample k takes draws first_draw + 2k, + 2k + 1 of the default-state pcg32. (res_theta *
        res_phi,) float64 of whole counts, the same bits on every run."""
        w = np.ascontiguousarray(wi, dtype=np.float32).reshape(3)
        alb = None if albedo is None else np.ascontiguousarray(albedo, dtype=np.float32).reshape(3)
        obs = np.zeros(max(res_theta, 0) * max(res_phi, 0), np.float64)
        self._check(_lib.nh_chi2_histogram(self._h, C.byref(bsdf), None if alb is None else _fptr(alb), _fptr(w),
                                           first_draw, n, res_theta, res_phi, obs.ctypes.data_as(_dp)), "chi2_histogram")
        return obs

    def chi2_expected(self, bsdf: nh_bsdf, wi, res_theta: int, res_phi: int, sample_count: int, albedo=None,
                      evals: bool = False):
        """nh_chi2_expected: ChiSquareTest's expected frequencies for the incident directions wi ((m, 3), or (3,)) by
        adaptiveSimpson2D of the device's bsdf_pdf over every cell, times sample_count. (m, cells) float64 ((cells,)
        for one direction); with evals=True also the pdf evaluations per cell (uint32) as a second element."""
        w = np.ascontiguousarray(wi, dtype=np.float32)
        single = w.ndim == 1
        w = np.ascontiguousarray(w.reshape(-1, 3))
        alb = None if albedo is None else np.ascontiguousarray(albedo, dtype=np.float32).reshape(3)
        cells = max(res_theta, 0) * max(res_phi, 0)
        exp = np.zeros((len(w), cells), np.float64)
        ev = np.zeros((len(w), cells), np.uint32) if evals else None
        self._check(_lib.nh_chi2_expected(self._h, C.byref(bsdf), None if alb is None else _fptr(alb), len(w), _fptr(w),
                                          res_theta, res_phi, sample_count, exp.ctypes.data_as(_dp),
                                          None if ev is None else ev.ctypes.data_as(_u32p)), "chi2_expected")
        if single:
            exp, ev = exp[0], (None if ev is None else ev[0])
        return (exp, ev) if evals else exp

    @staticmethod
    def _warp_wi(wi):
        return None if wi is None else _fptr(np.ascontiguousarray(wi, dtype=np.float32).reshape(3))

    def warp_query(self, type: int, parameter: float, mode: int, inp, wi=None) -> np.ndarray:
        """nh_warp_query: warpPoint (WARP_QUERY_SAMPLE: inp (n, 3) samples -> (n, 4) point and weight) or the matching
        pdf (WARP_QUERY_PDF: inp (n, 3) points -> (n,)) of warp `type` at the mapped parameter; wi for the BRDF."""
        inp = np.ascontiguousarray(inp, dtype=np.float32).reshape(-1, 3)
        out = np.zeros((len(inp), 4) if mode == WARP_QUERY_SAMPLE else (len(inp),), np.float32)
        self._check(_lib.nh_warp_query(self._h, type, parameter, self._warp_wi(wi), mode, len(inp), _fptr(inp),
                                       _fptr(out)), "warp_query")
        return out

    def warp_histogram(self, type: int, parameter: float, n: int, xres: int, yres: int, first_draw: int = 0,
                       draw_order: int = LENS_DRAWS_RTL, wi=None):
        """nh_warp_histogram: (obs, nan_points) -- runTest's table of n points of the default-state pcg32 from draw
        first_draw ((yres * xres,) float64 of whole counts, the same bits on every run) and the number of points left
        out because a coordinate was NaN."""
        obs = np.zeros(max(xres, 0) * max(yres, 0), np.float64)
        nan = _u32(0)
        self._check(_lib.nh_warp_histogram(self._h, type, parameter, self._warp_wi(wi), first_draw, draw_order, n, xres,
                                           yres, obs.ctypes.data_as(_dp), C.byref(nan)), "warp_histogram")
        return obs, int(nan.value)

    def warp_expected(self, type: int, parameter: float, xres: int, yres: int, sample_count: int, wi=None,
                      evals: bool = False):
        """nh_warp_expected: runTest's expected frequencies, (yres * xres,) float64; with evals=True also the pdf
        evaluations per cell (uint32) as a second element."""
        cells = max(xres, 0) * max(yres, 0)
        exp = np.zeros(cells, np.float64)
        ev = np.zeros(cells, np.uint32) if evals else None
        self._check(_lib.nh_warp_expected(self._h, type, parameter, self._warp_wi(wi), xres, yres, sample_count,
                                          exp.ctypes.data_as(_dp), None if ev is None else ev.ctypes.data_as(_u32p)),
                    "warp_expected")
        return (exp, ev) if evals else exp

    def trace(self, o: np.ndarray, d: np.ndarray, mint: np.ndarray, maxt: np.ndarray, any_hit=False,
              traversal: int = TRAVERSAL_REFERENCE) -> dict:
        n = len(o)
        cols = [np.ascontiguousarray(x, dtype=np.float32) for x in (o[:, 0], o[:, 1], o[:, 2], d[:, 0], d[:, 1],
                                                                     d[:, 2], mint, maxt)]
        r = nh_ray_soa(*[_fptr(c) for c in cols])
        res = {"hit": np.zeros(n, np.uint8), "t": np.zeros(n, np.float32), "u": np.zeros(n, np.float32),
               "v": np.zeros(n, np.float32), "prim": np.zeros(n, np.uint32), "shape": np.zeros(n, np.uint32)}
        h = nh_hit_soa(res["hit"].ctypes.data_as(C.POINTER(C.c_uint8)), _fptr(res["t"]), _fptr(res["u"]),
                       _fptr(res["v"]), res["prim"].ctypes.data_as(_u32p), res["shape"].ctypes.data_as(_u32p))
        self._check(_lib.nh_trace_rays(self._h, C.byref(r), n, int(any_hit), traversal, C.byref(h)), "trace_rays")
        return res


def tile_shard(width: int, height: int, world: int, rank: int) -> list:
    """32x32 image blocks (block id = by*nbx + bx, BlockGenerator numbering) dealt
    round-robin to ranks: the multi-GPU partition of the image."""
    nbx, nby = (width + 31) // 32, (height + 31) // 32
    return [b for b in range(nbx * nby) if b % world == rank]


def primary_mask_pad(width: int, height: int) -> int:
    """nh_primary_mask_pad: the pixels a block's rectangle is grown by on every side."""
    return int(_lib.nh_primary_mask_pad(width, height))


def primary_masks(camera: nh_camera, records: np.ndarray, blocks):
    """nh_primary_masks: per block of `blocks` (ids by * nbx + bx) a uint64 whose bit k says record k of `records`
    ((n, 12) float32 in the device's format, csrc/nh_traverse.h) can be hit by one of the block's camera rays. None when the feature is absent
    (more than 64 records, or a camera with a lens)."""
    rec = np.ascontiguousarray(records, dtype=np.float32).reshape(-1, 12)
    blk = np.ascontiguousarray(blocks, dtype=np.int32).ravel()
    out = np.zeros(len(blk), np.uint64)
    built = _i32(0)
    _host_check(_lib.nh_primary_masks(C.byref(camera), _fptr(rec), len(rec), blk.ctypes.data_as(C.POINTER(_i32)),
                                      len(blk), out.ctypes.data_as(C.POINTER(C.c_uint64)), C.byref(built)),
                "primary_masks")
    return out if built.value else None


def shadow_emitter_faces(desc: nh_scene_desc):
    """nh_shadow_emitter_faces: (n, 9) float32, the vertices of every emitter face of the scene when all its emitters
    are area lights on meshes without vertex normals; else empty."""
    out, n = np.zeros((max(int(desc.n_faces), 1), 9), np.float32), _i32(0)
    _host_check(_lib.nh_shadow_emitter_faces(C.byref(desc), _fptr(out), len(out), C.byref(n)), "shadow_emitter_faces")
    return out[:n.value].copy()


def shadow_masks(camera: nh_camera, records: np.ndarray, emit_faces, blocks):
    """nh_shadow_masks: (emitter_word, masks) for the light samples' any-hit queries. emit_faces: (n, 9) float32, the
    vertices of every emitter face when every emitter is an area light on a mesh without vertex normals, else None or
    empty. emitter_word: an int whose clear bit k says no shadow ray can be accepted by record k (all ones: nothing is
    left out). masks: per block of `blocks` a uint64 with the same meaning for the shadow rays of that block's first
    hits, or None when the per-block table is absent (as primary_masks)."""
    rec = np.ascontiguousarray(records, dtype=np.float32).reshape(-1, 12)
    blk = np.ascontiguousarray(blocks, dtype=np.int32).ravel()
    ef = np.zeros((0, 9), np.float32) if emit_faces is None else np.ascontiguousarray(emit_faces, np.float32).reshape(-1, 9)
    out = np.zeros(len(blk), np.uint64)
    word, built = C.c_uint64(0), _i32(0)
    _host_check(_lib.nh_shadow_masks(C.byref(camera), _fptr(rec), len(rec), _fptr(ef), len(ef),
                                     blk.ctypes.data_as(C.POINTER(_i32)), len(blk), C.byref(word),
                                     out.ctypes.data_as(C.POINTER(C.c_uint64)), C.byref(built)), "shadow_masks")
    return int(word.value), (out if built.value else None)


def pair_layout(records: np.ndarray, leaves, by_kind: bool = True):
    """nh_pair_layout: which records ((n, 12) float32, the device's format) share a pair record of a small scene's LDS
    image, for the leaf table `leaves` ((start, count) rows). Returns (slots, leaf_pairs): slots (n, 2) int32 per pair
    position -- (slot 0 record, slot 1 record or -1), (-1, -1) unused -- and leaf_pairs (n_leaves, 3) int32 -- first
    pair position, triangle pairs, sphere pairs. by_kind False: the reference arrangement."""
    rec = np.ascontiguousarray(records, dtype=np.float32).reshape(-1, 12)
    lv = np.ascontiguousarray(leaves, dtype=np.int32).reshape(-1, 2)
    slots, lp = np.zeros((len(rec), 2), np.int32), np.zeros((len(lv), 3), np.int32)
    ip = C.POINTER(_i32)
    _host_check(_lib.nh_pair_layout(_fptr(rec), len(rec), lv.ctypes.data_as(ip), len(lv), 1 if by_kind else 0,
                                    slots.ctypes.data_as(ip), lp.ctypes.data_as(ip)), "pair_layout")
    return slots, lp


def shadow_any_word(camera: nh_camera, records: np.ndarray, emit_faces) -> int:
    """nh_shadow_any_word: the scene-wide any-hit word, an int whose clear bit k says no shadow ray of any bounce can be
    accepted by record k (the emitter-side word's zeros and the supporting walls); all ones: nothing is left out.
    emit_faces: as for shadow_masks."""
    rec = np.ascontiguousarray(records, dtype=np.float32).reshape(-1, 12)
    ef = np.zeros((0, 9), np.float32) if emit_faces is None else np.ascontiguousarray(emit_faces, np.float32).reshape(-1, 9)
    word = C.c_uint64(0)
    _host_check(_lib.nh_shadow_any_word(C.byref(camera), _fptr(rec), len(rec), _fptr(ef), len(ef), C.byref(word)),
                "shadow_any_word")
    return int(word.value)


def flat_image(records: np.ndarray, leaves, boxes, allowed: bool = True, any_word: int | None = None):
    """nh_flat_image: the flat image of a tree of one leaf or of a root with two leaves -- `leaves` its (start, count)
    rows, `boxes` the root's, left child's and right child's boxes (18 floats: min xyz, max xyz each). Returns (image,
    box_equal): image (n, 4) float32 -- 6 header rows, then 6 rows per pair record -- or None when the scene is not flat;
    box_equal bit 0 / 1: the left / right child's box is bit-equal to the root's. any_word (nh_flat_image_any): the
    scene-wide any-hit word; unless it keeps every record the image has an any-hit section from row 6 + 6 * 16 on."""
    rec = np.ascontiguousarray(records, dtype=np.float32).reshape(-1, 12)
    lv = np.ascontiguousarray(leaves, dtype=np.int32).reshape(-1, 2)
    bx = np.ascontiguousarray(boxes, dtype=np.float32).ravel()
    assert bx.size == 18
    cap = 6 + 6 * 16 * (1 if any_word is None else 2)
    img, n, eq = np.zeros((cap, 4), np.float32), _i32(0), _i32(0)
    ip = lv.ctypes.data_as(C.POINTER(_i32))
    if any_word is None:
        _host_check(_lib.nh_flat_image(_fptr(rec), len(rec), ip, len(lv), _fptr(bx), 1 if allowed else 0, _fptr(img), cap,
                                       C.byref(n), C.byref(eq)), "flat_image")
    else:
        _host_check(_lib.nh_flat_image_any(_fptr(rec), len(rec), ip, len(lv), _fptr(bx), 1 if allowed else 0,
                                           C.c_uint64(any_word & ((1 << 64) - 1)), _fptr(img), cap, C.byref(n),
                                           C.byref(eq)), "flat_image_any")
    return (img[:n.value].copy() if n.value else None), int(eq.value)


def reduce_framebuffers(ctxs, root: int = 0):
    arr = (_vp * len(ctxs))(*[c._h for c in ctxs])
    rc = _lib.nh_reduce_framebuffers(arr, len(ctxs), root)
    if rc != NH_OK:
        raise NoriError(f"nh_reduce_framebuffers failed ({rc})")


def to_rgb(rgbw: np.ndarray, border: int) -> np.ndarray:
    """ImageBlock::toBitmap via the C-ABI (block.cpp:76-82)."""
    h, w = rgbw.shape[0] - 2 * border, rgbw.shape[1] - 2 * border
    src = np.ascontiguousarray(rgbw, dtype=np.float32)
    out = np.zeros((h, w, 3), np.float32)
    rc = _lib.nh_framebuffer_to_rgb(_fptr(src), w, h, border, _fptr(out))
    if rc != NH_OK:
        raise NoriError("framebuffer_to_rgb failed")
    return out


def write_exr(path: str, rgb: np.ndarray):
    rgb = np.ascontiguousarray(rgb, dtype=np.float32)
    _host_check(_lib.nh_write_exr(path.encode(), _fptr(rgb), rgb.shape[1], rgb.shape[0]), "write_exr")


def write_png(path: str, rgb: np.ndarray):
    """8-bit sRGB PNG as Bitmap::saveToLDR (src/utils/bitmap.cpp:122-140)."""
    rgb = np.ascontiguousarray(rgb, dtype=np.float32)
    _host_check(_lib.nh_write_png(path.encode(), _fptr(rgb), rgb.shape[1], rgb.shape[0]), "write_png")


def rgb_to_ldr(rgb: np.ndarray) -> np.ndarray:
    """The bytes write_png stores: (H, W, 3) uint8."""
    rgb = np.ascontiguousarray(rgb, dtype=np.float32)
    out = np.empty(rgb.shape[:2] + (3,), np.uint8)
    _host_check(_lib.nh_rgb_to_ldr(_fptr(rgb), rgb.shape[1], rgb.shape[0],
                                   out.ctypes.data_as(C.POINTER(C.c_uint8))), "rgb_to_ldr")
    return out


def write_pfm(path: str, rgb: np.ndarray):
    rgb = np.ascontiguousarray(rgb, dtype=np.float32)
    _host_check(_lib.nh_write_pfm(path.encode(), _fptr(rgb), rgb.shape[1], rgb.shape[0]), "write_pfm")


def load_png(path: str) -> np.ndarray:
    """PNG -> (H, W, 4) uint8 through the library's decoder (nh_image_load_png)."""
    w, h = _i32(), _i32()
    _host_check(_lib.nh_image_load_png(path.encode(), None, 0, C.byref(w), C.byref(h)), "load_png")
    out = np.zeros((h.value, w.value, 4), np.uint8)
    _host_check(_lib.nh_image_load_png(path.encode(), out.ctypes.data_as(C.POINTER(C.c_uint8)), out.nbytes,
                                       C.byref(w), C.byref(h)), "load_png")
    return out
