// nh_radiance_query, the t-test estimators nh_ttest_scene / nh_ttest_bsdf and the runner nh_test_run of the C-ABI
// (include/nori_hip.h): the host side of nh_query.hip's kernels.
#include <cmath>
#include <cstring>

#include "../host/nh_host.h"
#include "nh_ctx.h"

namespace {

constexpr int kQueryChunk = 1 << 20;  // paths per launch

struct Free {
    std::vector<void *> &v;
    ~Free() { free_all(v); }
};

template <typename T>
int q_alloc(nh_ctx *c, std::vector<void *> &owner, T **p, size_t n) {
    void *d = nullptr;
    HIP_TRY(c, hipMalloc(&d, std::max<size_t>(n, 1) * sizeof(T)));
    owner.push_back(d);
    *p = static_cast<T *>(d);
    return NH_OK;
}

// what nh_render asks of the uploaded scene before its integrator runs
int path_query_ready(nh_ctx *c, const std::string &who) {
    if (!c->has_scene || !c->has_bvh) return fail(c, who + ": scene and BVH must be uploaded"), NH_ERR_STATE;
    const bool volumetric = c->integrator == NH_INTEGRATOR_PATH_VOL_MATS || c->integrator == NH_INTEGRATOR_PATH_VOL_MIS;
    if ((c->integrator == NH_INTEGRATOR_PATH_MIS || c->integrator == NH_INTEGRATOR_DIRECT_MIS ||
         c->integrator == NH_INTEGRATOR_PATH_VOL_MIS) && c->n_emitters == 0)
        return fail(c, "No Emitter in scene!"), NH_ERR_INVALID;
    if (!volumetric && (c->bsdfless || c->has_media))
        return fail(c, "the scene has a participating medium or a shape without a BSDF: only the path_vol_mats and "
                       "path_vol_mis integrators render it"), NH_ERR_UNSUPPORTED;
    if (c->integrator == NH_INTEGRATOR_PHOTONMAPPER && !c->photon.built)
        return fail(c, who + ": the photon mapper needs a photon map (nh_photon_map_build)"), NH_ERR_STATE;
    if (c->integrator == NH_INTEGRATOR_AV && !c->av_set)
        return fail(c, who + ": the av integrator needs its length (nh_set_av_params)"), NH_ERR_STATE;
    if (c->integrator == NH_INTEGRATOR_ENVMAPTESTER && c->S.envmap < 0)  // EnvMapTester.cpp:19-23
        return fail(c, "This integrator requires an env map."), NH_ERR_INVALID;
    return NH_OK;
}

// mean and unbiased variance of lum[0..n) on the device, two passes, into out[0] / out[1] (device), then the host
int reduce_moments(nh_ctx *c, std::vector<void *> &bufs, const float *lum, int n, double *mean, double *variance) {
    double *partial = nullptr, *out = nullptr;
    if (int rc = q_alloc(c, bufs, &partial, (size_t)(n + kTtPerBlock - 1) / kTtPerBlock)) return rc;
    if (int rc = q_alloc(c, bufs, &out, 2)) return rc;
    nh_disney::nh::launch_ttest_reduce(lum, n, nullptr, (double)n, partial, out, c->stream);
    nh_disney::nh::launch_ttest_reduce(lum, n, out, (double)(n - 1), partial, out + 1, c->stream);
    HIP_TRY(c, hipGetLastError());
    double h[2];
    HIP_TRY(c, hipMemcpyAsync(h, out, sizeof(h), hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    *mean = h[0];
    *variance = h[1];
    return NH_OK;
}

}  // namespace

extern "C" {

int nh_radiance_query(nh_ctx *c, uint64_t seed, int32_t n, const int32_t *pixel, const int32_t *sample,
                      const float *pixel_sample, float *rgb, float *jitter) {
    if (!c) return NH_ERR_INVALID;
    if (n < 0 || n > NH_RADIANCE_QUERY_MAX) return fail(c, "nh_radiance_query: n outside [0, 2^24]"), NH_ERR_INVALID;
    if (!pixel || !sample || !rgb) return fail(c, "nh_radiance_query: null argument"), NH_ERR_INVALID;
    if (int rc = path_query_ready(c, "nh_radiance_query")) return rc;
    const int64_t n_pixels = (int64_t)c->width * c->height;
    for (int32_t i = 0; i < n; ++i) {
        if (pixel[i] < 0 || pixel[i] >= n_pixels)
            return fail(c, "nh_radiance_query: pixel " + std::to_string(pixel[i]) + " outside [0, width * height)"),
                   NH_ERR_INVALID;
        if (sample[i] < 0) return fail(c, "nh_radiance_query: negative sample index"), NH_ERR_INVALID;
        if (c->S.dof && sample[i] >= nhd::kLensLo * nhd::kLensHi)  // the lens tables' range, as nh_render
            return fail(c, "depth of field: sample rounds beyond 2^24"), NH_ERR_UNSUPPORTED;
    }
    if (n == 0) return NH_OK;
    HIP_TRY(c, hipSetDevice(c->device));
    if (int rc = pipeline_drain(c)) return rc;
    std::vector<void *> bufs;
    Free guard{bufs};
    const size_t chunk = (size_t)std::min(n, kQueryChunk);
    int *d_pixel = nullptr, *d_sample = nullptr;
    float2 *d_ps = nullptr, *d_jit = nullptr;
    float4 *d_rad = nullptr;
    int rc;
    if ((rc = q_alloc(c, bufs, &d_pixel, chunk)) || (rc = q_alloc(c, bufs, &d_sample, chunk)) ||
        (rc = q_alloc(c, bufs, &d_rad, chunk)) || (jitter && (rc = q_alloc(c, bufs, &d_jit, chunk))) ||
        (pixel_sample && (rc = q_alloc(c, bufs, &d_ps, chunk))))
        return rc;
    std::vector<float4> rad(chunk);
    for (size_t off = 0; off < (size_t)n; off += chunk) {
        const size_t m = std::min(chunk, (size_t)n - off);
        HIP_TRY(c, hipMemcpyAsync(d_pixel, pixel + off, m * sizeof(int), hipMemcpyHostToDevice, c->stream));
        HIP_TRY(c, hipMemcpyAsync(d_sample, sample + off, m * sizeof(int), hipMemcpyHostToDevice, c->stream));
        if (pixel_sample)
            HIP_TRY(c, hipMemcpyAsync(d_ps, pixel_sample + 2 * off, m * sizeof(float2), hipMemcpyHostToDevice, c->stream));
        PathQuery q{};
        q.seed = seed;
        q.n = (int)m;
        q.pixel = d_pixel;
        q.sample = d_sample;
        q.pixel_sample = d_ps;
        q.rad = d_rad;
        q.jitter = d_jit;
        nh_disney::nh::launch_path_query(c->d_scene, c->tv, q, c->depth, c->stream);
        HIP_TRY(c, hipGetLastError());
        HIP_TRY(c, hipMemcpyAsync(rad.data(), d_rad, m * sizeof(float4), hipMemcpyDeviceToHost, c->stream));
        if (jitter)
            HIP_TRY(c, hipMemcpyAsync(jitter + 2 * off, d_jit, m * sizeof(float2), hipMemcpyDeviceToHost, c->stream));
        HIP_TRY(c, hipStreamSynchronize(c->stream));
        for (size_t i = 0; i < m; ++i) {
            rgb[3 * (off + i)] = rad[i].x;
            rgb[3 * (off + i) + 1] = rad[i].y;
            rgb[3 * (off + i) + 2] = rad[i].z;
        }
    }
    return check_device(c, "nh_radiance_query");
}

int nh_ttest_scene(nh_ctx *c, uint64_t seed, int64_t first, int32_t n, double *mean, double *variance,
                   float *luminance) {
    if (!c) return NH_ERR_INVALID;
    if (!mean || !variance) return fail(c, "nh_ttest_scene: null argument"), NH_ERR_INVALID;
    if (n < 2 || n > NH_RADIANCE_QUERY_MAX || first < 0)
        return fail(c, "nh_ttest_scene: needs 2 <= n <= 2^24 samples and first >= 0"), NH_ERR_INVALID;
    if (int rc = path_query_ready(c, "nh_ttest_scene")) return rc;
    if (c->S.dof)
        return fail(c, "nh_ttest_scene: a thin-lens camera is not supported (the reference's static lens sampler is a "
                       "third sequential stream)"), NH_ERR_UNSUPPORTED;
    HIP_TRY(c, hipSetDevice(c->device));
    if (int rc = pipeline_drain(c)) return rc;
    std::vector<void *> bufs;
    Free guard{bufs};
    float *lum = nullptr;
    if (int rc = q_alloc(c, bufs, &lum, (size_t)n)) return rc;
    for (int off = 0; off < n; off += kQueryChunk) {
        PathQuery q{};
        q.seed = seed;
        q.n = std::min(kQueryChunk, n - off);
        q.first = (uint64_t)first + (uint64_t)off;
        q.lum = lum + off;
        nh_disney::nh::launch_path_query(c->d_scene, c->tv, q, c->depth, c->stream);
        HIP_TRY(c, hipGetLastError());
    }
    if (int rc = reduce_moments(c, bufs, lum, n, mean, variance)) return rc;
    if (luminance) HIP_TRY(c, hipMemcpy(luminance, lum, (size_t)n * sizeof(float), hipMemcpyDeviceToHost));
    return check_device(c, "nh_ttest_scene");
}

int nh_ttest_bsdf(nh_ctx *c, const nh_bsdf *b, const float *albedo, float angle_deg, uint64_t first_draw, int32_t n,
                  double *mean, double *variance, float *luminance) {
    if (!c) return NH_ERR_INVALID;
    if (!b || !mean || !variance) return fail(c, "nh_ttest_bsdf: null argument"), NH_ERR_INVALID;
    if (b->type < NH_BSDF_DIFFUSE || b->type > NH_BSDF_DISNEY) return fail(c, "unknown BSDF type"), NH_ERR_INVALID;
    if (n < 2 || n > NH_RADIANCE_QUERY_MAX) return fail(c, "nh_ttest_bsdf: needs 2 <= n <= 2^24 samples"), NH_ERR_INVALID;
    HIP_TRY(c, hipSetDevice(c->device));
    std::vector<void *> bufs;
    Free guard{bufs};
    BsdfTtest t;
    std::memset(&t, 0, sizeof(t));
    if (int rc = query_bsdf_record(c, bufs, b, albedo, t.bsdf, t.albedo)) return rc;
    // sphericalDirection(degToRad(angle), 0) (common.cpp:270-281; degToRad is value * (M_PI / 180.0f) in double,
    // common.h:218), sin / cos evaluated in fp64 and rounded
    const float theta = (float)((double)angle_deg * (3.14159265358979323846 / (double)180.0f));
    const float st = (float)std::sin((double)theta), ct = (float)std::cos((double)theta);
    const float sp = (float)std::sin(0.0), cp = (float)std::cos(0.0);
    t.wi[0] = st * cp;
    t.wi[1] = st * sp;
    t.wi[2] = ct;
    t.first_draw = first_draw;
    t.n = n;
    if (int rc = q_alloc(c, bufs, &t.lum, (size_t)n)) return rc;
    nh_disney::nh::launch_ttest_bsdf(t, c->stream);
    HIP_TRY(c, hipGetLastError());
    if (int rc = reduce_moments(c, bufs, t.lum, n, mean, variance)) return rc;
    if (luminance) HIP_TRY(c, hipMemcpy(luminance, t.lum, (size_t)n * sizeof(float), hipMemcpyDeviceToHost));
    return NH_OK;
}

int nh_test_run(int device, const char *path, uint64_t seed, nh_test_result *results, int32_t cap,
                int32_t *n_results) {
    if (!path || !n_results || cap < 0 || (cap > 0 && !results)) {
        nh::set_host_error("nh_test_run: invalid argument");
        return NH_ERR_INVALID;
    }
    *n_results = 0;
    struct Run {  // everything the run holds, released on every return
        nh_test *test = nullptr;
        nh_ctx *ctx = nullptr;
        nh_scene *scene = nullptr;
        nh_bvh *bvh = nullptr;
        void drop_scene() {
            if (bvh) nh_bvh_free(bvh);
            if (scene) nh_scene_free(scene);
            bvh = nullptr;
            scene = nullptr;
        }
        ~Run() {
            drop_scene();
            if (ctx) nh_destroy(ctx);
            nh_test_free(test);
        }
    } r;
    if (int rc = nh_test_load_xml(path, &r.test)) return rc;
    nh_test_desc td;
    nh_test_get_desc(r.test, &td);
    if (td.type == NH_TEST_CHI2TEST) {
        nh::set_host_error("chi2test is not supported by the HIP path");
        return NH_ERR_UNSUPPORTED;
    }
    if (td.sample_count < 2 || td.sample_count > NH_RADIANCE_QUERY_MAX) {
        nh::set_host_error("nh_test_run: sampleCount outside [2, 2^24]");
        return NH_ERR_INVALID;
    }
    if (nh_create(device, &r.ctx)) {
        nh::set_host_error("cannot create a context on device " + std::to_string(device));
        return NH_ERR_DEVICE;
    }
    const auto ctx_fail = [&](int rc) {
        nh::set_host_error(nh_last_error(r.ctx));
        return rc;
    };
    int32_t total = 0;
    const auto record = [&](double mean, double variance, float reference, float angle) {
        nh_test_result out{};
        out.mean = mean;
        out.variance = variance;
        out.reference = (double)reference;
        out.sample_count = td.sample_count;
        out.angle = angle;
        nh_students_t_test(mean, variance, out.reference, td.sample_count, (double)td.significance_level,
                           (int32_t)td.n_references, &out.accepted, &out.p_value);
        if (total < cap) results[total] = out;
        ++total;
    };
    if (td.n_bsdfs) {
        // ttest.cpp:158-189: every BSDF takes the same angles, the references run on; one `random` for all
        uint64_t first_draw = 0;
        uint32_t ctr = 0;
        for (uint32_t bi = 0; bi < td.n_bsdfs; ++bi)
            for (uint32_t i = 0; i < td.n_references; ++i) {
                if (ctr >= td.n_references) {  // the reference reads past its list here
                    nh::set_host_error("nh_test_run: the references run out before the BSDFs do");
                    return NH_ERR_INVALID;
                }
                if (td.bsdfs[bi].albedo_texture) {
                    nh::set_host_error("nh_test_run: a textured BSDF in a <test> is not supported");
                    return NH_ERR_UNSUPPORTED;
                }
                double mean = 0, variance = 0;
                if (int rc = nh_ttest_bsdf(r.ctx, &td.bsdfs[bi], nullptr, td.angles[i], first_draw, td.sample_count,
                                           &mean, &variance, nullptr))
                    return ctx_fail(rc);
                first_draw += 2 * (uint64_t)td.sample_count;
                record(mean, variance, td.references[ctr++], td.angles[i]);
            }
    } else {
        for (uint32_t i = 0; i < td.n_scenes; ++i) {
            if (int rc = nh_scene_load_xml_index(path, (int32_t)i, &r.scene)) return rc;
            nh_scene_desc sd;
            nh_scene_get_desc(r.scene, &sd);
            if (int rc = nh_bvh_build(&sd, 0, &r.bvh)) return rc;
            nh_bvh_desc bd;
            nh_bvh_get_desc(r.bvh, &bd);
            if (int rc = nh_upload_scene(r.ctx, &sd)) return ctx_fail(rc);
            if (int rc = nh_upload_bvh(r.ctx, &bd)) return ctx_fail(rc);
            if (sd.integrator == NH_INTEGRATOR_PHOTONMAPPER) {  // Integrator::preprocess, map seed 0 as the CLI
                nh_photon_params pp;
                nh_scene_get_photon_params(r.scene, &pp);
                if (int rc = nh_photon_map_build(r.ctx, &pp, 0, 0)) return ctx_fail(rc);
            }
            if (sd.integrator == NH_INTEGRATOR_AV) {
                nh_av_params ap;
                nh_scene_get_av_params(r.scene, &ap);
                if (int rc = nh_set_av_params(r.ctx, &ap)) return ctx_fail(rc);
            }
            double mean = 0, variance = 0;
            if (int rc = nh_ttest_scene(r.ctx, seed, 0, td.sample_count, &mean, &variance, nullptr)) return ctx_fail(rc);
            record(mean, variance, td.references[i], 0.f);
            r.drop_scene();
        }
    }
    *n_results = total;
    return NH_OK;
}

}  // extern "C"
