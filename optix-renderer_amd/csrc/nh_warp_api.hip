// nh_warp_query, nh_warp_histogram, nh_warp_expected and the runner nh_warp_run of the C-ABI (include/nori_hip.h): the
// host side of nh_warp.hip's kernels. The slider maps and argument checks are host code
// (host/warptest.cpp), the statistic is nh_chi2_test (host/chi2test.cpp).
#include <cmath>
#include <cstring>

#include "../host/nh_host.h"
#include "nh_ctx.h"

namespace {

struct Free {
    std::vector<void *> &v;
    ~Free() { free_all(v); }
};

template <typename T>
int w_alloc(nh_ctx *c, std::vector<void *> &owner, T **p, size_t n) {
    void *d = nullptr;
    HIP_TRY(c, hipMalloc(&d, std::max<size_t>(n, 1) * sizeof(T)));
    owner.push_back(d);
    *p = static_cast<T *>(d);
    return NH_OK;
}

// a refusal's message goes to the context when there is one and to nh_host_last_error in any case, so that the checks
// can be exercised without a device
int refuse(nh_ctx *c, int rc, const std::string &msg) {
    fail(c, msg);
    nh::set_host_error(msg);
    return rc;
}

// the checks every entry point shares, then the kernels' record of the test. The microfacet BRDF of warptest.cpp:177-185:
// alpha = parameter, kd = 0, so ks = 1 - kd.maxCoeff() = 1, microfacet.cpp's default indices of refraction
int warp_spec(nh_ctx *c, const char *who, int32_t type, float parameter, const float *wi, WarpSpec &w) {
    std::string msg;
    if (int rc = nh::warp_check_type(who, type, parameter, msg)) return refuse(c, rc, msg);
    if (type == NH_WARP_MICROFACET_BRDF && !wi) return refuse(c, NH_ERR_INVALID, std::string(who) + ": the microfacet BRDF needs wi");
    std::memset(&w, 0, sizeof(w));
    w.type = type;
    w.parameter = parameter;
    if (type == NH_WARP_MICROFACET_BRDF) {
        for (int k = 0; k < 3; ++k) w.wi[k] = wi[k];
        w.bsdf.type = NH_BSDF_MICROFACET;
        w.bsdf.alpha = parameter;
        w.bsdf.int_ior = 1.5046f;
        w.bsdf.ext_ior = 1.000277f;
        w.bsdf.ks = 1.f;
    }
    return NH_OK;
}

}  // namespace

extern "C" {

int nh_warp_query(nh_ctx *c, int32_t type, float parameter, const float *wi, int32_t mode, int32_t n, const float *in,
                  float *out) {
    WarpQuery q;
    std::memset(&q, 0, sizeof(q));
    if (int rc = warp_spec(c, "nh_warp_query", type, parameter, wi, q.w)) return rc;
    if (mode != NH_WARP_QUERY_SAMPLE && mode != NH_WARP_QUERY_PDF) return refuse(c, NH_ERR_INVALID, "nh_warp_query: unknown mode");
    if (n < 0 || !in || !out) return refuse(c, NH_ERR_INVALID, "nh_warp_query: null argument");
    if (!c) return refuse(c, NH_ERR_INVALID, "nh_warp_query: null context");
    if (n == 0) return NH_OK;
    HIP_TRY(c, hipSetDevice(c->device));
    std::vector<void *> bufs;
    Free guard{bufs};
    const size_t sn = (size_t)n, n_out = mode == NH_WARP_QUERY_SAMPLE ? 4 * sn : sn;
    q.mode = mode;
    q.n = n;
    if (int rc = upload(c, bufs, in, 3 * sn, &q.in)) return rc;
    if (int rc = w_alloc(c, bufs, &q.out, n_out)) return rc;
    nh_disney::nh::launch_warp_query(q, c->stream);
    HIP_TRY(c, hipGetLastError());
    HIP_TRY(c, hipMemcpyAsync(out, q.out, n_out * sizeof(float), hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    return NH_OK;
}

int nh_warp_histogram(nh_ctx *c, int32_t type, float parameter, const float *wi, uint64_t first_draw, int32_t draw_order,
                      int32_t n, int32_t xres, int32_t yres, double *obs, uint32_t *nan_points) {
    WarpHist h;
    std::memset(&h, 0, sizeof(h));
    std::string msg;
    if (int rc = warp_spec(c, "nh_warp_histogram", type, parameter, wi, h.w)) return rc;
    if (int rc = nh::warp_check_table("nh_warp_histogram", xres, yres, msg)) return refuse(c, rc, msg);
    if (n < 1) return refuse(c, NH_ERR_INVALID, "nh_warp_histogram: needs n >= 1 points");
    if (draw_order != NH_LENS_DRAWS_RTL && draw_order != NH_LENS_DRAWS_LTR)
        return refuse(c, NH_ERR_INVALID, "nh_warp_histogram: draw_order is NH_LENS_DRAWS_RTL or NH_LENS_DRAWS_LTR");
    if (!obs) return refuse(c, NH_ERR_INVALID, "nh_warp_histogram: null argument");
    if (!c) return refuse(c, NH_ERR_INVALID, "nh_warp_histogram: null context");
    HIP_TRY(c, hipSetDevice(c->device));
    std::vector<void *> bufs;
    Free guard{bufs};
    h.first_draw = first_draw;
    h.n = n;
    const int64_t max_lanes = (int64_t)kChi2MaxGroups * kChi2Block;
    h.run = (int)std::max<int64_t>(kChi2MinRun, ((int64_t)n + max_lanes - 1) / max_lanes);
    h.xres = xres;
    h.yres = yres;
    h.rtl = draw_order == NH_LENS_DRAWS_RTL ? 1 : 0;
    const int cells = xres * yres;
    h.sub_tables = cells * (kChi2Block / 64) <= NH_CHI2_MAX_CELLS ? 1 : 0;
    uint32_t *d_counts = nullptr;  // the table, then the NaN tally
    if (int rc = w_alloc(c, bufs, &d_counts, (size_t)cells + 1)) return rc;
    h.counts = d_counts;
    h.nan_points = d_counts + cells;
    HIP_TRY(c, hipMemsetAsync(d_counts, 0, ((size_t)cells + 1) * sizeof(uint32_t), c->stream));
    nh_disney::nh::launch_warp_histogram(h, c->stream);
    HIP_TRY(c, hipGetLastError());
    std::vector<uint32_t> counts((size_t)cells + 1);
    HIP_TRY(c, hipMemcpyAsync(counts.data(), d_counts, counts.size() * sizeof(uint32_t), hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    for (int i = 0; i < cells; ++i) obs[i] = (double)counts[(size_t)i];
    if (nan_points) *nan_points = counts[(size_t)cells];
    return NH_OK;
}

int nh_warp_expected(nh_ctx *c, int32_t type, float parameter, const float *wi, int32_t xres, int32_t yres,
                     int32_t sample_count, double *exp, uint32_t *evals) {
    WarpExpected q;
    std::memset(&q, 0, sizeof(q));
    std::string msg;
    if (int rc = warp_spec(c, "nh_warp_expected", type, parameter, wi, q.w)) return rc;
    if (int rc = nh::warp_check_table("nh_warp_expected", xres, yres, msg)) return refuse(c, rc, msg);
    if (!exp) return refuse(c, NH_ERR_INVALID, "nh_warp_expected: null argument");
    if (!c) return refuse(c, NH_ERR_INVALID, "nh_warp_expected: null context");
    HIP_TRY(c, hipSetDevice(c->device));
    std::vector<void *> bufs;
    Free guard{bufs};
    q.xres = xres;
    q.yres = yres;
    // warptest.cpp:531-537: double scale = sampleCount, times 1, 4 or 4 * M_PI with the float M_PI
    q.scale = (double)sample_count;
    if (type == NH_WARP_DISK) q.scale *= 4;
    else if (type != NH_WARP_NONE) q.scale *= (double)(4 * 3.14159265358979323846f);
    const size_t cells = (size_t)xres * yres;
    if (int rc = w_alloc(c, bufs, &q.exp, cells)) return rc;
    if (evals)
        if (int rc = w_alloc(c, bufs, &q.evals, cells)) return rc;
    nh_disney::nh::launch_warp_expected(q, c->stream);
    HIP_TRY(c, hipGetLastError());
    HIP_TRY(c, hipMemcpyAsync(exp, q.exp, cells * sizeof(double), hipMemcpyDeviceToHost, c->stream));
    if (evals) HIP_TRY(c, hipMemcpyAsync(evals, q.evals, cells * sizeof(uint32_t), hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    for (size_t i = 0; i < cells; ++i)
        if (exp[i] < 0) return refuse(c, NH_ERR_INVALID, "The Pdf() function returned negative values!");  // :548-549
    return NH_OK;
}

int nh_warp_run(int device, int32_t type, float parameter_slider, float angle_slider, int32_t draw_order, int32_t xres,
                int32_t yres, int32_t sample_count, nh_chi2_result *result, double *tables) {
    if (!result) {
        nh::set_host_error("nh_warp_run: null argument");
        return NH_ERR_INVALID;
    }
    float parameter = 0.f, wi[3] = {0.f, 0.f, 0.f};
    if (int rc = nh_warp_map_parameter(type, parameter_slider, &parameter)) return rc;
    const bool has_wi = type == NH_WARP_MICROFACET_BRDF || type == NH_WARP_ISO_PHASE || type == NH_WARP_ANISO_PHASE;
    if (has_wi)
        if (int rc = nh_warp_wi(angle_slider, wi)) return rc;
    if (xres == 0 && yres == 0 && sample_count == 0) {  // warptest.cpp:440-447
        xres = yres = 51;
        if (type != NH_WARP_NONE && type != NH_WARP_DISK) xres *= 2;
        sample_count = 1000 * xres * yres;
    }
    std::string msg;
    if (int rc = nh::warp_check_type("nh_warp_run", type, parameter, msg)) return nh::set_host_error(msg), rc;
    if (int rc = nh::warp_check_table("nh_warp_run", xres, yres, msg)) return nh::set_host_error(msg), rc;
    if (sample_count < 1) {
        nh::set_host_error("nh_warp_run: needs sample_count >= 1 (or xres = yres = sample_count = 0)");
        return NH_ERR_INVALID;
    }
    if (draw_order != NH_LENS_DRAWS_RTL && draw_order != NH_LENS_DRAWS_LTR) {
        nh::set_host_error("nh_warp_run: draw_order is NH_LENS_DRAWS_RTL or NH_LENS_DRAWS_LTR");
        return NH_ERR_INVALID;
    }
    struct Run {
        nh_ctx *ctx = nullptr;
        ~Run() {
            if (ctx) nh_destroy(ctx);
        }
    } r;
    if (nh_create(device, &r.ctx)) {
        nh::set_host_error("cannot create a context on device " + std::to_string(device));
        return NH_ERR_DEVICE;
    }
    const auto ctx_fail = [&](int rc) {
        nh::set_host_error(nh_last_error(r.ctx));
        return rc;
    };
    const int cells = xres * yres;
    std::vector<double> obs((size_t)cells), exp((size_t)cells);
    if (int rc = nh_warp_histogram(r.ctx, type, parameter, wi, 0, draw_order, sample_count, xres, yres, obs.data(), nullptr))
        return ctx_fail(rc);
    if (int rc = nh_warp_expected(r.ctx, type, parameter, wi, xres, yres, sample_count, exp.data(), nullptr))
        return ctx_fail(rc);
    nh_chi2_result out{};
    for (int k = 0; k < 3; ++k) out.wi[k] = wi[k];
    out.sample_count = sample_count;
    const double alpha = (double)0.01f;  // const float significanceLevel = 0.01f (warptest.cpp:558)
    out.level = 1.0 - std::pow(1.0 - alpha, 1.0);  // the Sidak correction of one test, as nh_chi2_run forms it
    for (int i = 0; i < cells; ++i) {
        out.obs_sum += obs[(size_t)i];
        out.exp_sum += exp[(size_t)i];
    }
    if (int rc = nh_chi2_test(cells, obs.data(), exp.data(), sample_count, 5.0, alpha, 1, &out.accepted, &out.p_value,
                              &out.statistic, &out.dof, &out.pooled_cells, &out.kind))
        return rc;
    *result = out;
    if (tables) {
        std::memcpy(tables, obs.data(), (size_t)cells * sizeof(double));
        std::memcpy(tables + cells, exp.data(), (size_t)cells * sizeof(double));
    }
    return NH_OK;
}

}  // extern "C"
