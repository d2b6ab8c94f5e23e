// nh_chi2_histogram, nh_chi2_expected and the runner nh_chi2_run of the C-ABI (include/nori_hip.h): the host side of
// nh_chi2.hip's kernels. The statistic itself is host code (host/chi2test.cpp).
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
int c_alloc(nh_ctx *c, std::vector<void *> &owner, T **p, size_t n) {
    void *d = nullptr;
    HIP_TRY(c, hipMalloc(&d, std::max<size_t>(n, 1) * sizeof(T)));
    owner.push_back(d);
    *p = static_cast<T *>(d);
    return NH_OK;
}

int check_table(nh_ctx *c, const char *who, const nh_bsdf *b, int32_t res_theta, int32_t res_phi) {
    if (b->type < NH_BSDF_DIFFUSE || b->type > NH_BSDF_DISNEY) return fail(c, "unknown BSDF type"), NH_ERR_INVALID;
    if (res_theta < 1 || res_phi < 1 || (int64_t)res_theta * res_phi > NH_CHI2_MAX_CELLS)
        return fail(c, std::string(who) + ": the table needs 1 <= res_theta, res_phi and at most " +
                           std::to_string(NH_CHI2_MAX_CELLS) + " cells"), NH_ERR_UNSUPPORTED;
    return NH_OK;
}

// the reference's `pcg32 random` on the host, for the two draws of a test's wi
struct HostPcg {
    uint64_t state = 0x853c49e6748fea9bULL, inc = 0xda3e39cb94b95bdbULL;
    uint32_t next_uint() {
        const uint64_t old = state;
        state = old * 0x5851f42d4c957f2dULL + inc;
        const uint32_t xs = (uint32_t)(((old >> 18u) ^ old) >> 27u), rot = (uint32_t)(old >> 59u);
        return (xs >> rot) | (xs << ((~rot + 1u) & 31u));
    }
    float next_float() {
        const uint32_t u = (next_uint() >> 9) | 0x3f800000u;
        float f;
        std::memcpy(&f, &u, sizeof(f));
        return f - 1.0f;
    }
    void advance(uint64_t delta) {  // pcg32::advance (pcg32.h:131-150)
        uint64_t cur_mult = 0x5851f42d4c957f2dULL, cur_plus = inc, acc_mult = 1u, acc_plus = 0u;
        for (; delta > 0; delta /= 2) {
            if (delta & 1) {
                acc_mult *= cur_mult;
                acc_plus = acc_plus * cur_mult + cur_plus;
            }
            cur_plus = (cur_mult + 1) * cur_plus;
            cur_mult *= cur_mult;
        }
        state = acc_mult * state + acc_plus;
    }
};

}  // namespace

extern "C" {

int nh_chi2_histogram(nh_ctx *c, const nh_bsdf *b, const float *albedo, const float *wi, uint64_t first_draw, int32_t n,
                      int32_t res_theta, int32_t res_phi, double *obs) {
    if (!c) return NH_ERR_INVALID;
    if (!b || !wi || !obs) return fail(c, "nh_chi2_histogram: null argument"), NH_ERR_INVALID;
    if (int rc = check_table(c, "nh_chi2_histogram", b, res_theta, res_phi)) return rc;
    if (n < 1) return fail(c, "nh_chi2_histogram: needs n >= 1 samples"), NH_ERR_INVALID;
    HIP_TRY(c, hipSetDevice(c->device));
    std::vector<void *> bufs;
    Free guard{bufs};
    Chi2Hist h;
    std::memset(&h, 0, sizeof(h));
    if (int rc = query_bsdf_record(c, bufs, b, albedo, h.bsdf, h.albedo)) return rc;
    for (int k = 0; k < 3; ++k) h.wi[k] = wi[k];
    h.first_draw = first_draw;
    h.n = n;
    const int64_t max_lanes = (int64_t)kChi2MaxGroups * kChi2Block;
    h.run = (int)std::max<int64_t>(kChi2MinRun, ((int64_t)n + max_lanes - 1) / max_lanes);
    h.res_theta = res_theta;
    h.res_phi = res_phi;
    const int cells = res_theta * res_phi;
    h.sub_tables = cells * (kChi2Block / 64) <= NH_CHI2_MAX_CELLS ? 1 : 0;
#ifdef NH_AB_CHI2_ONE_TABLE  // cost attribution builds only: one LDS table per workgroup at every size
    h.sub_tables = 0;
#endif
    if (int rc = c_alloc(c, bufs, &h.counts, (size_t)cells)) return rc;
    HIP_TRY(c, hipMemsetAsync(h.counts, 0, (size_t)cells * sizeof(uint32_t), c->stream));
    nh_disney::nh::launch_chi2_histogram(h, c->stream);
    HIP_TRY(c, hipGetLastError());
    std::vector<uint32_t> counts((size_t)cells);
    HIP_TRY(c, hipMemcpyAsync(counts.data(), h.counts, (size_t)cells * sizeof(uint32_t), hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    for (int i = 0; i < cells; ++i) obs[i] = (double)counts[(size_t)i];
    return NH_OK;
}

int nh_chi2_expected(nh_ctx *c, const nh_bsdf *b, const float *albedo, int32_t n_wi, const float *wi, int32_t res_theta,
                     int32_t res_phi, int32_t sample_count, double *exp, uint32_t *evals) {
    if (!c) return NH_ERR_INVALID;
    if (!b || !wi || !exp) return fail(c, "nh_chi2_expected: null argument"), NH_ERR_INVALID;
    if (int rc = check_table(c, "nh_chi2_expected", b, res_theta, res_phi)) return rc;
    const int64_t total = (int64_t)n_wi * res_theta * res_phi;
    if (n_wi < 1 || total > NH_CHI2_EXPECTED_MAX)
        return fail(c, "nh_chi2_expected: needs n_wi >= 1 and n_wi * cells <= 2^20"), NH_ERR_INVALID;
    HIP_TRY(c, hipSetDevice(c->device));
    std::vector<void *> bufs;
    Free guard{bufs};
    Chi2Expected q;
    std::memset(&q, 0, sizeof(q));
    float alb[3];
    if (int rc = query_bsdf_record(c, bufs, b, albedo, q.bsdf, alb)) return rc;
    q.n_wi = n_wi;
    q.res_theta = res_theta;
    q.res_phi = res_phi;
    q.sample_count = sample_count;
    float *d_wi = nullptr;
    if (int rc = c_alloc(c, bufs, &d_wi, 3 * (size_t)n_wi)) return rc;
    if (int rc = c_alloc(c, bufs, &q.exp, (size_t)total)) return rc;
    if (evals)
        if (int rc = c_alloc(c, bufs, &q.evals, (size_t)total)) return rc;
    q.wi = d_wi;
    HIP_TRY(c, hipMemcpyAsync(d_wi, wi, 3 * (size_t)n_wi * sizeof(float), hipMemcpyHostToDevice, c->stream));
    nh_disney::nh::launch_chi2_expected(q, c->stream);
    HIP_TRY(c, hipGetLastError());
    HIP_TRY(c, hipMemcpyAsync(exp, q.exp, (size_t)total * sizeof(double), hipMemcpyDeviceToHost, c->stream));
    if (evals)
        HIP_TRY(c, hipMemcpyAsync(evals, q.evals, (size_t)total * sizeof(uint32_t), hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    return NH_OK;
}

int nh_chi2_run_tables(int device, const char *path, nh_chi2_result *results, int32_t cap, int32_t *n_results,
                       double *tables) {
    if (!path || !n_results || cap < 0 || (cap > 0 && !results)) {
        nh::set_host_error("nh_chi2_run: invalid argument");
        return NH_ERR_INVALID;
    }
    *n_results = 0;
    struct Run {
        nh_test *test = nullptr;
        nh_ctx *ctx = nullptr;
        ~Run() {
            if (ctx) nh_destroy(ctx);
            nh_test_free(test);
        }
    } r;
    if (int rc = nh_test_load_xml(path, &r.test)) return rc;
    nh_test_desc td;
    nh_test_get_desc(r.test, &td);
    if (td.type != NH_TEST_CHI2TEST) {
        nh::set_host_error("nh_chi2_run: the file is not a chi2test (nh_test_run runs a ttest)");
        return NH_ERR_INVALID;
    }
    nh_chi2_params cp;
    nh_test_get_chi2_params(r.test, &cp);
    for (uint32_t bi = 0; bi < td.n_bsdfs; ++bi)
        if (td.bsdfs[bi].albedo_texture) {
            nh::set_host_error("nh_chi2_run: a textured BSDF in a <test> is not supported");
            return NH_ERR_UNSUPPORTED;
        }
    if (cp.test_count < 0 || (int64_t)cp.test_count * td.n_bsdfs > (1 << 16)) {
        nh::set_host_error("nh_chi2_run: testCount outside [0, 2^16 / the number of BSDFs]");
        return NH_ERR_INVALID;
    }
    if (cp.sample_count < 1) {
        nh::set_host_error("nh_chi2_run: sampleCount must be at least 1");
        return NH_ERR_INVALID;
    }
    const int64_t res_theta = cp.resolution, res_phi = 2 * res_theta;  // m_phiResolution (chi2test.cpp:70)
    if (res_theta < 1 || res_theta * res_phi > NH_CHI2_MAX_CELLS) {
        nh::set_host_error("nh_chi2_run: resolution outside [1, 64] (at most " + std::to_string(NH_CHI2_MAX_CELLS) +
                           " cells)");
        return NH_ERR_UNSUPPORTED;
    }
    const int cells = (int)(res_theta * res_phi), n = cp.sample_count, per_bsdf = cp.test_count;
    const int num_tests = per_bsdf * (int)td.n_bsdfs;
    if (num_tests == 0) return NH_OK;  // "Passed 0/0 tests."
    if (nh_create(device, &r.ctx)) {
        nh::set_host_error("cannot create a context on device " + std::to_string(device));
        return NH_ERR_DEVICE;
    }
    const auto ctx_fail = [&](int rc) {
        nh::set_host_error(nh_last_error(r.ctx));
        return rc;
    };
    // every test's wi is known up front: draws T (2 + 2n) and + 1 of the one stream (chi2test.cpp:151-155)
    const uint64_t stride = 2 + 2 * (uint64_t)n;
    std::vector<float> wi(3 * (size_t)num_tests);
    for (int t = 0; t < num_tests; ++t) {
        HostPcg rng;
        rng.advance((uint64_t)t * stride);
        const float cos_theta = rng.next_float();
        const float sin_theta = std::sqrt(std::max((float)0, 1 - cos_theta * cos_theta));
        // sincosf(2.0f * M_PI * u) with the float M_PI; sin / cos evaluated in fp64 and rounded, as nh_ttest_bsdf's wi
        const float phi = 2.0f * 3.14159265358979323846f * rng.next_float();
        const float sin_phi = (float)std::sin((double)phi), cos_phi = (float)std::cos((double)phi);
        wi[3 * (size_t)t] = cos_phi * sin_theta;
        wi[3 * (size_t)t + 1] = sin_phi * sin_theta;
        wi[3 * (size_t)t + 2] = cos_theta;
    }
    std::vector<double> obs((size_t)cells), exp((size_t)per_bsdf * cells);
    const double alpha = (double)td.significance_level;
    int32_t total = 0;
    for (uint32_t bi = 0; bi < td.n_bsdfs; ++bi) {
        if (int rc = nh_chi2_expected(r.ctx, &td.bsdfs[bi], nullptr, per_bsdf, &wi[3 * (size_t)bi * per_bsdf], (int)res_theta,
                                      (int)res_phi, n, exp.data(), nullptr))
            return ctx_fail(rc);
        for (int l = 0; l < per_bsdf; ++l) {
            const int t = (int)bi * per_bsdf + l;
            if (int rc = nh_chi2_histogram(r.ctx, &td.bsdfs[bi], nullptr, &wi[3 * (size_t)t], (uint64_t)t * stride + 2, n,
                                           (int)res_theta, (int)res_phi, obs.data()))
                return ctx_fail(rc);
            const double *e = &exp[(size_t)l * cells];
            nh_chi2_result out{};
            for (int k = 0; k < 3; ++k) out.wi[k] = wi[3 * (size_t)t + k];
            out.sample_count = n;
            out.level = 1.0 - std::pow(1.0 - alpha, 1.0 / num_tests);
            for (int i = 0; i < cells; ++i) {
                out.obs_sum += obs[(size_t)i];
                out.exp_sum += e[i];
            }
            if (int rc = nh_chi2_test(cells, obs.data(), e, n, (double)cp.min_exp_frequency, alpha, num_tests, &out.accepted,
                                      &out.p_value, &out.statistic, &out.dof, &out.pooled_cells, &out.kind))
                return rc;
            if (total < cap) {
                results[total] = out;
                if (tables) {
                    std::memcpy(tables + 2 * (size_t)total * cells, obs.data(), (size_t)cells * sizeof(double));
                    std::memcpy(tables + (2 * (size_t)total + 1) * cells, e, (size_t)cells * sizeof(double));
                }
            }
            ++total;
        }
    }
    *n_results = total;
    return NH_OK;
}

int nh_chi2_run(int device, const char *path, nh_chi2_result *results, int32_t cap, int32_t *n_results) {
    return nh_chi2_run_tables(device, path, results, cap, n_results, nullptr);
}

}  // extern "C"
