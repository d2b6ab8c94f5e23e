// C-ABI device side of the MI355X path_mis hot path (declared in include/nori_hip.h).
//
// One nh_ctx per GPU owns every device allocation: scene records, the GPU BVH, the
// (W+2b)x(H+2b) RGBW master framebuffer and the per-chunk sample records. Rendering
// a sample range launches, per chunk of sample rounds, the path megakernel (one
// thread per (pixel, round)) and the ImageBlock splat gather on one HIP stream.
// This replaces the reference's OptiX state (include/nori/optix/OptixState*.cpp) and the
// CPU render loop (src/utils/render.cpp:232-459) behind the same plugin boundary.
//
// This file: the context's lifetime and the small entry points -- ray and BSDF / emitter queries, synchronize,
// framebuffer, stats, the denoise driver and the RCCL reduce. nh_upload.hip holds the scene and BVH upload,
// nh_pipeline.hip nh_render and the wavefront pipeline; nh_ctx.h is what the three share.
#include <atomic>
#include <cmath>
#include <cstring>

#include "nh_ctx.h"

using nhd::DBsdf;

int query_bsdf_record(nh_ctx *c, std::vector<void *> &owner, const nh_bsdf *b, const float *albedo, DBsdf &o,
                      float alb[3]) {
    std::memset(&o, 0, sizeof(o));
    o.type = b->type;
    o.ar = b->albedo[0]; o.ag = b->albedo[1]; o.ab = b->albedo[2];
    o.alpha = b->alpha; o.int_ior = b->int_ior; o.ext_ior = b->ext_ior; o.ks = b->ks;
    o.kr = b->kd[0]; o.kg = b->kd[1]; o.kb = b->kd[2];
    // no texture table here: tex only selects a Disney BSDF's per-query route (albedo stands in for the lookup)
    o.tex = b->type == NH_BSDF_DISNEY && b->albedo_texture ? 1 : 0;
    for (int k = 0; k < 3; ++k) alb[k] = albedo ? albedo[k] : b->albedo[k];
    if (b->type == NH_BSDF_DISNEY) {
        nhd::DDisney *rec = nullptr;
        const std::vector<nhd::DDisney> recs{disney_record(*b)};
        const std::vector<float> a(alb, alb + 3);
        if (int rc = disney_upload(c, owner, recs, a, &rec)) return rc;
        disney_set_record(o, rec);
    }
    return NH_OK;
}

extern "C" {

const char *nh_last_error(const nh_ctx *ctx) { return ctx ? ctx->err.c_str() : "null context"; }

int nh_get_device_count(int *n) {
    if (!n) return NH_ERR_INVALID;
    int c = 0;
    if (hipGetDeviceCount(&c) != hipSuccess) c = 0;
    *n = c;
    return NH_OK;
}

int nh_create(int device, nh_ctx **out) {
    if (!out) return NH_ERR_INVALID;
    *out = nullptr;
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess || device < 0 || device >= n) return NH_ERR_DEVICE;
    auto *c = new nh_ctx();
    static std::atomic<uint64_t> next_id{1};
    c->id = next_id++;
    c->device = device;
    if (hipSetDevice(device) != hipSuccess || hipStreamCreateWithFlags(&c->stream, hipStreamNonBlocking) != hipSuccess ||
        hipMalloc(&c->counters, kStatShards * kStatStride * sizeof(unsigned long long)) != hipSuccess ||
        hipEventCreateWithFlags(&c->fb_ev, hipEventDisableTiming) != hipSuccess) {
        delete c;
        return NH_ERR_DEVICE;
    }
    (void)hipMemset(c->counters, 0, kStatShards * kStatStride * sizeof(unsigned long long));
    *out = c;
    return NH_OK;
}

void nh_destroy(nh_ctx *c) {
    if (!c) return;
    DeviceGuard guard;
    (void)hipSetDevice(c->device);
    (void)pipeline_drain(c);
    if (c->stream) (void)hipStreamSynchronize(c->stream);
    free_all(c->scene_bufs);
    free_all(c->bvh_bufs);
    (void)hipFree(c->fb);
    (void)hipFree(c->rec);
    c->px.release();
    (void)hipFree(c->pmask);
    (void)hipFree(c->smask);
    (void)hipFree(c->block_rank);
    (void)hipFree(c->staging);
    free_all(c->av_bufs);
    (void)hipFree(c->counters);
    photon_release(c, true);  // (clears the map's record in d_scene: before d_scene goes)
    (void)hipFree(c->d_scene);
    c->d_scene = nullptr;
    for (WfPool &p : c->pools) pool_free(p);
    adaptive_release(c);
    c->comms.reset();  // the communicators go with the last context of their set
    if (c->fb_ev) (void)hipEventDestroy(c->fb_ev);
    if (c->stream) (void)hipStreamDestroy(c->stream);
    delete c;
}

int nh_trace_rays(nh_ctx *c, const nh_ray_soa *r, int32_t n, int32_t any_hit, int32_t traversal, nh_hit_soa *out) {
    if (!c || !r || !out || n < 0) return NH_ERR_INVALID;
    if (!c->has_bvh) return fail(c, "nh_trace_rays: no BVH uploaded"), NH_ERR_STATE;
    if (n == 0) return NH_OK;
    HIP_TRY(c, hipSetDevice(c->device));
    if (int rc_ = pipeline_drain(c)) return rc_;
    std::vector<void *> tmp;
    const float *in[8];
    const float *src[8] = {r->ox, r->oy, r->oz, r->dx, r->dy, r->dz, r->mint, r->maxt};
    int rc;
    for (int i = 0; i < 8; ++i)
        if ((rc = upload(c, tmp, src[i], (size_t)n, &in[i]))) { free_all(tmp); return rc; }
    RayBatch rb{in[0], in[1], in[2], in[3], in[4], in[5], in[6], in[7]};
    HitBatch hb{};
    void *p;
    size_t nn = (size_t)n;
    HIP_TRY(c, hipMalloc(&p, nn)); tmp.push_back(p); hb.hit = (uint8_t *)p;
    HIP_TRY(c, hipMalloc(&p, nn * 4)); tmp.push_back(p); hb.t = (float *)p;
    HIP_TRY(c, hipMalloc(&p, nn * 4)); tmp.push_back(p); hb.u = (float *)p;
    HIP_TRY(c, hipMalloc(&p, nn * 4)); tmp.push_back(p); hb.v = (float *)p;
    HIP_TRY(c, hipMalloc(&p, nn * 4)); tmp.push_back(p); hb.k = (int *)p;
    if (traversal == NH_TRAVERSAL_WIDE && c->tv.wnodes) {
        HIP_TRY(c, hipMalloc(&p, nn * (size_t)c->depth_wide * sizeof(int2)));
        tmp.push_back(p);
        nh::launch_trace_wide(c->d_scene, c->tv, rb, hb, n, any_hit != 0, true, false, (int2 *)p, c->depth_wide,
                              c->counters, c->stream, c->wide_w);
    } else {
        nh::launch_trace(c->d_scene, c->tv, rb, hb, n, any_hit != 0, traversal != NH_TRAVERSAL_REFERENCE, false,
                         c->depth, c->counters, c->stream);
    }
    HIP_TRY(c, hipGetLastError());
    std::vector<int> k(nn);
    HIP_TRY(c, hipMemcpyAsync(out->hit, hb.hit, nn, hipMemcpyDeviceToHost, c->stream));
    if (!any_hit) {
        if (out->t) HIP_TRY(c, hipMemcpyAsync(out->t, hb.t, nn * 4, hipMemcpyDeviceToHost, c->stream));
        if (out->u) HIP_TRY(c, hipMemcpyAsync(out->u, hb.u, nn * 4, hipMemcpyDeviceToHost, c->stream));
        if (out->v) HIP_TRY(c, hipMemcpyAsync(out->v, hb.v, nn * 4, hipMemcpyDeviceToHost, c->stream));
        HIP_TRY(c, hipMemcpyAsync(k.data(), hb.k, nn * 4, hipMemcpyDeviceToHost, c->stream));
    }
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    free_all(tmp);
    if (!any_hit)
        for (size_t i = 0; i < nn; ++i) {
            uint32_t prim = 0xffffffffu, shape = 0xffffffffu;
            if (k[i] >= 0) {
                prim = c->bvh_indices[(size_t)k[i]];
                shape = (uint32_t)(std::upper_bound(c->shape_offset.begin(), c->shape_offset.end(), prim) -
                                   c->shape_offset.begin()) - 1;
            }
            if (out->prim) out->prim[i] = prim;
            if (out->shape) out->shape[i] = shape;
        }
    return NH_OK;
}

int nh_bsdf_query(nh_ctx *c, const nh_bsdf *b, const float *albedo, int32_t mode, int32_t n, const float *wi,
                  const float *wo, const float *sample, float *wo_out, float *value, float *pdf, int32_t *measure) {
    if (!c) return NH_ERR_INVALID;
    if (!b || n < 0 || !wi || !value || !pdf) return fail(c, "nh_bsdf_query: null argument"), NH_ERR_INVALID;
    if (b->type < NH_BSDF_DIFFUSE || b->type > NH_BSDF_DISNEY) return fail(c, "unknown BSDF type"), NH_ERR_INVALID;
    if (mode != NH_BSDF_QUERY_EVAL && mode != NH_BSDF_QUERY_SAMPLE)
        return fail(c, "nh_bsdf_query: unknown mode"), NH_ERR_INVALID;
    if (mode == NH_BSDF_QUERY_EVAL ? !wo : (!sample || !wo_out || !measure))
        return fail(c, "nh_bsdf_query: the mode's arrays are missing"), NH_ERR_INVALID;
    if (n == 0) return NH_OK;
    HIP_TRY(c, hipSetDevice(c->device));
    std::vector<void *> bufs;  // freed on every return
    struct Free {
        std::vector<void *> &v;
        ~Free() { free_all(v); }
    } guard{bufs};
    nh_disney::nh::BsdfQuery q;
    std::memset(&q, 0, sizeof(q));
    if (int rc = query_bsdf_record(c, bufs, b, albedo, q.bsdf, q.albedo)) return rc;
    q.mode = mode;
    q.n = n;
    const size_t sn = (size_t)n;
    if (int rc = upload(c, bufs, wi, 3 * sn, &q.wi)) return rc;
    if (mode == NH_BSDF_QUERY_EVAL) {
        if (int rc = upload(c, bufs, wo, 3 * sn, &q.wo)) return rc;
    } else {
        if (int rc = upload(c, bufs, sample, 2 * sn, &q.sample)) return rc;
    }
    void *out = nullptr;  // wo_out (3n), value (3n), pdf (n), measure (n)
    HIP_TRY(c, hipMalloc(&out, 8 * sn * sizeof(float)));
    bufs.push_back(out);
    float *f = static_cast<float *>(out);
    q.wo_out = f;
    q.value = f + 3 * sn;
    q.pdf = f + 6 * sn;
    q.measure = reinterpret_cast<int *>(f + 7 * sn);
    nh_disney::nh::launch_bsdf_query(q, c->stream);
    HIP_TRY(c, hipGetLastError());
    std::vector<float> host(8 * sn);
    HIP_TRY(c, hipMemcpyAsync(host.data(), out, host.size() * sizeof(float), hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    if (wo_out) std::memcpy(wo_out, host.data(), 3 * sn * sizeof(float));
    std::memcpy(value, host.data() + 3 * sn, 3 * sn * sizeof(float));
    std::memcpy(pdf, host.data() + 6 * sn, sn * sizeof(float));
    if (measure) std::memcpy(measure, host.data() + 7 * sn, sn * sizeof(float));
    return NH_OK;
}

int nh_emitter_query(nh_ctx *c, uint32_t emitter, int32_t mode, int32_t n, const float *ref, const float *sample,
                     float *out) {
    if (!c) return NH_ERR_INVALID;
    const bool photon = mode == NH_EMITTER_QUERY_SAMPLE_PHOTON;  // reads no reference point
    if (n < 0 || (!ref && !photon) || !sample || !out) return fail(c, "nh_emitter_query: null argument"), NH_ERR_INVALID;
    if (mode < NH_EMITTER_QUERY_SAMPLE || mode > NH_EMITTER_QUERY_SAMPLE_PHOTON)
        return fail(c, "nh_emitter_query: unknown mode"), NH_ERR_INVALID;
    if (!c->has_scene) return fail(c, "nh_emitter_query: no scene uploaded"), NH_ERR_STATE;
    if (emitter >= c->h_emitters.size()) return fail(c, "nh_emitter_query: emitter index out of range"), NH_ERR_INVALID;
    const nhd::DEmitter &e = c->h_emitters[emitter];
    if (e.type == NH_EMITTER_AREA && (e.shape < 0 || (size_t)e.shape >= c->h_shapes.size()))
        return fail(c, "nh_emitter_query: area light without a valid shape"), NH_ERR_INVALID;
    if (photon && e.type != NH_EMITTER_AREA)
        return fail(c, "nh_emitter_query: samplePhoton of an emitter that is not an area light is not supported"),
               NH_ERR_UNSUPPORTED;
    const size_t sn = (size_t)n;
    if (mode == NH_EMITTER_QUERY_SAMPLE || photon)  // (the CDF searches of the area and envmap samples index by it)
        for (size_t i = 0; i < (photon ? 4 : 2) * sn; ++i)
            if (!(sample[i] >= 0.f && sample[i] < 1.f))
                return fail(c, "nh_emitter_query: sample outside [0, 1)"), NH_ERR_INVALID;
    if (n == 0) return NH_OK;
    HIP_TRY(c, hipSetDevice(c->device));
    if (int rc_ = pipeline_drain(c)) return rc_;
    std::vector<void *> bufs;  // freed on every return
    struct Free {
        std::vector<void *> &v;
        ~Free() { free_all(v); }
    } guard{bufs};
    // the scene record as nh_upload_scene left it (the device copy the render kernels read exists only once a BVH is
    // uploaded; the emitter functions read no BVH field)
    const nhd::DScene *d_s = nullptr;
    if (int rc = upload(c, bufs, &c->S, 1, &d_s)) return rc;
    nh_disney::nh::EmitterQuery q;
    q.emitter = (int)emitter;
    q.mode = mode;
    q.n = n;
    const size_t in_stride = photon ? 4 : (mode == NH_EMITTER_QUERY_SAMPLE ? 2 : NH_EMITTER_QUERY_IN_STRIDE);
    const size_t out_stride = photon ? NH_EMITTER_QUERY_PHOTON_STRIDE
                                     : (mode == NH_EMITTER_QUERY_SAMPLE ? NH_EMITTER_QUERY_SAMPLE_STRIDE
                                                                        : (mode == NH_EMITTER_QUERY_EVAL ? 3 : 1));
    q.ref = nullptr;
    if (!photon)
        if (int rc = upload(c, bufs, ref, 3 * sn, &q.ref)) return rc;
    if (int rc = upload(c, bufs, sample, in_stride * sn, &q.in)) return rc;
    void *d_out = nullptr;
    HIP_TRY(c, hipMalloc(&d_out, out_stride * sn * sizeof(float)));
    bufs.push_back(d_out);
    q.out = static_cast<float *>(d_out);
    nh_disney::nh::launch_emitter_query(d_s, q, c->stream);
    HIP_TRY(c, hipGetLastError());
    HIP_TRY(c, hipMemcpyAsync(out, d_out, out_stride * sn * sizeof(float), hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    return NH_OK;
}

int nh_medium_query(nh_ctx *c, uint32_t medium, int32_t mode, int32_t n, const float *in, float *out) {
    if (!c) return NH_ERR_INVALID;
    if (n < 0 || !in || !out) return fail(c, "nh_medium_query: null argument"), NH_ERR_INVALID;
    if (mode < NH_MEDIUM_QUERY_FREE_PATH || mode > NH_MEDIUM_QUERY_PHASE_PDF)
        return fail(c, "nh_medium_query: unknown mode"), NH_ERR_INVALID;
    if (!c->has_scene) return fail(c, "nh_medium_query: no scene uploaded"), NH_ERR_STATE;
    if (medium >= (uint32_t)c->S.n_media) return fail(c, "nh_medium_query: medium index out of range"), NH_ERR_INVALID;
    if (n == 0) return NH_OK;
    HIP_TRY(c, hipSetDevice(c->device));
    if (int rc_ = pipeline_drain(c)) return rc_;
    std::vector<void *> bufs;  // freed on every return
    struct Free {
        std::vector<void *> &v;
        ~Free() { free_all(v); }
    } guard{bufs};
    // the scene record as nh_upload_scene left it (as nh_emitter_query: the medium functions read no BVH field)
    const nhd::DScene *d_s = nullptr;
    if (int rc = upload(c, bufs, &c->S, 1, &d_s)) return rc;
    static const size_t kIn[4] = {2, 6, 2, 3}, kOut[4] = {2, 3, 4, 1};
    const size_t sn = (size_t)n, in_stride = kIn[mode], out_stride = kOut[mode];
    nh_disney::nh::MediumQuery q;
    q.medium = (int)medium;
    q.mode = mode;
    q.n = n;
    if (int rc = upload(c, bufs, in, in_stride * sn, &q.in)) return rc;
    void *d_out = nullptr;
    HIP_TRY(c, hipMalloc(&d_out, out_stride * sn * sizeof(float)));
    bufs.push_back(d_out);
    q.out = static_cast<float *>(d_out);
    nh_disney::nh::launch_medium_query(d_s, q, c->stream);
    HIP_TRY(c, hipGetLastError());
    HIP_TRY(c, hipMemcpyAsync(out, d_out, out_stride * sn * sizeof(float), hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    return NH_OK;
}

int nh_synchronize(nh_ctx *c) {
    if (!c) return NH_ERR_INVALID;
    HIP_TRY(c, hipSetDevice(c->device));
    int rc = pipeline_drain(c);
    if (rc) return rc;
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    return check_device(c, "nh_synchronize");
}

int nh_get_framebuffer(nh_ctx *c, float *rgbw, size_t n) {
    if (!c || !rgbw) return NH_ERR_INVALID;
    if (!c->has_scene) return fail(c, "no scene"), NH_ERR_STATE;
    if (n < c->fb_floats) return fail(c, "framebuffer destination too small"), NH_ERR_INVALID;
    HIP_TRY(c, hipSetDevice(c->device));
    int rc = pipeline_drain(c);
    if (rc) return rc;
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    HIP_TRY(c, hipMemcpy(rgbw, c->fb, c->fb_floats * sizeof(float), hipMemcpyDeviceToHost));
    return NH_OK;
}

int nh_framebuffer_device_ptr(nh_ctx *c, void **dptr, size_t *n) {
    if (!c || !dptr || !n) return NH_ERR_INVALID;
    if (!c->has_scene) return fail(c, "no scene"), NH_ERR_STATE;
    // The pipeline advances only inside library calls (the host reads queue counts to enqueue the
    // next bounce): run every submitted chunk to completion first, so a caller that hands the
    // pointer to its own stream or collective (RCCL reduce) reads the finished image.
    HIP_TRY(c, hipSetDevice(c->device));
    if (int rc = pipeline_drain(c)) return rc;
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    *dptr = c->fb;
    *n = c->fb_floats;
    return NH_OK;
}

int nh_get_stats(nh_ctx *c, nh_render_stats *out) {
    if (!c || !out) return NH_ERR_INVALID;
    HIP_TRY(c, hipSetDevice(c->device));
    int rc = pipeline_drain(c);  // kernel times of chunks still in flight
    if (rc) return rc;
    *out = c->stats;
    out->comm_inits = c->stats_comm_inits;
    return NH_OK;
}

int nh_reset_stats(nh_ctx *c) {
    if (!c) return NH_ERR_INVALID;
    HIP_TRY(c, hipSetDevice(c->device));
    int rc = pipeline_drain(c);
    if (rc) return rc;
    std::memset(&c->stats, 0, sizeof(c->stats));
    return NH_OK;
}

// SimpleDenoiser on a device ImageBlock (nh_denoise.hip): `amount` passes, each the raw variance + its
// max / min, then the banded wavefront schedule of the in-place row-major sweep. Scratch is per call.
static int run_denoise(nh_ctx *c, float *fb, int W, int H, int bs, const nh_denoiser *p) {
    if (!p || p->type != NH_DENOISER_SIMPLE) return fail(c, "denoise: type must be NH_DENOISER_SIMPLE"), NH_ERR_INVALID;
    // SimpleDenoiser's constructor clamps (simple.cpp:15-24): anything outside is not a reference configuration
    if (!(p->sigma_d >= 1e-4f && p->sigma_d <= 10.f) || !(p->sigma_vr >= 1e-4f && p->sigma_vr <= 10.f) ||
        p->range < 0 || p->range > 50 || p->amount < 1 || p->amount > 10)
        return fail(c, "denoise: parameters outside SimpleDenoiser's clamps"), NH_ERR_INVALID;
    if (W <= 0 || H <= 0 || bs < 0) return fail(c, "denoise: empty image"), NH_ERR_INVALID;
    const int r = p->range, cols = W + 2 * bs;
    // g_sigma (simple.cpp:136-139) depends only on the squared pixel distance: the reference's float expf per
    // distance, tabulated
    std::vector<float> g((size_t)2 * r * r + 1);
    for (size_t d = 0; d < g.size(); ++d) g[d] = std::exp((float)-(int)d / 2.f / p->sigma_d / p->sigma_d);
    std::vector<void *> tmp;
    struct Free {
        std::vector<void *> &v;
        ~Free() { free_all(v); }
    } guard{tmp};
    float4 *B = nullptr;
    float *var = nullptr, *dg = nullptr;
    unsigned *minmax = nullptr;
    HIP_TRY(c, hipMalloc(&B, (size_t)W * H * sizeof(float4)));
    tmp.push_back(B);
    HIP_TRY(c, hipMalloc(&var, (size_t)W * H * sizeof(float)));
    tmp.push_back(var);
    HIP_TRY(c, hipMalloc(&dg, g.size() * sizeof(float)));
    tmp.push_back(dg);
    HIP_TRY(c, hipMalloc(&minmax, 2 * sizeof(unsigned)));
    tmp.push_back(minmax);
    HIP_TRY(c, hipMemcpyAsync(dg, g.data(), g.size() * sizeof(float), hipMemcpyHostToDevice, c->stream));
    float4 *F = reinterpret_cast<float4 *>(fb) + (size_t)bs * cols + bs;
    // schedule: bands of BH rows start (r+1) BH wavefront steps apart; a launch runs `chunk` steps of each
    // band in flight; band w's chunk k runs in launch w lag + k, lag = ceil((skew - 1) / chunk) + 1, so the
    // band above has finished every step this chunk reads before the launch starts
    const int BH = nh::denoise_band_rows();
    const int n_bands = (H + BH - 1) / BH, skew = BH * (r + 1);
    const int chunk = std::max(1, skew / 4);
    const int lag = (skew - 1 + chunk - 1) / chunk + 1;
    const int k_max = ((r + 1) * (BH - 1) + W + chunk - 1) / chunk;
    const int n_launch = (n_bands - 1) * lag + k_max;
    // LDS tile of a chunk's window (input + denoised pixels): rows BH + 2r, columns chunk + (r+1)(BH-1) + 2r
    const size_t tile_rows = (size_t)std::min(H, BH + 2 * r);
    const size_t tile_cols = (size_t)std::min(W, chunk + (r + 1) * (BH - 1) + 2 * r);
    size_t tile_bytes = 2 * tile_rows * tile_cols * sizeof(float4);
    // the tile plus the kernel's static LDS must fit one workgroup's LDS (and the 64 KiB of dynamic LDS a
    // launch may request without raising the function's attribute)
    int lds_per_block = 0;
    HIP_TRY(c, hipDeviceGetAttribute(&lds_per_block, hipDeviceAttributeMaxSharedMemoryPerBlock, c->device));
    const size_t static_lds = nh::denoise_tile_static_lds();
    if (tile_bytes > 64 * 1024 || tile_bytes + static_lds > (size_t)lds_per_block || chunk > nh::denoise_max_chunk() ||
        std::getenv("NH_DENOISE_NO_TILE"))
        tile_bytes = 0;
    hipEvent_t e0, e1;
    HIP_TRY(c, hipEventCreate(&e0));
    HIP_TRY(c, hipEventCreate(&e1));
    HIP_TRY(c, hipEventRecord(e0, c->stream));
    uint64_t launches = 0;
    for (int pass = 0; pass < p->amount; ++pass) {
        DenoiseLaunch P{};
        const bool even = (pass & 1) == 0;
        P.src = even ? F : B;
        P.src_stride = even ? cols : W;
        P.dst = even ? B : F;
        P.dst_stride = even ? W : cols;
        P.width = W;
        P.height = H;
        P.range = r;
        P.sigma_vr = p->sigma_vr;
        P.g = dg;
        P.var = var;
        P.minmax = minmax;
        P.lag = lag;
        P.chunk = chunk;
        HIP_TRY(c, hipMemsetD32Async(reinterpret_cast<hipDeviceptr_t>(minmax), 0, 1, c->stream));
        HIP_TRY(c, hipMemsetD32Async(reinterpret_cast<hipDeviceptr_t>(minmax + 1), 0x7f800000, 1, c->stream));
        nh::launch_denoise_variance(P, c->stream);
        launches += 1;
        for (int L = 0; L < n_launch; ++L) {
            const int w_lo = std::max(0, (L - k_max + 1 + lag - 1) / lag), w_hi = std::min(n_bands - 1, L / lag);
            if (w_hi < w_lo) continue;
            P.band_first = w_lo;
            nh::launch_denoise_band(P, L, w_hi - w_lo + 1, tile_bytes, c->stream);
            ++launches;
        }
    }
    if (p->amount & 1) {  // the last pass wrote the scratch image
        nh::launch_denoise_copy(B, W, F, cols, W, H, c->stream);
        ++launches;
    }
    HIP_TRY(c, hipEventRecord(e1, c->stream));
    HIP_TRY(c, hipGetLastError());
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    float ms = 0.f;
    (void)hipEventElapsedTime(&ms, e0, e1);
    (void)hipEventDestroy(e0);
    (void)hipEventDestroy(e1);
    c->stats.kernel_ms_denoise += ms;
    c->stats.launches_denoise += launches;
    return NH_OK;
}

int nh_denoise(nh_ctx *c, const nh_denoiser *params) {
    if (!c || !params) return NH_ERR_INVALID;
    if (!c->has_scene) return fail(c, "no scene"), NH_ERR_STATE;
    HIP_TRY(c, hipSetDevice(c->device));
    if (int rc = pipeline_drain(c)) return rc;
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    return run_denoise(c, c->fb, c->width, c->height, c->border, params);
}

int nh_denoise_image(nh_ctx *c, float *rgbw, int32_t width, int32_t height, int32_t border,
                     const nh_denoiser *params) {
    if (!c || !rgbw || !params || width <= 0 || height <= 0 || border < 0) return NH_ERR_INVALID;
    HIP_TRY(c, hipSetDevice(c->device));
    if (int rc = pipeline_drain(c)) return rc;
    const size_t n = 4 * (size_t)(width + 2 * border) * (size_t)(height + 2 * border);
    float *d = nullptr;
    HIP_TRY(c, hipMalloc(&d, n * sizeof(float)));
    std::vector<void *> own{d};
    struct Free {
        std::vector<void *> &v;
        ~Free() { free_all(v); }
    } guard{own};
    HIP_TRY(c, hipMemcpyAsync(d, rgbw, n * sizeof(float), hipMemcpyHostToDevice, c->stream));
    if (int rc = run_denoise(c, d, width, height, border, params)) return rc;
    HIP_TRY(c, hipMemcpy(rgbw, d, n * sizeof(float), hipMemcpyDeviceToHost));
    return NH_OK;
}

int nh_reduce_framebuffers(nh_ctx **ctxs, int32_t n, int32_t root) {
    if (!ctxs || n <= 0 || root < 0 || root >= n) return NH_ERR_INVALID;
    DeviceGuard guard;
    for (int i = 0; i < n; ++i)
        if (!ctxs[i] || !ctxs[i]->has_scene || ctxs[i]->fb_floats != ctxs[0]->fb_floats) return NH_ERR_INVALID;
    for (int i = 0; i < n; ++i) {
        (void)hipSetDevice(ctxs[i]->device);
        if (pipeline_drain(ctxs[i])) return NH_ERR_DEVICE;
    }
    // one communicator clique per set of contexts, reused across calls (ncclCommInitAll costs far more
    // than the reduce of a framebuffer); any change of members or order builds a new one
    std::vector<uint64_t> ids(n);
    for (int i = 0; i < n; ++i) ids[i] = ctxs[i]->id;
    std::shared_ptr<CommSet> cs = ctxs[0]->comms;
    if (!cs || cs->ids != ids) {
        for (int i = 0; i < n; ++i) ctxs[i]->comms.reset();
        cs = std::make_shared<CommSet>();
        cs->ids = ids;
        cs->devices.resize(n);
        cs->comms.resize(n);
        for (int i = 0; i < n; ++i) cs->devices[i] = ctxs[i]->device;
        if (ncclCommInitAll(cs->comms.data(), n, cs->devices.data()) != ncclSuccess) {
            cs->comms.clear();
            ctxs[root]->err = "ncclCommInitAll failed";
            return NH_ERR_DEVICE;
        }
        for (int i = 0; i < n; ++i) ctxs[i]->comms = cs;
        ctxs[root]->stats_comm_inits++;
    }
    ncclResult_t r = ncclGroupStart();
    for (int i = 0; i < n && r == ncclSuccess; ++i) {
        (void)hipSetDevice(ctxs[i]->device);
        r = ncclReduce(ctxs[i]->fb, ctxs[i]->fb, ctxs[i]->fb_floats, ncclFloat, ncclSum, root, cs->comms[i],
                       ctxs[i]->stream);
    }
    const ncclResult_t g = ncclGroupEnd();
    if (r == ncclSuccess) r = g;
    for (int i = 0; i < n; ++i) {
        (void)hipSetDevice(ctxs[i]->device);
        (void)hipStreamSynchronize(ctxs[i]->stream);
    }
    if (r != ncclSuccess) {
        ctxs[root]->err = std::string("ncclReduce failed: ") + ncclGetErrorString(r);
        for (int i = 0; i < n; ++i) ctxs[i]->comms.reset();
        return NH_ERR_DEVICE;
    }
    return NH_OK;
}

}  // extern "C"
