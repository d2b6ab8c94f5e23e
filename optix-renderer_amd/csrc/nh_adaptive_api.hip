// nh_render of a scene with the adaptive sampler, and the adaptive entry points of the C-ABI (include/nori_hip.h):
// the host side of nh_adaptive.hip's kernels. Per outer sample, a loop of passes -- decide, read how many blocks go
// on, paths, put -- then one merge into the master.
#include <cstdlib>
#include <cstring>

#include "../host/gpu_layout.h"
#include "nh_ctx.h"

namespace {

// pcg32::seed(initstate, initseq) (ext/pcg32/pcg32.h:74-80)
void pcg32_seed(uint64_t initstate, uint64_t initseq, uint64_t &state, uint64_t &inc) {
    const uint64_t mult = 0x5851f42d4c957f2dULL;
    state = 0u;
    inc = (initseq << 1u) | 1u;
    state = state * mult + inc;
    state += initstate;
    state = state * mult + inc;
}

size_t staging_budget() {
    if (const char *e = std::getenv("NH_ADAPTIVE_STAGING_MB")) return (size_t)std::max(1L, std::atol(e)) << 20;
    return NH_ADAPTIVE_STAGING_BYTES;
}

template <typename T>
int ad_alloc(nh_ctx *c, T **p, size_t n) {
    HIP_TRY(c, hipMalloc(reinterpret_cast<void **>(p), std::max<size_t>(n, 1) * sizeof(T)));
    return NH_OK;
}

// Block table, sampler clones (AdaptiveSampler::prepare) and work buffers for the context's image
int adaptive_begin(nh_ctx *c) {
    adaptive_release(c);
    AdaptiveState &a = c->ad;
    const std::vector<int> rank = nh::spiral_rank(c->width, c->height, kAdBlock, a.nbx, a.nby);
    a.n_blocks = a.nbx * a.nby;
    a.h_blocks.assign((size_t)a.n_blocks, int4{});
    std::vector<AdBlock> st((size_t)a.n_blocks);
    for (int by = 0; by < a.nby; ++by)
        for (int bx = 0; bx < a.nbx; ++bx) {
            const int r = rank[(size_t)by * a.nbx + bx], ox = bx * kAdBlock, oy = by * kAdBlock;
            a.h_blocks[r] = make_int4(ox, oy, std::min(kAdBlock, c->width - ox), std::min(kAdBlock, c->height - oy));
            AdBlock &s = st[r];
            std::memset(&s, 0, sizeof(s));
            pcg32_seed((uint64_t)ox, (uint64_t)oy, s.rng_state, s.rng_inc);
            s.old_norm = 10000.f;
            s.head = s.last = -1;
        }
    const size_t nb = (size_t)a.n_blocks;
    int rc;
    if ((rc = ad_alloc(c, &a.blocks, nb)) || (rc = ad_alloc(c, &a.block_rank, nb)) || (rc = ad_alloc(c, &a.active_list, nb)) ||
        (rc = ad_alloc(c, &a.state, nb)) || (rc = ad_alloc(c, &a.counts, (size_t)kAdPassStride)) ||
        (rc = ad_alloc(c, &a.pos, nb * kAdPaths)) || (rc = ad_alloc(c, &a.rad, nb * kAdPaths)) ||
        (rc = ad_alloc(c, &a.jit, nb * kAdPaths)) || (rc = ad_alloc(c, &a.stats, (size_t)4)))
        return rc;
    HIP_TRY(c, hipHostMalloc(reinterpret_cast<void **>(&a.h_count), sizeof(unsigned)));
    HIP_TRY(c, hipMemcpyAsync(a.blocks, a.h_blocks.data(), nb * sizeof(int4), hipMemcpyHostToDevice, c->stream));
    HIP_TRY(c, hipMemcpyAsync(a.block_rank, rank.data(), nb * sizeof(int), hipMemcpyHostToDevice, c->stream));
    HIP_TRY(c, hipMemcpyAsync(a.state, st.data(), nb * sizeof(AdBlock), hipMemcpyHostToDevice, c->stream));
    HIP_TRY(c, hipMemsetAsync(a.stats, 0, 4 * sizeof(unsigned long long), c->stream));
    HIP_TRY(c, hipStreamSynchronize(c->stream));  // (rank and st are locals)
    return NH_OK;
}

// room for `slots` staged images (and their chain entries), the ones already staged kept
int staging_reserve(nh_ctx *c, size_t slots) {
    AdaptiveState &a = c->ad;
    if (slots <= a.slot_cap) return NH_OK;
    const size_t img = kAdImagePx * sizeof(float4), budget = staging_budget();
    if (slots * img > budget)
        return fail(c, "adaptive sampler: the staged block images of one outer sample exceed the staging budget of " +
                           std::to_string(budget >> 20) + " MiB (NH_ADAPTIVE_STAGING_MB)"), NH_ERR_UNSUPPORTED;
    const size_t cap = std::min(std::max(slots, std::max<size_t>(2 * a.slot_cap, 4 * (size_t)a.n_blocks)), budget / img);
    float4 *ns = nullptr;
    int *nn = nullptr;
    HIP_TRY(c, hipMalloc(reinterpret_cast<void **>(&ns), cap * img));
    if (hipMalloc(reinterpret_cast<void **>(&nn), cap * sizeof(int)) != hipSuccess) {
        (void)hipFree(ns);
        return fail(c, "hipMalloc failed for the adaptive staging chain"), NH_ERR_DEVICE;
    }
    hipError_t e = hipSuccess;
    if (a.slot_cap) {
        e = hipMemcpyAsync(ns, a.staging, a.slot_cap * img, hipMemcpyDeviceToDevice, c->stream);
        if (e == hipSuccess) e = hipMemcpyAsync(nn, a.next, a.slot_cap * sizeof(int), hipMemcpyDeviceToDevice, c->stream);
        if (e == hipSuccess) e = hipStreamSynchronize(c->stream);
    }
    if (e != hipSuccess) {
        (void)hipFree(ns);
        (void)hipFree(nn);
        return fail(c, std::string("adaptive staging growth: ") + hipGetErrorString(e)), NH_ERR_DEVICE;
    }
    (void)hipFree(a.staging);
    (void)hipFree(a.next);
    a.staging = ns;
    a.next = nn;
    a.slot_cap = cap;
    return NH_OK;
}

}  // namespace

void adaptive_release(nh_ctx *c) {
    AdaptiveState &a = c->ad;
    (void)hipFree(a.blocks);
    (void)hipFree(a.block_rank);
    (void)hipFree(a.active_list);
    (void)hipFree(a.next);
    (void)hipFree(a.state);
    (void)hipFree(a.counts);
    (void)hipFree(a.pos);
    (void)hipFree(a.rad);
    (void)hipFree(a.jit);
    (void)hipFree(a.staging);
    (void)hipFree(a.stats);
    if (a.h_count) (void)hipHostFree(a.h_count);
    a = AdaptiveState{};
}

int render_adaptive(nh_ctx *c, const nh_render_req *q) {
    AdaptiveState &a = c->ad;
    if (q->blocks || q->n_blocks > 0)
        return fail(c, "adaptive sampler: a render of chosen 32x32 blocks is not supported (its blocks are 4x4 and "
                       "share the master's order)"), NH_ERR_UNSUPPORTED;
    if (c->S.dof)
        return fail(c, "adaptive sampler: a thin-lens camera is not supported (the lens stream's serial ray order "
                       "depends on the passes)"), NH_ERR_UNSUPPORTED;
    if (c->border > kAdMaxBorder)
        return fail(c, "adaptive sampler: reconstruction filters wider than border 2 are not supported"), NH_ERR_UNSUPPORTED;
    if (q->sample_end > NH_ADAPTIVE_MAX_SAMPLES)
        return fail(c, "adaptive sampler: the sample count overflows the int32 path sample index"), NH_ERR_UNSUPPORTED;
    if (q->sample_begin != 0 && q->sample_begin != a.next_sample)
        return fail(c, "adaptive sampler: the sample range must start at 0 or continue the previous render's (the "
                       "blocks' index streams live across calls)"), NH_ERR_STATE;
    if (q->clear) HIP_TRY(c, hipMemsetAsync(c->fb, 0, c->fb_floats * sizeof(float), c->stream));
    if (q->sample_begin == 0) {
        a.next_sample = -1;
        if (int rc = adaptive_begin(c)) return rc;
    }
    a.next_sample = -1;  // (an error below leaves the samplers mid-way: only a fresh start is accepted then)
    AdaptiveLaunch A{};
    A.n_blocks = a.n_blocks;
    A.nbx = a.nbx;
    A.nby = a.nby;
    A.width = c->width;
    A.height = c->height;
    A.border = c->border;
    A.initial_uniform = c->adaptive_initial_uniform;
    A.seed = q->seed;
    A.blocks = a.blocks;
    A.block_rank = a.block_rank;
    A.state = a.state;
    A.active_list = a.active_list;
    A.counts = a.counts;
    A.pos = a.pos;
    A.rad = a.rad;
    A.jit = a.jit;
    A.stats = a.stats;
    A.fb = c->fb;
    A.radius = c->filter.radius;
    A.lookup = c->filter.lookup_factor;
    std::memcpy(A.table, c->filter.table, sizeof(A.table));
    uint64_t passes = 0;
    for (int s = q->sample_begin; s < q->sample_end; ++s) {
        A.s = s;
        HIP_TRY(c, hipMemsetAsync(a.counts, 0, kAdPassStride * sizeof(unsigned), c->stream));
        size_t slots = 0;
        for (int k = 0;; ++k) {
            if (k >= kAdPassStride) return fail(c, "adaptive sampler: a block did not stop at round 1000"), NH_ERR_DEVICE;
            A.k = k;
            A.staging = a.staging;
            A.next = a.next;
            nh_disney::nh::launch_adaptive_decide(A, c->stream);
            HIP_TRY(c, hipGetLastError());
            HIP_TRY(c, hipMemcpyAsync(a.h_count, a.counts + k, sizeof(unsigned), hipMemcpyDeviceToHost, c->stream));
            HIP_TRY(c, hipStreamSynchronize(c->stream));
            const unsigned n = *a.h_count;
            if (n == 0) break;
            if (n > (unsigned)a.n_blocks) return fail(c, "adaptive sampler: active block count out of range"), NH_ERR_DEVICE;
            if (int rc = staging_reserve(c, slots + n)) return rc;
            A.staging = a.staging;
            A.next = a.next;
            A.n_active = (int)n;
            A.slot_base = (int)slots;
            nh_disney::nh::launch_adaptive_paths(c->d_scene, c->tv, A, c->depth, c->stream);
            nh_disney::nh::launch_adaptive_put(A, c->stream);
            HIP_TRY(c, hipGetLastError());
            slots += n;
            ++passes;
        }
        nh_disney::nh::launch_adaptive_merge(A, c->stream);
        HIP_TRY(c, hipGetLastError());
    }
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    if (int e = check_device(c, "nh_render")) return e;
    c->stats.launches_path += passes;
    c->stats.launches_splat += passes + (uint64_t)(q->sample_end - q->sample_begin);
    a.next_sample = q->sample_end;
    return NH_OK;
}

extern "C" {

int nh_get_adaptive_stats(nh_ctx *c, nh_adaptive_stats *out) {
    if (!c || !out) return NH_ERR_INVALID;
    if (!c->ad.stats) return fail(c, "nh_get_adaptive_stats: no adaptive render on this context"), NH_ERR_STATE;
    HIP_TRY(c, hipSetDevice(c->device));
    unsigned long long h[4];
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    HIP_TRY(c, hipMemcpy(h, c->ad.stats, sizeof(h), hipMemcpyDeviceToHost));
    out->total_samples = h[0];
    out->passes = h[1];
    out->max_passes = h[2];
    out->n_blocks = (uint64_t)c->ad.n_blocks;
    return NH_OK;
}

int nh_get_adaptive_variance(nh_ctx *c, float *out, size_t n) {
    if (!c || !out) return NH_ERR_INVALID;
    if (!c->ad.state) return fail(c, "nh_get_adaptive_variance: no adaptive render on this context"), NH_ERR_STATE;
    if (n < (size_t)c->width * (size_t)c->height) return fail(c, "variance destination too small"), NH_ERR_INVALID;
    HIP_TRY(c, hipSetDevice(c->device));
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    std::vector<AdBlock> st((size_t)c->ad.n_blocks);
    HIP_TRY(c, hipMemcpy(st.data(), c->ad.state, st.size() * sizeof(AdBlock), hipMemcpyDeviceToHost));
    // writeVarianceMatrix (adaptive.cpp:172-191): entry (i, j) of m_oldVariance at pixel (offset.y + i, offset.x + j)
    for (size_t r = 0; r < st.size(); ++r) {
        const int4 b = c->ad.h_blocks[r];
        for (int i = 0; i < b.w; ++i)
            for (int j = 0; j < b.z; ++j) out[(size_t)(b.y + i) * c->width + (b.x + j)] = st[r].old_var[i * 4 + j];
    }
    return NH_OK;
}

}  // extern "C"
