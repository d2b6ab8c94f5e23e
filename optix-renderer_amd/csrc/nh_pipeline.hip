// nh_render of the C-ABI (include/nori_hip.h) and the wavefront pipeline that runs its chunks. The context is
// nh_ctx.h's.
#include <cmath>
#include <cstdlib>
#include <cstring>
#include <thread>
#include <type_traits>

#include "../host/gpu_layout.h"
#include "nh_ctx.h"

// ============================================================================================
// Wavefront pipeline
//
// nh_render splits its sample rounds into chunks (jobs) and runs each chunk on a path pool:
// camera paths -> {extend, any-hit, shade} per bounce until no path is alive (the tail kernel
// finishes the last few in place) -> ImageBlock splat of the chunk's sample records into the
// master framebuffer. Queue lengths stay on the device (nh_internal.h count slots); the host
// enqueues bounce i+1 before it reads bounce i's counts (2 KB into pinned memory), so the GPU never
// idles on a host round trip, and exactly one empty bounce is enqueued at the end.
//
// The last bounces of a chunk carry few paths whose traversals are long latency chains: a lone
// pool leaves most of the GPU idle there. kPools pools on their own streams overlap that drain
// with the next chunk's full bounces (of the same call or of the next nh_render call: a wavefront
// nh_render returns once every chunk it submitted has started and every running pool is draining;
// anything that reads results -- nh_synchronize, nh_get_framebuffer, nh_get_stats, ... -- first
// runs the pipeline to completion). Splats are enqueued in submission order, each waiting for the
// previous write of the framebuffer, so the master ImageBlock receives chunks in the serial
// reference's order and the image is bit-identical to a one-pool run.
// ============================================================================================

constexpr size_t kWfBytesPerPath = 2 * (16 * 6 + 8 + 1) + 36;  // two buffers + shadow queue

static int pool_alloc(nh_ctx *c, WfPool &p, size_t n, size_t rec_n, size_t staging_f4, bool jit = false) {
    if (!p.stream) {  // the stream is created last: a pool with a stream has all of these
        if (!p.h_counts && hipHostMalloc(reinterpret_cast<void **>(&p.h_counts),
                                         (kRing * 2 * kCountGroup + kCountSlot) * sizeof(unsigned)) != hipSuccess) {
            p.h_counts = nullptr;
            return fail(c, "hipHostMalloc failed"), NH_ERR_DEVICE;
        }
        for (hipEvent_t &e : p.copy_ev)
            if (!e) HIP_TRY(c, hipEventCreateWithFlags(&e, hipEventDisableTiming));
        for (hipEvent_t *e : {&p.ev_begin, &p.ev_path, &p.ev_splat0, &p.ev_splat})
            if (!*e) HIP_TRY(c, hipEventCreate(e));
        if (!p.ev_handoff) HIP_TRY(c, hipEventCreateWithFlags(&p.ev_handoff, hipEventDisableTiming));
        HIP_TRY(c, hipStreamCreateWithFlags(&p.stream, hipStreamNonBlocking));
    }
    if (p.cap < n) {
        free_all(p.bufs);
        p.wf = WfState{};
        p.cap = 0;
        auto alloc = [&](auto *&ptr, size_t count) -> bool {
            void *q = nullptr;
            if (hipMalloc(&q, count * sizeof(*ptr)) != hipSuccess) return false;
            p.bufs.push_back(q);
            ptr = static_cast<std::remove_reference_t<decltype(ptr)>>(q);
            return true;
        };
        WfState &W = p.wf;
        const size_t nq = n + (size_t)(kQueueShards + 2) * 256;  // shard segments round up to whole shade blocks
        bool ok = true;
        for (WfBuf &B : W.buf)
            ok = ok && alloc(B.ray_o, nq) && alloc(B.ray_d, nq) && alloc(B.hit, nq) && alloc(B.rng, nq) &&
                 alloc(B.li, nq) && alloc(B.thr, nq) && alloc(B.pend, nq) && alloc(B.occl, nq);
        ok = ok && alloc(W.sh_o, nq) && alloc(W.sh_d, nq) && alloc(W.sh_slot, nq) && alloc(W.counts, 2 * kCountSlot);
        if (!ok) {
            free_all(p.bufs);
            p.wf = WfState{};
            return fail(c, "hipMalloc failed for wavefront path state"), NH_ERR_DEVICE;
        }
        p.cap = n;
    }
    // the chunk's sample records: owned by whichever pool or tail slot holds the chunk (they move with it)
    if (p.rec_cap < rec_n) {
        (void)hipFree(p.rec);
        p.rec = nullptr;
        p.rec_cap = 0;
        HIP_TRY(c, hipMalloc(&p.rec, rec_n * kRecFloats * sizeof(float)));
        p.rec_cap = rec_n;
    }
    if (jit && p.jit_cap < rec_n) {
        (void)hipFree(p.jit);
        p.jit = nullptr;
        p.jit_cap = 0;
        HIP_TRY(c, hipMalloc(&p.jit, rec_n * sizeof(float2)));
        p.jit_cap = rec_n;
    }
    if (p.staging_cap < staging_f4) {
        (void)hipFree(p.staging);
        p.staging = nullptr;
        p.staging_cap = 0;
        HIP_TRY(c, hipMalloc(&p.staging, staging_f4 * sizeof(float4)));
        p.staging_cap = staging_f4;
    }
    return NH_OK;
}

void pool_free(WfPool &p) {
    free_all(p.bufs);
    (void)hipFree(p.rec);
    (void)hipFree(p.jit);
    (void)hipFree(p.staging);
    (void)hipFree(p.spill);
    if (p.h_counts) (void)hipHostFree(p.h_counts);
    for (hipEvent_t e : p.events) (void)hipEventDestroy(e);
    for (hipEvent_t e : p.copy_ev)
        if (e) (void)hipEventDestroy(e);
    for (hipEvent_t e : {p.ev_begin, p.ev_path, p.ev_splat0, p.ev_splat, p.ev_handoff})
        if (e) (void)hipEventDestroy(e);
    if (p.stream) (void)hipStreamDestroy(p.stream);
    p = WfPool{};
}

static SplatLaunch make_splat(const nh_ctx *c, const float *rec, uint64_t seed, int s0, float4 *staging, int rounds,
                              bool staged) {
    SplatLaunch P{};
    P.staged = staged ? 1 : 0;
    P.fb = c->fb;
    P.width = c->width;
    P.height = c->height;
    P.border = c->border;
    P.reach = (int)std::floor(c->filter.radius + 0.5f);
    P.nbx = c->nbx;
    P.n_rounds = rounds;
    P.n_list = c->px.n_list;
    P.pixel_map = c->px.pixel_map;
    P.block_rank = c->block_rank;
    P.rec = rec;
    P.seed = seed;
    P.s0 = s0;
    P.radius = c->filter.radius;
    P.lookup = c->filter.lookup_factor;
    std::memcpy(P.table, c->filter.table, sizeof(P.table));
    P.blocks = c->px.block_ids;
    P.block_slot = c->px.block_slot;
    P.n_blocks = c->px.n_blocks;
    P.color_slots = c->px.color_slots;
    P.n_color0 = c->px.n_color0;
    P.staging = staging;
    return P;
}

// the splat layout of a chunk starting now: staged pair, or the fused tile splat (NH_SPLAT_FUSED=1)
static bool splat_staged(const nh_ctx *c) {
    return nh::splat_uses_staging(c->border, (int)std::floor(c->filter.radius + 0.5f));
}
// float4 entries of one (round, block) ImageBlock in the splat's staging buffer (0: the fused splat stages nothing)
static size_t block_px(const nh_ctx *c, bool staged) {
    if (!staged) return 0;
    return (size_t)(32 + 2 * c->border) * (size_t)stage_pitch(32 + 2 * c->border);
}

// path pools driven by pipeline_run (NH_POOLS: 1 = no overlap, for A/B and tests). Scenes with mirror or
// dielectric BSDFs get a third pool: their chunks end in tails of discrete chains that survive Russian roulette
// with probability 0.99 per bounce (path_mis.cpp:58-70), 5-6 ms whatever the chunk size, longer than a C1
// chunk's bounce phase; with three pools two tails overlap the next chunk (C1 2744 -> 3321 Msamples/s; C2,
// perf-1M and C5 unchanged). Each pool's stream needs its own hardware queue (GPU_MAX_HW_QUEUES >= 5; with HIP's
// default of 4, two pool streams share one and a tail blocks the other pool's bounces).
static int active_pools(const nh_ctx *c) {
    const char *np = std::getenv("NH_POOLS");
    const int def = c->specular ? NH_DEFAULT_POOLS + 1 : NH_DEFAULT_POOLS;
    return std::max(1, std::min(kPools, np ? std::atoi(np) : def));
}

// asynchronous tails: NH_TAIL_ASYNC=1 (default off until measured faster than in-place tails)
static bool tail_async_enabled() {
    const char *e = std::getenv("NH_TAIL_ASYNC");
    return e && e[0] == '1';
}

// start job j on idle pool p: buffers, traversal choice, initial queue (all n_paths camera paths)
static int pool_start(nh_ctx *c, WfPool &p, const WfJob &job) {
    WfJob j = job;
    j.staged = splat_staged(c);  // the staging below is sized for this layout; the chunk's splat uses the same
    const char *jv = std::getenv("NH_SPLAT_JITTER");
    j.jit = jv && std::strcmp(jv, "stored") == 0;
    const int n_paths = j.rounds * c->px.n_list;
    const size_t staging_f4 = (size_t)j.rounds * c->px.n_blocks * block_px(c, j.staged);  // the chunk's ImageBlocks
    int rc = pool_alloc(c, p, (size_t)n_paths, (size_t)n_paths, staging_f4, j.jit);
    if (rc) return rc;
    // the other pools in use get the same capacity now (idle ones only: nothing of theirs is in
    // flight), so the first render call, not a later one, pays for their allocation
    for (int i = 0; i < active_pools(c); ++i) {
        WfPool &o = c->pools[i];
        if (&o == &p || o.state != WfPool::IDLE) continue;
        if ((rc = pool_alloc(c, o, (size_t)n_paths, (size_t)n_paths, staging_f4, j.jit))) return rc;
    }
    // so do the idle tail slots' record and staging buffers: chunks hand theirs over at a tail hand-off and take the
    // slot's, and a pool that had to grow them later would free and allocate inside the pipeline (hipFree waits
    // for the whole device: a 6-9 ms stall behind the running tails)
    if (active_pools(c) > 1 && tail_async_enabled())
        for (int i = kPools; i < kPools + kTails; ++i) {
            WfPool &o = c->pools[i];
            if (o.state != WfPool::IDLE) continue;
            if ((rc = pool_alloc(c, o, (size_t)kTailCap, (size_t)n_paths, staging_f4, j.jit))) return rc;
        }
    p.job = j;
    WfLaunch &L = p.L;
    L = WfLaunch{};
    L.st = p.wf;
    L.n_paths = n_paths;
    L.n_list = c->px.n_list;
    L.s0 = j.s0;
    L.seed = j.seed;
    L.pixel_list = c->px.pixel_list;
    L.rec = p.rec;
    L.jit = j.jit ? p.jit : nullptr;
    L.counters = c->counters;
    // scenes whose BVH fits in a few KB (the Cornell box: < 1 KB) are traversed from an LDS copy
    const size_t scene_bytes = 16 * (size_t)(c->n_node_f4 + c->n_prim_f4) + 8 * (size_t)c->n_leaves;
    bool small = scene_bytes <= kSmallSceneBytes;
    if (const char *e = std::getenv("NH_LDS_SCENE")) small = small && e[0] != '0';
    if (small) {
        L.small_nodes = c->n_node_f4;
        L.small_leaves = c->n_leaves;
        L.small_prims = c->n_prim_f4;
        // the flat triangles' shading frames staged beside the records (hit_info reads them instead of a
        // normalize + frame construction per hit) while they add little LDS
        L.small_frames = c->n_prim_f4 / 3 <= kSmallFramesMaxPrims;
        if (const char *e = std::getenv("NH_LDS_FRAMES")) L.small_frames = L.small_frames && e[0] != '0';
        // (the counting kernels' any-hit primitive counts follow the reference's test order: its arrangement)
        L.small_image = j.stats && c->small_image_ref ? c->small_image_ref : c->small_image;
        for (int i = 0; i < 5; ++i) L.small_tab[i] = c->small_tab[i];
    }
    const int per_chunk = 256;  // wf_shade's chunk
    const int max_chunks = (n_paths + per_chunk - 1) / per_chunk;
    L.seg_cap = (max_chunks + kQueueShards - 1) / kQueueShards * per_chunk;
    // persistent traversal pays off on deep BVHs (long, divergent traversals); cbox-like scenes
    // traverse faster with one ray per lane
    p.persistent = c->depth > 20;
    if (const char *e = std::getenv("NH_PERSISTENT")) p.persistent = e[0] == '1';
    // the persistent kernels generate pinhole camera rays only (camera_ray<false>: the lens arithmetic spilled their
    // refill code): for a thin-lens scene wf_camera_rays writes bounce 0's rays first (WfLaunch::cam_rays)
    // the persistent kernels walk the 4-wide collapse of the tree (half the dependent node fetches)
    // unless the reference's own visit order was asked for
    p.wide = p.persistent && j.ordered && c->tv.wnodes != nullptr;
    if (const char *e = std::getenv("NH_WIDE")) p.wide = p.wide && e[0] != '0';
    // (the launchers have no wide kernel for the reference's visit order: they would launch nothing)
    if (p.wide && !j.ordered) return fail(c, "wavefront pool: the wide traversal needs an ordered job"), NH_ERR_STATE;
    // both queries of a bounce in one persistent launch (one tail per bounce instead of two) while the tree fits in
    // the 256 MB MALL (perf-1M +10 %, C3 +7 %); past it the two queries' node sets compete for the cache in one
    // grid (C5, 0.8 GB: 22.3 GB of HBM traffic per fused launch vs 6.9 + 12.3 GB split, 15 % slower), so the
    // closest-hit and any-hit launches stay separate. NH_TRACE2=0|1 overrides.
    p.trace2 = p.wide && scene_bytes <= (size_t)256 << 20;
    if (const char *e = std::getenv("NH_TRACE2")) p.trace2 = p.wide && e[0] != '0';
    c->stats.trace_fused = p.trace2 ? 1 : 0;
    // spill words per lane: binary entries are one word, wide entries two (8-B aligned)
    const int spill_words = p.wide ? 2 * c->depth_wide : (c->depth + 1) / 2 * 2;
    if (p.persistent && p.spill_words < spill_words) {
        HIP_TRY(c, hipStreamSynchronize(p.stream));
        (void)hipFree(p.spill);
        p.spill = nullptr;
        p.spill_words = 0;
        HIP_TRY(c, hipMalloc(&p.spill, (size_t)kPersistentBlocks * 128 * spill_words * sizeof(uint32_t)));
        p.spill_words = spill_words;
    }
    // BVHs staged in LDS: one fused bounce kernel instead of extend + any-hit + shade, its output queue
    // sorted by the next hit's BSDF type when the scene mixes BSDF types
    p.fused = small && !p.persistent && c->depth <= 16;
    if (const char *e = std::getenv("NH_FUSED")) p.fused = p.fused && e[0] != '0';
    p.sorted = p.fused && c->n_bsdf_types > 1;
    p.rr = p.fused;
    if (const char *e = std::getenv("NH_RR_AHEAD")) p.rr = p.fused && e[0] != '0';
    // material-sorted shading on deep BVHs is measured slower (C3 1640 -> 1590, C5 1542 -> 1526 Msamples/s:
    // the extra hit read and barriers cost more than the divergence saved): off unless NH_SORT_SHADE=1
    p.shade_sorted = false;
    if (const char *e = std::getenv("NH_SORT_SHADE")) p.shade_sorted = !p.fused && e[0] == '1';
    if (const char *e = std::getenv("NH_SORT")) p.sorted = p.fused && e[0] == '1';
    // the diffuse area-light instantiations of the RR-ahead kernels (near-first traversal, one material class);
    // NH_BOUNCE_TRAITS=0: the general lean kernels (A/B, tests)
    // (their scene tables come from the LDS image: a scene over the table budget takes the general kernels)
    p.trait = p.rr && c->diffuse_area && c->small_tab[0] > 0 && j.ordered && !p.sorted;
    if (const char *e = std::getenv("NH_BOUNCE_TRAITS")) p.trait = p.trait && e[0] != '0';
    c->stats.bounce_traits = p.rr ? (p.trait ? 2 : 1) : 0;
    // bounce 0's candidate masks (first_vertex of the RR-ahead kernels; the counting kernels test every record)
    const char *pm = std::getenv("NH_PRIMARY_MASKS");
    const bool masks = p.rr && c->pmask && !j.stats && !(pm && pm[0] == '0');
    L.pmask = masks ? c->pmask : nullptr;
    L.pmask_nbx = c->nbx;
    c->stats.primary_masks = masks ? 1 : 0;
    // bounce 0's light samples' candidate masks (rr_step of the same kernels): level 2, the per-block words.
    // NH_SHADOW_MASKS=0 or 1: none (level 1, the emitter-side word alone at every bounce, was measured and removed).
    const char *sm = std::getenv("NH_SHADOW_MASKS");
    const bool shadow = p.rr && c->smask && !j.stats && !(sm && (sm[0] == '0' || sm[0] == '1'));
    L.smask = shadow ? c->smask : nullptr;
    c->stats.shadow_masks = shadow ? 2 : 0;
    c->stats.pair_kinds = p.fused && c->pair_kinds && !j.stats ? 1 : 0;
    // flat scenes (nh_upload.hip build_small_image): the non-counting RR-ahead bounce kernels take their queries
    // without a tree walk (trace_flat). The Disney variant's kernels have no such copies.
    const bool flat = p.rr && c->flat_image && c->pair_kinds && !j.stats && !c->disney;
    L.flat = flat ? c->flat_image : nullptr;
    c->stats.flat_trace = flat ? 1 : 0;
    c->stats.any_list = flat ? (uint64_t)c->flat_any_records : 0;  // (the image's any-hit section, read by trace_flat)
    c->stats.fused_bounce = p.fused ? 1 : 0;
    c->stats.node_bytes = p.wide ? 16 * nhd::kWideF4 * (c->wide_w / 4) : 64;
    c->stats.lds_scene = small && !p.persistent && c->depth <= 16 ? 1 : 0;  // the SMALL instantiations (DEPTH 16)
    L.trav_spill = p.spill;
    L.spill_depth = p.spill_words;
    // measured on 16.7M-path chunks: C2 3025 / 3030 / 2692 Msamples/s at 64k / 262k / 1M,
    // bumpy-1M 708 / 744 / 739 / 603 at 64k / 262k / 1M / 3M; 67M-path C4 chunks 2102 / 2206 / 2226 / 2209
    // at 1M / 262k / 131k / 64k
    // at 67M / 16.7M paths with the fused bounce (round 2): C4 3134 / 3229 / 3254 Msamples/s at
    // 262k / 64k / 32k, C2 3680 / 3717 at 262k / 64k, bumpy-1M (persistent traversal) 1404 / 1378 at
    // 262k / 64k -- an LDS-staged bounce stays efficient down to fewer paths than a deep-tree one
    // round 5, with the scratch-free traversal: 64k / 32k / 16k / 8k -- C2 5567 / 5591 / 5577 / 5585, C1 4409 / 4408 /
    // 4459, C4 4891 / 4906 / 4929 Msamples/s (profiles/round5_ab_tail_threshold.txt)
    p.tail_at = p.fused ? std::min<int64_t>(std::max<int64_t>(n_paths / 1024, 8192), 16384)
                        : std::min<int64_t>(std::max<int64_t>(n_paths / 64, 8192), 262144);
    if (const char *e = std::getenv("NH_TAIL")) p.tail_at = std::atoll(e);
    // below this many live paths the pool counts as draining: the next chunk may start beside it
    p.drain_at = std::max<int64_t>(n_paths / 8, p.tail_at);
    HIP_TRY(c, hipEventRecord(p.ev_begin, p.stream));
    // bounce 0 reads the dense camera queue: shard 0 holds all n_paths
    unsigned *h_init = p.h_counts + kRing * 2 * kCountGroup;
    std::memset(h_init, 0, kCountSlot * sizeof(unsigned));
    h_init[0] = (unsigned)n_paths;
    HIP_TRY(c, hipMemcpyAsync(p.wf.counts, h_init, kCountSlot * sizeof(unsigned), hipMemcpyHostToDevice, p.stream));
    p.in_e.assign(1, (uint64_t)n_paths);
    p.in_s.assign(1, 0);
    p.it = 0;
    p.tail = false;
    p.draining = false;
    p.state = WfPool::ENQUEUE;
    return NH_OK;
}

// The chunk (everything but the pool's stream and path state) moves between a pool and a tail slot: its job and
// launch parameters, timing events, pinned count ring, bounce counts, sample records and staging.
static void chunk_swap(WfPool &a, WfPool &b) {
    std::swap(a.h_counts, b.h_counts);
    std::swap(a.copy_ev, b.copy_ev);
    std::swap(a.events, b.events);
    std::swap(a.ev_begin, b.ev_begin);
    std::swap(a.ev_path, b.ev_path);
    std::swap(a.ev_splat0, b.ev_splat0);
    std::swap(a.ev_splat, b.ev_splat);
    std::swap(a.job, b.job);
    std::swap(a.L, b.L);
    std::swap(a.persistent, b.persistent);
    std::swap(a.wide, b.wide);
    std::swap(a.trace2, b.trace2);
    std::swap(a.tail, b.tail);
    std::swap(a.draining, b.draining);
    std::swap(a.fused, b.fused);
    std::swap(a.sorted, b.sorted);
    std::swap(a.rr, b.rr);
    std::swap(a.trait, b.trait);
    std::swap(a.shade_sorted, b.shade_sorted);
    std::swap(a.tail_at, b.tail_at);
    std::swap(a.drain_at, b.drain_at);
    std::swap(a.it, b.it);
    std::swap(a.in_e, b.in_e);
    std::swap(a.in_s, b.in_s);
    std::swap(a.rec, b.rec);
    std::swap(a.rec_cap, b.rec_cap);
    std::swap(a.jit, b.jit);
    std::swap(a.jit_cap, b.jit_cap);
    std::swap(a.staging, b.staging);
    std::swap(a.staging_cap, b.staging_cap);
}

// an idle tail slot for pool p's chunk, or null: the tail then runs in place on the pool's stream. Off with one
// pool (the serialized roofline pass: kernels alone on the GPU) and unless NH_TAIL_ASYNC=1.
static WfPool *free_tail_slot(nh_ctx *c, const WfPool &p, int bound) {
    if (!p.rr || bound > kTailCap || active_pools(c) < 2) return nullptr;
    if (!tail_async_enabled()) return nullptr;
    for (int i = kPools; i < kPools + kTails; ++i)
        if (c->pools[i].state == WfPool::IDLE) return &c->pools[i];
    return nullptr;
}

// Hand the chunk's tail to tail slot T: pack the (at most bound) live paths into T's buffer on the pool's stream,
// move the chunk to T, and run its tail kernel on T's stream once the pack is done. The pool is idle at once:
// stream order keeps its next chunk's kernels behind the pack. The tail's paths, draws and arithmetic are the
// in-place tail's; the chunk's splat still waits for its turn (submission order), so the image is unchanged.
static int pool_handoff(nh_ctx *c, WfPool &p, WfPool &T, int bound, hipEvent_t *ev) {
    int rc = pool_alloc(c, T, (size_t)kTailCap, 0, 0);
    if (rc) return rc;
    HIP_TRY(c, hipMemsetAsync(T.wf.counts, 0, kCountSlot * sizeof(unsigned), p.stream));
    nh::launch_wf_pack_rr(p.L, T.wf.buf[0], T.wf.counts, bound, p.stream);
    HIP_TRY(c, hipGetLastError());
    HIP_TRY(c, hipEventRecord(p.ev_handoff, p.stream));
    chunk_swap(p, T);
    WfLaunch &L = T.L;  // the packed queue: buffer 0 of T, all paths in count shard 0
    L.st = T.wf;
    L.in_q = 0;
    L.cnt_in = T.wf.counts;  // (seg_cap stays the pool's: with one shard it does not address the packed queue, and
                             // it still bounds the pool's own counts the finish reads back)
    HIP_TRY(c, hipStreamWaitEvent(T.stream, p.ev_handoff, 0));
    HIP_TRY(c, hipEventRecord(ev[1], T.stream));
    HIP_TRY(c, hipEventRecord(ev[2], T.stream));
    NH_LAUNCH(c, launch_wf_tail_rr)(c->d_scene, c->tv, L, T.job.ordered, T.job.stats, bound, c->specular,
                          !c->specular && !c->textured, c->normal_mapped, T.trait, T.stream);
    HIP_TRY(c, hipGetLastError());
    HIP_TRY(c, hipEventRecord(ev[3], T.stream));
    T.tail = true;
    T.draining = true;
    T.state = WfPool::SPLAT;
    p.state = WfPool::IDLE;
    c->stats.tails_async++;
    return NH_OK;
}

// NH_COUNT_KERNEL=0: the runtime's device-to-host copy and memset per bounce instead of wf_counts_kernel (A/B)
static bool count_kernel() {
    static const bool on = [] {
        const char *e = std::getenv("NH_COUNT_KERNEL");
        return !(e && e[0] == '0');
    }();
    return on;
}

// after bounce `it`'s appending kernel: its output counts (slot `out`) to the pinned ring, its input slot `in_slot`
// (the next bounce's output) cleared, then the event the host polls before reading the ring
static int count_service(nh_ctx *c, WfPool &p, unsigned *out, unsigned *in_slot, int it) {
    unsigned *h = p.h_counts + (size_t)(it % kRing) * 2 * kCountGroup;
    if (count_kernel()) {
        nh::launch_wf_counts(out, h, 2 * kCountGroup, in_slot, kCountSlot, p.stream);
        HIP_TRY(c, hipGetLastError());
    } else {
        HIP_TRY(c, hipMemcpyAsync(h, out, 2 * kCountGroup * sizeof(unsigned), hipMemcpyDeviceToHost, p.stream));
    }
    HIP_TRY(c, hipEventRecord(p.copy_ev[it % kRing], p.stream));
    return NH_OK;
}

// enqueue bounce p.it (extend, any-hit, then shade or, once few paths are left, the tail kernel)
static int pool_enqueue(nh_ctx *c, WfPool &p) {
    WfLaunch &L = p.L;
    const int it = p.it, in = it & 1;
    unsigned *slot[2] = {p.wf.counts, p.wf.counts + kCountSlot};
    L.in_q = in;
    L.first = it == 0;
    L.cam_rays = it == 0 && p.persistent && c->S.dof ? 1 : 0;
    L.cnt_in = slot[in];
    L.cnt_out = slot[in ^ 1];
    while ((size_t)(it + 1) * 4 > p.events.size()) {
        hipEvent_t e;
        HIP_TRY(c, hipEventCreate(&e));
        p.events.push_back(e);
    }
    hipEvent_t *ev = &p.events[(size_t)it * 4];
    // upper bound of this bounce's live paths: the input of the previous bounce (known: the host
    // has read the counts up to bounce it-2)
    const int bound = (int)p.in_e[it == 0 ? 0 : it - 1];
    const bool ordered = p.job.ordered, stats = p.job.stats;
    // this bounce's output slot must start at zero: bounce 0's is cleared here, every later one by the count
    // kernel of the bounce before it (count_service)
    if (it == 0 || !count_kernel()) HIP_TRY(c, hipMemsetAsync(slot[in ^ 1], 0, kCountSlot * sizeof(unsigned), p.stream));
    HIP_TRY(c, hipEventRecord(ev[0], p.stream));
    if (p.fused) {  // one kernel per bounce: its input already carries the hits (and no pending light samples)
        if (it > 0 && (int64_t)bound <= p.tail_at)
            if (WfPool *T = free_tail_slot(c, p, bound)) return pool_handoff(c, p, *T, bound, ev);
        HIP_TRY(c, hipEventRecord(ev[1], p.stream));
        HIP_TRY(c, hipEventRecord(ev[2], p.stream));
        if (it > 0 && (int64_t)bound <= p.tail_at) {
            if (p.rr)
                NH_LAUNCH(c, launch_wf_tail_rr)(c->d_scene, c->tv, L, ordered, stats, bound, c->specular,
                                                !c->specular && !c->textured, c->normal_mapped, p.trait, p.stream);
            else NH_LAUNCH(c, launch_wf_tail)(c->d_scene, c->tv, L, ordered, stats, false, bound, c->depth, p.stream);
            HIP_TRY(c, hipGetLastError());
            HIP_TRY(c, hipEventRecord(ev[3], p.stream));
            p.tail = true;
            p.draining = true;
            p.state = WfPool::SPLAT;
            return NH_OK;
        }
        if (p.rr) NH_LAUNCH(c, launch_wf_bounce_rr)(c->d_scene, c->tv, L, ordered, stats, p.sorted,
                                                    !c->specular && !c->textured, c->normal_mapped, p.trait, bound,
                                                    p.stream);
        else NH_LAUNCH(c, launch_wf_bounce)(c->d_scene, c->tv, L, ordered, stats, p.sorted, bound, p.stream);
        HIP_TRY(c, hipGetLastError());
        HIP_TRY(c, hipEventRecord(ev[3], p.stream));
        if (int rc_ = count_service(c, p, slot[in ^ 1], slot[in], it)) return rc_;
        if (it == 0) p.it = 1;
        else p.state = WfPool::COUNTS;
        return NH_OK;
    }
    if (it == 0 && L.cam_rays) {
        nh::launch_wf_camera_rays(c->d_scene, L, bound, p.stream);
        HIP_TRY(c, hipGetLastError());
    }
    if (p.trace2) {  // both queries in one launch: its time counts as the extend stage's, the shadow stage's is 0
        nh::launch_wf_trace2(c->d_scene, c->tv, L, ordered, stats, c->wide_w, it == 0 ? bound : 2 * bound, p.stream);
        HIP_TRY(c, hipEventRecord(ev[1], p.stream));
        HIP_TRY(c, hipEventRecord(ev[2], p.stream));
    } else {
        nh::launch_wf_trace(c->d_scene, c->tv, L, ordered, stats, false, p.persistent, p.wide ? c->wide_w : 0, bound,
                            c->depth, p.stream);
        HIP_TRY(c, hipEventRecord(ev[1], p.stream));
        // bounce 0 has no shadow rays (the launch still runs: the kernels read the count on the device)
        nh::launch_wf_trace(c->d_scene, c->tv, L, ordered, stats, true, p.persistent, p.wide ? c->wide_w : 0,
                            it == 0 ? 0 : bound, c->depth, p.stream);
        HIP_TRY(c, hipEventRecord(ev[2], p.stream));
    }
    if (it > 0 && (int64_t)bound <= p.tail_at) {
        NH_LAUNCH(c, launch_wf_tail)(c->d_scene, c->tv, L, ordered, stats, p.wide ? c->wide_w : 0, bound, c->depth, p.stream);
        HIP_TRY(c, hipGetLastError());
        HIP_TRY(c, hipEventRecord(ev[3], p.stream));
        p.tail = true;
        p.draining = true;
        p.state = WfPool::SPLAT;
        return NH_OK;
    }
    NH_LAUNCH(c, launch_wf_shade)(c->d_scene, c->tv, L, p.shade_sorted, c->normal_mapped, bound, p.stream);
    HIP_TRY(c, hipGetLastError());
    HIP_TRY(c, hipEventRecord(ev[3], p.stream));
    if (int rc_ = count_service(c, p, slot[in ^ 1], slot[in], it)) return rc_;
    if (it == 0) {
        p.it = 1;  // bounce 1 is sized by bounce 0's input: enqueue it before reading any count
    } else {
        p.state = WfPool::COUNTS;
    }
    return NH_OK;
}

// counts appended by bounce b (live paths, shadow rays entering bounce b+1)
static int pool_counts(nh_ctx *c, WfPool &p, int b, uint64_t &ne, uint64_t &ns) {
    const unsigned *hp = p.h_counts + (size_t)(b % kRing) * 2 * kCountGroup;
    ne = ns = 0;
    for (int s = 0; s < kQueueShards; ++s) {
        const unsigned ce = hp[s * kCountStride], cs = hp[kCountGroup + s * kCountStride];
        if (ce > (unsigned)p.L.seg_cap || cs > ce) return fail(c, "wavefront queue counts out of range"), NH_ERR_DEVICE;
        ne += ce;
        ns += cs;
    }
    if (ne > (uint64_t)p.L.n_paths) return fail(c, "wavefront queue counts out of range"), NH_ERR_DEVICE;
    return NH_OK;
}

// bounce it-1's counts have arrived: bounce it was enqueued empty (done) or enqueue bounce it+1
static int pool_read(nh_ctx *c, WfPool &p) {
    uint64_t ne, ns;
    int rc = pool_counts(c, p, p.it - 1, ne, ns);
    if (rc) return rc;
    p.in_e.push_back(ne);
    p.in_s.push_back(ns);
    if ((int64_t)ne < p.drain_at) p.draining = true;
    if (ne == 0) {
        p.state = WfPool::SPLAT;
        return NH_OK;
    }
    if (++p.it > 100000) return fail(c, "wavefront did not terminate"), NH_ERR_DEVICE;
    p.state = WfPool::ENQUEUE;
    return NH_OK;
}

// the chunk's paths are enqueued to completion: splat its records into the master ImageBlock
// after the previous write of the framebuffer (called in submission order)
static int pool_splat(nh_ctx *c, WfPool &p) {
    HIP_TRY(c, hipEventRecord(p.ev_path, p.stream));
    if (p.job.stats) nh::launch_count_invalid(p.rec, (size_t)p.L.n_paths, c->counters, p.stream);
    if (c->fb_ev_set) HIP_TRY(c, hipStreamWaitEvent(p.stream, c->fb_ev, 0));
    HIP_TRY(c, hipEventRecord(p.ev_splat0, p.stream));
    SplatLaunch sp = make_splat(c, p.rec, p.L.seed, p.L.s0, p.staging, p.job.rounds, p.job.staged);
    sp.jit = p.L.jit;
    nh::launch_splat(sp, p.stream);
    HIP_TRY(c, hipGetLastError());
    HIP_TRY(c, hipEventRecord(p.ev_splat, p.stream));
    HIP_TRY(c, hipEventRecord(c->fb_ev, p.stream));
    c->fb_ev_set = true;
    c->splat_seq++;
    p.draining = true;
    p.state = WfPool::FINISH;
    return NH_OK;
}

// the chunk has finished on the device: kernel times and byte accounting into the stats
static int pool_finish(nh_ctx *c, WfPool &p) {
    if (p.tail) {  // the last regular bounce's output counts, for the byte accounting below
        uint64_t ne, ns;
        int rc = pool_counts(c, p, p.it - 1, ne, ns);
        if (rc) return rc;
        p.in_e.push_back(ne);
        p.in_s.push_back(ns);
    }
    static const bool trace_counts = std::getenv("NH_TRACE_COUNTS") != nullptr;  // diagnostics: per-bounce profile
    if (trace_counts) {
        float t_all = 0.f;
        (void)hipEventElapsedTime(&t_all, p.ev_begin, p.ev_path);
        std::fprintf(stderr, "[nh] chunk seq %llu: %d paths, %d bounces%s, %.3f ms, live/bounce(ms):",
                     (unsigned long long)p.job.seq, p.L.n_paths, p.it + 1, p.tail ? " (last = tail kernel)" : "", t_all);
        for (int b = 0; b <= p.it && b < (int)p.in_e.size(); ++b) {
            float d = 0.f, e = 0.f, sh = 0.f;
            (void)hipEventElapsedTime(&d, p.events[(size_t)b * 4], p.events[(size_t)b * 4 + 3]);
            (void)hipEventElapsedTime(&e, p.events[(size_t)b * 4], p.events[(size_t)b * 4 + 1]);
            (void)hipEventElapsedTime(&sh, p.events[(size_t)b * 4 + 1], p.events[(size_t)b * 4 + 2]);
            std::fprintf(stderr, " %llu(%.3f e%.3f s%.3f)", (unsigned long long)p.in_e[b], d, e, sh);
        }
        std::fprintf(stderr, "\n");
    }
    for (int b = 0; b <= p.it; ++b) {
        hipEvent_t *ev = &p.events[(size_t)b * 4];
        float a = 0.f, sh = 0.f, d = 0.f;
        (void)hipEventElapsedTime(&a, ev[0], ev[1]);
        (void)hipEventElapsedTime(&sh, ev[1], ev[2]);
        (void)hipEventElapsedTime(&d, ev[2], ev[3]);
        c->stats.kernel_ms_extend += a;
        c->stats.kernel_ms_shadow += sh;
        c->stats.launches_extend++;
        c->stats.launches_shadow++;
        if (p.tail && b == p.it) {
            c->stats.kernel_ms_tail += d;
            c->stats.launches_tail++;
        } else {
            c->stats.kernel_ms_shade += d;
            c->stats.launches_shade++;
        }
    }
    float tp = 0.f, ts = 0.f;
    (void)hipEventElapsedTime(&tp, p.ev_begin, p.ev_path);
    (void)hipEventElapsedTime(&ts, p.ev_splat0, p.ev_splat);
    c->stats.kernel_ms_path += tp;
    c->stats.kernel_ms_splat += ts;
    c->stats.launches_splat++;
    c->stats.samples += (uint64_t)p.L.n_paths;
    // bytes by construction (nh_wavefront.hip), per bounce shaded by wf_shade (the tail kernel's work
    // is not part of this account); extend moves 48 B per ray (16 at bounce 0: no ray load).
    for (size_t b = 0; b + 1 < p.in_e.size(); ++b) {
        const uint64_t shaded = p.in_e[b], nsh = p.in_s[b], ne = p.in_e[b + 1], ns = p.in_s[b + 1];
        // bounce 0: hit in, sample record out. Later: path state (ray_o, ray_d, li, thr 16 B each,
        // rng 8 B) + hit in, the occlusion byte of a queued light sample (its 16-B pending term is
        // read only when unoccluded, not counted); out: survivors' state, the pending term + shadow
        // ray of each queued light sample, the radiance of each finished path
        c->stats.paths_shaded += shaded;
        if (p.fused) {  // wf_bounce: state + hit in (none at bounce 0), survivors' state + hit out, records
            const uint64_t loads = b == 0 ? 0 : shaded * (72 + 16);
            c->stats.shade_state_bytes += loads + (b == 0 ? shaded * 20 : 0) + ne * (72 + 16) + (shaded - ne) * 12;
            continue;
        }
        const uint64_t loads = b == 0 ? shaded * (16 + 20) : shaded * (72 + 16) + nsh * 1;
        c->stats.shade_state_bytes += loads + ne * 72 + ns * (16 + 36) + (shaded - ne) * 12;
        c->stats.extend_queue_bytes += shaded * (b == 0 ? 16 : 48);
        c->stats.shadow_queue_bytes += nsh * 37;  // ray in, path slot, occlusion byte out
    }
    p.state = WfPool::IDLE;
    return NH_OK;
}

// 1 = the event completed, 0 = pending; an error (a fault in the work before the event) goes to err
static int event_done(hipEvent_t e, hipError_t &err) {
    const hipError_t q = hipEventQuery(e);
    if (q == hipSuccess) return 1;
    if (q != hipErrorNotReady) err = q;
    return 0;
}

// Device errors of this context's work so far (HIP errors are sticky per thread): checked at the end of
// nh_render / nh_synchronize, so a fault in a render's kernels is reported by the call that submitted or
// completed them, not by the next unrelated call (a denoise, a framebuffer read).
// Judged from this context's own streams only: the thread's last-error slot may hold another context's (or the
// host application's) error, which must not fail this call nor be cleared by it. Launch errors of this context's
// kernels are caught right after each launch (HIP_TRY(hipGetLastError())); a fault while they run shows in
// the status of their stream.
int check_device(nh_ctx *c, const char *where) {
    hipError_t e = hipSuccess;
    {
        for (WfPool &p : c->pools) {
            if (!p.stream) continue;
            const hipError_t q = hipStreamQuery(p.stream);
            if (q != hipSuccess && q != hipErrorNotReady) { e = q; break; }
        }
    }
    if (e == hipSuccess && c->stream) {
        const hipError_t q = hipStreamQuery(c->stream);
        if (q != hipSuccess && q != hipErrorNotReady) e = q;
    }
    if (e != hipSuccess) {
        c->err = std::string(where) + ": device error in the rendering kernels: " + hipGetErrorString(e);
        return NH_ERR_DEVICE;
    }
    return NH_OK;
}

static void pipeline_reset(nh_ctx *c) {
    for (WfPool &p : c->pools)
        if (p.stream) (void)hipStreamSynchronize(p.stream);
    for (WfPool &p : c->pools) p.state = WfPool::IDLE;
    c->jobs.clear();
    c->splat_seq = c->job_seq;
}

// Drive the pools. all = run until every chunk has finished; otherwise return once every
// submitted chunk has started and every busy pool is draining.
static int pipeline_run(nh_ctx *c, bool all) {
    const int n_pools = active_pools(c);
    c->stats.pools_active = (uint64_t)n_pools;
    for (;;) {
        bool progress = false;
        hipError_t ev_err = hipSuccess;
        for (WfPool &p : c->pools) {
            int rc = NH_OK;
            // a chunk starts on an idle pool once every running chunk is draining (staggered pools)
            bool others_draining = true;
            for (const WfPool &o : c->pools) others_draining = others_draining && (o.state == WfPool::IDLE || o.draining);
            if (p.state == WfPool::IDLE && !c->jobs.empty() && &p - c->pools < n_pools && others_draining) {
                rc = pool_start(c, p, c->jobs.front());
                c->jobs.pop_front();
                progress = true;
            }
            if (!rc && p.state == WfPool::ENQUEUE) {
                rc = pool_enqueue(c, p);
                progress = true;
            }
            if (!rc && p.state == WfPool::COUNTS && event_done(p.copy_ev[(p.it - 1) % kRing], ev_err)) {
                rc = pool_read(c, p);
                progress = true;
            }
            if (!rc && p.state == WfPool::SPLAT && p.job.seq == c->splat_seq) {
                rc = pool_splat(c, p);
                progress = true;
            }
            if (!rc && p.state == WfPool::FINISH && event_done(p.ev_splat, ev_err)) {
                rc = pool_finish(c, p);
                progress = true;
            }
            if (!rc && ev_err != hipSuccess) {
                c->err = std::string("wavefront pipeline: ") + hipGetErrorString(ev_err);
                rc = NH_ERR_DEVICE;
            }
            if (rc) {
                pipeline_reset(c);
                return rc;
            }
        }
        if (c->jobs.empty()) {
            bool idle = true, draining = true;
            for (const WfPool &p : c->pools) {
                idle = idle && p.state == WfPool::IDLE;
                draining = draining && (p.state == WfPool::IDLE || p.draining);
            }
            if (idle || (!all && draining)) return NH_OK;
        }
        if (!progress) std::this_thread::yield();  // waiting on the device
    }
}

int pipeline_drain(nh_ctx *c) {
    int rc = pipeline_run(c, true);
    if (rc) return rc;
    for (WfPool &p : c->pools)
        if (p.stream) HIP_TRY(c, hipStreamSynchronize(p.stream));
    return NH_OK;
}

static int ensure_pixel_list(nh_ctx *c, const nh_render_req *q) {
    std::vector<int32_t> key;
    if (q->n_blocks > 0 && q->blocks) key.assign(q->blocks, q->blocks + q->n_blocks);
    if (c->px.have_list && key == c->px.list_key) return NH_OK;
    if (int rc = pipeline_drain(c)) return rc;  // chunks in flight read the current list
    std::vector<int32_t> blocks = key;
    if (blocks.empty())
        for (int i = 0; i < c->nbx * c->nby; ++i) blocks.push_back(i);
    std::vector<int> list, map((size_t)c->width * c->height, -1);
    for (int32_t bid : blocks) {
        if (bid < 0 || bid >= c->nbx * c->nby) return fail(c, "block id out of range"), NH_ERR_INVALID;
        int bx = bid % c->nbx, by = bid / c->nbx;
        for (int y = by * 32; y < std::min(c->height, by * 32 + 32); ++y)
            for (int x = bx * 32; x < std::min(c->width, bx * 32 + 32); ++x) {
                int pix = y * c->width + x;
                if (map[pix] >= 0) return fail(c, "duplicate block id"), NH_ERR_INVALID;
                map[pix] = (int)list.size();
                list.push_back(pix);
            }
    }
    std::vector<int> slot_map((size_t)c->nbx * c->nby, -1);
    for (size_t i = 0; i < blocks.size(); ++i) slot_map[blocks[i]] = (int)i;
    std::vector<int> color_slots;
    for (int col = 0; col < 2; ++col)
        for (size_t i = 0; i < blocks.size(); ++i)
            if (((blocks[i] % c->nbx + blocks[i] / c->nbx) & 1) == col) color_slots.push_back((int)i);
    // The new list is built whole, every allocation and copy done, before it replaces the context's: on a failure
    // the context keeps the list it had
    PixelList n;
    struct Guard {
        PixelList &l;
        ~Guard() { l.release(); }  // the unfinished list on a failure; the replaced one on success
    } guard{n};
    for (int32_t bid : blocks) n.n_color0 += ((bid % c->nbx + bid / c->nbx) & 1) == 0;
    n.n_blocks = (int)blocks.size();
    n.n_list = (int)list.size();
    n.list_key = key;
    n.have_list = true;
    // (at least one element each: the kernels are handed non-null tables)
    const auto table = [&](int *&dst, const std::vector<int> &src) -> int {
        HIP_TRY(c, hipMalloc(&dst, std::max<size_t>(src.size(), 1) * sizeof(int)));
        if (!src.empty())
            HIP_TRY(c, hipMemcpyAsync(dst, src.data(), src.size() * sizeof(int), hipMemcpyHostToDevice, c->stream));
        return NH_OK;
    };
    int rc;
    if ((rc = table(n.color_slots, color_slots)) || (rc = table(n.block_ids, blocks)) ||
        (rc = table(n.block_slot, slot_map)) || (rc = table(n.pixel_list, list)) || (rc = table(n.pixel_map, map)))
        return rc;
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    std::swap(c->px, n);
    drop_primary_masks(c);  // the masks follow the list's blocks (the pipeline was drained above)
    return NH_OK;
}

// The camera rays' candidate masks (WfLaunch::pmask) for the uploaded scene and the current pixel list: one entry per
// block of the image's block grid, those of the rendered blocks filled in. Absent (null) unless the scene is small
// enough for the LDS-staged kernels and nh::primary_masks accepts it (at most 64 records, a pinhole camera).
static int ensure_primary_masks(nh_ctx *c) {
    if (c->pmask_known) return NH_OK;
    if (int rc = pipeline_drain(c)) return rc;  // chunks in flight read the current table
    drop_primary_masks(c);
    c->pmask_known = true;
    const size_t scene_bytes = 16 * (size_t)(c->n_node_f4 + c->n_prim_f4) + 8 * (size_t)c->n_leaves;
    if (c->h_prims.empty() || scene_bytes > kSmallSceneBytes) return NH_OK;
    std::vector<int32_t> blocks = c->px.list_key;
    if (blocks.empty())
        for (int i = 0; i < c->nbx * c->nby; ++i) blocks.push_back(i);
    std::vector<uint64_t> m;
    if (!nh::primary_masks(c->camera, reinterpret_cast<const nh::f4 *>(c->h_prims.data()), (int)(c->h_prims.size() / 12),
                           blocks.data(), (int)blocks.size(), m))
        return NH_OK;
    std::vector<unsigned long long> grid((size_t)c->nbx * c->nby, 0ull);
    for (size_t i = 0; i < blocks.size(); ++i) grid[(size_t)blocks[i]] = m[i];
    unsigned long long *d = nullptr;
    HIP_TRY(c, hipMalloc(&d, std::max<size_t>(grid.size(), 1) * sizeof(unsigned long long)));
    const hipError_t e = hipMemcpy(d, grid.data(), grid.size() * sizeof(unsigned long long), hipMemcpyHostToDevice);
    if (e != hipSuccess) {
        (void)hipFree(d);
        HIP_TRY(c, e);
    }
    c->pmask = d;
    // the light samples' candidate masks, for the same records and blocks (absent with the table above)
    const int n_faces = (int)(c->h_emit_tris.size() / 9);
    const nh::f4 *recs = reinterpret_cast<const nh::f4 *>(c->h_prims.data());
    const int n_recs = (int)(c->h_prims.size() / 12);
    if (n_faces == 0 ||
        !nh::shadow_block_masks(c->camera, recs, n_recs, c->h_emit_tris.data(), n_faces, blocks.data(), (int)blocks.size(), m))
        return NH_OK;
    for (size_t i = 0; i < blocks.size(); ++i) grid[(size_t)blocks[i]] = m[i];
    HIP_TRY(c, hipMalloc(&d, std::max<size_t>(grid.size(), 1) * sizeof(unsigned long long)));
    const hipError_t e2 = hipMemcpy(d, grid.data(), grid.size() * sizeof(unsigned long long), hipMemcpyHostToDevice);
    if (e2 != hipSuccess) {
        (void)hipFree(d);
        HIP_TRY(c, e2);
    }
    c->smask = d;
    return NH_OK;
}

// ---- the av integrator's split pipeline (nh_av.hip) ----
// device bytes per path of a chunk: camera ray and queue ray (32 each), closest hit (17), stream state (8), queue path
// index (4), any-hit result (1)
constexpr size_t kAvBytesPerPath = 94;

// The wide tree walks the chunk's batches when a wavefront pool would pick it for the same request (pool_start: a
// deep tree, a near-first request); every order returns the same hits.
static bool av_wide(const nh_ctx *c, const nh_render_req *q) {
    return q->traversal != NH_TRAVERSAL_REFERENCE && c->depth > 20 && c->tv.wnodes != nullptr;
}
static size_t av_bytes_per_path(const nh_ctx *c, const nh_render_req *q) {
    return kAvBytesPerPath + (av_wide(c, q) ? (size_t)c->depth_wide * sizeof(int2) : 0);
}

// the chunk buffers, kept by the context for the next chunk of at most `paths` paths
static int av_reserve(nh_ctx *c, size_t paths, bool wide) {
    const int spill_depth = wide ? c->depth_wide : 0;
    if (c->av_cap >= paths && c->av_spill_depth >= spill_depth) return NH_OK;
    free_all(c->av_bufs);
    c->av_cap = 0;
    c->av_spill_depth = 0;
    c->av_spill = nullptr;
    AvLaunch &L = c->av;
    L = AvLaunch{};
    const auto get = [&](auto **p, size_t n) -> int {
        void *d = nullptr;
        HIP_TRY(c, hipMalloc(&d, std::max<size_t>(n, 1) * sizeof(**p)));
        c->av_bufs.push_back(d);
        *p = static_cast<std::remove_reference_t<decltype(*p)>>(d);
        return NH_OK;
    };
    int rc = NH_OK;
    for (int i = 0; i < 8 && !rc; ++i)
        if (!(rc = get(&L.ray[i], paths))) rc = get(&L.q_ray[i], paths);
    if (rc || (rc = get(&L.hit.hit, paths)) || (rc = get(&L.hit.t, paths)) || (rc = get(&L.hit.u, paths)) ||
        (rc = get(&L.hit.v, paths)) || (rc = get(&L.hit.k, paths)) || (rc = get(&L.rng, paths)) ||
        (rc = get(&L.q_path, paths)) || (rc = get(&L.q_hit, paths)) || (rc = get(&L.q_count, 1)) ||
        (spill_depth && (rc = get(&c->av_spill, paths * (size_t)spill_depth)))) {
        free_all(c->av_bufs);
        return rc;
    }
    c->av_cap = paths;
    c->av_spill_depth = spill_depth;
    return NH_OK;
}

// One chunk's paths through the stages, on the context's stream: what launch_path does for the megakernel, into the
// same sample records. Only a render that collects statistics reads the queue's length back (its any-hit launch then
// covers exactly the queue, so the padding is not counted as queries).
static int av_chunk(nh_ctx *c, const nh_render_req *q, const PathLaunch &P) {
    AvLaunch L = c->av;
    L.n_paths = P.n_paths;
    L.n_list = P.n_list;
    L.s0 = P.s0;
    L.seed = P.seed;
    L.pixel_list = P.pixel_list;
    L.rec = P.rec;
    const bool wide = av_wide(c, q), ordered = q->traversal != NH_TRAVERSAL_REFERENCE, stats = q->collect_stats != 0;
    const auto batch = [&](float *const r[8], const HitBatch &hb, int n, bool any) {
        const RayBatch rb{r[0], r[1], r[2], r[3], r[4], r[5], r[6], r[7]};
        // the any-hit work goes to the counters' any-hit share, as the wavefront pools' shadow rays do
        unsigned long long *ctr = c->counters + (any ? kStatAny : 0);
        if (wide) nh::launch_trace_wide(c->d_scene, c->tv, rb, hb, n, any, true, stats, c->av_spill, c->av_spill_depth, ctr,
                                        c->stream, c->wide_w);
        else nh::launch_trace(c->d_scene, c->tv, rb, hb, n, any, ordered, stats, c->depth, ctr, c->stream);
    };
    HIP_TRY(c, hipMemsetAsync(L.q_count, 0, sizeof(unsigned), c->stream));
    nh::launch_av_primary(c->d_scene, L, c->stream);
    batch(L.ray, L.hit, L.n_paths, false);
    nh::launch_av_shade(c->d_scene, c->tv, L, c->stream);
    HIP_TRY(c, hipGetLastError());
    int n_queue = L.n_paths;
    if (stats) {
        unsigned n = 0;
        HIP_TRY(c, hipMemcpyAsync(&n, L.q_count, sizeof(n), hipMemcpyDeviceToHost, c->stream));
        HIP_TRY(c, hipStreamSynchronize(c->stream));
        n_queue = (int)n;
    }
    HitBatch occl{};
    occl.hit = L.q_hit;
    batch(L.q_ray, occl, n_queue, true);
    nh::launch_av_resolve(L, n_queue, c->stream);
    return NH_OK;
}

extern "C" {

int nh_render(nh_ctx *c, const nh_render_req *q) {
    if (!c || !q) return NH_ERR_INVALID;
    if (!c->has_scene || !c->has_bvh) return fail(c, "nh_render: scene and BVH must be uploaded"), NH_ERR_STATE;
    if (q->sample_end < q->sample_begin || q->sample_begin < 0) return fail(c, "invalid sample range"), NH_ERR_INVALID;
    if (c->S.dof && q->sample_end > nhd::kLensLo * nhd::kLensHi)  // the lens tables' range (nh_shade.h lens_uniform)
        return fail(c, "depth of field: sample rounds beyond 2^24"), NH_ERR_UNSUPPORTED;
    // path_mis throws it (path_mis.cpp:76-79); direct_mis would pick from an empty emitter list
    if ((c->integrator == NH_INTEGRATOR_PATH_MIS || c->integrator == NH_INTEGRATOR_DIRECT_MIS) && c->n_emitters == 0)
        return fail(c, "No Emitter in scene!"), NH_ERR_INVALID;
    if (q->mode != NH_MODE_MEGAKERNEL && q->mode != NH_MODE_WAVEFRONT) return fail(c, "unknown render mode"), NH_ERR_INVALID;
    const bool volumetric = c->integrator == NH_INTEGRATOR_PATH_VOL_MATS || c->integrator == NH_INTEGRATOR_PATH_VOL_MIS;
    // the surface integrators dereference every hit shape's BSDF and know no medium (the reference would crash, or
    // silently drop the media): their kernels keep the "every shape has a BSDF" assumption
    if (!volumetric && (c->bsdfless || c->has_media))
        return fail(c, "the scene has a participating medium or a shape without a BSDF: only the path_vol_mats and "
                       "path_vol_mis integrators render it"), NH_ERR_UNSUPPORTED;
    if (c->integrator == NH_INTEGRATOR_PATH_VOL_MIS && c->n_emitters == 0)  // sampleEmitter would pick from an empty list
        return fail(c, "No Emitter in scene!"), NH_ERR_INVALID;
    // the photon mapper's Li gathers from the map preprocess() builds (nh_photon_map_build); like the volumetric path
    // tracers it has its own megakernel (nh_photon.hip), which also serves a wavefront request
    const bool photon = c->integrator == NH_INTEGRATOR_PHOTONMAPPER;
    if (photon && !c->photon.built)
        return fail(c, "nh_render: the photon mapper needs a photon map (nh_photon_map_build)"), NH_ERR_STATE;
    if (photon && c->sampler == NH_SAMPLER_ADAPTIVE)
        return fail(c, "photonmapper: the adaptive sampler is not supported"), NH_ERR_UNSUPPORTED;
    if (c->integrator == NH_INTEGRATOR_AV && !c->av_set)
        return fail(c, "nh_render: the av integrator needs its length (nh_set_av_params)"), NH_ERR_STATE;
    if (c->integrator == NH_INTEGRATOR_ENVMAPTESTER && c->S.envmap < 0)  // EnvMapTester.cpp:19-23
        return fail(c, "This integrator requires an env map."), NH_ERR_INVALID;
    // av in wavefront mode: its own split pipeline over the megakernel's chunks (nh_av.hip), the camera paths that
    // escape leaving before the occlusion query. envmaptester traces nothing: the megakernel, like the direct ones
    const bool av_split = q->mode == NH_MODE_WAVEFRONT && c->integrator == NH_INTEGRATOR_AV;
    // the single-bounce direct integrators always run as the megakernel: one closest hit, the light
    // sample(s) and at most one BSDF ray per path leave no bounce loop for path queues to balance. The volumetric
    // path tracers have no wavefront version yet: a wavefront request runs their megakernel (nh_volume.hip)
    const bool wavefront = q->mode == NH_MODE_WAVEFRONT && c->integrator <= NH_INTEGRATOR_PATH_MATS;
    if (q->traversal < NH_TRAVERSAL_REFERENCE || q->traversal > NH_TRAVERSAL_WIDE)
        return fail(c, "unknown traversal"), NH_ERR_INVALID;
    if (c->border > 4) return fail(c, "reconstruction filters wider than border 4 are not supported"), NH_ERR_UNSUPPORTED;
    HIP_TRY(c, hipSetDevice(c->device));
    // only asynchronous wavefront renders overlap earlier chunks still in flight
    int rc = NH_OK;
    if (!wavefront || q->collect_stats || q->clear || c->sampler == NH_SAMPLER_ADAPTIVE) rc = pipeline_drain(c);
    if (rc) return rc;
    // <sampler type="adaptive">: its own loop of passes over 4x4 blocks (nh_adaptive_api.hip); mode and traversal
    // change nothing there
    if (c->sampler == NH_SAMPLER_ADAPTIVE) return render_adaptive(c, q);
    rc = ensure_pixel_list(c, q);
    if (rc) return rc;
    if (wavefront && (rc = ensure_primary_masks(c))) return rc;
    c->stats.node_bytes = 64;  // binary tree unless a wavefront pool picks the 4-wide one
    if (av_split && av_wide(c, q)) c->stats.node_bytes = 16 * nhd::kWideF4 * (c->wide_w / 4);
    c->stats.primary_masks = 0;
    c->stats.shadow_masks = 0;
    c->stats.pair_kinds = 0;
    c->stats.flat_trace = 0;
    c->stats.any_list = 0;
    c->stats.trace_fused = 0;
    c->stats.lds_scene = 0;
    c->stats.fused_bounce = 0;
    if (q->clear) {
        HIP_TRY(c, hipMemsetAsync(c->fb, 0, c->fb_floats * sizeof(float), c->stream));
        HIP_TRY(c, hipEventRecord(c->fb_ev, c->stream));  // pools' splats wait for it
        c->fb_ev_set = true;
    }
    const int rounds = q->sample_end - q->sample_begin;
    if (rounds == 0 || c->px.n_list == 0) return NH_OK;
    if (q->collect_stats)
        HIP_TRY(c, hipMemsetAsync(c->counters, 0, kStatShards * kStatStride * sizeof(unsigned long long), c->stream));
    const size_t per_round = (size_t)c->px.n_list;
    const char *jv = std::getenv("NH_SPLAT_JITTER");  // stored jitter (A/B): 8 more bytes per sample record
    const size_t rec_bytes = kRecFloats * 4 + (wavefront && jv && std::strcmp(jv, "stored") == 0 ? 8 : 0);
    const size_t per_round_bytes = per_round * rec_bytes + (size_t)c->px.n_blocks * block_px(c, splat_staged(c)) * 16 +
                                   (wavefront ? per_round * kWfBytesPerPath : 0) +
                                   (av_split ? per_round * av_bytes_per_path(c, q) : 0);
    // device memory per chunk: sample records + block ImageBlocks (+ path state, per pool). Every
    // wavefront chunk ends in a tail whose length is set by its longest path (C4: ~5-7 ms of
    // dielectric / mirror chains, whatever the chunk's size), so chunks are as large as the 26-bit
    // path ids allow: one chunk per C4 step (67M paths, ~18 GB per pool) instead of 7 + 7 + 2 rounds
    // under an 8 GiB budget (C4 2590 -> 3140 Msamples/s); 288 GB of HBM holds two such pools.
    size_t budget = wavefront ? (size_t)24 << 30 : (size_t)1 << 30;
    if (const char *e = std::getenv(wavefront ? "NH_WF_BUDGET_MB" : "NH_RECORD_BUDGET_MB"))
        budget = (size_t)std::max(1L, std::atol(e)) << 20;
    if (wavefront) {
        // every active pool is sized for the chunk: cap the budget at this device's free memory (plus what
        // the pools already hold) shared by the pools, with headroom, so several contexts on one GPU get
        // smaller chunks instead of a failed allocation
        size_t free_b = 0, total_b = 0;
        if (hipMemGetInfo(&free_b, &total_b) == hipSuccess) {
            size_t held = 0;
            for (const WfPool &p : c->pools)
                held += p.cap * kWfBytesPerPath + p.rec_cap * kRecFloats * 4 + p.jit_cap * 8 + p.staging_cap * sizeof(float4);
            // asynchronous tails: each tail slot also holds a whole chunk's sample records and staging (and
            // kTailCap paths of state), so it counts as one more chunk-sized share
            const int shares = active_pools(c) + (active_pools(c) > 1 && tail_async_enabled() ? kTails : 0);
            const size_t avail = (size_t)((double)(free_b + held) * 0.85) / (size_t)shares;
            budget = std::min(budget, std::max(avail, per_round_bytes));
        }
    }
    int chunk = (int)std::max<size_t>(1, std::min<size_t>((size_t)rounds, budget / per_round_bytes));
    while ((size_t)chunk * per_round > (size_t)0x7fffffff) chunk = std::max(1, chunk / 2);
    if (wavefront) {  // path ids of a chunk are packed into 26 bits of the path state (nh_wavefront.hip)
        if (per_round > ((size_t)1 << 26))
            return fail(c, "wavefront mode renders at most 2^26 pixels per context"), NH_ERR_UNSUPPORTED;
        chunk = std::min(chunk, (int)(((size_t)1 << 26) / per_round));
    }

    if (wavefront) {
        HIP_TRY(c, hipStreamSynchronize(c->stream));  // pixel list / clear / counters are in place
        for (int s = q->sample_begin; s < q->sample_end; s += chunk)
            c->jobs.push_back(WfJob{c->job_seq++, s, std::min(chunk, q->sample_end - s), q->seed,
                                    q->traversal != NH_TRAVERSAL_REFERENCE, q->collect_stats != 0});
        rc = q->collect_stats ? pipeline_drain(c) : pipeline_run(c, false);
        if (rc) return rc;
        if (int e = check_device(c, "nh_render")) return e;
    } else {
        if (c->rec_cap < (size_t)chunk * per_round) {
            (void)hipFree(c->rec);
            c->rec = nullptr;
            c->rec_cap = 0;
            const size_t cap = (size_t)chunk * per_round;
            HIP_TRY(c, hipMalloc(&c->rec, cap * kRecFloats * sizeof(float)));
            c->rec_cap = cap;
        }
        if (av_split && (rc = av_reserve(c, (size_t)chunk * per_round, av_wide(c, q)))) return rc;
        const bool staged = splat_staged(c);
        if (c->staging_cap < (size_t)chunk * c->px.n_blocks * block_px(c, staged)) {
            (void)hipFree(c->staging);
            c->staging = nullptr;
            c->staging_cap = 0;
            const size_t cap = (size_t)chunk * c->px.n_blocks * block_px(c, staged);
            HIP_TRY(c, hipMalloc(&c->staging, cap * sizeof(float4)));
            c->staging_cap = cap;
        }
        struct Ev {
            hipEvent_t a, b, d;
        };
        std::vector<Ev> evs;
        for (int s = q->sample_begin; s < q->sample_end; s += chunk) {
            const int k = std::min(chunk, q->sample_end - s);
            PathLaunch L{};
            L.n_paths = k * c->px.n_list;
            L.n_list = c->px.n_list;
            L.s0 = s;
            L.seed = q->seed;
            L.pixel_list = c->px.pixel_list;
            L.rec = c->rec;
            L.counters = c->counters;
            Ev ev;
            HIP_TRY(c, hipEventCreate(&ev.a));
            HIP_TRY(c, hipEventCreate(&ev.b));
            HIP_TRY(c, hipEventCreate(&ev.d));
            HIP_TRY(c, hipEventRecord(ev.a, c->stream));
            if (av_split) {
                if ((rc = av_chunk(c, q, L))) return rc;
            } else if (photon)
                nh_disney::nh::launch_photon_path(c->d_scene, c->tv, L, q->collect_stats != 0, c->depth, c->stream);
            else if (volumetric)
                nh_disney::nh::launch_vol_path(c->d_scene, c->tv, L, c->integrator == NH_INTEGRATOR_PATH_VOL_MIS,
                                               q->collect_stats != 0, c->depth, c->stream);
            else
                NH_LAUNCH(c, launch_path)(c->d_scene, c->tv, L, q->traversal != NH_TRAVERSAL_REFERENCE, q->collect_stats != 0,
                            c->depth, c->integrator == NH_INTEGRATOR_PATH_MIS && !c->normal_mapped, c->stream);
            HIP_TRY(c, hipGetLastError());
            HIP_TRY(c, hipEventRecord(ev.b, c->stream));
            if (q->collect_stats) nh::launch_count_invalid(c->rec, (size_t)L.n_paths, c->counters, c->stream);
            nh::launch_splat(make_splat(c, c->rec, q->seed, s, c->staging, k, staged), c->stream);
            HIP_TRY(c, hipGetLastError());
            HIP_TRY(c, hipEventRecord(ev.d, c->stream));
            evs.push_back(ev);
        }
        HIP_TRY(c, hipStreamSynchronize(c->stream));
        for (auto &ev : evs) {
            float a = 0, b = 0;
            (void)hipEventElapsedTime(&a, ev.a, ev.b);
            (void)hipEventElapsedTime(&b, ev.b, ev.d);
            c->stats.kernel_ms_path += a;
            c->stats.kernel_ms_splat += b;
            c->stats.launches_path++;
            c->stats.launches_splat++;
            (void)hipEventDestroy(ev.a);
            (void)hipEventDestroy(ev.b);
            (void)hipEventDestroy(ev.d);
        }
        c->stats.samples += (uint64_t)rounds * (uint64_t)c->px.n_list;
    }
    if (q->collect_stats) {
        unsigned long long hs[kStatShards * kStatStride], h[kStatStride] = {};
        HIP_TRY(c, hipMemcpy(hs, c->counters, sizeof(hs), hipMemcpyDeviceToHost));
        for (int sh = 0; sh < kStatShards; ++sh)
            for (int j = 0; j < kStatStride; ++j) h[j] += hs[sh * kStatStride + j];
        h[kStatTailClk + 5] = 0;  // the longest tail chain: a max over the shards, not a sum
        for (int sh = 0; sh < kStatShards; ++sh)
            h[kStatTailClk + 5] = std::max(h[kStatTailClk + 5], hs[sh * kStatStride + kStatTailClk + 5]);
        c->stats.tail_cycles_body += h[kStatTailClk];
        c->stats.tail_cycles_shadow += h[kStatTailClk + 1];
        c->stats.tail_cycles_closest += h[kStatTailClk + 2];
        c->stats.tail_cycles_head += h[kStatTailClk + 3];
        c->stats.tail_bounces += h[kStatTailClk + 4];
        c->stats.tail_max_bounces = std::max<uint64_t>(c->stats.tail_max_bounces, h[kStatTailClk + 5]);
        c->stats.tail_coop_cycles_body += h[kStatTailCoopClk];
        c->stats.tail_coop_cycles_shadow += h[kStatTailCoopClk + 1];
        c->stats.tail_coop_cycles_closest += h[kStatTailCoopClk + 2];
        c->stats.tail_coop_cycles_head += h[kStatTailCoopClk + 3];
        c->stats.tail_coop_bounces += h[kStatTailCoopClk + 4];
        c->stats.bounce_cycles_load += h[kStatBounceClk];
        c->stats.bounce_cycles_body += h[kStatBounceClk + 1];
        c->stats.bounce_cycles_shadow += h[kStatBounceClk + 2];
        c->stats.bounce_cycles_closest += h[kStatBounceClk + 3];
        c->stats.bounce_cycles_head += h[kStatBounceClk + 4];
        c->stats.bounce_cycles_store += h[kStatBounceClk + 5];
        c->stats.bounce_bounces += h[kStatBounceClk + 6];
        const unsigned long long *cl = h, *an = h + kStatAny, *tc = h + kStatTail, *ta = h + kStatTailAny;
        c->stats.ray_queries += cl[0] + an[0] + tc[0] + ta[0];
        c->stats.nodes_visited += cl[1] + an[1] + tc[1] + ta[1];
        c->stats.boxes_tested += cl[2] + an[2] + tc[2] + ta[2];
        c->stats.prims_tested += cl[3] + an[3] + tc[3] + ta[3];
        c->stats.invalid_samples += h[4];
        c->stats.shadow_queries += an[0] + ta[0];
        c->stats.shadow_nodes_visited += an[1] + ta[1];
        c->stats.shadow_boxes_tested += an[2] + ta[2];
        c->stats.shadow_prims_tested += an[3] + ta[3];
        c->stats.tail_queries += tc[0] + ta[0];
        c->stats.tail_nodes_visited += tc[1] + ta[1];
        c->stats.tail_boxes_tested += tc[2] + ta[2];
        c->stats.tail_prims_tested += tc[3] + ta[3];
        c->stats.tail_shadow_queries += ta[0];
        c->stats.tail_shadow_nodes_visited += ta[1];
        c->stats.tail_shadow_boxes_tested += ta[2];
        c->stats.tail_shadow_prims_tested += ta[3];
    }
    return NH_OK;
}

}  // extern "C"
