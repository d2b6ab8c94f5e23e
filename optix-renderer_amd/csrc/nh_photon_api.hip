// nh_photon_map_build, nh_get_photon_stats, nh_get_photons and nh_photon_query of the C-ABI (include/nori_hip.h): the
// host side of nh_photon.hip's kernels.
#include <climits>
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
int p_alloc(nh_ctx *c, std::vector<void *> &owner, T **p, size_t n) {
    void *d = nullptr;
    HIP_TRY(c, hipMalloc(&d, std::max<size_t>(n, 1) * sizeof(T)));
    owner.push_back(d);
    *p = static_cast<T *>(d);
    return NH_OK;
}

// PhotonData's tables on the device, uploaded once per context
int ensure_tables(nh_ctx *c) {
    PhotonState &ps = c->photon;
    if (ps.tables) return NH_OK;
    ps.h_tables.assign(5 * 256, 0.f);
    float *t = ps.h_tables.data();
    // the order of nh_photon.h's PM_* offsets
    if (nh_photon_tables(t, t + 256, t + 512, t + 768, t + 1024)) return fail(c, "nh_photon_tables failed"), NH_ERR_INVALID;
    void *d = nullptr;
    HIP_TRY(c, hipMalloc(&d, ps.h_tables.size() * sizeof(float)));
    if (hipMemcpy(d, t, ps.h_tables.size() * sizeof(float), hipMemcpyHostToDevice) != hipSuccess) {
        (void)hipFree(d);
        return fail(c, "photon tables: upload failed"), NH_ERR_DEVICE;
    }
    ps.tables = static_cast<const float *>(d);
    return NH_OK;
}

constexpr long long kGuardPaths = 1 << 16;  // paths that must deposit something
constexpr int kMaxBatch = 1 << 22;

}  // namespace

void photon_release(nh_ctx *c, bool tables) {
    PhotonState &ps = c->photon;
    free_all(ps.bufs);
    ps.built = false;
    ps.pos = nullptr;
    ps.bytes = nullptr;
    ps.path = nullptr;
    ps.bounce = nullptr;
    ps.stats = nh_photon_stats{};
    c->S.pm = nhd::DPhotonMap{};
    // the device copy of the scene record must not keep pointers into the freed map (a failed build leaves none)
    if (c->d_scene)
        (void)hipMemcpy(reinterpret_cast<char *>(c->d_scene) + offsetof(nhd::DScene, pm), &c->S.pm, sizeof(c->S.pm),
                        hipMemcpyHostToDevice);
    if (tables) {
        (void)hipFree(const_cast<float *>(ps.tables));
        ps.tables = nullptr;
    }
}

extern "C" {

int nh_photon_map_build(nh_ctx *c, const nh_photon_params *params, uint64_t seed, int32_t batch_paths) {
    if (!c) return NH_ERR_INVALID;
    if (!params || params->photon_count < 1 || !(params->photon_radius >= 0.f) || !std::isfinite(params->photon_radius) ||
        batch_paths < 0)
        return fail(c, "nh_photon_map_build: invalid argument"), NH_ERR_INVALID;
    if (!c->has_scene || !c->has_bvh) return fail(c, "nh_photon_map_build: scene and BVH must be uploaded"), NH_ERR_STATE;
    if (c->integrator != NH_INTEGRATOR_PHOTONMAPPER)
        return fail(c, "nh_photon_map_build: the scene's integrator is not the photon mapper: not supported"),
               NH_ERR_UNSUPPORTED;
    // what the loader refuses, for scenes that were described by hand
    if (c->n_emitters == 0) return fail(c, "photonmapper: a scene without an emitter is not supported"), NH_ERR_UNSUPPORTED;
    for (const nhd::DEmitter &e : c->h_emitters)
        if (e.type != NH_EMITTER_AREA || e.shape < 0 || (size_t)e.shape >= c->h_shapes.size())
            return fail(c, "photonmapper: an emitter that is not an area light is not supported"), NH_ERR_UNSUPPORTED;
    if (c->bsdfless || c->has_media)
        return fail(c, "photonmapper: a participating medium or a shape without a BSDF is not supported"),
               NH_ERR_UNSUPPORTED;
    for (const nhd::DBsdf &b : c->h_bsdfs)
        if ((b.type == NH_BSDF_DIFFUSE || b.type == NH_BSDF_DISNEY) && b.tex)
            return fail(c, "photonmapper: a textured diffuse or Disney albedo is not supported"), NH_ERR_UNSUPPORTED;
    HIP_TRY(c, hipSetDevice(c->device));
    if (int rc = pipeline_drain(c)) return rc;
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    photon_release(c);
    if (int rc = ensure_tables(c)) return rc;
    PhotonState &ps = c->photon;
    const float radius = params->photon_radius == 0.f ? nh::photon_auto_radius(c->S.root_min, c->S.root_max)
                                                      : params->photon_radius;
    if (!(radius > 0.f) || !std::isfinite(radius))
        return fail(c, "photonmapper: the gather radius is not a positive finite number: not supported"), NH_ERR_UNSUPPORTED;
    const size_t cap = (size_t)params->photon_count;
    const int batch = std::min(batch_paths == 0 ? NH_PHOTON_DEFAULT_BATCH : batch_paths, kMaxBatch);

    struct Drop {  // a failed build leaves no map
        nh_ctx *c;
        bool keep = false;
        ~Drop() { if (!keep) photon_release(c); }
    } drop{c};
    int rc;
    if ((rc = p_alloc(c, ps.bufs, &ps.pos, 3 * cap)) || (rc = p_alloc(c, ps.bufs, &ps.bytes, cap)) ||
        (rc = p_alloc(c, ps.bufs, &ps.path, cap)) || (rc = p_alloc(c, ps.bufs, &ps.bounce, cap)))
        return rc;
    std::vector<void *> tmp;
    Free guard{tmp};
    long long *counts = nullptr, *offsets = nullptr;
    int *d_emitted = nullptr;
    if ((rc = p_alloc(c, tmp, &counts, (size_t)batch + 1)) || (rc = p_alloc(c, tmp, &offsets, (size_t)batch + 1)) ||
        (rc = p_alloc(c, tmp, &d_emitted, 1)))
        return rc;
    // the scan's temporary storage, once for every batch (a temporary size grows with the item count)
    const size_t scan_bytes = nh_disney::nh::photon_scan_temp_bytes(batch + 1);
    char *scan_tmp = nullptr;
    if (!scan_bytes) return fail(c, "nh_photon_map_build: the scan's temporary size query failed"), NH_ERR_DEVICE;
    if ((rc = p_alloc(c, tmp, &scan_tmp, scan_bytes))) return rc;
    HIP_TRY(c, hipMemsetAsync(d_emitted, 0, sizeof(int), c->stream));

    // ---- the photon pass: batches of paths, each counted, scanned and re-traced into its slots ----
    long long stored = 0, k0 = 0;
    while (stored < (long long)cap) {
        if (k0 >= (long long)INT_MAX)
            return fail(c, "photonmapper: the emitted photon count would pass INT32_MAX: not supported"), NH_ERR_UNSUPPORTED;
        long long n = std::min<long long>(batch, (long long)INT_MAX - k0);
        if (k0 < kGuardPaths) n = std::min(n, kGuardPaths - k0);  // no batch straddles the guard: it sees the same paths
        PhotonTrace P{};
        P.seed = seed;
        P.k0 = (uint64_t)k0;
        P.n_paths = (int)n;
        P.counts = counts;
        P.base = stored;
        P.cap = (int)cap;
        P.pos = ps.pos;
        P.bytes = ps.bytes;
        P.path = ps.path;
        P.bounce = ps.bounce;
        P.emitted = d_emitted;
        // (one entry past the paths, zero: the scan's last output is then the batch's total)
        HIP_TRY(c, hipMemsetAsync(counts + n, 0, sizeof(long long), c->stream));
        nh_disney::nh::launch_photon_trace(c->d_scene, c->tv, P, c->depth, c->stream);
        HIP_TRY(c, hipGetLastError());
        HIP_TRY(c, nh_disney::nh::photon_scan(counts, offsets, (int)n + 1, scan_tmp, scan_bytes, c->stream));
        // the write pass follows in stream order (a batch without deposits writes nothing); one wait per batch, for
        // the total the loop's end depends on
        P.offsets = offsets;
        nh_disney::nh::launch_photon_trace(c->d_scene, c->tv, P, c->depth, c->stream);
        HIP_TRY(c, hipGetLastError());
        long long total = 0;
        HIP_TRY(c, hipMemcpyAsync(&total, offsets + n, sizeof(long long), hipMemcpyDeviceToHost, c->stream));
        HIP_TRY(c, hipStreamSynchronize(c->stream));
        stored += total;
        k0 += n;
        if (k0 == kGuardPaths && stored == 0)
            return fail(c, "photonmapper: no photon reaches a diffuse surface (the first 65536 photon paths deposit "
                           "nothing; the reference would loop forever): not supported"), NH_ERR_UNSUPPORTED;
    }
    if (int e = check_device(c, "nh_photon_map_build")) return e;
    int emitted = 0;
    HIP_TRY(c, hipMemcpy(&emitted, d_emitted, sizeof(int), hipMemcpyDeviceToHost));
    if (emitted < 1) return fail(c, "nh_photon_map_build: the emitted count was not written"), NH_ERR_DEVICE;

    // ---- the search structure: a uniform grid of cells no smaller than the radius, 21 bits per axis ----
    nhd::DPhotonMap pm{};
    pm.n = (int)cap;
    pm.emitted = emitted;
    pm.radius = radius;
    float ext = 0.f;
    for (int k = 0; k < 3; ++k) ext = std::max(ext, c->S.root_max[k] - c->S.root_min[k]);
    // 1.01 r: the two ends of a query's span, 2.002 r apart, then lie in at most three cells per axis; and no more
    // than 2^20 cells across the scene box
    pm.cell = std::max(radius * 1.01f, ext / 1048576.0f);
    for (int k = 0; k < 3; ++k) pm.origin[k] = c->S.root_min[k] - 2.f * pm.cell;
    float4 *s_pos = nullptr, *s_dir = nullptr, *s_pow = nullptr;
    uint64_t *s_keys = nullptr, *keys = nullptr;
    uint32_t *index = nullptr, *s_index = nullptr;
    unsigned long long *cells = nullptr;
    if ((rc = p_alloc(c, ps.bufs, &s_pos, cap)) || (rc = p_alloc(c, ps.bufs, &s_dir, cap)) ||
        (rc = p_alloc(c, ps.bufs, &s_pow, cap)) || (rc = p_alloc(c, ps.bufs, &s_keys, cap)) ||
        (rc = p_alloc(c, tmp, &keys, cap)) || (rc = p_alloc(c, tmp, &index, cap)) ||
        (rc = p_alloc(c, tmp, &s_index, cap)) || (rc = p_alloc(c, tmp, &cells, 1)))
        return rc;
    pm.pos = s_pos;
    pm.dir = s_dir;
    pm.power = s_pow;
    pm.keys = s_keys;
    PhotonFinalize F{};
    F.n = (int)cap;
    F.pos = ps.pos;
    F.bytes = ps.bytes;
    F.tab = ps.tables;
    F.pm = pm;
    F.keys = keys;
    F.index = index;
    F.sorted_index = s_index;
    F.cells = cells;
    HIP_TRY(c, hipMemsetAsync(cells, 0, sizeof(unsigned long long), c->stream));
    nh_disney::nh::launch_photon_keys(F, c->stream);
    HIP_TRY(c, hipGetLastError());
    HIP_TRY(c, nh_disney::nh::photon_sort(keys, s_keys, index, s_index, (int)cap, c->stream));
    nh_disney::nh::launch_photon_scatter(F, c->stream);
    HIP_TRY(c, hipGetLastError());
    unsigned long long h_cells = 0;
    HIP_TRY(c, hipMemcpyAsync(&h_cells, cells, sizeof(h_cells), hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    if (int e = check_device(c, "nh_photon_map_build")) return e;

    c->S.pm = pm;
    HIP_TRY(c, hipMemcpy(c->d_scene, &c->S, sizeof(nhd::DScene), hipMemcpyHostToDevice));
    ps.stats.stored = (int32_t)cap;
    ps.stats.emitted = emitted;
    ps.stats.radius = radius;
    ps.stats.cell_size = pm.cell;
    ps.stats.occupied_cells = h_cells;
    ps.built = true;
    drop.keep = true;
    return NH_OK;
}

int nh_get_photon_stats(nh_ctx *c, nh_photon_stats *out) {
    if (!c || !out) return NH_ERR_INVALID;
    if (!c->photon.built) return fail(c, "nh_get_photon_stats: no photon map"), NH_ERR_STATE;
    *out = c->photon.stats;
    return NH_OK;
}

int nh_get_photons(nh_ctx *c, int32_t first, int32_t n, float *position, float *direction, float *power,
                   uint8_t *bytes, int32_t *path, int32_t *bounce) {
    if (!c) return NH_ERR_INVALID;
    const PhotonState &ps = c->photon;
    if (!ps.built) return fail(c, "nh_get_photons: no photon map"), NH_ERR_STATE;
    if (first < 0 || n < 0 || (int64_t)first + n > ps.stats.stored)
        return fail(c, "nh_get_photons: range outside the map"), NH_ERR_INVALID;
    if (n == 0) return NH_OK;
    HIP_TRY(c, hipSetDevice(c->device));
    const size_t sn = (size_t)n, f = (size_t)first;
    if (position) HIP_TRY(c, hipMemcpy(position, ps.pos + 3 * f, 3 * sn * sizeof(float), hipMemcpyDeviceToHost));
    if (path) HIP_TRY(c, hipMemcpy(path, ps.path + f, sn * sizeof(int32_t), hipMemcpyDeviceToHost));
    if (bounce) HIP_TRY(c, hipMemcpy(bounce, ps.bounce + f, sn * sizeof(int32_t), hipMemcpyDeviceToHost));
    if (direction || power || bytes) {
        std::vector<uint2> b(sn);
        HIP_TRY(c, hipMemcpy(b.data(), ps.bytes + f, sn * sizeof(uint2), hipMemcpyDeviceToHost));
        // PhotonData::getDirection / getPower through the tables the device holds a copy of: single fp32 products
        const float *ct = ps.h_tables.data(), *st = ct + 256, *cp = ct + 512, *sp = ct + 768, *ex = ct + 1024;
        for (size_t i = 0; i < sn; ++i) {
            const uint32_t rgbe = b[i].x, theta = b[i].y & 0xffu, phi = (b[i].y >> 8) & 0xffu;
            if (bytes) {
                uint8_t *o = bytes + 6 * i;
                o[0] = (uint8_t)theta;
                o[1] = (uint8_t)phi;
                o[2] = (uint8_t)(rgbe & 0xffu);
                o[3] = (uint8_t)((rgbe >> 8) & 0xffu);
                o[4] = (uint8_t)((rgbe >> 16) & 0xffu);
                o[5] = (uint8_t)(rgbe >> 24);
            }
            if (direction) {
                direction[3 * i] = cp[phi] * st[theta];
                direction[3 * i + 1] = sp[phi] * st[theta];
                direction[3 * i + 2] = ct[theta];
            }
            if (power) {
                const float e = ex[rgbe >> 24];
                power[3 * i] = (float)(rgbe & 0xffu) * e;
                power[3 * i + 1] = (float)((rgbe >> 8) & 0xffu) * e;
                power[3 * i + 2] = (float)((rgbe >> 16) & 0xffu) * e;
            }
        }
    }
    return NH_OK;
}

int nh_photon_query(nh_ctx *c, int32_t mode, int32_t n, const float *in, uint8_t *bytes, int32_t *count, float *out) {
    if (!c) return NH_ERR_INVALID;
    if (mode != NH_PHOTON_QUERY_CODEC && mode != NH_PHOTON_QUERY_GATHER)
        return fail(c, "nh_photon_query: unknown mode"), NH_ERR_INVALID;
    const bool codec = mode == NH_PHOTON_QUERY_CODEC;
    if (n < 0 || !in || !out || (codec ? !bytes : !count)) return fail(c, "nh_photon_query: null argument"), NH_ERR_INVALID;
    if (!codec && !c->photon.built) return fail(c, "nh_photon_query: no photon map"), NH_ERR_STATE;
    if (n == 0) return NH_OK;
    HIP_TRY(c, hipSetDevice(c->device));
    if (int rc = pipeline_drain(c)) return rc;
    if (int rc = ensure_tables(c)) return rc;
    std::vector<void *> bufs;
    Free guard{bufs};
    const size_t sn = (size_t)n, in_stride = codec ? 6 : 3, out_stride = codec ? 6 : 3;
    PhotonQuery q{};
    q.mode = mode;
    q.n = n;
    q.tab = c->photon.tables;
    int rc;
    if ((rc = upload(c, bufs, in, in_stride * sn, &q.in)) || (rc = p_alloc(c, bufs, &q.out, out_stride * sn)) ||
        (codec ? (rc = p_alloc(c, bufs, &q.bytes, 6 * sn)) : (rc = p_alloc(c, bufs, &q.count, sn))))
        return rc;
    nh_disney::nh::launch_photon_query(codec ? nullptr : c->d_scene, q, c->stream);
    HIP_TRY(c, hipGetLastError());
    HIP_TRY(c, hipMemcpyAsync(out, q.out, out_stride * sn * sizeof(float), hipMemcpyDeviceToHost, c->stream));
    if (codec) HIP_TRY(c, hipMemcpyAsync(bytes, q.bytes, 6 * sn, hipMemcpyDeviceToHost, c->stream));
    else HIP_TRY(c, hipMemcpyAsync(count, q.count, sn * sizeof(int32_t), hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    return check_device(c, "nh_photon_query");
}

}  // extern "C"
