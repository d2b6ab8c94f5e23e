// Host-side layout of what the kernels walk (gpu_layout.h). Built without floating-point contraction like the rest
// of the library: collapse_wide and number_top_first order children by float surface areas.
#include "gpu_layout.h"

#include <algorithm>
#include <cmath>
#include <cstdlib>
#include <cstring>
#include <functional>

#include "../csrc/nh_layout.h"
#include "nh_host.h"

namespace nh {

namespace {
// the HIP vector types' names, for the code below that fills the kernels' records
using float4 = f4;
using int2 = i2;
struct int4 {
    int x, y, z, w;
};
inline float4 make_float4(float x, float y, float z, float w) { return float4{x, y, z, w}; }
inline int2 make_int2(int x, int y) { return int2{x, y}; }
inline int4 make_int4(int x, int y, int z, int w) { return int4{x, y, z, w}; }
inline u64x2 make_ulonglong2(uint64_t x, uint64_t y) { return u64x2{x, y}; }
}  // namespace

// BlockGenerator spiral order (src/utils/block.cpp:151-199) -> rank per block id
std::vector<int> spiral_rank(int w, int h, int bs, int &nbx, int &nby) {
    nbx = (int)std::ceil(w / (float)bs);
    nby = (int)std::ceil(h / (float)bs);
    std::vector<int> rank((size_t)nbx * nby, 0);
    int left = nbx * nby, dir = 0, bx = nbx / 2, by = nby / 2, steps_left = 1, num_steps = 1, r = 0;
    while (left > 0) {
        rank[(size_t)by * nbx + bx] = r++;
        if (--left == 0) break;
        do {
            switch (dir) {
                case 0: ++bx; break;
                case 1: ++by; break;
                case 2: --bx; break;
                case 3: --by; break;
            }
            if (--steps_left == 0) {
                dir = (dir + 1) % 4;
                if (dir == 0 || dir == 2) ++num_steps;
                steps_left = num_steps;
            }
        } while (bx < 0 || by < 0 || bx >= nbx || by >= nby);
    }
    return rank;
}

// The position of each pixel's camera ray within one sample round of the reference's serial render order: blocks
// in BlockGenerator order (edge blocks clipped, block.cpp:174-176), then Independent::getSampleIndices' x-major
// pixel order (independent.cpp:85-99: x outer, y inner)
std::vector<uint32_t> serial_ray_index(int w, int h, int bs) {
    int nbx = 0, nby = 0;
    const std::vector<int> rank = spiral_rank(w, h, bs, nbx, nby);
    std::vector<int> by_rank(rank.size());
    for (size_t b = 0; b < rank.size(); ++b) by_rank[(size_t)rank[b]] = (int)b;
    std::vector<uint32_t> idx((size_t)w * h);
    uint32_t k = 0;
    for (int b : by_rank) {
        const int ox = (b % nbx) * bs, oy = (b / nbx) * bs;
        const int sx = std::min(bs, w - ox), sy = std::min(bs, h - oy);
        for (int x = 0; x < sx; ++x)
            for (int y = 0; y < sy; ++y) idx[(size_t)(oy + y) * w + (ox + x)] = k++;
    }
    return idx;
}

namespace {
// pcg32::advance (pcg32.h:131-150) as an affine map of the state: advance(x, delta) = a * x + c (mod 2^64)
struct PcgAffine {
    uint64_t a = 1u, c = 0u;
};
PcgAffine pcg_affine(uint64_t inc, uint64_t delta) {
    uint64_t cur_mult = 0x5851f42d4c957f2dULL, cur_plus = inc;
    PcgAffine r;
    while (delta > 0) {
        if (delta & 1) {
            r.a *= cur_mult;
            r.c = r.c * cur_mult + cur_plus;
        }
        cur_plus = (cur_mult + 1) * cur_plus;
        cur_mult *= cur_mult;
        delta /= 2;
    }
    return r;
}
// g after f: x -> g.a * (f.a * x + f.c) + g.c
PcgAffine pcg_then(const PcgAffine &f, const PcgAffine &g) {
    PcgAffine r;
    r.a = g.a * f.a;
    r.c = g.a * f.c + g.c;
    return r;
}

// Lens-stream tables (nh_shade.h lens_uniform): camera ray k = round * W * H + pos[pixel] starts at draw 2k of the
// default-state stream, i.e. state(2k) = A_pos * (A_lo * S_hi + C_lo) + C_pos with round = 256 h + l,
// S_hi[h] = state(2 * 256 h * W * H), (A_lo, C_lo)[l] = advance by 2 l W H, (A_pos, C_pos) = advance by 2 pos:
// two 64-bit multiply-adds per ray instead of pcg_advance's O(log k) loop, and the same state (the maps commute)
constexpr uint64_t kLensDefaultState = 0x853c49e6748fea9bULL, kLensDefaultStream = 0xda3e39cb94b95bdbULL;
}  // namespace
LensTables lens_tables(int w, int h) {
    LensTables t;
    const std::vector<uint32_t> pos = serial_ray_index(w, h, 32);
    const uint64_t wh = (uint64_t)w * (uint64_t)h;
    // per pixel, in serial order: advance by 2 pos
    std::vector<PcgAffine> by_pos(wh);
    const PcgAffine two = pcg_affine(kLensDefaultStream, 2);
    PcgAffine cur;
    for (uint64_t k = 0; k < wh; ++k) {
        by_pos[k] = cur;
        cur = pcg_then(cur, two);
    }
    t.pix.resize(wh);
    for (uint64_t i = 0; i < wh; ++i) t.pix[i] = make_ulonglong2(by_pos[pos[i]].a, by_pos[pos[i]].c);
    const PcgAffine round1 = pcg_affine(kLensDefaultStream, 2 * wh);
    cur = PcgAffine();
    t.lo.resize(nhd::kLensLo);
    for (int l = 0; l < nhd::kLensLo; ++l) {
        t.lo[l] = make_ulonglong2(cur.a, cur.c);
        cur = pcg_then(cur, round1);
    }
    const PcgAffine round_hi = pcg_affine(kLensDefaultStream, 2 * wh * (uint64_t)nhd::kLensLo);
    uint64_t st = kLensDefaultState;
    t.hi.resize(nhd::kLensHi);
    for (int hh = 0; hh < nhd::kLensHi; ++hh) {
        t.hi[hh] = st;
        st = round_hi.a * st + round_hi.c;
    }
    return t;
}

// Can a light sample ever be non-finite, or land on a discrete-BSDF (mirror / dielectric) shading point? No, when:
// every emitter is an area light or the envmap, with finite radiance (and a finite constant env colour); every
// shape's box is finite and well inside float range (no overflow in the sample's squared distance); and the box of
// every area light's shape, widened by a relative margin for rounding, is disjoint from the widened box of every
// shape with a discrete BSDF (so the sampled point p and the shading point ref always differ: a zero distance is the
// only way the area light's pdf becomes 0/0, emitter_pdf). Then the wavefront shade may skip the light sample of a
// discrete BSDF sample, which is zeroed by the reference anyway (path_mis.cpp:136-140).
// A non-constant envmap also needs a finite, positive luminance normalization.
bool nee_finite(const nh_scene_desc *d) {
    auto fin = [](float x) { return std::fabs(x) < 1e15f; };
    for (uint32_t i = 0; i < d->n_emitters; ++i) {
        const nh_emitter &e = d->emitters[i];
        // (point and spot lights divide by the squared distance to the shading point; a directional light is left
        // out with them, conservatively: nobody has shown its sample finite at every discrete-BSDF point)
        if (e.type != NH_EMITTER_AREA && e.type != NH_EMITTER_ENVMAP) return false;
        for (int k = 0; k < 3; ++k)
            if (!std::isfinite(e.radiance[k])) return false;
    }
    if (d->envmap >= 0 && d->env.constant && d->env.rgba)
        for (int k = 0; k < 3; ++k)
            if (!std::isfinite(d->env.rgba[k])) return false;
    // a PNG envmap's luminance table must be a proper distribution: an all-black image leaves its normalization
    // 1/0, and the reference's light sample is then NaN, which ImageBlock drops with the whole sample
    if (d->envmap >= 0 && !d->env.constant && !(std::isfinite(d->env.normalization) && d->env.normalization > 0.f))
        return false;
    struct Box { float lo[3], hi[3]; };
    auto widened = [&](const nh_shape &s, Box &b) {
        float ext = 0.f;
        for (int k = 0; k < 3; ++k) {
            if (!fin(s.bbox_min[k]) || !fin(s.bbox_max[k])) return false;
            ext = std::max(ext, std::max(std::fabs(s.bbox_min[k]), std::fabs(s.bbox_max[k])));
        }
        const float m = 1e-3f * ext + 1e-6f;
        for (int k = 0; k < 3; ++k) {
            b.lo[k] = s.bbox_min[k] - m;
            b.hi[k] = s.bbox_max[k] + m;
        }
        return true;
    };
    for (uint32_t i = 0; i < d->n_shapes; ++i) {
        const nh_shape &si = d->shapes[i];
        Box bi;
        if (!widened(si, bi)) return false;
        if (si.emitter < 0) continue;
        for (uint32_t j = 0; j < d->n_shapes; ++j) {
            const nh_shape &sj = d->shapes[j];
            if (sj.bsdf < 0) continue;  // (no BSDF: a medium boundary)
            const int t = d->bsdfs[sj.bsdf].type;
            if (t != NH_BSDF_MIRROR && t != NH_BSDF_DIELECTRIC) continue;
            Box bj;
            if (!widened(sj, bj)) return false;
            bool apart = false;
            for (int k = 0; k < 3; ++k) apart = apart || bi.hi[k] < bj.lo[k] || bj.hi[k] < bi.lo[k];
            if (!apart) return false;
        }
    }
    return true;
}

// Isolated spheres (nhd::kPrimIsolated, nh_traverse.h trace_next): a dielectric sphere's record whose box grown by 2m
// lies apart from every other primitive's box gets the bit (only a dielectric sends its rays inside: for the others
// the sphere test would almost always be a wasted one), and m in its record 1 .x (only read by the sphere shortcut). m is
// 1e-4 of the scene's largest extent -- far above the float rounding of any hit point, far below the gaps of
// real scenes (the Cornell box's spheres clear its floor by 6e-3). Boxes are compared in double, closed: a box
// that touches or holds a NaN is not apart. NH_ISO_SPHERE=0 leaves every sphere unmarked (every ray walks the
// tree). Spheres x primitives box tests, skipped (no marks) past 2e8. Returns the number marked.
// Primitives whose box meets the query box [qlo, qhi] (double): a walk of the uploaded binary tree (child boxes in
// the parent, float) with the query grown by `slack` at the node tests, so a node box that rounds inward of its
// primitives' double boxes cannot hide one; the primitive boxes themselves decide (was a linear scan of
// every primitive per dielectric sphere).
static void prims_near_box(const std::vector<float4> &nodes, const std::vector<int2> &leaves, int root_kind,
                           const double qlo[3], const double qhi[3], double slack, std::vector<uint32_t> &out) {
    out.clear();
    auto leaf = [&](int l) {
        const int2 lf = leaves[(size_t)l];
        for (int k = 0; k < lf.y; ++k) out.push_back((uint32_t)(lf.x + k));
    };
    if (root_kind == 2) leaf(0);
    if (root_kind != 1) return;
    auto meets = [&](const float lo[3], const float hi[3]) {
        for (int a = 0; a < 3; ++a)
            if ((double)hi[a] < qlo[a] - slack || (double)lo[a] > qhi[a] + slack) return false;
        return true;
    };
    std::vector<int> st{0};
    while (!st.empty()) {
        const int g = st.back();
        st.pop_back();
        const float4 *n = &nodes[4 * (size_t)g];
        const float llo[3] = {n[0].x, n[0].y, n[0].z}, lhi[3] = {n[0].w, n[1].x, n[1].y};
        const float rlo[3] = {n[1].z, n[1].w, n[2].x}, rhi[3] = {n[2].y, n[2].z, n[2].w};
        int4 r4;
        std::memcpy(&r4, &n[3], sizeof(int4));
        const int ref[2] = {r4.x, r4.y};
        const bool hit[2] = {meets(llo, lhi), meets(rlo, rhi)};
        for (int ch = 0; ch < 2; ++ch)
            if (hit[ch]) {
                if (ref[ch] >= 0) st.push_back(ref[ch]);
                else leaf(~ref[ch]);
            }
    }
}

// Marks dielectric spheres whose box, grown by 2m (m = 1e-4 of the scene extent), is apart from every other
// primitive's box (the isolated-sphere closest hit of nh_traverse.h `trace_next`); m goes into the record.
static int mark_isolated_spheres(std::vector<float4> &prims, const std::vector<float4> &nodes,
                                 const std::vector<int2> &leaves, int root_kind, const std::vector<int> &shape_bsdf) {
    const char *e = std::getenv("NH_ISO_SPHERE");
    if (e && e[0] == '0') return 0;
    const size_t n = prims.size() / 3;
    std::vector<size_t> sph;
    for (size_t k = 0; k < n; ++k) {
        int bits, shape;
        std::memcpy(&bits, &prims[3 * k + 2].w, 4);
        std::memcpy(&shape, &prims[3 * k + 1].w, 4);  // (the record's key bits may be a Disney BSDF's borrowed key)
        if ((bits & nhd::kPrimSphere) && shape_bsdf[(size_t)shape] == NH_BSDF_DIELECTRIC) sph.push_back(k);
    }
    if (sph.empty()) return 0;
    auto prim_box = [&](size_t k, double lo[3], double hi[3]) {
        const float4 *p = &prims[3 * k];
        int bits;
        std::memcpy(&bits, &p[2].w, 4);
        for (int a = 0; a < 3; ++a) {
            const double v0 = a == 0 ? p[0].x : a == 1 ? p[0].y : p[0].z;
            if (bits & nhd::kPrimSphere) {
                lo[a] = v0 - (double)p[0].w;
                hi[a] = v0 + (double)p[0].w;
            } else {
                const double v1 = a == 0 ? p[1].x : a == 1 ? p[1].y : p[1].z;
                const double v2 = a == 0 ? p[2].x : a == 1 ? p[2].y : p[2].z;
                lo[a] = std::min(v0, std::min(v1, v2));
                hi[a] = std::max(v0, std::max(v1, v2));
            }
        }
    };
    // the scene extent from the root box (the union of every primitive's float box)
    double ext = 0.0, mag = 0.0;
    if (root_kind == 0) return 0;
    {
        double slo[3] = {INFINITY, INFINITY, INFINITY}, shi[3] = {-INFINITY, -INFINITY, -INFINITY};
        for (size_t k = 0; k < n; ++k) {
            double lo[3], hi[3];
            prim_box(k, lo, hi);
            for (int a = 0; a < 3; ++a) {
                slo[a] = std::min(slo[a], lo[a]);
                shi[a] = std::max(shi[a], hi[a]);
            }
        }
        ext = std::max(shi[0] - slo[0], std::max(shi[1] - slo[1], shi[2] - slo[2]));
        for (int a = 0; a < 3; ++a) mag = std::max(mag, std::max(std::fabs(slo[a]), std::fabs(shi[a])));
    }
    if (!(ext > 0.0) || !std::isfinite(ext)) return 0;
    const float m = (float)(1e-4 * ext);
    // far above the float rounding (2^-24 relative) of any node box coordinate in the scene
    const double slack = 1e-6 * (ext + mag);
    int marked = 0;
    std::vector<uint32_t> near;
    for (size_t s : sph) {
        const float4 a = prims[3 * s];
        if (!(a.w > 0.f) || !std::isfinite(a.w) || !std::isfinite(a.x) || !std::isfinite(a.y) || !std::isfinite(a.z))
            continue;
        const double g = (double)a.w + 2.0 * (double)m;
        const double glo[3] = {(double)a.x - g, (double)a.y - g, (double)a.z - g};
        const double ghi[3] = {(double)a.x + g, (double)a.y + g, (double)a.z + g};
        prims_near_box(nodes, leaves, root_kind, glo, ghi, slack, near);
        bool apart = true;
        for (uint32_t k : near) {
            if (k == s) continue;
            double lo[3], hi[3];
            prim_box(k, lo, hi);
            bool sep = false;
            for (int ax = 0; ax < 3; ++ax) sep = sep || hi[ax] < glo[ax] || lo[ax] > ghi[ax];
            if (!sep) {
                apart = false;
                break;
            }
        }
        if (!apart) continue;
        int bits;
        std::memcpy(&bits, &prims[3 * s + 2].w, 4);
        bits |= nhd::kPrimIsolated;
        std::memcpy(&prims[3 * s + 2].w, &bits, 4);
        prims[3 * s + 1].x = m;
        ++marked;
    }
    return marked;
}

// W-wide collapse (W = 4 or 8) of the GPU binary tree (nh_traverse.h Tracer4 / Tracer8): every wide node takes
// the two children of a binary node and, while it has fewer than W, replaces its largest-area inner child by that
// child's two children in place (left-first DFS order of the slots is kept). Wide nodes are numbered depth first,
// the first child next to its parent. Boxes are the binary tree's own. An 8-wide node is two 4-wide lines
// (children 0-3, 4-7), each in the 4-wide layout.
std::vector<float4> collapse_wide(const std::vector<float4> &nodes, const std::vector<int2> &leaves, int &depth_out,
                                  int W) {
    struct Child {
        float mn[3], mx[3];
        int ref;  // binary: >= 0 inner node, < 0 leaf ~index
    };
    auto child = [&](int g, int side) {
        const float *f = reinterpret_cast<const float *>(&nodes[4 * (size_t)g]);
        Child ch;
        const int o = side ? 6 : 0;
        for (int i = 0; i < 3; ++i) { ch.mn[i] = f[o + i]; ch.mx[i] = f[o + 3 + i]; }
        int refs[2];
        std::memcpy(refs, &nodes[4 * (size_t)g + 3], 8);
        ch.ref = refs[side];
        return ch;
    };
    auto area = [](const Child &c) {
        const float x = c.mx[0] - c.mn[0], y = c.mx[1] - c.mn[1], z = c.mx[2] - c.mn[2];
        return x * y + y * z + z * x;
    };
    std::vector<float4> wide;
    depth_out = 0;
    if (nodes.empty()) return wide;
    const int lines = W / 4, nf4 = lines * nhd::kWideF4;
    std::function<int(int, int)> make = [&](int g, int depth) -> int {
        depth_out = std::max(depth_out, depth);
        const int idx = (int)(wide.size() / nf4);
        wide.resize(wide.size() + nf4);
        std::vector<Child> ch{child(g, 0), child(g, 1)};
        while ((int)ch.size() < W) {
            int best = -1;
            float best_a = -1.f;
            for (int i = 0; i < (int)ch.size(); ++i)
                if (ch[i].ref >= 0 && area(ch[i]) > best_a) { best = i; best_a = area(ch[i]); }
            if (best < 0) break;
            const int gi = ch[best].ref;
            ch[best] = child(gi, 1);
            ch.insert(ch.begin() + best, child(gi, 0));
        }
        int refs[8];
        float box[6][8];
        for (int j = 0; j < 8; ++j) {
            refs[j] = nhd::kWideEmpty;
            for (int a = 0; a < 3; ++a) { box[a][j] = 0.f; box[3 + a][j] = 0.f; }
        }
        for (int j = 0; j < (int)ch.size(); ++j) {
            for (int a = 0; a < 3; ++a) { box[a][j] = ch[j].mn[a]; box[3 + a][j] = ch[j].mx[a]; }
            if (ch[j].ref >= 0) {
                refs[j] = make(ch[j].ref, depth + 1);
            } else {
                const int2 lf = leaves[(size_t)~ch[j].ref];
                refs[j] = lf.y > 0 ? ~lf.x : nhd::kWideEmpty;  // an empty leaf holds nothing to hit
            }
        }
        for (int h = 0; h < lines; ++h) {
            float4 *n = &wide[(size_t)idx * nf4 + (size_t)h * nhd::kWideF4];
            for (int a = 0; a < 6; ++a)
                n[a] = make_float4(box[a][4 * h], box[a][4 * h + 1], box[a][4 * h + 2], box[a][4 * h + 3]);
            std::memcpy(&n[6], refs + 4 * h, 16);
            n[7] = make_float4(0.f, 0.f, 0.f, 0.f);
        }
        return idx;
    };
    make(0, 1);
    return wide;
}

// Number the K wide nodes most rays visit first, so the persistent traversal can keep them in LDS: the
// connected top of the tree grown from the root by the largest child-box surface area (a ray's chance
// of entering a box grows with its area). The other nodes keep their depth-first order. Renumbering
// moves no box and changes no visit order: every answer is unchanged. Returns the top's size.
int number_top_first(std::vector<float4> &wide, const float root_min[3], const float root_max[3], int K, int W) {
    const int lines = W / 4, nf4 = lines * nhd::kWideF4;
    const int n = (int)(wide.size() / nf4);
    if (n == 0 || K <= 0) return 0;
    auto area = [](const float *mn, const float *mx) {
        const float x = mx[0] - mn[0], y = mx[1] - mn[1], z = mx[2] - mn[2];
        return x * y + y * z + z * x;
    };
    std::vector<int> order;  // new index -> old index, for the top
    std::vector<char> in_top(n, 0);
    std::vector<std::pair<float, int>> heap{{area(root_min, root_max), 0}};
    while (!heap.empty() && (int)order.size() < K) {
        std::pop_heap(heap.begin(), heap.end());
        const int g = heap.back().second;
        heap.pop_back();
        order.push_back(g);
        in_top[g] = 1;
        for (int h = 0; h < lines; ++h) {
            const float *f = reinterpret_cast<const float *>(&wide[(size_t)g * nf4 + (size_t)h * nhd::kWideF4]);
            int refs[4];
            std::memcpy(refs, f + 24, 16);
            for (int j = 0; j < 4; ++j) {
                if (refs[j] < 0) continue;  // a leaf or an empty slot
                const float mn[3] = {f[j], f[4 + j], f[8 + j]}, mx[3] = {f[12 + j], f[16 + j], f[20 + j]};
                heap.push_back({area(mn, mx), refs[j]});
                std::push_heap(heap.begin(), heap.end());
            }
        }
    }
    std::vector<int> perm(n);  // old -> new
    for (int i = 0; i < (int)order.size(); ++i) perm[order[i]] = i;
    int next = (int)order.size();
    for (int g = 0; g < n; ++g)
        if (!in_top[g]) perm[g] = next++;
    std::vector<float4> out(wide.size());
    for (int g = 0; g < n; ++g) {
        float4 *dst = &out[(size_t)perm[g] * nf4];
        std::memcpy(dst, &wide[(size_t)g * nf4], nf4 * sizeof(float4));
        for (int h = 0; h < lines; ++h) {
            int refs[4];
            std::memcpy(refs, &dst[h * nhd::kWideF4 + 6], 16);
            for (int j = 0; j < 4; ++j)
                if (refs[j] >= 0) refs[j] = perm[refs[j]];
            std::memcpy(&dst[h * nhd::kWideF4 + 6], refs, 16);
        }
    }
    wide.swap(out);
    return (int)order.size();
}

int build_gpu_bvh(const nh_bvh_desc &desc, const std::vector<nh_shape> &shapes, const std::vector<float> &V,
                  const std::vector<uint32_t> &F, const std::vector<int> &shape_mat_key,
                  const std::vector<int> &shape_bsdf_real, int wide_w, int top_k, GpuBvh &S, std::string &err) {
    const nh_bvh_desc *b = &desc;
    auto fail = [&](const std::string &m) {
        err = m;
        return false;
    };
    S = GpuBvh{};
    // primitive id -> (shape, local)
    std::vector<uint32_t> &off = S.shape_offset;
    off.assign(1, 0u);
    for (auto &s : shapes) off.push_back(off.back() + (s.type == NH_SHAPE_MESH ? s.n_faces : 1u));
    if (b->n_indices != off.back()) return fail("BVH primitive count does not match the scene"), NH_ERR_INVALID;
    if (b->n_indices > 0 && b->n_nodes == 0) return fail("empty BVH for a non-empty scene"), NH_ERR_INVALID;

    std::vector<float4> &nodes = S.nodes;
    std::vector<int2> &leaves = S.leaves;
    uint32_t &tree_depth = S.tree_depth;
    if (b->n_nodes == 0) {
        S.root_kind = 0;
    } else {
        const nh_bvh_node *N = b->nodes;
        for (int i = 0; i < 3; ++i) { S.root_min[i] = N[0].bbox_min[i]; S.root_max[i] = N[0].bbox_max[i]; }
        if (N[0].word0 & 1u) {
            S.root_kind = 2;
            leaves.push_back(make_int2((int)N[0].word1, (int)(N[0].word0 >> 1)));
        } else {
            S.root_kind = 1;
            // DFS (left first) over inner nodes assigning GPU ids in visit order
            // (the tree's depth is measured here, not taken from nh_bvh_desc::max_depth: it sizes the
            // traversal stacks)
            std::vector<int> gid(b->n_nodes, -1);
            std::vector<uint32_t> order;
            std::vector<std::pair<uint32_t, uint32_t>> st{{0u, 0u}};  // (node, level)
            while (!st.empty()) {
                const uint32_t i = st.back().first, lvl = st.back().second;
                st.pop_back();
                tree_depth = std::max(tree_depth, lvl);
                if (N[i].word0 & 1u) continue;
                if (gid[i] >= 0) return fail("corrupt BVH: node reached twice"), NH_ERR_INVALID;
                gid[i] = (int)order.size();
                order.push_back(i);
                if (N[i].word1 >= b->n_nodes || i + 1 >= b->n_nodes)
                    return fail("corrupt BVH child index"), NH_ERR_INVALID;
                st.push_back({N[i].word1, lvl + 1});
                st.push_back({i + 1, lvl + 1});
            }
            nodes.resize(4 * order.size());
            auto child_ref = [&](uint32_t ch) -> int {
                if (N[ch].word0 & 1u) {
                    leaves.push_back(make_int2((int)N[ch].word1, (int)(N[ch].word0 >> 1)));
                    return ~(int)(leaves.size() - 1);
                }
                return gid[ch];
            };
            for (size_t g = 0; g < order.size(); ++g) {
                uint32_t i = order[g];
                const nh_bvh_node &L = N[i + 1], &R = N[N[i].word1];
                int lr = child_ref(i + 1), rr = child_ref(N[i].word1);
                nodes[4 * g] = make_float4(L.bbox_min[0], L.bbox_min[1], L.bbox_min[2], L.bbox_max[0]);
                nodes[4 * g + 1] = make_float4(L.bbox_max[1], L.bbox_max[2], R.bbox_min[0], R.bbox_min[1]);
                nodes[4 * g + 2] = make_float4(R.bbox_min[2], R.bbox_max[0], R.bbox_max[1], R.bbox_max[2]);
                int4 r4 = make_int4(lr, rr, 0, 0);
                std::memcpy(&nodes[4 * g + 3], &r4, sizeof(int4));
            }
        }
    }
    // primitives in leaf order
    std::vector<float4> &prims = S.prims;
    prims.resize(3 * (size_t)b->n_indices);
    for (uint32_t k = 0; k < b->n_indices; ++k) {
        uint32_t g = b->indices[k];
        if (g >= off.back()) return fail("BVH index out of range"), NH_ERR_INVALID;
        uint32_t s = (uint32_t)(std::upper_bound(off.begin(), off.end(), g) - off.begin()) - 1;
        uint32_t local = g - off[s];
        const nh_shape &sh = shapes[s];
        float4 *p = &prims[3 * (size_t)k];
        int si = (int)s, one = 1, zero = 0;
        float fs, f1, f0;
        std::memcpy(&fs, &si, 4);
        std::memcpy(&f1, &one, 4);
        std::memcpy(&f0, &zero, 4);
        const int mat = shape_mat_key[s] << nhd::kPrimMatShift;
        if (sh.type == NH_SHAPE_SPHERE) {
            const int flags = 1 | mat;
            std::memcpy(&f1, &flags, 4);
            p[0] = make_float4(sh.center[0], sh.center[1], sh.center[2], sh.radius);
            p[1] = make_float4(0, 0, 0, fs);
            p[2] = make_float4(0, 0, 0, f1);
        } else {
            std::memcpy(&f0, &mat, 4);
            const uint32_t *f = &F[3 * ((size_t)sh.f_offset + local)];
            const float *p0 = &V[3 * ((size_t)sh.v_offset + f[0])], *p1 = &V[3 * ((size_t)sh.v_offset + f[1])],
                        *p2 = &V[3 * ((size_t)sh.v_offset + f[2])];
            int li = (int)local;
            float fl;
            std::memcpy(&fl, &li, 4);
            p[0] = make_float4(p0[0], p0[1], p0[2], fl);
            p[1] = make_float4(p1[0], p1[1], p1[2], fs);
            p[2] = make_float4(p2[0], p2[1], p2[2], f0);
        }
    }
    S.iso_spheres = mark_isolated_spheres(prims, nodes, leaves, S.root_kind, shape_bsdf_real);
    // leaf-end bits: the 4-wide traversal walks a leaf's records until this bit
    for (const int2 &lf : leaves)
        if (lf.y > 0) {
            float4 &w = prims[3 * ((size_t)lf.x + lf.y - 1) + 2];
            int bits;
            std::memcpy(&bits, &w.w, 4);
            bits |= nhd::kPrimLeafEnd;
            std::memcpy(&w.w, &bits, 4);
        }
    // The binary-tree kernels keep a per-lane stack of at most kMaxStack entries (the deferred
    // children of one root-to-leaf path; the reference keeps 64, bvh.cpp:403)
    if (tree_depth + 2 > (uint32_t)nhd::kMaxStack)
        return fail("BVH deeper than " + std::to_string(nhd::kMaxStack - 2) + " levels is not supported"), NH_ERR_UNSUPPORTED;
    // the wide tree of the persistent kernels (wide_w children per node), the top_k nodes most rays visit numbered first
    int depth4 = 0;
    S.wide = collapse_wide(nodes, leaves, depth4, wide_w);
    S.n_top = S.root_kind == 1 ? number_top_first(S.wide, S.root_min, S.root_max, top_k, wide_w) : 0;
    // deferred entries: at most W - 1 per wide level (+1 slack)
    S.depth_wide = (wide_w - 1) * depth4 + 1;
    // one zero record past the end: the 4-wide traversal loads record k+1 together with record k
    // (and tests it only when k does not end its leaf)
    prims.resize(prims.size() + 3, make_float4(0.f, 0.f, 0.f, 0.f));
    return NH_OK;
}

PairLayout pair_layout(const i2 *leaves, int n_leaves, const f4 *prims, int n_records, bool by_kind) {
    PairLayout out;
    out.slots.assign((size_t)n_records, make_int2(-1, -1));
    out.leaves.resize((size_t)n_leaves);
    if (!by_kind) {
        for (int p = 0; p < n_records; ++p) out.slots[(size_t)p] = make_int2(p, p + 1 < n_records ? p + 1 : -1);
        for (int l = 0; l < n_leaves; ++l) out.leaves[(size_t)l] = make_int2(leaves[l].x, 0);
        return out;
    }
    std::vector<int> kind[2];  // a leaf's triangles / spheres, in record order
    for (int l = 0; l < n_leaves; ++l) {
        const int2 lf = leaves[l];
        kind[0].clear();
        kind[1].clear();
        for (int k = lf.x; k < lf.x + lf.y; ++k) {
            int bits;
            std::memcpy(&bits, &prims[3 * (size_t)k + 2].w, 4);
            kind[bits & nhd::kPrimSphere ? 1 : 0].push_back(k);
        }
        // (pairs never outnumber records: ceil(t / 2) + ceil(s / 2) <= t + s, so the positions stay inside the leaf's own)
        int p = lf.x;
        for (const std::vector<int> &v : kind)
            for (size_t i = 0; i < v.size(); i += 2) out.slots[(size_t)p++] = make_int2(v[i], i + 1 < v.size() ? v[i + 1] : -1);
        const int n_tri = ((int)kind[0].size() + 1) / 2, n_sph = ((int)kind[1].size() + 1) / 2;
        out.leaves[(size_t)l] = make_int2(lf.x, n_tri | (n_sph << 16));
    }
    return out;
}

bool flat_trace_knob() {
    const char *e = std::getenv("NH_FLAT_TRACE");
    return !(e && e[0] == '0');
}

FlatImage flat_image(const float boxes[18], const i2 *leaves, int n_leaves, const f4 *prims, int n_records,
                     const PairLayout &pl, bool allowed, uint64_t any_word) {
    FlatImage out;
    if (!allowed || n_leaves < 1 || n_leaves > 2 || n_records < 1 || (int)pl.leaves.size() != n_leaves) return out;
    int n_pairs = 0;
    for (int l = 0; l < n_leaves; ++l) {
        const int2 p = pl.leaves[(size_t)l];
        if (p.y == 0 && leaves[l].y > 0) return out;  // (not an arrangement by kind)
        n_pairs += (p.y & 0xffff) + (p.y >> 16);
    }
    if (n_pairs < 1 || n_pairs > nhd::kFlatMaxPairs) return out;
    const auto same_bits = [](const float *a, const float *b) { return std::memcmp(a, b, 6 * sizeof(float)) == 0; };
    const auto as_float = [](int v) {
        float f;
        std::memcpy(&f, &v, 4);
        return f;
    };
    const float *root = boxes, *lb = n_leaves == 2 ? boxes + 6 : boxes, *rb = n_leaves == 2 ? boxes + 12 : boxes;
    // The any-hit section: each leaf's kept records (any_word) paired again by pair_layout's rules -- a leaf of their
    // own ranges would split the records, so the kept ones are listed and paired here the same way: triangles two by
    // two in record order, then spheres, a lone record repeated. None when nothing is left out.
    const uint64_t in_use = n_records < 64 ? ~(~(uint64_t)0 << n_records) : ~(uint64_t)0;
    const bool any_list = n_records <= 64 && (any_word & in_use) != in_use;
    std::vector<int2> any_slots[2];
    int any_counts[2] = {0, 0};
    if (any_list)
        for (int l = 0; l < n_leaves; ++l) {
            std::vector<int> kind[2];
            for (int k = leaves[l].x; k < leaves[l].x + leaves[l].y; ++k) {
                if (k < 0 || k >= n_records) return out;
                if (!((any_word >> k) & 1)) continue;
                int bits;
                std::memcpy(&bits, &prims[3 * (size_t)k + 2].w, 4);
                kind[bits & nhd::kPrimSphere ? 1 : 0].push_back(k);
            }
            for (const std::vector<int> &v : kind)
                for (size_t i = 0; i < v.size(); i += 2)
                    any_slots[l].push_back(make_int2(v[i], i + 1 < v.size() ? v[i + 1] : -1));
            any_counts[l] = ((int)kind[0].size() + 1) / 2 | (((int)kind[1].size() + 1) / 2) << 16;
        }
    out.any_list = any_list;
    out.box_equal = n_leaves == 1 ? nhd::kFlatLeftEq
                                  : (same_bits(lb, root) ? nhd::kFlatLeftEq : 0) | (same_bits(rb, root) ? nhd::kFlatRightEq : 0);
    out.data.reserve((size_t)nhd::kFlatHeaderF4 + (size_t)nhd::kPairF4 * (any_list ? 2 * nhd::kFlatMaxPairs : n_pairs));
    out.data.push_back(make_float4(root[0], root[1], root[2], as_float(out.box_equal | (any_list ? nhd::kFlatAnyList : 0))));
    out.data.push_back(make_float4(root[3], root[4], root[5], as_float(n_leaves)));
    out.data.push_back(make_float4(lb[0], lb[1], lb[2], as_float(pl.leaves[0].y)));
    out.data.push_back(make_float4(lb[3], lb[4], lb[5], as_float(any_counts[0])));
    out.data.push_back(make_float4(rb[0], rb[1], rb[2], as_float(n_leaves == 2 ? pl.leaves[1].y : 0)));
    out.data.push_back(make_float4(rb[3], rb[4], rb[5], as_float(any_counts[1])));
    const auto pair_record = [&](int2 s) {
        const int k = s.x, k1 = s.y < 0 ? k : s.y;
        if (k < 0 || k >= n_records || k1 >= n_records) return false;  // (a layout of other leaves)
        // the pair record of build_pairs_frames (csrc/nh_wavefront.hip), by the same float subtractions
        const float4 a = prims[3 * (size_t)k], b = prims[3 * (size_t)k + 1], c = prims[3 * (size_t)k + 2];
        const float4 a1 = prims[3 * (size_t)k1], b1 = prims[3 * (size_t)k1 + 1], c1 = prims[3 * (size_t)k1 + 2];
        out.data.push_back(make_float4(a.x, a1.x, a.y, a1.y));
        out.data.push_back(make_float4(a.z, a1.z, a.w, a1.w));
        out.data.push_back(make_float4(b.x - a.x, b1.x - a1.x, b.y - a.y, b1.y - a1.y));
        out.data.push_back(make_float4(b.z - a.z, b1.z - a1.z, c.x - a.x, c1.x - a1.x));
        out.data.push_back(make_float4(c.y - a.y, c1.y - a1.y, c.z - a.z, c1.z - a1.z));
        out.data.push_back(make_float4(c.w, c1.w, as_float(k), as_float(k1)));
        return true;
    };
    for (int l = 0; l < n_leaves; ++l) {
        const int2 p = pl.leaves[(size_t)l];
        for (int i = 0, n = (p.y & 0xffff) + (p.y >> 16); i < n; ++i)
            if (!pair_record(pl.slots[(size_t)(p.x + i)])) return FlatImage{};
    }
    if (any_list) {
        // at its fixed offset, behind room for kFlatMaxPairs closest-hit records (the unused ones zero)
        out.data.resize((size_t)nhd::kFlatHeaderF4 + (size_t)nhd::kPairF4 * nhd::kFlatMaxPairs, make_float4(0.f, 0.f, 0.f, 0.f));
        for (int l = 0; l < n_leaves; ++l)
            for (const int2 &s : any_slots[l])
                if (!pair_record(s)) return FlatImage{};
    }
    out.flat = true;
    return out;
}

}  // namespace nh

extern "C" {

int nh_flat_image_any(const float *records, int32_t n_records, const int32_t *leaves, int32_t n_leaves,
                      const float *boxes, int32_t allowed, uint64_t any_word, float *image, int32_t image_cap_f4,
                      int32_t *n_f4, int32_t *box_equal) {
    bool ok = n_records >= 0 && n_leaves >= 0 && (n_records == 0 || records) && (n_leaves == 0 || leaves) && boxes &&
              n_f4 && box_equal && image_cap_f4 >= 0 && (image_cap_f4 == 0 || image);
    std::vector<char> used((size_t)std::max(n_records, 0), 0);  // (as nh_pair_layout)
    for (int l = 0; ok && l < n_leaves; ++l) {
        const int64_t s = leaves[2 * l], n = leaves[2 * l + 1];
        ok = s >= 0 && n >= 0 && n < 65535 && s + n <= n_records;
        for (int64_t k = s; ok && k < s + n; ++k) {
            ok = !used[(size_t)k];
            used[(size_t)k] = 1;
        }
    }
    if (!ok) {
        nh::set_host_error("nh_flat_image: invalid argument");
        return NH_ERR_INVALID;
    }
    const nh::i2 *lv = reinterpret_cast<const nh::i2 *>(leaves);
    const nh::f4 *rec = reinterpret_cast<const nh::f4 *>(records);
    const nh::PairLayout pl = nh::pair_layout(lv, n_leaves, rec, n_records, true);
    const nh::FlatImage fi = nh::flat_image(boxes, lv, n_leaves, rec, n_records, pl, allowed != 0 && nh::flat_trace_knob(),
                                            nh::any_list_knob() ? any_word : ~(uint64_t)0);
    *n_f4 = fi.flat ? (int32_t)fi.data.size() : 0;
    *box_equal = fi.box_equal;
    if (fi.flat) {
        if ((size_t)image_cap_f4 < fi.data.size()) {
            nh::set_host_error("nh_flat_image: image buffer too small");
            return NH_ERR_INVALID;
        }
        std::memcpy(image, fi.data.data(), fi.data.size() * sizeof(nh::f4));
    }
    return NH_OK;
}

int nh_flat_image(const float *records, int32_t n_records, const int32_t *leaves, int32_t n_leaves, const float *boxes,
                  int32_t allowed, float *image, int32_t image_cap_f4, int32_t *n_f4, int32_t *box_equal) {
    return nh_flat_image_any(records, n_records, leaves, n_leaves, boxes, allowed, ~(uint64_t)0, image, image_cap_f4, n_f4,
                             box_equal);
}

int nh_pair_layout(const float *records, int32_t n_records, const int32_t *leaves, int32_t n_leaves, int32_t by_kind,
                   int32_t *slots, int32_t *leaf_pairs) {
    bool ok = n_records >= 0 && n_leaves >= 0 && (n_records == 0 || (records && slots)) &&
              (n_leaves == 0 || (leaves && leaf_pairs));
    // the leaves' ranges: inside the records, no record in two leaves, fewer than 2^15 pairs of a kind
    std::vector<char> used((size_t)std::max(n_records, 0), 0);
    for (int l = 0; ok && l < n_leaves; ++l) {
        const int64_t s = leaves[2 * l], n = leaves[2 * l + 1];
        ok = s >= 0 && n >= 0 && n < 65535 && s + n <= n_records;
        for (int64_t k = s; ok && k < s + n; ++k) {
            ok = !used[(size_t)k];
            used[(size_t)k] = 1;
        }
    }
    if (!ok) {
        nh::set_host_error("nh_pair_layout: invalid argument");
        return NH_ERR_INVALID;
    }
    static_assert(sizeof(nh::f4) == 4 * sizeof(float) && sizeof(nh::i2) == 2 * sizeof(int32_t), "plain arrays");
    const nh::PairLayout pl = nh::pair_layout(reinterpret_cast<const nh::i2 *>(leaves), n_leaves,
                                              reinterpret_cast<const nh::f4 *>(records), n_records, by_kind != 0);
    if (n_records > 0) std::memcpy(slots, pl.slots.data(), (size_t)n_records * sizeof(nh::i2));
    for (int l = 0; l < n_leaves; ++l) {
        leaf_pairs[3 * l] = pl.leaves[(size_t)l].x;
        leaf_pairs[3 * l + 1] = pl.leaves[(size_t)l].y & 0xffff;
        leaf_pairs[3 * l + 2] = pl.leaves[(size_t)l].y >> 16;
    }
    return NH_OK;
}

}  // extern "C"
