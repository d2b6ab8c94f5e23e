// CPU check of the host-side GPU layout code (optix-renderer_amd/host/gpu_layout.cpp): the arrays every traversal
// kernel walks, the isolated-sphere marks, the block spiral and the lens-stream tables, each against a property
// derived independently from the scene and the reference-layout BVH. Run by tests/test_gpu_layout_host.py.
//
//   gpu_layout_check tables                          spiral_rank, serial_ray_index, lens_tables
//   gpu_layout_check scene FILE.xml [iso=N] [nee=B] [split]
//       everything that depends on a scene; iso: isolated spheres expected, nee: nee_finite expected, split: a
//       two-triangle scene under a hand-made BVH of one inner node and two leaves instead of the builder's one leaf
// Exits non-zero with a message on the first violated property.
#include <algorithm>
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <map>
#include <string>
#include <utility>
#include <vector>

#include "gpu_layout.h"
#include "nh_layout.h"
#include "nori_hip.h"

namespace {

[[noreturn]] void die(const std::string &what) {
    std::fprintf(stderr, "gpu_layout_check: FAILED: %s\n", what.c_str());
    std::exit(1);
}
#define CHECK(cond, what)                                                       \
    do {                                                                        \
        if (!(cond)) die(std::string(what) + "  [" #cond "]");                  \
    } while (0)

int bits_of(float f) {
    int b;
    std::memcpy(&b, &f, 4);
    return b;
}
std::string num(long long v) { return std::to_string(v); }

// ---------------------------------------------------------------- tables
void check_permutation(const std::vector<uint32_t> &v, const std::string &what) {
    std::vector<char> seen(v.size(), 0);
    for (uint32_t x : v) {
        CHECK(x < v.size(), what + ": value out of range");
        CHECK(!seen[x], what + ": value " + num(x) + " twice");
        seen[x] = 1;
    }
}

void check_spiral(int w, int h) {
    const std::string tag = "spiral_rank " + num(w) + "x" + num(h);
    int nbx = 0, nby = 0;
    const std::vector<int> rank = nh::spiral_rank(w, h, 32, nbx, nby);
    CHECK(nbx == (w + 31) / 32 && nby == (h + 31) / 32, tag + ": block counts");
    CHECK(rank.size() == (size_t)nbx * nby, tag + ": size");
    check_permutation(std::vector<uint32_t>(rank.begin(), rank.end()), tag);
    CHECK(rank[(size_t)(nby / 2) * nbx + nbx / 2] == 0, tag + ": the centre block is not first");
    check_permutation(nh::serial_ray_index(w, h, 32), "serial_ray_index " + num(w) + "x" + num(h));
}

void check_lens(int w, int h) {
    const std::string tag = "lens_tables " + num(w) + "x" + num(h);
    const nh::LensTables t = nh::lens_tables(w, h);
    const uint64_t wh = (uint64_t)w * h;
    CHECK(t.pix.size() == wh && t.lo.size() == (size_t)nhd::kLensLo && t.hi.size() == (size_t)nhd::kLensHi, tag + ": sizes");
    const std::vector<uint32_t> pos = nh::serial_ray_index(w, h, 32);
    std::vector<uint32_t> pixel_at(wh);  // serial position -> pixel
    for (uint64_t i = 0; i < wh; ++i) pixel_at[pos[i]] = (uint32_t)i;
    const int rounds[] = {0, 1, 255, 256, 257, 65535};
    // the default-stream pcg32 LCG (pcg32.h:29-30, :95-97), stepped one draw at a time
    uint64_t state = 0x853c49e6748fea9bULL, step = 0;
    const uint64_t mult = 0x5851f42d4c957f2dULL, inc = 0xda3e39cb94b95bdbULL;
    for (int round : rounds) {
        const nh::u64x2 lo = t.lo[round & (nhd::kLensLo - 1)];
        const uint64_t s_round = lo.x * t.hi[round / nhd::kLensLo] + lo.y;
        for (uint64_t p = 0; p < wh; ++p) {
            const uint64_t target = 2 * ((uint64_t)round * wh + p);
            for (; step < target; ++step) state = state * mult + inc;
            const nh::u64x2 pa = t.pix[pixel_at[p]];
            CHECK(pa.x * s_round + pa.y == state, tag + ": round " + num(round) + " position " + num((long long)p));
        }
    }
}

// ---------------------------------------------------------------- scene
struct Scene {
    nh_scene_desc d{};
    nh_bvh_desc b{};
    std::vector<nh_shape> shapes;
    std::vector<float> V;
    std::vector<uint32_t> F;
    std::vector<int> key, real;
    std::vector<uint32_t> off;  // first primitive id per shape
};

struct Box6 {
    float v[6];  // min xyz, max xyz
    bool operator==(const Box6 &o) const { return std::memcmp(v, o.v, sizeof(v)) == 0; }
};

// child `side` of GPU binary node g: its box and ref
void bin_child(const std::vector<nh::f4> &nodes, int g, int side, Box6 &box, int &ref) {
    const float *f = reinterpret_cast<const float *>(&nodes[4 * (size_t)g]);
    for (int i = 0; i < 6; ++i) box.v[i] = f[(side ? 6 : 0) + i];
    ref = bits_of(f[12 + side]);
}

int build(const Scene &s, const nh_bvh_desc &b, int W, int top_k, nh::GpuBvh &g, std::string &err) {
    return nh::build_gpu_bvh(b, s.shapes, s.V, s.F, s.key, s.real, W, top_k, g, err);
}

void check_flatten(const Scene &s, const nh::GpuBvh &g) {
    const nh_bvh_desc &b = s.b;
    const size_t n = b.n_indices;
    CHECK(g.prims.size() == 3 * (n + 1), "flatten: record count (one zero record past the end)");
    for (int i = 0; i < 3; ++i) {
        const nh::f4 z = g.prims[3 * n + i];
        CHECK(bits_of(z.x) == 0 && bits_of(z.y) == 0 && bits_of(z.z) == 0 && bits_of(z.w) == 0, "flatten: the appended record is not zero");
    }
    CHECK(g.root_kind == (b.n_nodes == 0 ? 0 : (b.nodes[0].word0 & 1u) ? 2 : 1), "flatten: root_kind");
    CHECK(g.shape_offset == s.off, "flatten: shape offsets");
    // the BVH's indices are a permutation, and the leaves tile the leaf-order positions
    check_permutation(std::vector<uint32_t>(b.indices, b.indices + n), "flatten: BVH indices");
    std::vector<int> covered(n, 0);
    std::vector<char> ends(n, 0);
    for (const nh::i2 &lf : g.leaves) {
        CHECK(lf.x >= 0 && lf.y >= 0 && (size_t)lf.x + lf.y <= n, "flatten: leaf range outside the records");
        for (int k = 0; k < lf.y; ++k) ++covered[(size_t)lf.x + k];
        if (lf.y > 0) ends[(size_t)lf.x + lf.y - 1] = 1;
    }
    for (size_t k = 0; k < n; ++k) {
        CHECK(covered[k] == 1, "flatten: primitive position " + num((long long)k) + " is in " + num(covered[k]) + " leaves");
        const nh::f4 *p = &g.prims[3 * k];
        const int bits = bits_of(p[2].w);
        CHECK(((bits & nhd::kPrimLeafEnd) != 0) == (ends[k] != 0), "flatten: leaf-end bit of record " + num((long long)k));
        const uint32_t id = b.indices[k];
        const uint32_t sh = (uint32_t)(std::upper_bound(s.off.begin(), s.off.end(), id) - s.off.begin()) - 1;
        const nh_shape &S = s.shapes[sh];
        CHECK(bits_of(p[1].w) == (int)sh, "flatten: shape id of record " + num((long long)k));
        CHECK(((bits >> nhd::kPrimMatShift) & 3) == s.key[sh], "flatten: material key of record " + num((long long)k));
        CHECK(((bits & nhd::kPrimSphere) != 0) == (S.type == NH_SHAPE_SPHERE), "flatten: sphere bit of record " + num((long long)k));
        if (S.type == NH_SHAPE_SPHERE) {
            CHECK(p[0].x == S.center[0] && p[0].y == S.center[1] && p[0].z == S.center[2] && p[0].w == S.radius, "flatten: sphere record");
        } else {
            const uint32_t local = id - s.off[sh];
            CHECK(bits_of(p[0].w) == (int)local, "flatten: local face of record " + num((long long)k));
            const uint32_t *f = &s.F[3 * ((size_t)S.f_offset + local)];
            for (int v = 0; v < 3; ++v) {
                const float *q = &s.V[3 * ((size_t)S.v_offset + f[v])];
                CHECK(p[v].x == q[0] && p[v].y == q[1] && p[v].z == q[2], "flatten: vertices of record " + num((long long)k));
            }
        }
    }
    // the GPU binary tree against nh_bvh_desc, node by node (left child i + 1, right child word1), and the depth
    uint32_t depth = 0;
    size_t inner = 0, leaves_seen = 0;
    if (g.root_kind == 2) {
        CHECK(g.leaves.size() == 1 && g.nodes.empty(), "flatten: a leaf root has one leaf and no node");
        CHECK(g.leaves[0].x == (int)b.nodes[0].word1 && g.leaves[0].y == (int)(b.nodes[0].word0 >> 1), "flatten: root leaf range");
        leaves_seen = 1;
    }
    if (g.root_kind == 1) {
        struct It { uint32_t i; int g; uint32_t lvl; };
        std::vector<It> st{{0u, 0, 0u}};
        std::vector<char> leaf_seen(g.leaves.size(), 0);
        while (!st.empty()) {
            const It it = st.back();
            st.pop_back();
            ++inner;
            CHECK(it.g >= 0 && (size_t)it.g < g.nodes.size() / 4, "flatten: node ref out of range");
            const uint32_t kids[2] = {it.i + 1, b.nodes[it.i].word1};
            for (int side = 0; side < 2; ++side) {
                const nh_bvh_node &c = b.nodes[kids[side]];
                Box6 box;
                int ref;
                bin_child(g.nodes, it.g, side, box, ref);
                Box6 want;
                for (int a = 0; a < 3; ++a) { want.v[a] = c.bbox_min[a]; want.v[3 + a] = c.bbox_max[a]; }
                CHECK(box == want, "flatten: child box differs from the BVH's");
                depth = std::max(depth, it.lvl + 1);
                if (c.word0 & 1u) {
                    CHECK(ref < 0 && (size_t)~ref < g.leaves.size(), "flatten: leaf ref");
                    CHECK(!leaf_seen[(size_t)~ref], "flatten: leaf referenced twice");
                    leaf_seen[(size_t)~ref] = 1;
                    ++leaves_seen;
                    CHECK(g.leaves[(size_t)~ref].x == (int)c.word1 && g.leaves[(size_t)~ref].y == (int)(c.word0 >> 1), "flatten: leaf range");
                } else {
                    CHECK(ref >= 0, "flatten: inner ref");
                    st.push_back({kids[side], ref, it.lvl + 1});
                }
            }
        }
        CHECK(inner == g.nodes.size() / 4, "flatten: inner node count");
    }
    CHECK(leaves_seen == g.leaves.size(), "flatten: leaf count");
    CHECK(g.tree_depth == depth, "flatten: tree_depth " + num(g.tree_depth) + " != walked depth " + num(depth));
}

// the binary tree's non-empty leaves in left-first DFS order, and per inner node its range of them
struct BinInfo {
    std::vector<int> leaf_start;                            // DFS order, non-empty leaves
    std::map<int, Box6> leaf_box;                           // by first primitive
    std::map<std::pair<int, int>, std::vector<Box6>> inner_box;  // [first, last) range of leaf_start -> boxes
    bool empty_leaf = false;
};
void bin_walk(const nh::GpuBvh &g, int node, BinInfo &bi) {
    for (int side = 0; side < 2; ++side) {
        Box6 box;
        int ref;
        bin_child(g.nodes, node, side, box, ref);
        if (ref < 0) {
            const nh::i2 lf = g.leaves[(size_t)~ref];
            if (lf.y > 0) {
                bi.leaf_start.push_back(lf.x);
                bi.leaf_box[lf.x] = box;
            } else {
                bi.empty_leaf = true;
            }
        } else {
            const int first = (int)bi.leaf_start.size();
            bin_walk(g, ref, bi);
            bi.inner_box[{first, (int)bi.leaf_start.size()}].push_back(box);
        }
    }
}

struct WideWalk {
    const std::vector<nh::f4> &wide;
    const BinInfo &bi;
    int W, depth = 0;
    std::vector<int> leaf_seq;
    std::vector<char> seen;
    void node(int idx, int level) {
        const int lines = W / 4, nf4 = lines * nhd::kWideF4;
        CHECK(idx >= 0 && (size_t)idx < wide.size() / nf4, "wide: child ref out of range");
        CHECK(!seen[idx], "wide: node " + num(idx) + " reached twice");
        seen[idx] = 1;
        depth = std::max(depth, level);
        bool open = true;  // slots are filled from slot 0 (while no empty leaf sits among them)
        for (int j = 0; j < W; ++j) {
            // line j / 4 in the 4-wide layout: [0..5] min xyz / max xyz of 4 slots, [6] refs, [7] zero
            const float *f = reinterpret_cast<const float *>(&wide[(size_t)idx * nf4 + (size_t)(j / 4) * nhd::kWideF4]);
            for (int q = 28; q < 32; ++q) CHECK(bits_of(f[q]) == 0, "wide: float4 7 of a line is not zero");
            Box6 box;
            for (int a = 0; a < 6; ++a) box.v[a] = f[4 * a + (j & 3)];
            const int ref = bits_of(f[24 + (j & 3)]);
            if (ref == nhd::kWideEmpty) {
                if (!bi.empty_leaf) {
                    open = false;
                    for (int a = 0; a < 6; ++a) CHECK(bits_of(box.v[a]) == 0, "wide: unused slot with a non-zero box");
                }
            } else if (ref < 0) {
                CHECK(open, "wide: used slot after an unused one");
                const auto it = bi.leaf_box.find(~ref);
                CHECK(it != bi.leaf_box.end(), "wide: leaf ref names no binary leaf");
                CHECK(box == it->second, "wide: leaf child box differs from the binary tree's");
                leaf_seq.push_back(~ref);
            } else {
                CHECK(open, "wide: used slot after an unused one");
                const int first = (int)leaf_seq.size();
                node(ref, level + 1);
                const auto it = bi.inner_box.find({first, (int)leaf_seq.size()});
                CHECK(it != bi.inner_box.end(), "wide: inner child covers no binary node's leaves");
                CHECK(std::find(it->second.begin(), it->second.end(), box) != it->second.end(),
                      "wide: inner child box differs from the binary tree's");
            }
        }
    }
};

void check_wide_tree(const std::vector<nh::f4> &wide, const BinInfo &bi, int W, int depth_reported, uint32_t tree_depth,
                     const std::string &tag) {
    const int nf4 = W / 4 * nhd::kWideF4;
    CHECK(wide.size() % nf4 == 0 && !wide.empty(), tag + ": size");
    WideWalk ww{wide, bi, W, 0, {}, {}};
    ww.seen.assign(wide.size() / nf4, 0);
    ww.node(0, 1);
    CHECK(ww.leaf_seq == bi.leaf_start, tag + ": reachable leaves are not the binary tree's non-empty leaves, each once, in order");
    for (char c : ww.seen) CHECK(c, tag + ": unreachable wide node");
    if (depth_reported >= 0) {
        CHECK(ww.depth == depth_reported, tag + ": reported depth " + num(depth_reported) + " != walked " + num(ww.depth));
        CHECK((uint32_t)depth_reported <= tree_depth, tag + ": deeper than the binary tree");
    }
}

// children of wide node g: refs of its W slots
void wide_refs(const std::vector<nh::f4> &wide, int g, int W, int *refs) {
    const int nf4 = W / 4 * nhd::kWideF4;
    for (int h = 0; h < W / 4; ++h) std::memcpy(refs + 4 * h, &wide[(size_t)g * nf4 + (size_t)h * nhd::kWideF4 + 6], 16);
}

void check_top_first(const std::vector<nh::f4> &in, const nh::GpuBvh &g, const BinInfo &bi, int W, int K) {
    const std::string tag = "number_top_first W=" + num(W) + " K=" + num(K);
    const int nf4 = W / 4 * nhd::kWideF4, n = (int)(in.size() / nf4);
    std::vector<nh::f4> out = in;
    const int n_top = nh::number_top_first(out, g.root_min, g.root_max, K, W);
    CHECK(out.size() == in.size(), tag + ": size changed");
    CHECK(n_top >= 0 && n_top <= K && n_top <= n, tag + ": n_top " + num(n_top));
    if (K == 0) {
        CHECK(std::memcmp(out.data(), in.data(), in.size() * sizeof(nh::f4)) == 0, tag + ": K = 0 changed the tree");
        return;
    }
    CHECK(n_top == std::min(K, n), tag + ": the top is smaller than asked and than the tree");
    // the permutation, by walking both trees together from the root (slot order is unchanged)
    std::vector<int> perm(n, -1), inv(n, -1), parent(n, -1);
    std::vector<std::pair<int, int>> st{{0, 0}};
    perm[0] = 0;
    inv[0] = 0;
    while (!st.empty()) {
        const auto [o, nw] = st.back();
        st.pop_back();
        int ro[8], rn[8];
        wide_refs(in, o, W, ro);
        wide_refs(out, nw, W, rn);
        for (int j = 0; j < W; ++j) {
            if (ro[j] < 0) {
                CHECK(rn[j] == ro[j], tag + ": a leaf or empty slot changed");
                continue;
            }
            CHECK(rn[j] >= 0 && rn[j] < n, tag + ": child ref out of range");
            CHECK(perm[ro[j]] < 0 && inv[rn[j]] < 0, tag + ": not a renumbering (node mapped twice)");
            perm[ro[j]] = rn[j];
            inv[rn[j]] = ro[j];
            parent[rn[j]] = nw;
            st.push_back({ro[j], rn[j]});
        }
    }
    for (int i = 0; i < n; ++i) CHECK(perm[i] >= 0, tag + ": node lost");
    // undoing the permutation and the remap of the refs restores the input bytes
    std::vector<nh::f4> back(in.size());
    for (int i = 0; i < n; ++i) {
        nh::f4 *dst = &back[(size_t)i * nf4];
        std::memcpy(dst, &out[(size_t)perm[i] * nf4], nf4 * sizeof(nh::f4));
        for (int h = 0; h < W / 4; ++h) {
            int refs[4];
            std::memcpy(refs, &dst[h * nhd::kWideF4 + 6], 16);
            for (int &r : refs)
                if (r >= 0) r = inv[r];
            std::memcpy(&dst[h * nhd::kWideF4 + 6], refs, 16);
        }
    }
    CHECK(std::memcmp(back.data(), in.data(), in.size() * sizeof(nh::f4)) == 0, tag + ": undoing the renumbering does not restore the input");
    for (int i = 1; i < n_top; ++i) CHECK(parent[i] >= 0 && parent[i] < n_top, tag + ": top node " + num(i) + " hangs below the top");
    check_wide_tree(out, bi, W, -1, g.tree_depth, tag);
}

void check_wide(const Scene &s, const nh::GpuBvh &g) {
    if (g.root_kind != 1) {
        for (int W : {4, 8}) {
            int d = -1;
            CHECK(nh::collapse_wide(g.nodes, g.leaves, d, W).empty() && d == 0, "wide: a tree without inner nodes has no wide nodes");
        }
        CHECK(g.wide.empty() && g.n_top == 0 && g.depth_wide == 1, "wide: build_gpu_bvh of a tree without inner nodes");
        return;
    }
    BinInfo bi;
    bin_walk(g, 0, bi);
    for (int W : {4, 8}) {
        int d = -1;
        const std::vector<nh::f4> wide = nh::collapse_wide(g.nodes, g.leaves, d, W);
        check_wide_tree(wide, bi, W, d, g.tree_depth, "collapse_wide W=" + num(W));
        const int n = (int)(wide.size() / (W / 4 * nhd::kWideF4));
        for (int K : {0, 1, 3, n / 2, n + 5}) check_top_first(wide, g, bi, W, K);
        // build_gpu_bvh runs the same two steps
        nh::GpuBvh gw;
        std::string err;
        const int K = std::max(1, n / 2);
        CHECK(build(s, s.b, W, K, gw, err) == NH_OK, "build_gpu_bvh W=" + num(W) + ": " + err);
        std::vector<nh::f4> want = wide;
        const int n_top = nh::number_top_first(want, g.root_min, g.root_max, K, W);
        CHECK(gw.n_top == n_top && gw.wide.size() == want.size() &&
                  std::memcmp(gw.wide.data(), want.data(), want.size() * sizeof(nh::f4)) == 0,
              "build_gpu_bvh W=" + num(W) + ": wide nodes differ from collapse_wide + number_top_first");
        CHECK(gw.depth_wide == (W - 1) * d + 1, "build_gpu_bvh W=" + num(W) + ": depth_wide");
        CHECK(K >= n || n_top < n, "build_gpu_bvh: top_k below the node count keeps the top below it");
    }
}

int count_isolated(const Scene &s, const nh::GpuBvh &g, float m_want) {
    int marked = 0;
    for (size_t k = 0; k < s.b.n_indices; ++k) {
        const nh::f4 *p = &g.prims[3 * k];
        if (!(bits_of(p[2].w) & nhd::kPrimIsolated)) continue;
        ++marked;
        const int sh = bits_of(p[1].w);
        CHECK(bits_of(p[2].w) & nhd::kPrimSphere, "isolated spheres: a triangle is marked");
        CHECK(s.real[(size_t)sh] == NH_BSDF_DIELECTRIC, "isolated spheres: a non-dielectric sphere is marked");
        CHECK(p[1].x == m_want, "isolated spheres: the record's margin is not 1e-4 of the scene extent");
    }
    CHECK(marked == g.iso_spheres, "isolated spheres: iso_spheres " + num(g.iso_spheres) + " != marked records " + num(marked));
    return marked;
}

void check_isolated(const Scene &s, const nh::GpuBvh &g, int expect) {
    // the scene extent from the scene itself: the union of every primitive's box, in double
    double lo[3] = {INFINITY, INFINITY, INFINITY}, hi[3] = {-INFINITY, -INFINITY, -INFINITY};
    for (const nh_shape &S : s.shapes)
        for (int a = 0; a < 3; ++a) {
            if (S.type == NH_SHAPE_SPHERE) {
                lo[a] = std::min(lo[a], (double)S.center[a] - (double)S.radius);
                hi[a] = std::max(hi[a], (double)S.center[a] + (double)S.radius);
            } else {
                for (uint32_t f = 0; f < 3 * S.n_faces; ++f) {
                    const double v = s.V[3 * ((size_t)S.v_offset + s.F[3 * (size_t)S.f_offset + f]) + a];
                    lo[a] = std::min(lo[a], v);
                    hi[a] = std::max(hi[a], v);
                }
            }
        }
    const double ext = std::max(hi[0] - lo[0], std::max(hi[1] - lo[1], hi[2] - lo[2]));
    const int marked = count_isolated(s, g, (float)(1e-4 * ext));
    if (expect >= 0) CHECK(marked == expect, "isolated spheres: " + num(marked) + " marked, " + num(expect) + " expected");
    setenv("NH_ISO_SPHERE", "0", 1);
    nh::GpuBvh off;
    std::string err;
    CHECK(build(s, s.b, 4, 0, off, err) == NH_OK, "build_gpu_bvh with NH_ISO_SPHERE=0: " + err);
    unsetenv("NH_ISO_SPHERE");
    CHECK(off.iso_spheres == 0 && count_isolated(s, off, 0.f) == 0, "isolated spheres: NH_ISO_SPHERE=0 marks some");
}

void check_corrupt(const Scene &s) {
    const nh_bvh_desc &b = s.b;
    nh::GpuBvh g;
    std::string err;
    const auto expect = [&](const nh_bvh_desc &bad, const char *msg) {
        err.clear();
        const int rc = build(s, bad, 4, 4, g, err);
        CHECK(rc == NH_ERR_INVALID && err == msg, std::string("corrupt input: wanted \"") + msg + "\", got rc " + num(rc) + " \"" + err + "\"");
    };
    if (b.n_indices > 0) {
        std::vector<uint32_t> idx(b.indices, b.indices + b.n_indices);
        idx[0] = b.n_indices;
        nh_bvh_desc bad = b;
        bad.indices = idx.data();
        expect(bad, "BVH index out of range");
    }
    if (b.n_nodes > 0 && !(b.nodes[0].word0 & 1u)) {
        std::vector<nh_bvh_node> nodes(b.nodes, b.nodes + b.n_nodes);
        nh_bvh_desc bad = b;
        bad.nodes = nodes.data();
        nodes[0].word1 = b.n_nodes + 3;
        expect(bad, "corrupt BVH child index");
        nodes[0].word1 = b.nodes[0].word1;
        // an inner node whose left child (the next node) is inner too: both children name it
        for (uint32_t i = 0; i + 1 < b.n_nodes; ++i)
            if (!(nodes[i].word0 & 1u) && !(nodes[i + 1].word0 & 1u)) {
                nodes[i].word1 = i + 1;
                expect(bad, "corrupt BVH: node reached twice");
                break;
            }
    }
    nh_bvh_desc fewer = b;
    fewer.n_indices = b.n_indices + 1;
    err.clear();
    CHECK(build(s, fewer, 4, 4, g, err) == NH_ERR_INVALID && err == "BVH primitive count does not match the scene", "corrupt input: primitive count");
}

// A one-inner-node BVH over a scene of two triangles, one leaf each (the SAH builder keeps two primitives in one
// leaf: a split costs it 2 + ..., a leaf 2)
struct SplitBvh {
    nh_bvh_node nodes[3];
    uint32_t indices[2] = {0u, 1u};
    SplitBvh(const Scene &s, nh_bvh_desc &b) {
        CHECK(b.n_indices == 2 && s.d.n_faces == 2, "split: the scene is not two triangles");
        std::memset(nodes, 0, sizeof(nodes));
        for (int a = 0; a < 3; ++a) { nodes[0].bbox_min[a] = INFINITY; nodes[0].bbox_max[a] = -INFINITY; }
        for (uint32_t t = 0; t < 2; ++t) {
            nh_bvh_node &n = nodes[1 + t];
            n.word0 = 1u | (1u << 1);  // a leaf of one primitive
            n.word1 = t;
            for (int a = 0; a < 3; ++a) {
                n.bbox_min[a] = INFINITY;
                n.bbox_max[a] = -INFINITY;
                for (int v = 0; v < 3; ++v) {
                    const float x = s.V[3 * ((size_t)s.shapes[0].v_offset + s.F[3 * t + v]) + a];
                    n.bbox_min[a] = std::min(n.bbox_min[a], x);
                    n.bbox_max[a] = std::max(n.bbox_max[a], x);
                }
                nodes[0].bbox_min[a] = std::min(nodes[0].bbox_min[a], n.bbox_min[a]);
                nodes[0].bbox_max[a] = std::max(nodes[0].bbox_max[a], n.bbox_max[a]);
            }
        }
        nodes[0].word1 = 2;  // inner: left child node 1, right child node 2
        b.n_nodes = 3;
        b.nodes = nodes;
        b.indices = indices;
        b.max_depth = 1;
    }
};

int run_scene(const char *path, int expect_iso, int expect_nee, bool split) {
    nh_scene *scene = nullptr;
    nh_bvh *bvh = nullptr;
    if (nh_scene_load_xml(path, &scene) != NH_OK) die(std::string("loading ") + path + ": " + nh_host_last_error());
    Scene s;
    if (nh_scene_get_desc(scene, &s.d) != NH_OK) die("nh_scene_get_desc");
    if (nh_bvh_build(&s.d, 1, &bvh) != NH_OK) die(std::string("nh_bvh_build: ") + nh_host_last_error());
    if (nh_bvh_get_desc(bvh, &s.b) != NH_OK) die("nh_bvh_get_desc");
    s.shapes.assign(s.d.shapes, s.d.shapes + s.d.n_shapes);
    s.V.assign(s.d.V, s.d.V + 3 * (size_t)s.d.n_vertices);
    s.F.assign(s.d.F, s.d.F + 3 * (size_t)s.d.n_faces);
    s.off.assign(1, 0u);
    for (const nh_shape &S : s.shapes) {
        s.real.push_back(s.d.bsdfs[S.bsdf].type);
        s.key.push_back(s.d.bsdfs[S.bsdf].type & 3);
        s.off.push_back(s.off.back() + (S.type == NH_SHAPE_MESH ? S.n_faces : 1u));
    }
    std::vector<SplitBvh> hand;
    if (split) hand.emplace_back(s, s.b);
    nh::GpuBvh g;
    std::string err;
    CHECK(build(s, s.b, 4, 0, g, err) == NH_OK, "build_gpu_bvh: " + err);
    check_flatten(s, g);
    check_wide(s, g);
    check_isolated(s, g, expect_iso);
    check_corrupt(s);
    if (expect_nee >= 0) CHECK(nh::nee_finite(&s.d) == (expect_nee != 0), "nee_finite is not " + num(expect_nee));
    std::printf("gpu_layout_check: ok: %s: root_kind %d, %u primitives, %zu inner nodes, depth %u, %d isolated\n", path,
                g.root_kind, s.b.n_indices, g.nodes.size() / 4, g.tree_depth, g.iso_spheres);
    nh_bvh_free(bvh);
    nh_scene_free(scene);
    return 0;
}

}  // namespace

int main(int argc, char **argv) {
    if (argc >= 2 && std::strcmp(argv[1], "tables") == 0) {
        const int sizes[][2] = {{32, 32}, {96, 64}, {160, 160}, {33, 65}, {70, 40}};
        for (const auto &wh : sizes) check_spiral(wh[0], wh[1]);
        check_lens(5, 3);
        check_lens(33, 2);
        std::printf("gpu_layout_check: ok: tables\n");
        return 0;
    }
    if (argc >= 3 && std::strcmp(argv[1], "scene") == 0) {
        int iso = -1, nee = -1;
        bool split = false;
        for (int i = 3; i < argc; ++i) {
            if (std::strncmp(argv[i], "iso=", 4) == 0) iso = std::atoi(argv[i] + 4);
            else if (std::strncmp(argv[i], "nee=", 4) == 0) nee = std::atoi(argv[i] + 4);
            else if (std::strcmp(argv[i], "split") == 0) split = true;
            else die(std::string("unknown argument ") + argv[i]);
        }
        return run_scene(argv[2], iso, nee, split);
    }
    std::fprintf(stderr, "usage: gpu_layout_check tables | scene FILE.xml [iso=N] [nee=0|1] [split]\n");
    return 2;
}
