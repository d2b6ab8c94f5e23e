// Candidate masks for the light sample's any-hit query ("Shadow candidate masks").
//
// A shadow ray of the bounce kernels starts on an emitter face, leaves on the face's front side and ends at a path
// vertex (csrc/nh_shade.h emitter_sample: so = p, sd = -wi, maxt = |p - ref| - eps; the light sample is dropped
// unless the float dot(n, sd) >= 0). An any-hit answer is an OR over the records' tests, so a record whose float test
// cannot accept any such ray can be left out. Two tables, both conservative, both double precision on the float
// inputs the kernels read:
//   - the emitter-side word (valid at every bounce): the records that lie wholly behind every emitter face's plane;
//   - one word per 32x32 image block (bounce 0, pinhole camera): the records whose box comes near the box of the
//     emitter faces and of what the block's camera rays can hit first, less the records the first word leaves out.
// At run time the kernels read the per-block words only (rr_step<.., SMASK>): tested per pair at the later bounces the
// emitter-side word did not pay. Its static use is the third result, the scene-wide any-hit word: the
// emitter-side word less the supporting walls (supporting_walls below), decided once at upload; the flat image gets
// pair records of their own for the records it keeps (gpu_layout.cpp flat_image), which every any-hit query of the
// flat bounce kernels loops over instead of all records.
// Both rest on one bound per record, rho: whenever the float test of record K accepts a ray that starts on an emitter
// face with maxt no longer than the scene, the exact ray passes within rho_K of K at a parameter within rho_K of
// [0, maxt]. DESIGN.md has the derivation; the constants below are its.
//
// Plain C++ (no HIP): part of both libraries; checked on the CPU by tests/test_shadow_masks_host.py.
#include <algorithm>
#include <cmath>
#include <cstdlib>
#include <cstring>

#include "gpu_layout.h"
#include "nh_host.h"

#include "../csrc/nh_layout.h"

namespace nh {

namespace {

struct V3 {
    double x, y, z;
};
V3 operator-(V3 a, V3 b) { return V3{a.x - b.x, a.y - b.y, a.z - b.z}; }
V3 operator+(V3 a, V3 b) { return V3{a.x + b.x, a.y + b.y, a.z + b.z}; }
V3 operator*(double s, V3 a) { return V3{s * a.x, s * a.y, s * a.z}; }
double dot(V3 a, V3 b) { return a.x * b.x + a.y * b.y + a.z * b.z; }
V3 cross(V3 a, V3 b) { return V3{a.y * b.z - a.z * b.y, a.z * b.x - a.x * b.z, a.x * b.y - a.y * b.x}; }
double norm(V3 a) { return std::sqrt(dot(a, a)); }

const double kU = std::ldexp(1.0, -24);  // unit roundoff of the kernels' arithmetic

struct AABB {
    V3 lo{INFINITY, INFINITY, INFINITY}, hi{-INFINITY, -INFINITY, -INFINITY};
    void add(V3 p) {
        lo = V3{std::min(lo.x, p.x), std::min(lo.y, p.y), std::min(lo.z, p.z)};
        hi = V3{std::max(hi.x, p.x), std::max(hi.y, p.y), std::max(hi.z, p.z)};
    }
    bool empty() const { return !(lo.x <= hi.x); }
    // closed boxes, this one grown by g on every side
    bool meets(const AABB &o, double g) const {
        return lo.x - g <= o.hi.x && o.lo.x <= hi.x + g && lo.y - g <= o.hi.y && o.lo.y <= hi.y + g &&
               lo.z - g <= o.hi.z && o.lo.z <= hi.z + g;
    }
};

struct Face {
    V3 p[3], n;
};

struct Record {
    bool sphere;
    V3 p[3];        // triangle: vertices; sphere: p[0] the centre
    double r;       // sphere radius
    V3 n;           // triangle: unit normal (zero when degenerate)
    double sin_t;   // triangle: sine of the angle between its edges e1, e2
    double len;     // triangle: the longer of e1, e2
    double rho;     // the bound of the header; INFINITY: the record is never left out
    double s;       // triangle with a finite rho: the emitter vertices' least distance from its plane, less eps_o
    int side;       // ... and the side of the plane they lie on (+1: the normal's)
    double reach;   // ... and the largest distance from an emitter vertex to one of its vertices
    double grown;   // sphere: half side of its grown box (rho = grown - r)
    AABB box;       // the record's own box
};

// sphere_test's float discriminant near the silhouette (primary_masks.cpp has the reasoning): the half side the
// sphere's box is grown to, for rays from at most far_d away. 1.5 times the primary masks' growth g: the accepted root
// lies within g of the ray's closest approach to the centre, which lies within g of the centre.
double sphere_grown(double r, double far_d) {
    const double g = r + 1e-3 * r + 64.0 * kU * far_d * far_d / std::max(r, 1e-300);
    return 1.5 * g;
}

struct Analysis {
    bool ok = false;  // false: no record may be left out
    std::vector<Face> faces;
    std::vector<Record> rec;
    AABB scene, emit;
    double eps_o = 0, eta = 0, d_e = 0, m = 0;
    uint64_t emitter_word = ~(uint64_t)0;
    uint64_t any_word = ~(uint64_t)0;  // the emitter-side word less the supporting walls
};

const double kEpsD = 1e-4f;  // kEps (csrc/nh_device.h): a shadow ray ends this far short of the path vertex

// The supporting-wall rule ("The any-hit list"): bit k clear when triangle record k has every
// emitter vertex at least s in front of its plane and every possible far end of a shadow ray -- a float hit point on any
// record -- on that closed side up to eps_f, with the bound closing: the ray from an emitter point p to a far end ref
// crosses K's plane no earlier than |ref - p| s / (s + eps_f), the float t is within rho_t of that, and the ray ends
// kEps before ref. A far end on a triangle record is the float barycentric point (within hit_round of the record); on
// a sphere it is o + t d with the float root t, within g_hit of the centre (the residual of the float root in
// |o + t d - c|^2 - r^2 is at most 64u far^2, far the longest ray that can reach the sphere), of whose box every
// corner is taken. An emitter's own record has s = 0 and stays; a sphere always stays.
uint64_t supporting_walls(const Analysis &A, int n_records, const V3 *origin, double origin_radius) {
    uint64_t keep = ~(uint64_t)0;
    if (!A.ok) return keep;
    AABB from = A.scene;  // where rays start that end on a record: path vertices, emitter points, the camera
    if (origin) {
        from.add(V3{origin->x - origin_radius, origin->y - origin_radius, origin->z - origin_radius});
        from.add(V3{origin->x + origin_radius, origin->y + origin_radius, origin->z + origin_radius});
    }
    if (!std::isfinite(from.lo.x + from.lo.y + from.lo.z + from.hi.x + from.hi.y + from.hi.z)) return keep;
    double max_abs = 0;
    for (const V3 &q : {from.lo, from.hi}) max_abs = std::max({max_abs, std::fabs(q.x), std::fabs(q.y), std::fabs(q.z)});
    const double hit_round = 8.0 * kU * max_abs;
    std::vector<V3> ends;  // the far ends' hull: every triangle vertex, every corner of a sphere's hit box
    for (const Record &R : A.rec) {
        if (!R.sphere) {
            ends.insert(ends.end(), R.p, R.p + 3);
            continue;
        }
        double far_d = 0;
        for (int i = 0; i < 8; ++i) {
            const V3 q{i & 1 ? from.hi.x : from.lo.x, i & 2 ? from.hi.y : from.lo.y, i & 4 ? from.hi.z : from.lo.z};
            far_d = std::max(far_d, norm(q - R.p[0]) + R.r);
        }
        if (!(R.r > 0.0)) return keep;
        const double g_hit = R.r + 64.0 * kU * far_d * far_d / R.r + hit_round;
        for (int i = 0; i < 8; ++i)
            ends.push_back(V3{R.p[0].x + (i & 1 ? g_hit : -g_hit), R.p[0].y + (i & 2 ? g_hit : -g_hit),
                              R.p[0].z + (i & 4 ? g_hit : -g_hit)});
    }
    for (int k = 0; k < n_records; ++k) {
        const Record &R = A.rec[(size_t)k];
        if (R.sphere || !std::isfinite(R.rho)) continue;  // (finite rho: one side, s > 0, s sin >= 32u R)
        double depth = 0;
        for (const V3 &q : ends) depth = std::max(depth, -R.side * dot(R.n, q - R.p[0]));
        const double eps_f = depth + hit_round;
        const double rho_t = 8.0 * kU * A.d_e * (R.reach + 2.0 * A.d_e) / (R.s * R.sin_t);
        // (a crossing behind the origin lies at t <= -s: the float t stays negative)
        if (!(R.s > 2.0 * rho_t) || !(kEpsD > 2.0 * (A.d_e * eps_f / R.s + rho_t + 4.0 * kU * A.d_e))) continue;
        keep &= ~((uint64_t)1 << k);
    }
    return keep;
}

// origin: where a path's first ray starts (the camera: the supporting-wall rule's far ends include its rays' hits) and
// how far from that point at most (a lens); null: no such ray
Analysis analyse(const f4 *prims, int n_records, const float *emit_faces, int n_faces, const V3 *origin = nullptr,
                 double origin_radius = 0.0) {
    Analysis A;
    if (n_records <= 0 || n_records > 64 || n_faces <= 0 || !emit_faces) return A;
    double min_sin = 1.0, max_abs = 0.0;
    for (int f = 0; f < n_faces; ++f) {
        Face F;
        for (int j = 0; j < 3; ++j) {
            F.p[j] = V3{emit_faces[9 * f + 3 * j], emit_faces[9 * f + 3 * j + 1], emit_faces[9 * f + 3 * j + 2]};
            A.emit.add(F.p[j]);
            max_abs = std::max({max_abs, std::fabs(F.p[j].x), std::fabs(F.p[j].y), std::fabs(F.p[j].z)});
        }
        const V3 e1 = F.p[1] - F.p[0], e2 = F.p[2] - F.p[0], c = cross(e1, e2);
        const double a2 = norm(c), l = norm(e1) * norm(e2);
        if (!(a2 > 0.0) || !std::isfinite(a2) || !(l > 0.0)) return A;
        min_sin = std::min(min_sin, a2 / l);
        F.n = (1.0 / a2) * c;
        A.faces.push_back(F);
    }
    if (!(min_sin >= 1.0 / 16)) return A;  // a sliver's float normal is not accurate enough to reason from
    A.rec.resize((size_t)n_records);
    for (int k = 0; k < n_records; ++k) {
        const f4 a = prims[3 * k], b = prims[3 * k + 1], c = prims[3 * k + 2];
        int bits;
        std::memcpy(&bits, &c.w, sizeof(bits));
        Record &R = A.rec[(size_t)k];
        R.sphere = (bits & nhd::kPrimSphere) != 0;
        R.p[0] = V3{a.x, a.y, a.z};
        R.rho = INFINITY;
        if (R.sphere) {
            R.r = std::fabs((double)a.w);
            R.box.add(V3{a.x - R.r, a.y - R.r, a.z - R.r});
            R.box.add(V3{a.x + R.r, a.y + R.r, a.z + R.r});
        } else {
            R.p[1] = V3{b.x, b.y, b.z};
            R.p[2] = V3{c.x, c.y, c.z};
            for (int j = 0; j < 3; ++j) R.box.add(R.p[j]);
        }
        A.scene.add(R.box.lo);
        A.scene.add(R.box.hi);
    }
    if (!std::isfinite(A.scene.lo.x + A.scene.lo.y + A.scene.lo.z + A.scene.hi.x + A.scene.hi.y + A.scene.hi.z)) return A;
    const V3 ext = A.scene.hi - A.scene.lo;
    A.m = 1e-4 * std::max({ext.x, ext.y, ext.z});  // the isolated spheres' margin (gpu_layout.cpp)
    // the longest shadow ray: from an emitter vertex to a corner of the scene's box (path vertices lie in that box)
    for (const Face &F : A.faces)
        for (int j = 0; j < 3; ++j)
            for (int i = 0; i < 8; ++i) {
                const V3 q{i & 1 ? A.scene.hi.x : A.scene.lo.x, i & 2 ? A.scene.hi.y : A.scene.lo.y,
                           i & 4 ? A.scene.hi.z : A.scene.lo.z};
                A.d_e = std::max(A.d_e, norm(q - F.p[j]));
            }
    A.eps_o = 8.0 * kU * max_abs;   // the sampled point's distance from its face's plane and from the face
    A.eta = 32.0 * kU / min_sin;    // exact dot(n, sd) >= -eta when the float dot(n_float, sd) >= 0
    for (Record &R : A.rec) {
        if (R.sphere) {
            double far_d = 0;
            for (const Face &F : A.faces)
                for (int j = 0; j < 3; ++j) far_d = std::max(far_d, norm(F.p[j] - R.p[0]) + R.r);
            R.grown = sphere_grown(R.r, far_d);
            R.rho = R.grown - R.r;
            continue;
        }
        const V3 e1 = R.p[1] - R.p[0], e2 = R.p[2] - R.p[0], c = cross(e1, e2);
        const double a2 = norm(c), l1 = norm(e1), l2 = norm(e2);
        R.n = V3{0, 0, 0};
        R.sin_t = 0;
        R.len = std::max(l1, l2);
        if (!(a2 > 0.0) || !(l1 * l2 > 0.0)) continue;
        R.n = (1.0 / a2) * c;
        R.sin_t = a2 / (l1 * l2);
        // every emitter vertex strictly on one side of the record's plane: s = the smallest distance
        double s = INFINITY, reach = 0;
        int side = 0;
        bool one_side = true;
        for (const Face &F : A.faces)
            for (int j = 0; j < 3; ++j) {
                const double h = dot(R.n, F.p[j] - R.p[0]);
                const int sg = h > 0 ? 1 : h < 0 ? -1 : 0;
                if (sg == 0 || (side && sg != side)) one_side = false;
                side = sg;
                s = std::min(s, std::fabs(h));
                for (int i = 0; i < 3; ++i) reach = std::max(reach, norm(F.p[j] - R.p[i]));
            }
        s -= A.eps_o;
        // (the second condition: the numerator of t keeps its sign and three quarters of its size in float)
        if (!one_side || !(s > 0.0) || !(32.0 * kU * reach <= s * R.sin_t)) continue;
        R.rho = 64.0 * kU * (reach + R.len + A.d_e) * A.d_e / (s * R.sin_t);
        R.s = s;
        R.side = side;
        R.reach = reach;
    }
    A.ok = true;
    // the emitter-side word: record k is left out when it lies behind every face's plane by more than delta_k
    uint64_t word = n_records < 64 ? ~(uint64_t)0 << n_records : 0;  // (no record: nothing to leave out)
    for (int k = 0; k < n_records; ++k) {
        const Record &R = A.rec[(size_t)k];
        bool behind = std::isfinite(R.rho);
        const double delta = A.eps_o + 1.01 * A.d_e * A.eta + (R.sphere ? 0.0 : R.rho);
        for (size_t f = 0; f < A.faces.size() && behind; ++f) {
            const Face &F = A.faces[f];
            if (R.sphere) {
                for (int i = 0; i < 8 && behind; ++i) {
                    const V3 q{R.p[0].x + (i & 1 ? R.grown : -R.grown), R.p[0].y + (i & 2 ? R.grown : -R.grown),
                               R.p[0].z + (i & 4 ? R.grown : -R.grown)};
                    behind = dot(F.n, q - F.p[0]) <= -delta;
                }
            } else {
                for (int j = 0; j < 3 && behind; ++j) behind = dot(F.n, R.p[j] - F.p[0]) <= -delta;
            }
        }
        if (!behind) word |= (uint64_t)1 << k;
    }
    A.emitter_word = word;
    // The any-hit word, for the scene as a whole: the emitters stand in an enclosure -- every triangle record that is
    // not an emitter's own is left out by one of the two rules -- or nothing is left out. (A triangle that neither rule
    // can place is the sign of a scene the rules were not made for: a mesh through or outside a wall, a light on a wall.)
    A.any_word = word & supporting_walls(A, n_records, origin, origin_radius);
    for (int k = 0; k < n_records; ++k) {
        const Record &R = A.rec[(size_t)k];
        if (R.sphere || !((A.any_word >> k) & 1)) continue;
        bool own = false;  // its three vertices are a face's (the records and the faces hold the same floats)
        for (const Face &F : A.faces) {
            int hit = 0;
            for (int i = 0; i < 3; ++i)
                for (int j = 0; j < 3; ++j)
                    hit += R.p[i].x == F.p[j].x && R.p[i].y == F.p[j].y && R.p[i].z == F.p[j].z;
            own = own || hit >= 3;
        }
        if (!own) A.any_word = ~(uint64_t)0;
    }
    return A;
}

// Sutherland-Hodgman: the part of polygon `in` with dot(n, p - org) >= 0
void clip(const std::vector<V3> &in, V3 org, V3 n, std::vector<V3> &out) {
    out.clear();
    const size_t k = in.size();
    for (size_t i = 0; i < k; ++i) {
        const V3 a = in[i], b = in[(i + 1) % k];
        const double da = dot(n, a - org), db = dot(n, b - org);
        if (da >= 0) out.push_back(a);
        if ((da >= 0) != (db >= 0)) out.push_back(a + (da / (da - db)) * (b - a));
    }
}

}  // namespace

std::vector<float> shadow_emitter_faces(const nh_scene_desc &d) {
    std::vector<float> out;
    if (d.n_emitters == 0) return out;
    for (uint32_t i = 0; i < d.n_emitters; ++i) {
        const nh_emitter &e = d.emitters[i];
        if (e.type != NH_EMITTER_AREA || e.shape < 0 || (uint32_t)e.shape >= d.n_shapes) return out;
        const nh_shape &s = d.shapes[e.shape];
        if (s.type != NH_SHAPE_MESH || s.has_normals || s.emitter < 0) return out;
    }
    for (uint32_t i = 0; i < d.n_shapes; ++i) {
        const nh_shape &s = d.shapes[i];
        if (s.emitter < 0) continue;
        if (s.type != NH_SHAPE_MESH || s.has_normals || (uint64_t)s.f_offset + s.n_faces > d.n_faces) return {};
        for (uint32_t f = 0; f < s.n_faces; ++f)
            for (int j = 0; j < 3; ++j) {
                const uint64_t v = (uint64_t)s.v_offset + d.F[3 * ((size_t)s.f_offset + f) + j];
                if (v >= d.n_vertices) return {};
                out.insert(out.end(), d.V + 3 * v, d.V + 3 * v + 3);
            }
    }
    return out;
}

uint64_t shadow_emitter_mask(const f4 *prims, int n_records, const float *emit_faces, int n_faces) {
    return analyse(prims, n_records, emit_faces, n_faces).emitter_word;
}

uint64_t shadow_any_word(const nh_camera &cam, const f4 *prims, int n_records, const float *emit_faces, int n_faces) {
    const float *cw = cam.camera_to_world;
    const V3 org{(double)cw[3] / cw[15], (double)cw[7] / cw[15], (double)cw[11] / cw[15]};
    const double lens = std::fabs((double)cam.lens_radius);
    if (!std::isfinite(org.x + org.y + org.z + lens)) return ~(uint64_t)0;
    return analyse(prims, n_records, emit_faces, n_faces, &org, lens).any_word;
}

bool any_list_knob() {
    const char *e = std::getenv("NH_ANY_LIST");
    return !(e && e[0] == '0');
}

bool shadow_block_masks(const nh_camera &cam, const f4 *prims, int n_records, const float *emit_faces, int n_faces,
                        const int32_t *blocks, int n_blocks, std::vector<uint64_t> &masks) {
    masks.clear();
    std::vector<uint64_t> pm;
    std::vector<char> in_front;
    if (!primary_masks(cam, prims, n_records, blocks, n_blocks, pm) ||
        !primary_mask_in_front(cam, prims, n_records, in_front))
        return false;
    const Analysis A = analyse(prims, n_records, emit_faces, n_faces);
    masks.assign((size_t)std::max(n_blocks, 0), 0);
    bool all_in_front = true;
    for (char c : in_front) all_in_front = all_in_front && c;
    const int nbx = (cam.width + 31) / 32, nby = (cam.height + 31) / 32;
    const double pad = primary_mask_pad(cam.width, cam.height);
    const float *cw = cam.camera_to_world;
    const V3 org{(double)cw[3] / cw[15], (double)cw[7] / cw[15], (double)cw[11] / cw[15]};
    // camera_ray's direction through raster position (x, y), unit length
    const auto direction = [&](double x, double y, V3 &d) {
        const float *m = cam.sample_to_camera;
        const double sx = x / cam.width, sy = y / cam.height;
        double r[4];
        for (int i = 0; i < 4; ++i) r[i] = m[4 * i] * sx + m[4 * i + 1] * sy + m[4 * i + 3];
        const V3 l{r[0] / r[3], r[1] / r[3], r[2] / r[3]};
        d = V3{cw[0] * l.x + cw[1] * l.y + cw[2] * l.z, cw[4] * l.x + cw[5] * l.y + cw[6] * l.z,
               cw[8] * l.x + cw[9] * l.y + cw[10] * l.z};
        const double len = norm(d);
        if (!(len > 0.0) || !std::isfinite(len)) return false;
        d = (1.0 / len) * d;
        return true;
    };
    std::vector<V3> poly, tmp;
    for (int i = 0; i < n_blocks; ++i) {
        const uint64_t p = pm[(size_t)i];
        if (!p) continue;  // no camera ray of the block hits anything: no light sample
        masks[(size_t)i] = A.emitter_word;
        const int bid = blocks[i];
        if (!A.ok || !all_in_front || bid < 0 || bid >= nbx * nby) continue;
        const int bx = bid % nbx, by = bid / nbx;
        const double x0 = 32.0 * bx - pad, x1 = std::min(32.0 * bx + 32.0, (double)cam.width) + pad;
        const double y0 = 32.0 * by - pad, y1 = std::min(32.0 * by + 32.0, (double)cam.height) + pad;
        V3 d[4], mid;
        if (!direction(x0, y0, d[0]) || !direction(x1, y0, d[1]) || !direction(x1, y1, d[2]) ||
            !direction(x0, y1, d[3]) || !direction(0.5 * (x0 + x1), 0.5 * (y0 + y1), mid))
            continue;
        V3 pn[4];
        bool planes_ok = true;
        double cone_cos = 1.0;
        for (int e = 0; e < 4; ++e) {
            pn[e] = cross(d[e], d[(e + 1) & 3]);
            const double s = dot(pn[e], mid);
            if (s < 0) pn[e] = -1.0 * pn[e];
            planes_ok = planes_ok && s != 0.0;
            for (int j = 0; j < 4; ++j) cone_cos = std::min(cone_cos, dot(d[e], d[j]));
        }
        if (!planes_ok || !(cone_cos > 0.5)) continue;
        // R_b: where the block's camera rays can be accepted first; w: how far from it the float hit point can lie
        AABB region;
        double w = 0;
        bool grazing = false;
        for (int k = 0; k < n_records && !grazing; ++k) {
            if (!((p >> k) & 1)) continue;
            const Record &R = A.rec[(size_t)k];
            if (R.sphere) {
                double dist = norm(R.p[0] - org);
                const double G = sphere_grown(R.r, dist + R.r), reach = std::sqrt(3.0) * G;
                const double t0 = std::max(dist - reach, 0.0), t1 = (dist + reach) / cone_cos;
                AABB fr, sb;
                for (int e = 0; e < 4; ++e) {
                    fr.add(org + t0 * d[e]);
                    fr.add(org + t1 * d[e]);
                }
                sb.add(V3{R.p[0].x - G, R.p[0].y - G, R.p[0].z - G});
                sb.add(V3{R.p[0].x + G, R.p[0].y + G, R.p[0].z + G});
                if (!fr.meets(sb, 0.0)) continue;
                region.add(V3{std::max(fr.lo.x, sb.lo.x), std::max(fr.lo.y, sb.lo.y), std::max(fr.lo.z, sb.lo.z)});
                region.add(V3{std::min(fr.hi.x, sb.hi.x), std::min(fr.hi.y, sb.hi.y), std::min(fr.hi.z, sb.hi.z)});
                continue;
            }
            // the block's rays against the record's plane: all from one side, no flatter than c_min
            double c_min = INFINITY, reach = 0;
            int side = 0;
            for (int e = 0; e < 4; ++e) {
                const double c = dot(R.n, d[e]);
                const int sg = c > 0 ? 1 : c < 0 ? -1 : 0;
                if (sg == 0 || (side && sg != side)) grazing = true;
                side = sg;
                c_min = std::min(c_min, std::fabs(c));
            }
            for (int j = 0; j < 3; ++j) reach = std::max(reach, norm(R.p[j] - org));
            if (grazing || !(R.sin_t > 0.0)) {
                grazing = true;
                break;
            }
            w = std::max(w, 64.0 * kU * (reach + R.len) / (R.sin_t * c_min));
            poly.assign(R.p, R.p + 3);
            for (int e = 0; e < 4 && !poly.empty(); ++e) {
                clip(poly, org, pn[e], tmp);
                poly.swap(tmp);
            }
            for (const V3 &q : poly) region.add(q);
        }
        if (grazing || !std::isfinite(w)) continue;
        AABB target = A.emit;
        if (!region.empty()) {
            target.add(region.lo);
            target.add(region.hi);
        }
        uint64_t keep = 0;
        for (int k = 0; k < n_records; ++k) {
            const Record &R = A.rec[(size_t)k];
            if (!std::isfinite(R.rho) || R.box.meets(target, A.m + A.eps_o + w + R.rho)) keep |= (uint64_t)1 << k;
        }
        if (n_records < 64) keep |= ~(uint64_t)0 << n_records;
        masks[(size_t)i] = keep & A.emitter_word;
    }
    return true;
}

}  // namespace nh

extern "C" {

int nh_shadow_emitter_faces(const nh_scene_desc *scene, float *faces, int32_t cap_faces, int32_t *n_faces) {
    if (!scene || !n_faces || cap_faces < 0 || (cap_faces > 0 && !faces)) {
        nh::set_host_error("nh_shadow_emitter_faces: invalid argument");
        return NH_ERR_INVALID;
    }
    const std::vector<float> f = nh::shadow_emitter_faces(*scene);
    *n_faces = (int32_t)(f.size() / 9);
    if (*n_faces > cap_faces) {
        nh::set_host_error("nh_shadow_emitter_faces: more faces than the caller has room for");
        return NH_ERR_INVALID;
    }
    if (!f.empty()) std::memcpy(faces, f.data(), f.size() * sizeof(float));
    return NH_OK;
}

int nh_shadow_masks(const nh_camera *camera, const float *records, int32_t n_records, const float *emit_faces,
                    int32_t n_emit_faces, const int32_t *blocks, int32_t n_blocks, uint64_t *emitter_mask,
                    uint64_t *masks, int32_t *built) {
    if (!camera || !built || !emitter_mask || n_records < 0 || n_blocks < 0 || (n_records > 0 && !records) ||
        (n_emit_faces > 0 && !emit_faces) || (n_blocks > 0 && (!blocks || !masks))) {
        nh::set_host_error("nh_shadow_masks: invalid argument");
        return NH_ERR_INVALID;
    }
    const nh::f4 *prims = reinterpret_cast<const nh::f4 *>(records);
    *emitter_mask = nh::shadow_emitter_mask(prims, n_records, emit_faces, n_emit_faces);
    std::vector<uint64_t> m;
    *built = nh::shadow_block_masks(*camera, prims, n_records, emit_faces, n_emit_faces, blocks, n_blocks, m) ? 1 : 0;
    if (*built && n_blocks > 0) std::memcpy(masks, m.data(), (size_t)n_blocks * sizeof(uint64_t));
    return NH_OK;
}

int nh_shadow_any_word(const nh_camera *camera, const float *records, int32_t n_records, const float *emit_faces,
                       int32_t n_emit_faces, uint64_t *word) {
    if (!camera || !word || n_records < 0 || (n_records > 0 && !records) || (n_emit_faces > 0 && !emit_faces)) {
        nh::set_host_error("nh_shadow_any_word: invalid argument");
        return NH_ERR_INVALID;
    }
    *word = nh::shadow_any_word(*camera, reinterpret_cast<const nh::f4 *>(records), n_records, emit_faces, n_emit_faces);
    return NH_OK;
}

}  // extern "C"
