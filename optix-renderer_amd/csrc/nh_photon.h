// The photon mapper on the device (src/integrators/photonmapper.cpp, src/utils/photon.cpp, include/nori/photon.h;
// DESIGN.md section 7e), as device functions shared by the photon pass and the camera pass (nh_photon.hip) and by the
// query kernels (nh_query.hip, nh_emitter_query.hip):
//
//   pm_encode / pm_decode_*    PhotonData's constructor and getDirection / getPower
//   emitter_sample_photon      AreaEmitter::samplePhoton with Mesh / Sphere::sampleSurface
//   pm_cell / pm_key           the uniform search grid that stands in for PointKDTree
//   pm_gather                  PointKDTree::search's result set, visited in ascending (cell key, deposit index) order
//   li_photonmapper            PhotonMapper::Li
//
// Built with -DNH_DISNEY only (Makefile): isDiffuse() is true for the diffuse and the Disney BSDF.
#pragma once
#include "nh_internal.h"
#include "nh_shade.h"
#include "nh_traverse.h"

#ifndef NH_DISNEY
#error "nh_photon.h is built with -DNH_DISNEY"
#endif

using namespace nhd;

namespace nh_disney {

// PhotonData's decode tables (photon.cpp:24-41), 256 floats each, in this order in one device array
enum { PM_COS_THETA = 0, PM_SIN_THETA = 256, PM_COS_PHI = 512, PM_SIN_PHI = 768, PM_EXP = 1024, PM_TABLE_FLOATS = 1280 };

// BSDF::isDiffuse(): overridden to true by diffuse.cpp and disney.cpp only (the microfacet BSDF keeps the default)
NHD bool pm_is_diffuse(const DBsdf &b) { return b.type == BSDF_DIFFUSE || b.type == BSDF_DISNEY; }

// PhotonData::PhotonData (photon.cpp:43-74). tp = theta | phi << 8; rgbe = rgbe[0] | rgbe[1] << 8 | rgbe[2] << 16 |
// rgbe[3] << 24. std::acos / std::atan2 on float are the float libm (fp64 evaluated, rounded once, as every f_*
// function); M_PI is Nori's float constant, so 256.0f / M_PI and 256.0f / (2.0f * M_PI) are float quotients; the float
// -> int and float -> uint8_t conversions are x86's cvttss2si (to 32 bits, then the low byte).
NHD void pm_encode(F3 dir, F3 power, uint32_t &tp, uint32_t &rgbe) {
    const int th = x86_f2i(f_acos(dir.z) * (256.0f / kPi));
    const uint32_t theta = (uint32_t)(th < 255 ? th : 255) & 0xffu;  // std::min(255, .), then (uint8_t)
    const int ph = x86_f2i(f_atan2(dir.y, dir.x) * (256.0f / (2.0f * kPi)));
    const int tmp = ph < 255 ? ph : 255;
    const uint32_t phi = (uint32_t)(tmp < 0 ? tmp + 256 : tmp) & 0xffu;
    tp = theta | (phi << 8);
    float mx = max_coeff(power);
    if ((double)mx < 1e-32) {  // the literal is a double
        rgbe = 0u;
        return;
    }
    int e;
    mx = frexpf(mx, &e) * 256.0f / mx;
    const uint32_t r = (uint32_t)x86_f2i(power.x * mx) & 0xffu, g = (uint32_t)x86_f2i(power.y * mx) & 0xffu,
                   b = (uint32_t)x86_f2i(power.z * mx) & 0xffu;
    rgbe = r | (g << 8) | (b << 16) | (((uint32_t)(e + 128) & 0xffu) << 24);
}
// PhotonData::getDirection / getPower (photon.h:44-55)
NHD F3 pm_decode_dir(const float *tab, uint32_t tp) {
    const uint32_t theta = tp & 0xffu, phi = (tp >> 8) & 0xffu;
    return f3(tab[PM_COS_PHI + phi] * tab[PM_SIN_THETA + theta], tab[PM_SIN_PHI + phi] * tab[PM_SIN_THETA + theta],
              tab[PM_COS_THETA + theta]);
}
NHD F3 pm_decode_power(const float *tab, uint32_t rgbe) {
    const float ex = tab[PM_EXP + (rgbe >> 24)];
    return f3((float)(rgbe & 0xffu) * ex, (float)((rgbe >> 8) & 0xffu) * ex, (float)((rgbe >> 16) & 0xffu) * ex);
}

// AreaEmitter::samplePhoton (arealight.cpp:127-144) of area light e: Mesh::sampleSurface (mesh.cpp:50-71, the
// operations of emitter_sample's area branch, nh_shade.h) or Sphere::sampleSurface (sphere.cpp:126-132), then
// Frame(n).toWorld(squareToCosineHemisphere(sample2)). Returns M_PI / pdf * radiance; the ray is Ray3f(p, dir): mint
// Epsilon, maxt infinity.
NHD F3 emitter_sample_photon(const DScene &S, const DEmitter &e, float s1x, float s1y, float s2x, float s2y, F3 &o,
                             F3 &d, float &pdf) {
    const DShape sh = S.shapes[e.shape];
    F3 p, n;
    if (sh.type == SHAPE_MESH) {
        const float *cdf = S.area_cdf + sh.pdf_off;
        const int idt = dpdf_sample(cdf, sh.n_faces, s1x);
        s1x = (s1x - cdf[idt]) / (cdf[idt + 1] - cdf[idt]);  // sampleReuse
        const float su1 = f_sqrt(s1x);                        // squareToUniformTriangle (warp.cpp:162-166)
        const float bu = 1.f - su1, bv = s1y * su1, bw = 1.f - bu - bv;
        if (sh.ef_off >= 0) {
            const float4 *q = S.emit_faces + 3 * (size_t)(sh.ef_off + idt);
            const float4 q0 = q[0], q1 = q[1], q2 = q[2];
            p = add(add(scl(bu, f3(q0.x, q0.y, q0.z)), scl(bv, f3(q1.x, q1.y, q1.z))), scl(bw, f3(q2.x, q2.y, q2.z)));
            n = f3(q0.w, q1.w, q2.w);
        } else {
            const uint32_t *f = S.F + 3 * (size_t)(sh.f_off + idt);
            const uint32_t i0 = sh.v_off + f[0], i1 = sh.v_off + f[1], i2 = sh.v_off + f[2];
            const F3 p0 = ldv(S.V, i0), p1 = ldv(S.V, i1), p2 = ldv(S.V, i2);
            p = add(add(scl(bu, p0), scl(bv, p1)), scl(bw, p2));
            if (sh.has_n)
                n = normalized(add(add(scl(bu, ldv(S.N, i0)), scl(bv, ldv(S.N, i1))), scl(bw, ldv(S.N, i2))));
            else
                n = normalized(cross(sub(p1, p0), sub(p2, p0)));
        }
        pdf = sh.pdf_norm;
    } else {
        const F3 q = uniform_sphere(s1x, s1y);
        p = add(f3(sh.cx, sh.cy, sh.cz), scl(sh.radius, q));
        n = q;
        // std::pow(1.f / r, 2) (double, exact square) * squareToUniformSpherePdf = 0.25f / M_PI, rounded on assignment
        pdf = (float)((double)(1.f / sh.radius) * (double)(1.f / sh.radius) * (double)(0.25f / kPi));
    }
    o = p;
    d = to_world(frame_from_n(n), cosine_hemisphere(s2x, s2y));
    const float a = kPi / pdf;
    return f3(a * e.lr, a * e.lg, a * e.lb);
}

// ---- the search grid ---------------------------------------------------------------------------------------------
// Cell coordinates are 21 bits per axis; pm_cell is monotone non-decreasing in x (a difference, a quotient by a
// positive cell, two clamps and a truncation of a non-negative float), which is all pm_gather relies on.
constexpr float kPmMaxCell = 2097151.0f;  // 2^21 - 1
NHD int pm_cell(float x, float origin, float cell) {
    float t = (x - origin) / cell;
    t = t >= 0.f ? t : 0.f;  // NaN -> 0
    t = t < kPmMaxCell ? t : kPmMaxCell;
    return (int)t;
}
NHD uint64_t pm_key(int cx, int cy, int cz) { return (uint64_t)cx | ((uint64_t)cy << 21) | ((uint64_t)cz << 42); }
NHD uint64_t pm_key_of(const DPhotonMap &pm, F3 p) {
    return pm_key(pm_cell(p.x, pm.origin[0], pm.cell), pm_cell(p.y, pm.origin[1], pm.cell),
                  pm_cell(p.z, pm.origin[2], pm.cell));
}
// the first index whose key is not below k
NHD int pm_lower_bound(const uint64_t *keys, int n, uint64_t k) {
    int lo = 0, hi = n;
    while (lo < hi) {
        const int mid = (lo + hi) >> 1;
        if (keys[mid] < k) lo = mid + 1;
        else hi = mid;
    }
    return lo;
}

// PointKDTree::search(q, r): f(i) for every photon i with (photon.p - q).squaredNorm() < r * r -- strict, fp32, the
// squared norm grouped as Eigen sums a Vector3f (dot) -- in ascending sorted index, i.e. ascending (cell key, deposit
// index): a function of the map and q alone. An accepted photon has |p.x - q.x| <= r (1 + 2^-21), so it lies in
// [fl(q.x - rr), fl(q.x + rr)] for rr = 1.001 r (rounding to nearest never crosses the float p.x), and pm_cell being
// monotone its cell lies between the cells of those two ends; the same per axis. The keys of one (cy, cz) row are
// contiguous in the sorted order, so a row is one binary search and a linear walk.
template <class F>
NHD void pm_gather(const DPhotonMap &pm, F3 q, F &&f) {
    const float rr = pm.radius * 1.001f, r2 = pm.radius * pm.radius;
    const int x0 = pm_cell(q.x - rr, pm.origin[0], pm.cell), x1 = pm_cell(q.x + rr, pm.origin[0], pm.cell);
    const int y0 = pm_cell(q.y - rr, pm.origin[1], pm.cell), y1 = pm_cell(q.y + rr, pm.origin[1], pm.cell);
    const int z0 = pm_cell(q.z - rr, pm.origin[2], pm.cell), z1 = pm_cell(q.z + rr, pm.origin[2], pm.cell);
    for (int cz = z0; cz <= z1; ++cz)
        for (int cy = y0; cy <= y1; ++cy) {
            const uint64_t khi = pm_key(x1, cy, cz);
            for (int i = pm_lower_bound(pm.keys, pm.n, pm_key(x0, cy, cz)); i < pm.n && pm.keys[i] <= khi; ++i) {
                const float4 p = pm.pos[i];
                const F3 dv = sub(f3(p.x, p.y, p.z), q);
                if (dot(dv, dv) < r2) f(i);
            }
        }
}

// PhotonMapper::Li (photonmapper.cpp:156-270). Closest hits go nearer child first (every order returns the same hit).
template <int DEPTH, bool STATS>
__device__ F3 li_photonmapper(const DScene &S, const Traversal &tv, Rng &rng, F3 o, F3 d, float mint, float maxt,
                              uint32_t *stk, int stride, TravStats &st, uint32_t &queries) {
    F3 li = f3(0, 0, 0), t = f3(1, 1, 1);
    int counter = 0;
    for (;;) {
        Hit h;
        bool found = false;
        if (!(d.x == 0 && d.y == 0 && d.z == 0)) {  // a zero direction misses every primitive
            if (STATS) queries++;
            found = trace<DEPTH, true, false, STATS>(tv, S, o, d, mint, maxt, h, stk, stride, st);
        }
        if (!found) {  // :180-190 (the loader refuses environment maps; the shape of the code is kept)
            if (S.envmap >= 0) li = add(li, mulc(t, env_eval(S, d)));
            break;
        }
        Its its;
        hit_info(S, tv, h, o, d, its);
        const DShape shape = S.shapes[its.shape];
        const DBsdf bsdf = S.bsdfs[shape.bsdf];
        const F3 alb = bsdf_albedo(S, bsdf, its.u, its.v);
        if (shape.emitter >= 0)  // :197-202, unweighted
            li = add(li, mulc(t, emitter_eval(S.emitters[shape.emitter], o, its.sh.n, normalized(sub(its.p, o)))));
        const F3 wi_l = to_local(its.sh, neg(d));
        if (pm_is_diffuse(bsdf)) {  // :204-236
            F3 pc = f3(0, 0, 0);
            int count = 0;
            const float den = kPi * S.pm.radius * S.pm.radius;  // M_PI * m_photonRadius * m_photonRadius
            pm_gather(S.pm, its.p, [&](int i) {
                const float4 pd = S.pm.dir[i], pw = S.pm.power[i];
                const F3 ev = bsdf_eval(bsdf, wi_l, to_local(its.sh, f3(pd.x, pd.y, pd.z)), M_SOLID_ANGLE, alb);
                pc = add(pc, divs(mulc(f3(pw.x, pw.y, pw.z), ev), den));
                ++count;
            });
            if (count > 0) li = add(li, divs(mulc(t, pc), (float)S.pm.emitted));
            break;
        }
        const float succ = e_min(max_coeff(t), 0.99f);  // :238-250
        if (counter < 3) counter++;
        else if (rng.next1d() > succ) break;
        else t = divs(t, succ);
        const float bx = rng.next1d(), by = rng.next1d();
        F3 wo;
        int measure;
        const F3 col = bsdf_sample(bsdf, wi_l, bx, by, wo, measure, alb);
        if (is_zero(col)) break;
        t = mulc(t, col);
        o = its.p;
        d = to_world(its.sh, wo);
        mint = kEps;
        maxt = INFINITY;
    }
    return li;
}

// One photon path of PhotonMapper::preprocess (photonmapper.cpp:88-148) on its own stream. deposit(bounce, p, dir, W) is
// called at every diffuse hit, with no cap; returns the number of deposits. Draw order: the emitter choice, sample1 (x,
// y), sample2 (x, y), then per bounce the roulette draw (from the fourth bounce on) and the BSDF's two.
template <int DEPTH, class D>
__device__ int photon_path(const DScene &S, const Traversal &tv, uint64_t seed, uint64_t k, uint32_t *stk, int stride,
                           D &&deposit) {
    Rng rng = path_rng(seed, NH_PHOTON_STREAM, k);
    const DEmitter em = S.emitters[emitter_pick(S, rng.next1d())];
    const float s1x = rng.next1d(), s1y = rng.next1d(), s2x = rng.next1d(), s2y = rng.next1d();
    F3 o, d;
    float pdf;
    F3 W = scl((float)S.n_emitters, emitter_sample_photon(S, em, s1x, s1y, s2x, s2y, o, d, pdf));
    TravStats st{0, 0, 0};
    int counter = 0, n = 0;
    for (int bounce = 0;; ++bounce) {
        Hit h;
        if (d.x == 0 && d.y == 0 && d.z == 0) break;
        if (!trace<DEPTH, true, false, false>(tv, S, o, d, kEps, INFINITY, h, stk, stride, st)) break;
        Its its;
        hit_info(S, tv, h, o, d, its);
        const DBsdf bsdf = S.bsdfs[S.shapes[its.shape].bsdf];
        if (pm_is_diffuse(bsdf)) {
            deposit(bounce, its.p, neg(d), W);
            ++n;
        }
        const float succ = e_min(max_coeff(W), 0.99f);
        if (counter < 3) counter++;
        else if (rng.next1d() > succ) break;
        else W = divs(W, succ);
        // BSDFQueryRecord bqr(its.toLocal(-sampleRay.d)): no uv (the loader refuses textured albedos)
        const float bx = rng.next1d(), by = rng.next1d();
        F3 wo;
        int measure;
        const F3 col = bsdf_sample(bsdf, to_local(its.sh, neg(d)), bx, by, wo, measure, f3(bsdf.ar, bsdf.ag, bsdf.ab));
        if (is_zero(col)) break;
        o = its.p;
        d = to_world(its.sh, wo);
        W = mulc(W, col);
    }
    return n;
}

}  // namespace nh_disney
