// The integrators' Li as device function templates, one per reference integrator, for the kernels that run a camera
// path per thread: nh_path_kernel (nh_kernels.hip) and ad_path_kernel (nh_adaptive.hip). (The volumetric ones are in
// nh_volume.h; the wavefront pipeline restates path_mis stage by stage, nh_wavefront.hip.)
//
//   li_path_mis / li_path_mats        PathMISIntegrator::Li / PathMatsIntegrator::Li
//   li_direct_{ems,mats,mis,simple}   the single-bounce direct integrators
//   li_normals                        NormalIntegrator::Li
//   li_av / li_envmaptester           AverageVisibilityIntegrator::Li / EnvMapTester::Li
//
// With -DNH_DISNEY the functions are nh_disney's, as the kernels that call them are (nh_internal.h).
#pragma once
#include "nh_internal.h"
#include "nh_traverse.h"
#include "nh_shade.h"

using namespace nhd;

#ifdef NH_DISNEY
namespace nh_disney {
#endif

namespace {

// PathMISIntegrator::Li (src/integrators/path_mis.cpp:16-150). Lanes of a wave stay in
// lockstep: shade, then one shadow traversal (any hit, :89) for the lanes that sample a
// light, then one closest-hit traversal of the BSDF-sampled ray for every lane -- that ray
// is both the MIS probe (:117-119) and the next bounce (:146 -> :34) and is traced once.
// Everything that does not depend on a traversal result is evaluated before it (pure
// functions, same operands, same random-number draw order: traversals draw nothing), which
// keeps the state that is live across traversals small.
template <int DEPTH, bool ORDERED, bool STATS, bool NMAP = true>
__device__ F3 li_path_mis(const DScene &S, const Traversal &tv, Rng &rng, F3 o, F3 d, float mint, float maxt,
                          uint32_t *stk, int stride, TravStats &st, uint32_t &queries) {
    F3 li = f3(0, 0, 0), t = f3(1, 1, 1);
    float w_mats = 1.f, w_ems = 0.f;
    const float n_lights = (float)S.n_emitters;
    Hit h;
    if (STATS) queries++;
    bool found = trace<DEPTH, ORDERED, false, STATS>(tv, S, o, d, mint, maxt, h, stk, stride, st);
    for (;;) {
        if (!found) {  // path_mis.cpp:32-44: escaped rays see the environment map, no MIS weight
            if (S.envmap >= 0) li = add(li, mulc(t, env_eval(S, d)));
            break;
        }
        Its its;
        hit_info<NMAP>(S, tv, h, o, d, its);
        const DShape shape = S.shapes[its.shape];
        const DBsdf bsdf = S.bsdfs[shape.bsdf];
        const F3 alb = bsdf_albedo(S, bsdf, its.u, its.v);
        if (shape.emitter >= 0) {  // path_mis.cpp:51-56
            const DEmitter em = S.emitters[shape.emitter];
            const F3 wi = normalized(sub(its.p, o));
            li = add(li, mulc(scl(w_mats, t), emitter_eval(em, o, its.sh.n, wi)));
        }
        float succ = e_min(max_coeff(t), 0.99f);  // RR from depth 0 (path_mis.cpp:58-71)
        succ = e_max(succ, kEps);
        if (rng.next1d() > succ) break;
        t = divs(t, succ);

        // emitter sampling (path_mis.cpp:75-102)
        const int ei = emitter_pick(S, rng.next1d());
        const DEmitter em = S.emitters[ei];
        const float ex = rng.next1d(), ey = rng.next1d();
        ESample es;
        const F3 ems_col = emitter_sample(S, em, its.p, ex, ey, es);
        const F3 wi_l = to_local(its.sh, neg(d));
        const bool nee = !is_zero(ems_col);
        F3 li_ems = f3(0, 0, 0);
        float pdfems = 0.f, pdfems_mats = 0.f;
        if (nee) {
            const F3 we = to_local(its.sh, es.wi);
            const F3 f = bsdf_eval(bsdf, wi_l, we, M_SOLID_ANGLE, alb);
            const float cs = we.z;
            li_ems = f3(ems_col.x * cs * f.x * n_lights, ems_col.y * cs * f.y * n_lights,
                        ems_col.z * cs * f.z * n_lights);
            pdfems_mats = bsdf_pdf(bsdf, wi_l, we, M_SOLID_ANGLE);
            pdfems = emitter_pdf(S, em, its.p, es.p, es.n, es.wi) / n_lights;
        }
        // BSDF sampling (path_mis.cpp:109-113)
        const float bx = rng.next1d(), by = rng.next1d();
        F3 wo;
        int measure;
        const F3 bsdf_col = bsdf_sample(bsdf, wi_l, bx, by, wo, measure, alb);
        const float pdfmat = bsdf_pdf(bsdf, wi_l, wo, measure);  // used only if the probe hits an emitter
        const F3 nd = to_world(its.sh, wo);
        const F3 no = its.p;

        // A discrete BSDF sample zeroes w_ems (path_mis.cpp:136-140): the light term (0 * t) * li_ems then
        // adds exactly zero whether or not the shadow ray is occluded, as long as it is finite (Li never
        // holds -0, so +-0 leaves it unchanged) -- that query is not traced (same draws, same result;
        // the wavefront shade makes the same decision)
        bool trace_shadow = nee;
        if (nee && measure == M_DISCRETE) {
            const F3 c = mulc(scl(0.f, t), li_ems), z = mulc(scl(0.f, t), f3(0, 0, 0));
            if (c.x == 0.f && c.y == 0.f && c.z == 0.f && z.x == 0.f && z.y == 0.f && z.z == 0.f) trace_shadow = false;
        }
        if (trace_shadow) {  // shadow ray (path_mis.cpp:89): occluded -> no contribution, pdfs stay 0
            Hit hs;
            if (STATS) queries++;
            if (trace<DEPTH, ORDERED, true, STATS>(tv, S, es.so, es.sd, es.smint, es.smaxt, hs, stk, stride, st)) {
                li_ems = f3(0, 0, 0);
                pdfems = 0.f;
                pdfems_mats = 0.f;
            }
        }
        if ((pdfems_mats + pdfems) > kEps) w_ems = pdfems / (pdfems_mats + pdfems);

        // probe ray == next bounce (path_mis.cpp:115-146); a zero direction misses every
        // primitive (det == 0 / NaN roots), so its traversal is skipped
        if (nd.x == 0 && nd.y == 0 && nd.z == 0) {
            found = false;
        } else {
            if (STATS) queries++;
            found = trace_next<DEPTH, ORDERED, STATS>(tv, S, h.k, no, nd, kEps, INFINITY, h, stk, stride, st);
        }
        if (!is_zero(bsdf_col) && found) {
            const int hs_shape = __float_as_int(tv.prims[3 * h.k + 1].w);
            const int hem = S.shapes[hs_shape].emitter;
            if (hem >= 0) {
                Its its_s;
                hit_info<NMAP>(S, tv, h, no, nd, its_s);
                const DEmitter em2 = S.emitters[hem];
                const F3 wim = normalized(sub(its_s.p, no));
                const float pdfmat_ems = emitter_pdf(S, em2, no, its_s.p, its_s.sh.n, wim) / n_lights;
                if ((pdfmat + pdfmat_ems) > kEps) w_mats = pdfmat / (pdfmat + pdfmat_ems);
            }
        }
        if (measure == M_DISCRETE) {
            w_ems = 0.f;
            w_mats = 1.f;
        }
        li = add(li, mulc(scl(w_ems, t), li_ems));
        t = mulc(t, bsdf_col);
        o = no;
        d = nd;
    }
    return li;
}

// PathMatsIntegrator::Li (src/integrators/path_mats.cpp:16-78)
template <int DEPTH, bool ORDERED, bool STATS>
__device__ F3 li_path_mats(const DScene &S, const Traversal &tv, Rng &rng, F3 o, F3 d, float mint, float maxt,
                           uint32_t *stk, int stride, TravStats &st, uint32_t &queries) {
    F3 li = f3(0, 0, 0), t = f3(1, 1, 1);
    int counter = 0;
    Hit h;
    h.k = -1;  // the camera ray leaves no surface
    for (;;) {
        bool found;
        if (d.x == 0 && d.y == 0 && d.z == 0) {
            found = false;
        } else {
            if (STATS) queries++;
            found = trace_next<DEPTH, ORDERED, STATS>(tv, S, h.k, o, d, mint, maxt, h, stk, stride, st);
        }
        if (!found) {  // path_mats.cpp:26-35
            if (S.envmap >= 0) li = add(li, mulc(t, env_eval(S, d)));
            break;
        }
        Its its;
        hit_info(S, tv, h, o, d, its);
        const DShape shape = S.shapes[its.shape];
        const DBsdf bsdf = S.bsdfs[shape.bsdf];
        const F3 alb = bsdf_albedo(S, bsdf, its.u, its.v);
        if (shape.emitter >= 0) {
            F3 wi = normalized(sub(its.p, o));
            li = add(li, mulc(t, emitter_eval(S.emitters[shape.emitter], o, its.sh.n, wi)));
        }
        float succ = e_min(max_coeff(t), 0.99f);
        if (counter < 3) counter++;
        else if (rng.next1d() > succ) break;
        else t = divs(t, succ);
        const float bx = rng.next1d(), by = rng.next1d();
        F3 wo;
        int measure;
        F3 col = bsdf_sample(bsdf, to_local(its.sh, neg(d)), bx, by, wo, measure, alb);
        t = mulc(t, col);
        d = to_world(its.sh, wo);
        o = its.p;
        mint = kEps;
        maxt = INFINITY;
    }
    return li;
}

}  // namespace

// ---- single-bounce direct integrators (one closest hit from the camera) --------------------
// Miss: the environment map, if any (direct_*.cpp:17-26). Hit on an emitter: its radiance toward
// the camera, unweighted (:33-39).
#define NH_DIRECT_PROLOGUE                                                                       \
    Hit h;                                                                                       \
    if (STATS) queries++;                                                                        \
    if (!trace<DEPTH, ORDERED, false, STATS>(tv, S, o, d, mint, maxt, h, stk, stride, st))      \
        return S.envmap >= 0 ? env_eval(S, d) : f3(0, 0, 0);                                     \
    Its its;                                                                                     \
    hit_info(S, tv, h, o, d, its);                                                               \
    const DShape shape = S.shapes[its.shape];                                                    \
    const DBsdf bsdf = S.bsdfs[shape.bsdf];                                                      \
    const F3 alb = bsdf_albedo(S, bsdf, its.u, its.v);                                           \
    F3 result = f3(0, 0, 0);                                                                     \
    if (shape.emitter >= 0)                                                                      \
        result = add(result, emitter_eval(S.emitters[shape.emitter], o, its.sh.n, normalized(sub(its.p, o))));

// DirectEMSIntegrator::Li (src/integrators/direct_ems.cpp:14-70): one light sample per emitter, in
// scene order, each with its own 2D sample; unoccluded ones add li * |cos| * f.
template <int DEPTH, bool ORDERED, bool STATS>
__device__ F3 li_direct_ems(const DScene &S, const Traversal &tv, Rng &rng, F3 o, F3 d, float mint, float maxt,
                            uint32_t *stk, int stride, TravStats &st, uint32_t &queries) {
    NH_DIRECT_PROLOGUE
    const F3 wo = to_local(its.sh, neg(d));
    for (int l = 0; l < S.n_emitters; ++l) {
        const float ex = rng.next1d(), ey = rng.next1d();
        ESample es;
        const F3 li = emitter_sample(S, S.emitters[l], its.p, ex, ey, es);
        if (is_zero(li)) continue;
        Hit hs;
        if (STATS) queries++;
        if (trace<DEPTH, ORDERED, true, STATS>(tv, S, es.so, es.sd, es.smint, es.smaxt, hs, stk, stride, st)) continue;
        const F3 we = to_local(its.sh, es.wi);
        const F3 f = bsdf_eval(bsdf, wo, we, M_SOLID_ANGLE, alb);
        result = add(result, mulc(scl(fabsf(we.z), li), f));
    }
    return result;
}

// DirectMATSIntegrator::Li (src/integrators/direct_mats.cpp:16-83): one BSDF sample (the record's
// measure preset to ESolidAngle); its ray adds the environment on a miss or the emitter it hits.
template <int DEPTH, bool ORDERED, bool STATS>
__device__ F3 li_direct_mats(const DScene &S, const Traversal &tv, Rng &rng, F3 o, F3 d, float mint, float maxt,
                             uint32_t *stk, int stride, TravStats &st, uint32_t &queries) {
    NH_DIRECT_PROLOGUE
    const float bx = rng.next1d(), by = rng.next1d();
    F3 wo;
    int measure;
    const F3 col = bsdf_sample(bsdf, to_local(its.sh, neg(d)), bx, by, wo, measure, alb);
    if (is_zero(col)) return result;
    const F3 nd = to_world(its.sh, wo);
    Hit h2;
    if (STATS) queries++;
    if (!trace<DEPTH, ORDERED, false, STATS>(tv, S, its.p, nd, kEps, INFINITY, h2, stk, stride, st)) {
        if (S.envmap >= 0) result = add(result, mulc(env_eval(S, nd), col));
        return result;
    }
    Its its2;
    hit_info(S, tv, h2, its.p, nd, its2);
    const int hem = S.shapes[its2.shape].emitter;
    if (hem >= 0)
        result = add(result, mulc(emitter_eval(S.emitters[hem], its.p, its2.sh.n, normalized(sub(its2.p, its.p))), col));
    return result;
}

// DirectMISIntegrator::Li (src/integrators/direct_mis.cpp:15-143): one emitter picked at random and
// one BSDF sample, balance-heuristic weights; result + w_ems * result_ems + w_mat * result_mats.
// Occluded light samples and BSDF rays that miss emitters still fill result_ems / result_mats with
// the environment (:84-92, :127-135) under a weight of 0.
template <int DEPTH, bool ORDERED, bool STATS>
__device__ F3 li_direct_mis(const DScene &S, const Traversal &tv, Rng &rng, F3 o, F3 d, float mint, float maxt,
                            uint32_t *stk, int stride, TravStats &st, uint32_t &queries) {
    NH_DIRECT_PROLOGUE
    const float n_lights = (float)S.n_emitters;
    F3 result_ems = f3(0, 0, 0), result_mats = f3(0, 0, 0);
    float w_ems = 0.f, w_mat = 0.f;
    const int ei = emitter_pick(S, rng.next1d());
    const DEmitter em = S.emitters[ei];
    const float ex = rng.next1d(), ey = rng.next1d();
    ESample es;
    const F3 li = emitter_sample(S, em, its.p, ex, ey, es);
    const F3 wi_l = to_local(its.sh, neg(d));
    if (!is_zero(li)) {
        Hit hs;
        if (STATS) queries++;
        if (!trace<DEPTH, ORDERED, true, STATS>(tv, S, es.so, es.sd, es.smint, es.smaxt, hs, stk, stride, st)) {
            const F3 we = to_local(its.sh, es.wi);
            const F3 f = bsdf_eval(bsdf, wi_l, we, M_SOLID_ANGLE, alb);
            const float cs = we.z;
            const float pdf_ems = emitter_pdf(S, em, its.p, es.p, es.n, es.wi) / n_lights;
            const float pdf_mat = bsdf_pdf(bsdf, wi_l, we, M_SOLID_ANGLE);
            result_ems = f3(li.x * cs * f.x * n_lights, li.y * cs * f.y * n_lights, li.z * cs * f.z * n_lights);
            if (pdf_ems + pdf_mat > kEps) w_ems = pdf_ems / (pdf_ems + pdf_mat);
        } else if (S.envmap >= 0) {
            result_ems = mulc(li, env_eval(S, es.sd));
        }
    }
    const float bx = rng.next1d(), by = rng.next1d();
    F3 wo;
    int measure;
    const F3 col = bsdf_sample(bsdf, wi_l, bx, by, wo, measure, alb);
    if (measure == M_UNKNOWN) measure = M_SOLID_ANGLE;  // bqr_mat.measure = ESolidAngle before sample (:102)
    if (!is_zero(col)) {
        const F3 nd = to_world(its.sh, wo);
        Hit h2;
        if (STATS) queries++;
        const bool hit2 = trace<DEPTH, ORDERED, false, STATS>(tv, S, its.p, nd, kEps, INFINITY, h2, stk, stride, st);
        int hem = -1;
        Its its2;
        if (hit2) {
            hit_info(S, tv, h2, its.p, nd, its2);
            hem = S.shapes[its2.shape].emitter;
        }
        if (hem >= 0) {
            const DEmitter e2 = S.emitters[hem];
            const F3 wim = normalized(sub(its2.p, its.p));
            result_mats = mulc(col, emitter_eval(e2, its.p, its2.sh.n, wim));
            const float pdf_mat = bsdf_pdf(bsdf, wi_l, wo, measure);
            const float pdf_e = emitter_pdf(S, e2, its.p, its2.p, its2.sh.n, wim) / n_lights;
            if (pdf_mat + pdf_e > kEps) w_mat = pdf_mat / (pdf_mat + pdf_e);
        } else if (S.envmap >= 0) {
            result_mats = mulc(col, env_eval(S, nd));
        }
    }
    return add(add(result, scl(w_ems, result_ems)), scl(w_mat, result_mats));
}
#undef NH_DIRECT_PROLOGUE

// DirectIntegrator::Li (src/integrators/direct.cpp:17-63, the point-light integrator of scenes/pa1):
// every emitter sampled once in scene order (its own 2D sample), its shadow ray always traced;
// unoccluded samples add li * |wi . n| / |wi| * f(wi = toward the light, wo = toward the ray
// origin). No emitter-hit term.
template <int DEPTH, bool ORDERED, bool STATS>
__device__ F3 li_direct_simple(const DScene &S, const Traversal &tv, Rng &rng, F3 o, F3 d, float mint, float maxt,
                               uint32_t *stk, int stride, TravStats &st, uint32_t &queries) {
    Hit h;
    if (STATS) queries++;
    if (!trace<DEPTH, ORDERED, false, STATS>(tv, S, o, d, mint, maxt, h, stk, stride, st))
        return S.envmap >= 0 ? env_eval(S, d) : f3(0, 0, 0);
    Its its;
    hit_info(S, tv, h, o, d, its);
    const DBsdf bsdf = S.bsdfs[S.shapes[its.shape].bsdf];
    const F3 alb = bsdf_albedo(S, bsdf, its.u, its.v);
    const F3 wo = to_local(its.sh, normalized(sub(o, its.p)));
    F3 result = f3(0, 0, 0);
    for (int l = 0; l < S.n_emitters; ++l) {
        const float ex = rng.next1d(), ey = rng.next1d();
        ESample es;
        const F3 li = emitter_sample(S, S.emitters[l], its.p, ex, ey, es);
        const F3 wi = to_local(its.sh, es.wi);
        Hit hs;
        if (STATS) queries++;
        if (trace<DEPTH, ORDERED, true, STATS>(tv, S, es.so, es.sd, es.smint, es.smaxt, hs, stk, stride, st)) continue;
        const F3 f = bsdf_eval(bsdf, wi, wo, M_SOLID_ANGLE, alb);
        const float cs = fabsf(dot(es.wi, its.sh.n)) / f_sqrt(dot(es.wi, es.wi));
        result = add(result, mulc(scl(cs, li), f));
    }
    return result;
}

// NormalIntegrator::Li (src/integrators/normals.cpp:15-33): the shading frame of the first hit, as
// |shFrame.toWorld(direction)| (Frame::toWorld = s x + t y + n z); a miss sees the envmap (EnvMap::eval, wi = ray.d)
template <int DEPTH, bool ORDERED, bool STATS>
__device__ F3 li_normals(const DScene &S, const Traversal &tv, F3 o, F3 d, float mint, float maxt, uint32_t *stk,
                         int stride, TravStats &st, uint32_t &queries) {
    Hit h;
    if (STATS) queries++;
    if (!trace<DEPTH, ORDERED, false, STATS>(tv, S, o, d, mint, maxt, h, stk, stride, st))
        return S.envmap >= 0 ? env_eval(S, d) : f3(0, 0, 0);
    Its its;
    hit_info(S, tv, h, o, d, its);
    const F3 n = to_world(its.sh, f3(S.ndir[0], S.ndir[1], S.ndir[2]));
    return f3(fabsf(n.x), fabsf(n.y), fabsf(n.z));
}

// Warp::sampleUniformHemisphere(sampler, pole) (warp.cpp:25-39): rejection from the cube, three draws per try, the
// accepted point mirrored into the pole's hemisphere and divided by its norm. squaredNorm and dot in Eigen's grouping
// (nh_device.h dot); `v /= v.norm()` divides each component by sqrt(squaredNorm). A point at the origin leaves NaN
// there and here.
__device__ __forceinline__ F3 av_sample_hemisphere(Rng &rng, F3 pole) {
    F3 v;
    do {
        v.x = 1.f - 2.f * rng.next1d();
        v.y = 1.f - 2.f * rng.next1d();
        v.z = 1.f - 2.f * rng.next1d();
    } while (dot(v, v) > 1.f);
    if (dot(v, pole) < 0.f) v = neg(v);
    return divs(v, f_sqrt(dot(v, v)));
}

// AverageVisibilityIntegrator::Li (src/integrators/av.cpp:18-43): 1 for a camera ray that escapes; otherwise one
// occlusion ray Ray3f(its.p, dir, Epsilon, length) along a uniform direction of the shading normal's hemisphere, 0 if it
// hits, 1 if not. The reference asks for that ray's closest hit and reads only whether there is one: the any-hit
// traversal tests the same primitives against the same [mint, maxt] and returns that boolean.
template <int DEPTH, bool ORDERED, bool STATS>
__device__ F3 li_av(const DScene &S, const Traversal &tv, Rng &rng, F3 o, F3 d, float mint, float maxt, uint32_t *stk,
                    int stride, TravStats &st, uint32_t &queries) {
    Hit h;
    if (STATS) queries++;
    if (!trace<DEPTH, ORDERED, false, STATS>(tv, S, o, d, mint, maxt, h, stk, stride, st)) return f3(1, 1, 1);
    Its its;
    hit_info(S, tv, h, o, d, its);
    const F3 dir = av_sample_hemisphere(rng, its.sh.n);
    Hit hs;
    if (STATS) queries++;
    const float v = trace<DEPTH, ORDERED, true, STATS>(tv, S, its.p, dir, kEps, S.av_length, hs, stk, stride, st) ? 0.f : 1.f;
    return f3(v, v, v);
}

// EnvMapTester::Li (src/integrators/EnvMapTester.cpp:16-26): EnvMap::pdf of the camera ray's direction, over 100
__device__ __forceinline__ F3 li_envmaptester(const DScene &S, F3 d) {
    const float v = env_pdf(S, d) / 100.f;
    return f3(v, v, v);
}

#ifdef NH_DISNEY
}  // namespace nh_disney
#endif
