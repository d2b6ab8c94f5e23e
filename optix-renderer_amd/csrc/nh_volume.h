// Homogeneous participating media as device functions, for the kernels that run a camera path per thread
// (nh_vol_path_kernel in nh_volume.hip, ad_path_kernel in nh_adaptive.hip) and the medium query kernel.
//
// The media themselves: VacuumMedium (src/media/vacuum.cpp), HomogeneousMedium (homogmedium.cpp:61-73), IsoPhase
// (src/bsdf/isophase.cpp), AnisoPhase (anisophase.cpp, Warp::squareToHenyeyGreenstein{,Pdf}, warp.cpp:168-205).
// li_path_vol is PathVolMATSIntegrator::Li / PathVolMISIntegrator::Li (src/integrators/path_vol_mats.cpp:20-122,
// path_vol_mis.cpp:26-243), reproduced as written, quirks included: throughput is multiplied by the
// transmittance and never divided by the free-path density, no albedo at a scattering event, a miss ends the path
// before any medium is sampled, the MIS light sample of a medium interaction is taken from the surface point behind it.
//
// Always nh_disney's: the units that include this are built with -DNH_DISNEY only, with every BSDF and emitter type
// the HIP path has (nh_device.h kDisney, kExtLights). Traversal, hit information, BSDFs, emitters, camera and pcg32 are
// the shared device functions of nh_traverse.h / nh_shade.h / nh_device.h.
#pragma once
#include "nh_internal.h"
#include "nh_traverse.h"
#include "nh_shade.h"

#ifndef NH_DISNEY
#error "nh_volume.h is for units built with -DNH_DISNEY"
#endif

using namespace nhd;

namespace nh_disney {

namespace {

// A medium handle is 1 + its index in DScene::media, 0 = the default ambient VacuumMedium (scene.cpp:74-75).
// The record is uniform across a wave only by accident, so it is loaded per lane (64 B, two cache lines at most).
struct Medium {
    bool homog;
    F3 mu_t;
    int phase;
    float g;
};
NHD Medium medium_load(const DScene &S, int handle) {
    Medium m;
    m.homog = false;
    m.mu_t = f3(0, 0, 0);
    m.phase = PHASE_ISO;
    m.g = 0.f;
    if (handle > 0) {
        const DMedium r = S.media[handle - 1];
        m.homog = r.type == MEDIUM_HOMOG;
        m.mu_t = f3(r.mu_t[0], r.mu_t[1], r.mu_t[2]);
        m.phase = r.phase;
        m.g = r.g;
    }
    return m;
}

// HomogeneousMedium::sampleFreePath (homogmedium.cpp:61-67) / VacuumMedium::sampleFreePath (vacuum.cpp:29-32): a
// channel (int)(3 u) from one draw, a second draw only when that channel's mu_t >= Epsilon; vacuum draws nothing.
// draw(): the sampler's next1D. -std::log(float) is logf: fp64, rounded once (nh_device.h f_log).
template <class Draw>
NHD float medium_free_path(const Medium &m, Draw &draw) {
    if (!m.homog) return INFINITY;
    int ch = (int)(3.f * draw());
    ch = ch < 0 ? 0 : (ch > 2 ? 2 : ch);  // (u in [0, 1) gives 0..2: 3 (1 - 2^-24) rounds below 3; the clamp bounds a query's u)
    const float mu = ch == 0 ? m.mu_t.x : (ch == 1 ? m.mu_t.y : m.mu_t.z);
    if (mu < kEps) return INFINITY;
    return -f_log(draw()) / mu;
}
// HomogeneousMedium::getTransmittance (homogmedium.cpp:69-73): (-mu_t * |from - to|).exp(), std::exp(float) per channel
// (fp64, rounded once); vacuum: 1 (vacuum.cpp:34-38)
NHD F3 medium_transmittance(const Medium &m, F3 from, F3 to) {
    if (!m.homog) return f3(1.f, 1.f, 1.f);
    const F3 dd = sub(from, to);
    const float len = f_sqrt(dot(dd, dd));
    return f3(f_exp(-m.mu_t.x * len), f_exp(-m.mu_t.y * len), f_exp(-m.mu_t.z * len));
}
// Warp::squareToHenyeyGreenstein (warp.cpp:168-198); a 1 - cos^2 that rounds below zero gives the reference's NaN
NHD F3 henyey_greenstein(float sx, float sy, float g) {
    float ct;
    if (fabsf(g) < kEps) {
        ct = 1.f - 2.f * sx;
    } else {
        const float factor = (1.f - g * g) / (1.f - g + 2.f * g * sx);
        ct = (1.f + g * g - factor * factor) / (2.f * g);
    }
    const float phi = 2.f * kPi * sy;
    const float st = f_sqrt(1.f - ct * ct);
    float sp, cp;
    f_sincos(phi, sp, cp);
    return f3(st * cp, st * sp, ct);
}
// IsoPhase::sample (isophase.cpp:25-28) / AnisoPhase::sample (anisophase.cpp:30-33): wo in the frame whose +z is wi
NHD F3 phase_sample(const Medium &m, float sx, float sy) {
    return m.phase == PHASE_HG ? henyey_greenstein(sx, sy, m.g) : uniform_sphere(sx, sy);
}
// IsoPhase::pdf (isophase.cpp:20-23) / Warp::squareToHenyeyGreensteinPdf (warp.cpp:200-205; std::pow(float, 1.5f) is
// powf: fp64, rounded once)
NHD float phase_pdf(const Medium &m, F3 wo) {
    if (m.phase != PHASE_HG) return 0.25f / kPi;
    const float g2 = m.g * m.g;
    return 0.25f / kPi * (1.f - g2) / f_pow(1.f + g2 - 2.f * m.g * wo.z, 1.5f);
}

// Intersection::geoFrame.n: the face normal (mesh.cpp:163) / the sphere's normal before its normal map (sphere.cpp:99, :109)
NHD F3 geo_normal(const DScene &S, const Traversal &tv, const Hit &h, const Its &its) {
    const DShape sh = S.shapes[its.shape];
    if (sh.type == SHAPE_SPHERE) return normalized(sub(its.p, f3(sh.cx, sh.cy, sh.cz)));
    const float4 a = tv.prims[3 * h.k], b = tv.prims[3 * h.k + 1], c = tv.prims[3 * h.k + 2];
    const F3 p0 = f3(a.x, a.y, a.z), p1 = f3(b.x, b.y, b.z), p2 = f3(c.x, c.y, c.z);
    return normalized(cross(sub(p1, p0), sub(p2, p0)));
}
// the medium a ray along w continues in after crossing the surface of `shape` (path_vol_mats.cpp:110-113,
// path_vol_mis.cpp:37-39, :73-75, :231-234): the shape's when it points against the geometric normal and the shape
// has one, else the ambient medium. Overlapping media are unhandled, as in the reference.
NHD int crossed_medium(const DScene &S, int shape, F3 w, F3 gn) {
    const int sm = S.shape_medium ? S.shape_medium[shape] : 0;
    return (dot(w, gn) < 0.f && sm) ? sm : S.ambient_medium;
}

struct RngDraw {
    Rng &rng;
    NHD float operator()() { return rng.next1d(); }
};

// A shadow ray crosses at most this many BSDF-less boundaries; one that would cross more counts as occluded. The
// reference's loop is unbounded; each crossing moves the origin on by at least the ray epsilon, so only a scene with
// thousands of nested medium boundaries reaches the bound.
constexpr int kMaxShadowCrossings = 4096;

// PathVolMISIntegrator::traceShadowray (path_vol_mis.cpp:26-46): closest hits along the shadow ray; a shape with a
// BSDF occludes, any other multiplies tr by the current shadow medium's transmittance up to the hit, switches the
// medium, moves the origin to the hit and shortens maxt by its t (mint stays Epsilon: the traversal re-derives the
// adaptive epsilon from the new origin, as Scene::rayIntersect does for every ray).
template <int DEPTH, bool STATS>
__device__ bool shadow_walk(const DScene &S, const Traversal &tv, int med, F3 o, F3 d, float mint, float maxt, F3 &tr,
                            uint32_t *stk, int stride, TravStats &st, uint32_t &queries) {
    for (int it = 0; it < kMaxShadowCrossings; ++it) {
        Hit h;
        if (STATS) queries++;
        if (!trace<DEPTH, true, false, STATS>(tv, S, o, d, mint, maxt, h, stk, stride, st)) return false;
        const int shape = __float_as_int(tv.prims[3 * h.k + 1].w);
        if (S.shapes[shape].bsdf >= 0) return true;
        Its its;
        hit_info<false>(S, tv, h, o, d, its);  // p only: a normal map does not move it
        tr = mulc(tr, medium_transmittance(medium_load(S, med), o, its.p));
        med = crossed_medium(S, shape, d, geo_normal(S, tv, h, its));
        o = its.p;
        maxt -= h.t;
    }
    return true;
}

// PathVolMATSIntegrator::Li (path_vol_mats.cpp:20-122) and PathVolMISIntegrator::Li with its sampleEmitter
// (path_vol_mis.cpp:53-243). Draws per loop iteration, in this order: the free path's (0, 1 or 2), the
// roulette's if due, then at a medium interaction the phase sample's two and (MIS) the emitter pick and the light
// sample's two; at a surface with a BSDF the BSDF sample's two and (MIS, solid-angle measure) the same three.
template <int DEPTH, bool STATS, bool MIS>
__device__ F3 li_path_vol(const DScene &S, const Traversal &tv, Rng &rng, F3 o, F3 d, float mint, float maxt,
                          uint32_t *stk, int stride, TravStats &st, uint32_t &queries) {
    F3 li = f3(0, 0, 0), t = f3(1, 1, 1);
    int med = S.ambient_medium;
    float pdf_mat = 1.f;  // (path_vol_mis.cpp:117-118: the camera counts as a discrete BSDF)
    int pdf_measure = M_DISCRETE;
    const float n_lights = (float)S.n_emitters;
    RngDraw draw{rng};
    for (int bounces = 0;; ++bounces) {
        Hit h;
        bool found = false;
        if (!(d.x == 0 && d.y == 0 && d.z == 0)) {  // (a zero direction misses every primitive, as in li_path_mats)
            if (STATS) queries++;
            found = trace<DEPTH, true, false, STATS>(tv, S, o, d, mint, maxt, h, stk, stride, st);
        }
        // a miss ends the path before any medium is sampled. path_vol_mats builds its record as
        // EmitterQueryRecord(ray.d), which leaves the wi EnvMap::eval reads unset; ray.d is what path_vol_mis and
        // path_mats pass, and what is evaluated here
        if (!found) {
            if (S.envmap >= 0) li = add(li, mulc(t, env_eval(S, d)));
            break;
        }
        Its its;
        hit_info(S, tv, h, o, d, its);
        const DShape shape = S.shapes[its.shape];
        const Medium m = medium_load(S, med);
        const float tm = medium_free_path(m, draw);
        const bool in_medium = tm < h.t;
        const F3 p = in_medium ? add(o, scl(tm, d)) : its.p;
        t = mulc(t, medium_transmittance(m, o, p));

        // emission: none inside a medium (a medium's emitter is not supported); a hit emitter, MIS-weighted by the
        // last sample's density (path_vol_mats.cpp:61-68, path_vol_mis.cpp:157-173)
        if (!in_medium && shape.emitter >= 0) {
            const DEmitter em = S.emitters[shape.emitter];
            const F3 wi = normalized(sub(its.p, o));
            const F3 le = emitter_eval(em, o, its.sh.n, wi);
            if (MIS) {
                const float pdf_mat_em = emitter_pdf(S, em, o, its.p, its.sh.n, wi) / n_lights;
                const float w_mat = pdf_measure == M_DISCRETE ? 1.f
                                                               : (pdf_mat > kEps ? pdf_mat / (pdf_mat + pdf_mat_em) : 0.f);
                li = add(li, mulc(scl(w_mat, t), le));
            } else {
                li = add(li, mulc(t, le));
            }
        }
        const bool has_bsdf = shape.bsdf >= 0;
        if (bounces >= 3 && (in_medium || has_bsdf)) {  // path_vol_mats.cpp:71-79
            const float succ = e_min(max_coeff(t), 0.99f);
            if (rng.next1d() > succ || succ < kEps) break;
            t = divs(t, succ);
        }

        F3 wo = d;  // a surface without a BSDF leaves the ray as it is
        DBsdf bsdf{};
        F3 alb = f3(0, 0, 0), col = f3(1, 1, 1);
        const bool surface = !in_medium && has_bsdf;
        bool nee = false;  // sampleEmitter's measure test (path_vol_mis.cpp:58-59): no draws for a discrete sample
        if (in_medium) {
            const float sx = rng.next1d(), sy = rng.next1d();
            const F3 wl = phase_sample(m, sx, sy);
            wo = to_world(frame_from_n(d), wl);  // Frame(ray.d).toWorld(pRec.wo)
            if (MIS) {
                pdf_mat = phase_pdf(m, wl);
                pdf_measure = M_SOLID_ANGLE;
                nee = true;
            }
        } else if (has_bsdf) {
            bsdf = S.bsdfs[shape.bsdf];
            alb = bsdf_albedo(S, bsdf, its.u, its.v);
            const float bx = rng.next1d(), by = rng.next1d();
            F3 wl;
            int measure;
            col = bsdf_sample(bsdf, to_local(its.sh, neg(d)), bx, by, wl, measure, alb);
            wo = to_world(its.sh, wl);
            if (MIS) {
                pdf_mat = bsdf_pdf(bsdf, to_local(its.sh, neg(d)), wl, measure);
                pdf_measure = measure;
                nee = measure == M_SOLID_ANGLE;
            }
        }
        if (MIS && nee) {
            // sampleEmitter (path_vol_mis.cpp:53-105), as written. At a medium interaction the emitter is still
            // sampled from its.p, the surface point behind the interaction; the phase density is taken at
            // its.toLocal(shadowRay.d); the shadow medium follows its.geoFrame.n / its.shape; and the "phase value" is
            // |wi . shadowRay.d|. At a surface it runs before the throughput takes the BSDF sample's weight (:223-227).
            const int ei = emitter_pick(S, rng.next1d());
            const DEmitter em = S.emitters[ei];
            const float ex = rng.next1d(), ey = rng.next1d();
            ESample es;
            const F3 ev = emitter_sample(S, em, its.p, ex, ey, es);
            const F3 le = scl(n_lights, ev);
            const float pdf_em = emitter_pdf(S, em, its.p, es.p, es.n, es.wi) / n_lights;
            if (pdf_em > kEps) {  // (else w_em = 0 and nothing is added, whatever the shadow ray meets)
                const int smed = dot(d, es.sd) > 0.f ? crossed_medium(S, its.shape, es.sd, geo_normal(S, tv, h, its)) : med;
                F3 str = f3(1.f, 1.f, 1.f);
                if (!shadow_walk<DEPTH, STATS>(S, tv, smed, es.so, es.sd, es.smint, es.smaxt, str, stk, stride, st,
                                               queries)) {
                    const F3 wi_l = to_local(its.sh, neg(d)), we = to_local(its.sh, es.wi);
                    const float pdf_em_mat =
                        surface ? bsdf_pdf(bsdf, wi_l, we, M_SOLID_ANGLE) : phase_pdf(m, to_local(its.sh, es.sd));
                    const float w_em = pdf_em / (pdf_em + pdf_em_mat);
                    if (w_em > kEps) {
                        F3 x;
                        if (surface) {
                            x = scl(fabsf(dot(es.wi, its.sh.n)), bsdf_eval(bsdf, wi_l, we, M_SOLID_ANGLE, alb));
                        } else {
                            const float ph = fabsf(dot(es.wi, es.sd));
                            x = f3(ph, ph, ph);
                        }
                        li = add(li, mulc(mulc(mulc(scl(w_em, str), t), le), x));
                    }
                }
            }
        }
        if (surface) t = mulc(t, col);
        // entering or leaving the hit shape (path_vol_mats.cpp:109-113): only at a surface, only when the ray goes on
        // through it
        if (!in_medium && dot(d, wo) > 0.f) med = crossed_medium(S, its.shape, wo, geo_normal(S, tv, h, its));
        o = p;
        d = wo;
        mint = kEps;
        maxt = INFINITY;
    }
    return li;
}

}  // namespace

}  // namespace nh_disney
