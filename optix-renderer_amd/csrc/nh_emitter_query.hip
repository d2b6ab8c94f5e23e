// The kernel of nh_emitter_query: point queries of one emitter of the uploaded scene through emitter_sample /
// emitter_eval / emitter_pdf (nh_shade.h), the device functions the megakernel and the wavefront kernels call -- the
// emitter counterpart of the BSDF query (nh_disney.hip), after the reference's chi2test / ttest hooks.
// Built with -DNH_DISNEY (Makefile), like nh_disney.hip: the spot / directional branches exist only then (nh_device.h
// kExtLights).
#include "nh_internal.h"
#include "nh_photon.h"
#include "nh_shade.h"

#ifndef NH_DISNEY
#error "nh_emitter_query.hip is built with -DNH_DISNEY"
#endif

using namespace nhd;

namespace nh_disney {

// One thread per query
__global__ __launch_bounds__(64) void emitter_query_kernel(const DScene *__restrict__ Sp, nh::EmitterQuery q) {
    const int i = blockIdx.x * 64 + threadIdx.x;
    if (i >= q.n) return;
    const DScene &S = *Sp;
    const DEmitter e = S.emitters[q.emitter];
    if (q.mode == NH_EMITTER_QUERY_SAMPLE_PHOTON) {  // samplePhoton, with the photon pass's `* lights.size()`
        const float *s = q.in + 4 * (size_t)i;
        F3 po, pd;
        float pdf;
        const F3 W = scl((float)S.n_emitters, emitter_sample_photon(S, e, s[0], s[1], s[2], s[3], po, pd, pdf));
        float *o = q.out + (size_t)NH_EMITTER_QUERY_PHOTON_STRIDE * i;
        o[0] = po.x; o[1] = po.y; o[2] = po.z;
        o[3] = pd.x; o[4] = pd.y; o[5] = pd.z;
        o[6] = W.x; o[7] = W.y; o[8] = W.z;
        o[9] = pdf;
        o[10] = o[11] = 0.f;
        return;
    }
    const F3 ref = f3(q.ref[3 * i], q.ref[3 * i + 1], q.ref[3 * i + 2]);
    if (q.mode == NH_EMITTER_QUERY_SAMPLE) {
        ESample es;
        const F3 col = emitter_sample(S, e, ref, q.in[2 * i], q.in[2 * i + 1], es);
        const float pdf = emitter_pdf(S, e, ref, es.p, es.n, es.wi);
        float *o = q.out + (size_t)NH_EMITTER_QUERY_SAMPLE_STRIDE * i;
        o[0] = col.x; o[1] = col.y; o[2] = col.z;
        o[3] = es.wi.x; o[4] = es.wi.y; o[5] = es.wi.z;
        o[6] = pdf;
        o[7] = es.so.x; o[8] = es.so.y; o[9] = es.so.z;
        o[10] = es.sd.x; o[11] = es.sd.y; o[12] = es.sd.z;
        o[13] = es.smint;
        o[14] = es.smaxt;
        o[15] = 0.f;
        return;
    }
    const float *in = q.in + (size_t)NH_EMITTER_QUERY_IN_STRIDE * i;
    const F3 wi = f3(in[0], in[1], in[2]), p = f3(in[3], in[4], in[5]), n = f3(in[6], in[7], in[8]);
    if (q.mode == NH_EMITTER_QUERY_EVAL) {
        const F3 v = emitter_eval(S, e, ref, n, wi);
        q.out[3 * (size_t)i] = v.x;
        q.out[3 * (size_t)i + 1] = v.y;
        q.out[3 * (size_t)i + 2] = v.z;
    } else {
        q.out[i] = emitter_pdf(S, e, ref, p, n, wi);
    }
}

namespace nh {

void launch_emitter_query(const DScene *S, const EmitterQuery &q, hipStream_t st) {
    if (q.n <= 0) return;
    hipLaunchKernelGGL(emitter_query_kernel, dim3((q.n + 63) / 64), dim3(64), 0, st, S, q);
}

}  // namespace nh
}  // namespace nh_disney
