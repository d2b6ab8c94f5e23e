// Disney-only kernels (built with -DNH_DISNEY, Makefile): the upload-time fold of a Disney BSDF's constants and the
// BSDF query kernel of nh_bsdf_query. Both call the device functions of nh_device.h that the render kernels call.
#include "nh_internal.h"

#ifndef NH_DISNEY
#error "nh_disney.hip is built with -DNH_DISNEY"
#endif

using namespace nhd;

namespace nh_disney {

// One thread per record: the parameter-only scalars, then the colour terms of the record's constant albedo
// (disney_colors, the function eval runs per hit for a textured albedo: the two routes give the same bits)
__global__ __launch_bounds__(64) void disney_fold_kernel(DDisney *recs, const float *albedo, int n) {
    const int i = blockIdx.x * 64 + threadIdx.x;
    if (i >= n) return;
    DDisney p = recs[i];
    disney_fold_params(p);
    const DisneyCol c = disney_colors(p.specular, p.specular_tint, p.metallic, p.sheen_tint,
                                      f3(albedo[3 * i], albedo[3 * i + 1], albedo[3 * i + 2]));
    p.cdlin[0] = c.cdlin.x; p.cdlin[1] = c.cdlin.y; p.cdlin[2] = c.cdlin.z;
    p.cspec0[0] = c.cspec0.x; p.cspec0[1] = c.cspec0.y; p.cspec0[2] = c.cspec0.z;
    p.csheen[0] = c.csheen.x; p.csheen[1] = c.csheen.y; p.csheen[2] = c.csheen.z;
    recs[i] = p;
}

// One thread per query. mode 0: eval and pdf of (wi, wo) in the solid-angle measure; mode 1: sample from
// (wi, sample2d), then pdf of the sampled wo in the sampled measure (as the reference's chi2test / ttest hooks)
__global__ __launch_bounds__(64) void bsdf_query_kernel(nh::BsdfQuery q) {
    const int i = blockIdx.x * 64 + threadIdx.x;
    if (i >= q.n) return;
    const DBsdf b = q.bsdf;
    const F3 alb = f3(q.albedo[0], q.albedo[1], q.albedo[2]);
    const F3 wi = f3(q.wi[3 * i], q.wi[3 * i + 1], q.wi[3 * i + 2]);
    F3 wo, val;
    int measure = M_SOLID_ANGLE;
    if (q.mode == 0) {
        wo = f3(q.wo[3 * i], q.wo[3 * i + 1], q.wo[3 * i + 2]);
        val = bsdf_eval(b, wi, wo, measure, alb);
    } else {
        val = bsdf_sample(b, wi, q.sample[2 * i], q.sample[2 * i + 1], wo, measure, alb);
    }
    q.pdf[i] = bsdf_pdf(b, wi, wo, measure);
    q.value[3 * i] = val.x;
    q.value[3 * i + 1] = val.y;
    q.value[3 * i + 2] = val.z;
    if (q.wo_out) {
        q.wo_out[3 * i] = wo.x;
        q.wo_out[3 * i + 1] = wo.y;
        q.wo_out[3 * i + 2] = wo.z;
    }
    if (q.measure) q.measure[i] = measure;
}

namespace nh {

void launch_disney_fold(DDisney *recs, const float *albedo, int n, hipStream_t st) {
    if (n <= 0) return;
    hipLaunchKernelGGL(disney_fold_kernel, dim3((n + 63) / 64), dim3(64), 0, st, recs, albedo, n);
}

void launch_bsdf_query(const BsdfQuery &q, hipStream_t st) {
    if (q.n <= 0) return;
    hipLaunchKernelGGL(bsdf_query_kernel, dim3((q.n + 63) / 64), dim3(64), 0, st, q);
}

}  // namespace nh
}  // namespace nh_disney
