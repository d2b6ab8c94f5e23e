// Host side of the photon mapper: PhotonData's decode tables (src/utils/photon.cpp:30-41) and PhotonMapper's automatic
// gather radius (src/integrators/photonmapper.cpp:75-76). No GPU runtime.
#include <cmath>

#include "nh_host.h"

namespace nh {

float photon_auto_radius(const float bbox_min[3], const float bbox_max[3]) {
    const float ex = bbox_max[0] - bbox_min[0], ey = bbox_max[1] - bbox_min[1], ez = bbox_max[2] - bbox_min[2];
    const float n2 = ex * ex + (ey * ey + ez * ez);
    return std::sqrt(n2) / 500.0f;
}

}  // namespace nh

extern "C" int nh_photon_tables(float *cos_theta, float *sin_theta, float *cos_phi, float *sin_phi, float *exp_table) {
    if (!cos_theta || !sin_theta || !cos_phi || !sin_phi || !exp_table) {
        nh::set_host_error("null argument");
        return NH_ERR_INVALID;
    }
    const float pi = 3.14159265358979323846f;  // Nori's M_PI is a float constant (common.h:61)
    for (int i = 0; i < 256; i++) {
        const float angle = (float)i * (pi / 256.0f);
        cos_phi[i] = std::cos(2.0f * angle);
        sin_phi[i] = std::sin(2.0f * angle);
        cos_theta[i] = std::cos(angle);
        sin_theta[i] = std::sin(angle);
        exp_table[i] = std::ldexp((float)1, i - (128 + 8));
    }
    exp_table[0] = 0;
    return NH_OK;
}
