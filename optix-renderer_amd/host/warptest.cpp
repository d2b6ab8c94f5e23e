// The host side of the reference's warp test (src/utils/warptest.cpp): the slider maps and the argument checks of the
// nh_warp_* entry points (csrc/nh_warp_api.hip). No device needed.
#include <cmath>

#include "nh_host.h"

namespace nh {

int warp_check_type(const char *who, int32_t type, float parameter, std::string &msg) {
    if (type == NH_WARP_SCHLICK) {
        msg = std::string(who) + ": NH_WARP_SCHLICK is not supported: squareToSchlick leaves [-1, 1], and the "
              "reference then bins a NaN through an (int) cast, which is undefined";
        return NH_ERR_UNSUPPORTED;
    }
    if (type < NH_WARP_NONE || type > NH_WARP_ANISO_PHASE) {
        msg = std::string(who) + ": unknown warp type";
        return NH_ERR_INVALID;
    }
    if (!std::isfinite(parameter)) {
        msg = std::string(who) + ": the parameter must be finite";
        return NH_ERR_INVALID;
    }
    return NH_OK;
}

int warp_check_table(const char *who, int32_t xres, int32_t yres, std::string &msg) {
    if (xres < 1 || yres < 1 || (int64_t)xres * yres > NH_CHI2_MAX_CELLS) {
        msg = std::string(who) + ": the table needs 1 <= xres, yres and at most " + std::to_string(NH_CHI2_MAX_CELLS) +
              " cells";
        return NH_ERR_UNSUPPORTED;
    }
    return NH_OK;
}

}  // namespace nh

extern "C" {

// std::exp / std::log / std::sin / std::cos of a float are the float library functions: evaluated in fp64 and rounded
// once, as everywhere in this library
int nh_warp_map_parameter(int32_t type, float slider, float *value) {
    std::string msg;
    if (!value) {
        nh::set_host_error("nh_warp_map_parameter: null argument");
        return NH_ERR_INVALID;
    }
    if (int rc = nh::warp_check_type("nh_warp_map_parameter", type, slider, msg)) {
        nh::set_host_error(msg);
        return rc;
    }
    float v = slider;
    if (type == NH_WARP_BECKMANN || type == NH_WARP_MICROFACET_BRDF) {  // warptest.cpp:89-91
        const float log_lo = (float)std::log((double)0.05f), log_hi = (float)std::log((double)1.f);
        const float e = log_lo * (1 - v) + log_hi * v;
        v = (float)std::exp((double)e);
    } else if (type == NH_WARP_HENYEY_GREENSTEIN || type == NH_WARP_ANISO_PHASE) {  // :92-95
        v = 2 * v - 1;
    }
    *value = v;
    return NH_OK;
}

int nh_warp_wi(float angle_slider, float wi[3]) {
    if (!wi) {
        nh::set_host_error("nh_warp_wi: null argument");
        return NH_ERR_INVALID;
    }
    const float angle = 3.14159265358979323846f * (angle_slider - 0.5f);  // warptest.cpp:183
    const float x = (float)std::sin((double)angle), c = (float)std::cos((double)angle);
    const float z = c < 1e-4f ? 1e-4f : c;  // std::max(cos, 1e-4f)
    // Vector3f::normalized(): the squared norm grouped as Eigen sums a Vector3f, a division per component
    const float n = x * x + (0.f * 0.f + z * z);
    if (n > 0.f) {
        const float s = std::sqrt(n);
        wi[0] = x / s;
        wi[1] = 0.f / s;
        wi[2] = z / s;
    } else {
        wi[0] = x;
        wi[1] = 0.f;
        wi[2] = z;
    }
    return NH_OK;
}

}  // extern "C"
