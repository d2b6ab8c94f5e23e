// Internal declarations shared by the host-side translation units.
#pragma once
#include <cstdint>
#include <string>
#include <vector>

#include "nori_hip.h"

namespace nh {
void set_host_error(const std::string &msg);
// PNG -> 8-bit RGBA (png_decode.cpp); false with a message on malformed or unsupported files
bool png_decode_rgba8(const std::string &path, std::vector<uint8_t> &out, unsigned &width, unsigned &height,
                      std::string &err);
// Radiance RGBE .hdr -> float RGBA as the reference's HDRLoader decodes it (hdr_decode.cpp); false with a message on
// malformed or unsupported files
bool hdr_decode_rgba(const std::string &path, std::vector<float> &out, unsigned &width, unsigned &height,
                     std::string &err);
// PhotonMapper's automatic radius (photonmapper.cpp:75-76) of a scene box: getExtents().norm() / 500.0f in fp32, the
// squared norm grouped x*x + (y*y + z*z) as Eigen sums a Vector3f (photon_host.cpp)
float photon_auto_radius(const float bbox_min[3], const float bbox_max[3]);
// The warp test's argument checks (warptest.cpp): NH_OK, or the code of the refusal with its message in `msg`.
// warp_check_type: an NH_WARP_* type the HIP path runs (Schlick refused by name) and a finite parameter;
// warp_check_table: 1 <= xres, yres and at most NH_CHI2_MAX_CELLS cells
int warp_check_type(const char *who, int32_t type, float parameter, std::string &msg);
int warp_check_table(const char *who, int32_t xres, int32_t yres, std::string &msg);
}
