// SPDX-License-Identifier: MIT
// sfmx — host side of the scene outputs (include/sfmx_report.h): the two reprojection-error CSV texts of
// SceneUtils.cpp:28-144, the bytes of the cloud PLY (PclUtils.cpp:401-460) and of the camera PLY
// (PclUtils.cpp:466-590), and the pixel gather of Scene::colorizePointcloud for images in host memory.
// Header only, no HIP: csrc/report.hip wraps it into the C ABI and tests/cpp/report_host_main.cpp builds it
// stand-alone under the host sanitizers.  The numbers of the CSVs are cloudhost::statistics / histogram
// (csrc/cloud_host.hpp), which put NaN errors behind the ordered ones before they sort.
//
// Build the including file with -ffp-contract=off: the frustum corners are sums in a fixed association.
#pragma once
#include <algorithm>
#include <cstdint>
#include <string>
#include <vector>

#include "cloud_host.hpp"

namespace sfmx {
namespace reporthost {

using cloudhost::E_INVAL;
using cloudhost::OK;
using cloudhost::put_f6;
using cloudhost::put_raw;
using cloudhost::Stats;

inline std::string stats_csv(const Stats& s) {   // SceneUtils.cpp:31-33, :75-77
    std::string o = "N_Points,Max_Error,Min_Error,Avg_Error,Median_Error,Variance_Error,Deviation_Error\n";
    o += std::to_string((long long)s.n_points);
    for (double v : {s.max, s.min, s.mean, s.median, s.variance, s.deviation}) { o += ','; put_f6(o, v); }
    o += '\n';
    return o;
}

inline std::string hist_csv(const double* key, const uint64_t* count, int64_t n) {   // SceneUtils.cpp:137-141
    std::string o = "Error,Count\n";
    for (int64_t i = 0; i < n; ++i) {
        put_f6(o, key[i]);
        o += ',';
        o += std::to_string((unsigned long long)count[i]);
        o += '\n';
    }
    return o;
}

// PclUtils.cpp:401-460, binary = true on a little-endian host; points in cloud order.  rgb null: 0, 0, 0.
inline std::string pointcloud_ply(const double* xyz, int64_t n_points, const uint8_t* rgb) {
    const int64_t n = n_points > 0 ? n_points : 0;
    std::string o = "ply\nformat binary_little_endian 1.0\nelement vertex " + std::to_string((long long)n) +
                    "\nproperty float x\nproperty float y\nproperty float z\nproperty uchar red\nproperty uchar green\n"
                    "property uchar blue\nend_header\n";
    o.reserve(o.size() + 15 * (size_t)n);
    for (int64_t i = 0; i < n; ++i) {
        put_raw<float>(o, (float)xyz[3 * i]);
        put_raw<float>(o, (float)xyz[3 * i + 1]);
        put_raw<float>(o, (float)xyz[3 * i + 2]);
        for (int c = 0; c < 3; ++c) put_raw<uint8_t>(o, rgb ? rgb[3 * i + c] : (uint8_t)0);
    }
    return o;
}

struct Camera { int32_t width, height; double fx, fy, cx, cy; };
struct Shot { int32_t camera, recovered; double pose[12]; };

// PclUtils.cpp:466-590.  color null: 255, 255, 0.  A written shot without a camera: E_INVAL.
inline int cameras_ply(const Camera* cameras, int32_t n_cameras, const Shot* shots, int32_t n_shots, const uint8_t* color,
                       bool only_recovered, std::string& o, std::string& err) {
    std::vector<const Shot*> use;
    for (int32_t i = 0; i < n_shots; ++i) {
        if (only_recovered && !shots[i].recovered) continue;
        if (shots[i].camera < 0 || shots[i].camera >= n_cameras) { err = "shot without a camera"; return E_INVAL; }
        use.push_back(&shots[i]);
    }
    const long long n = (long long)use.size();
    const int r = color ? color[0] : 255, g = color ? color[1] : 255, b = color ? color[2] : 0;
    const std::string rgb = " " + std::to_string(r) + " " + std::to_string(g) + " " + std::to_string(b) + "\n";
    o = "ply\nformat ascii 1.0\nelement vertex " + std::to_string(n * 5 + 4) +
        "\nproperty float x\nproperty float y\nproperty float z\nproperty uchar red\nproperty uchar green\n"
        "property uchar blue\nelement edge " + std::to_string(n * 8 + 3) +
        "\nproperty int vertex1\nproperty int vertex2\nproperty uchar red\nproperty uchar green\nproperty uchar blue\n"
        "end_header\n"
        "0 0 0 0 0 0\n1 0 0 255 0 0\n0 1 0 0 255 0\n0 0 1 0 0 255\n";   // the coordinate system: integer literals
    for (const Shot* s : use) {
        const Camera& c = cameras[s->camera];
        const double norm = 1.0 / (double)std::max(c.width, c.height);
        const double width = (double)c.width * norm, height = (double)c.height * norm;
        const double focal = ((c.fx == c.fy) ? c.fx : (c.fx + c.fy) / 2.0) * norm;   // ICamera.cpp:62-66
        const double cx = c.cx * norm, cy = c.cy * norm;
        const double left = -cx, right = width - cx, top = -cy, bottom = height - cy;
        const double pts[5][3] = {{0, 0, 0}, {left, top, focal}, {right, top, focal}, {left, bottom, focal}, {right, bottom, focal}};
        const double* m = s->pose;
        for (const auto& p : pts) {   // cv::Affine3d(pose) * point
            for (int k = 0; k < 3; ++k) {
                put_f6(o, m[4 * k] * p[0] + m[4 * k + 1] * p[1] + m[4 * k + 2] * p[2] + m[4 * k + 3]);
                o += ' ';
            }
            o.pop_back();
            o += rgb;
        }
    }
    for (long long i = 0; i < n; ++i) {
        const long long f = 4 + i * 5, tl = f + 1, tr = f + 2, bl = f + 3, br = f + 4;
        const long long edges[8][2] = {{f, tl}, {f, tr}, {f, bl}, {f, br}, {tl, tr}, {tr, br}, {br, bl}, {bl, tl}};
        for (const auto& e : edges) o += std::to_string(e[0]) + " " + std::to_string(e[1]) + rgb;
    }
    o += "0 1 255 0 0\n0 2 0 255 0\n0 3 0 0 255\n";
    return OK;
}

struct Image { const uint8_t* data; int32_t width, height; int64_t pitch; };

// Scene.cpp:601-605 for the record each point's colour comes from (selected and rounded on the device):
// record[p] < 0 or a position outside the image gives the default colour.
inline void gather_colors(int64_t n_points, const int64_t* record, const int32_t* px, const int32_t* py,
                          const int32_t* origin_shot, const Image* images, const uint8_t* def, uint8_t* out_rgb) {
    for (int64_t p = 0; p < n_points; ++p) {
        uint8_t* o = out_rgb + 3 * p;
        o[0] = def[0]; o[1] = def[1]; o[2] = def[2];
        if (record[p] < 0) continue;
        const Image& im = images[origin_shot[record[p]]];
        const int32_t x = px[p], y = py[p];
        if (x < 0 || x >= im.width || y < 0 || y >= im.height) continue;
        const uint8_t* pix = im.data + (int64_t)y * im.pitch + 3 * (int64_t)x;
        o[0] = pix[2]; o[1] = pix[1]; o[2] = pix[0];
    }
}

}  // namespace reporthost
}  // namespace sfmx
