// SPDX-License-Identifier: MIT
// Stand-alone driver of csrc/report_host.hpp for tests/test_report_host_san.py (built with the host sanitizers).
//
//   report_host_main write <in> <dir>
//     in: int64 head[8] = n_err, n_points, has_rgb, n_cameras, n_shots, only_recovered, has_color, n_images
//         | double err[n_err] | double xyz[3 n_points] | uint8 rgb[3 n_points] (has_rgb)
//         | double camera[6 n_cameras] (width, height, fx, fy, cx, cy) | double shot[14 n_shots] (camera, recovered, pose)
//         | uint8 color[3] (has_color)
//         | int64 n_origins | int32 origin_shot[n_origins] | int64 record[n_points] | int32 px[n_points] | int32 py[n_points]
//         | per image: int64 width, height, pitch | uint8 data[height * pitch]
//     writes stats.csv, hist.csv, cloud.ply, cameras.ply (or cameras.rc holding the error code) and, with
//     n_images > 0, colors.bin (the host gather with the default colour 9, 8, 7) into dir
#include <cstdio>
#include <fstream>
#include <string>
#include <vector>

#include "../../sfm-mvs-pipeline_amd/csrc/report_host.hpp"

using namespace sfmx;

template <class T> static bool get(std::ifstream& f, std::vector<T>& v, size_t n) {
    v.resize(n);
    return n == 0 || (bool)f.read(reinterpret_cast<char*>(v.data()), (std::streamsize)(sizeof(T) * n));
}

static int do_write(const char* in, const std::string& dir) {
    std::ifstream f(in, std::ios::binary);
    std::vector<int64_t> head;
    if (!f || !get(f, head, 8)) return 1;
    const size_t n_err = (size_t)head[0], n = (size_t)head[1], n_cam = (size_t)head[3], n_shot = (size_t)head[4], n_img = (size_t)head[7];
    std::vector<double> err, xyz, cam, shot;
    std::vector<uint8_t> rgb, color;
    if (!get(f, err, n_err) || !get(f, xyz, 3 * n) || !get(f, rgb, head[2] ? 3 * n : 0) || !get(f, cam, 6 * n_cam) ||
        !get(f, shot, 14 * n_shot) || !get(f, color, head[6] ? 3 : 0))
        return 2;
    std::string e;
    const cloudhost::Stats s = cloudhost::statistics(err.data(), (int64_t)err.size(), (int64_t)err.size());
    if (cloudhost::write_file((dir + "/stats.csv").c_str(), reporthost::stats_csv(s), e) != cloudhost::OK) return 3;
    std::vector<double> key;
    std::vector<uint64_t> count;
    cloudhost::histogram(err.data(), (int64_t)err.size(), -1.0, key, count);
    if (cloudhost::write_file((dir + "/hist.csv").c_str(), reporthost::hist_csv(key.data(), count.data(), (int64_t)key.size()), e) != cloudhost::OK)
        return 4;
    if (cloudhost::write_file((dir + "/cloud.ply").c_str(), reporthost::pointcloud_ply(xyz.data(), (int64_t)n, head[2] ? rgb.data() : nullptr), e) !=
        cloudhost::OK)
        return 5;
    std::vector<reporthost::Camera> cams(n_cam);
    for (size_t i = 0; i < n_cam; ++i)
        cams[i] = reporthost::Camera{(int32_t)cam[6 * i], (int32_t)cam[6 * i + 1], cam[6 * i + 2], cam[6 * i + 3], cam[6 * i + 4], cam[6 * i + 5]};
    std::vector<reporthost::Shot> shots(n_shot);
    for (size_t i = 0; i < n_shot; ++i) {
        shots[i].camera = (int32_t)shot[14 * i];
        shots[i].recovered = (int32_t)shot[14 * i + 1];
        for (int k = 0; k < 12; ++k) shots[i].pose[k] = shot[14 * i + 2 + k];
    }
    std::string bytes;
    const int rc = reporthost::cameras_ply(cams.data(), (int32_t)n_cam, shots.data(), (int32_t)n_shot, head[6] ? color.data() : nullptr,
                                           head[5] != 0, bytes, e);
    if (rc == cloudhost::OK) {
        if (cloudhost::write_file((dir + "/cameras.ply").c_str(), bytes, e) != cloudhost::OK) return 6;
    } else {
        if (e.empty() || cloudhost::write_file((dir + "/cameras.rc").c_str(), std::to_string(rc), e) != cloudhost::OK) return 7;
    }
    if (n_img) {
        std::vector<int64_t> m, record;
        std::vector<int32_t> oshot, px, py;
        if (!get(f, m, 1) || !get(f, oshot, (size_t)m[0]) || !get(f, record, n) || !get(f, px, n) || !get(f, py, n)) return 8;
        std::vector<std::vector<uint8_t>> data(n_img);
        std::vector<reporthost::Image> images(n_img);
        for (size_t i = 0; i < n_img; ++i) {
            std::vector<int64_t> whp;
            if (!get(f, whp, 3) || !get(f, data[i], (size_t)(whp[1] * whp[2]))) return 9;
            images[i] = reporthost::Image{data[i].data(), (int32_t)whp[0], (int32_t)whp[1], whp[2]};
        }
        const uint8_t def[3] = {9, 8, 7};
        std::vector<uint8_t> out(3 * n);
        reporthost::gather_colors((int64_t)n, record.data(), px.data(), py.data(), oshot.data(), images.data(), def, out.data());
        if (cloudhost::write_file((dir + "/colors.bin").c_str(), std::string(out.begin(), out.end()), e) != cloudhost::OK) return 10;
    }
    return 0;
}

int main(int argc, char** argv) {
    if (argc == 4 && std::string(argv[1]) == "write") return do_write(argv[2], argv[3]);
    std::fprintf(stderr, "usage: report_host_main write <in> <dir>\n");
    return 64;
}
