// SPDX-License-Identifier: MIT
// sfmx scene outputs for gfx950 (include/sfmx_report.h): the reprojection error of every origin
// record (SceneUtils.cpp:43-62) and the colour of every point (Scene::colorizePointcloud, Scene.cpp:569-617),
// and the C ABI of the four writers of csrc/report_host.hpp.
//
// Two kernels, one launch each:
//   reproject_kernel   one thread per origin record.  The record's point is found by a binary search over
//                      origin_offsets (a few records per point: the offsets stay in L2); the loads of
//                      origin_shot / origin_xy and the store are coalesced.  The projection is the text
//                      triangulate.hip compiles (project_device.hpp); the difference and the norm are fp64.
//   colorize_kernel    one thread per point: the record with the lowest shot index, the first such in CSR
//                      order; its position rounded half to even; with device images the pixel gather.
// The per-shot table (pose, then the camera's nine parameters) is built on the host and read from global
// memory: every lane reads a row of 168 bytes that the caches hold.  The file is compiled with
// -ffp-contract=off and calls no libm function but sqrt.
#include <hip/hip_runtime.h>
#include <climits>
#include <cstdint>
#include <cstring>
#include <new>
#include <string>
#include <vector>

#include "../../include/sfmx_report.h"
#include "device_call.hpp"
#include "match_common.hpp"
#include "project_device.hpp"
#include "report_host.hpp"

namespace sfmx {
namespace report {

struct ShotR {            // one shot: its pose, then its camera
    double P[12];         // 3x4 [R|t] row-major
    double fx, fy, cx, cy, k1, k2, p1, p2, k3;
};

struct ImageD { const uint8_t* data; int32_t width, height; int64_t pitch; };

constexpr int BLOCK = 256;

// largest p in [0, n_points - 1] with off[p] <= g: the point whose list holds record g (empty rows are passed over)
__device__ __forceinline__ int64_t search_point(int64_t g, const int64_t* __restrict__ off, int64_t n_points) {
    int64_t lo = 0, hi = n_points - 1;
    while (lo < hi) {
        const int64_t mid = (lo + hi + 1) >> 1;
        if (off[mid] <= g) lo = mid; else hi = mid - 1;
    }
    return lo;
}

__global__ __launch_bounds__(BLOCK)
void reproject_kernel(const ShotR* __restrict__ shots, int n_shots, const double* __restrict__ xyz,
                      const int64_t* __restrict__ off, int64_t n_points, const int32_t* __restrict__ oshot,
                      const double2* __restrict__ oxy, int64_t n, double* __restrict__ out_err, int64_t* __restrict__ res) {
    const int64_t g = (int64_t)blockIdx.x * BLOCK + threadIdx.x;
    if (g >= n) return;
    const int64_t p = search_point(g, off, n_points);   // in [0, n_points) whatever the offsets hold
    const int32_t s = oshot[g];
    if (!(off[p] <= g && g < off[p + 1]) || s < 0 || s >= n_shots) {   // offsets that do not cover g, a shot out of range
        res[0] = 1;
        return;
    }
    const float X = (float)xyz[3 * p], Y = (float)xyz[3 * p + 1], Z = (float)xyz[3 * p + 2];   // cv::Point3f(getCoordinates())
    const double2 q = oxy[g];
    float u, v;
    project_point(shots + s, X, Y, Z, u, v);
    const double du = q.x - (double)u, dv = q.y - (double)v;   // point2d - cv::Point2d(point2dReprojected)
    out_err[g] = canon(sqrt(du * du + dv * dv));
}

// images null: the pixels are gathered on the host from (out_record, out_px, out_py).
__global__ __launch_bounds__(BLOCK)
void colorize_kernel(const int64_t* __restrict__ off, const int32_t* __restrict__ oshot, const double2* __restrict__ oxy,
                     int64_t n_points, int64_t n_origins, int n_shots, const ImageD* __restrict__ images, int def_r,
                     int def_g, int def_b, uint8_t* __restrict__ out_rgb, int64_t* __restrict__ out_record,
                     int32_t* __restrict__ out_px, int32_t* __restrict__ out_py, int64_t* __restrict__ res) {
    const int64_t p = (int64_t)blockIdx.x * BLOCK + threadIdx.x;
    if (p >= n_points) return;
    int64_t b = off[p], e = off[p + 1];
    if (b < 0 || e < b || e > n_origins) {   // a row outside the record arrays
        res[0] = 1;
        b = e = 0;
    }
    int64_t rec = -1;
    int best = INT_MAX;
    for (int64_t i = b; i < e; ++i) {
        const int32_t s = oshot[i];
        if (s < 0 || s >= n_shots) { res[0] = 1; continue; }
        if (s < best) { best = s; rec = i; }
    }
    int32_t px = -1, py = -1;   // a position that is not finite counts as outside every image
    if (rec >= 0) {
        const double2 q = oxy[rec];
        const double big = 1.7976931348623157e308;
        if (fabs(q.x) <= big && fabs(q.y) <= big) {   // finite
            px = __double2int_rn(q.x);   // cvRound: round half to even
            py = __double2int_rn(q.y);
        }
    }
    if (out_record) out_record[p] = rec;
    if (images) {
        int r = def_r, g = def_g, bl = def_b;
        if (rec >= 0) {
            const ImageD im = images[best];
            if (px >= 0 && px < im.width && py >= 0 && py < im.height) {
                const uint8_t* pix = im.data + (int64_t)py * im.pitch + 3 * (int64_t)px;
                r = pix[2]; g = pix[1]; bl = pix[0];
            }
        }
        out_rgb[3 * p] = (uint8_t)r;
        out_rgb[3 * p + 1] = (uint8_t)g;
        out_rgb[3 * p + 2] = (uint8_t)bl;
    } else {
        out_px[p] = px;
        out_py[p] = py;
    }
}

thread_local float g_reproject_ms = -1.f;
thread_local float g_colorize_ms = -1.f;

Slot g_slot[64];   // csrc/device_call.hpp; both kernels share it

static int fail(const char* msg) { set_last_error(msg); return SFMX_EINVAL; }
static int fail(int rc, const std::string& msg) { set_last_error(msg.c_str()); return rc; }

// the checks of the origin CSR that need its contents: host memory only
static const char* check_csr(const int64_t* off, int64_t n_points, const int32_t* oshot, int64_t n_origins, int32_t n_shots) {
    if (off[0] != 0) return "origin offsets do not start at 0";
    for (int64_t p = 0; p < n_points; ++p)
        if (off[p + 1] < off[p]) return "origin offsets not ascending";
    if (off[n_points] != n_origins) return "origin offsets do not end at n_origins";
    for (int64_t i = 0; i < n_origins; ++i)
        if (oshot[i] < 0 || oshot[i] >= n_shots) return "origin shot index out of range";
    return nullptr;
}

}  // namespace report
}  // namespace sfmx

using namespace sfmx;
using namespace sfmx::report;

extern "C" {

float sfmx_reprojection_last_kernel_ms(void) { return g_reproject_ms; }
float sfmx_colorize_last_kernel_ms(void) { return g_colorize_ms; }

int sfmx_reprojection_errors(const double* xyz, int64_t n_points, const int64_t* origin_offsets, const int32_t* origin_shot,
                             const double* origin_xy, int64_t n_origins, const sfmx_tri_camera* cameras, int32_t n_cameras,
                             const int32_t* shot_camera, const double* shot_pose, int32_t n_shots, int32_t inputs_on_device,
                             int32_t device, void* stream, double* out_err) {
    if (n_points < 0 || n_origins < 0 || n_cameras < 0 || n_shots < 0) return fail("negative count");
    if (!origin_offsets || (n_cameras && !cameras) || (n_shots && (!shot_camera || !shot_pose)) || (n_points && !xyz) ||
        (n_origins && (!origin_shot || !origin_xy || !out_err)))
        return fail("null argument");
    for (int c = 0; c < n_cameras; ++c)
        if (cameras[c].K[0] == 0.0 || cameras[c].K[4] == 0.0) return fail("camera with zero focal length");
    for (int s = 0; s < n_shots; ++s)
        if (shot_camera[s] < 0 || shot_camera[s] >= n_cameras) return fail("shot camera index out of range");
    if (n_origins && !n_points) return fail("origin records without a point");
    if (!inputs_on_device) {
        const char* bad = check_csr(origin_offsets, n_points, origin_shot, n_origins, n_shots);
        if (bad) return fail(bad);
    }
    if (n_origins == 0) {   // no record: nothing is launched
        g_reproject_ms = 0.f;
        return SFMX_OK;
    }
    const int64_t n = n_origins, n_blocks = (n + BLOCK - 1) / BLOCK;
    if (n_blocks > INT32_MAX) return fail("too many origin records");
    DeviceCall F(stream, !inputs_on_device);
    const hipStream_t st = F.st;
    {
        const int orc = F.open(g_slot, device);
        if (orc != SFMX_OK) return orc;
    }
    Slot* const S = F.S;
    int rc = SFMX_OK;
    {
        // device block: [shot table | result word | (host inputs: xyz, offsets, shots, positions, errors)]
        const bool H = F.host;
        BlockLayout L;
        ShotR* shd;
        int64_t *resd, *od;
        double *xd, *qd, *ed;
        int32_t* sd;
        L.want(shd, n_shots);
        L.want(resd, 1);
        const size_t b_tab = L.need;   // up to here: staged in pinned memory, one upload
        L.want(xd, 3 * (size_t)n_points, H);
        L.want(od, (size_t)n_points + 1, H);
        L.want(sd, n, H);
        L.want(qd, 2 * (size_t)n, H);
        L.want(ed, n, H);
        if ((rc = F.reserve(L, b_tab)) != SFMX_OK) goto done;
        ShotR* hs = F.pinned(shd);
        for (int i = 0; i < n_shots; ++i) {
            const sfmx_tri_camera& c = cameras[shot_camera[i]];
            ShotR& t = hs[i];
            std::memcpy(t.P, shot_pose + 12 * (size_t)i, sizeof(double) * 12);
            t.fx = c.K[0]; t.fy = c.K[4]; t.cx = c.K[2]; t.cy = c.K[5];
            t.k1 = c.dist[0]; t.k2 = c.dist[1]; t.p1 = c.dist[2]; t.p2 = c.dist[3]; t.k3 = c.dist[4];
        }
        int64_t* hres = F.pinned(resd);
        hres[0] = 0;
        SFMX_HIP_CHK(F.upload(b_tab));   // table, result word = 0
        const double* dx = F.in(xyz, xd, 3 * (size_t)n_points);
        const int64_t* doff = F.in(origin_offsets, od, (size_t)n_points + 1);
        const int32_t* dsh = F.in(origin_shot, sd, n);
        const double* dq = F.in(origin_xy, qd, 2 * (size_t)n);
        SFMX_HIP_CHK(F.err);
        double* de = F.out(out_err, ed);
        (void)hipEventRecord(S->e0, st);
        reproject_kernel<<<(unsigned)n_blocks, BLOCK, 0, st>>>(shd, n_shots, dx, doff, n_points, dsh,
                                                               reinterpret_cast<const double2*>(dq), n, de, resd);
        (void)hipEventRecord(S->e1, st);
        SFMX_HIP_CHK(hipGetLastError());
        SFMX_HIP_CHK(hipMemcpyAsync(hres, resd, sizeof(int64_t), hipMemcpyDeviceToHost, st));
        SFMX_HIP_CHK(F.back(out_err, ed, n));
        SFMX_HIP_CHK(hipStreamSynchronize(st));
        if (hres[0] != 0) { set_last_error("origin offsets or origin shot index out of range"); rc = SFMX_EINVAL; goto done; }
        float ms = -1.f;
        (void)hipEventElapsedTime(&ms, S->e0, S->e1);
        g_reproject_ms = ms;
    }
done:;
    return F.finish(rc, "sfmx_reprojection_errors");
}

int sfmx_colorize_pointcloud(int64_t n_points, const int64_t* origin_offsets, const int32_t* origin_shot, const double* origin_xy,
                             int64_t n_origins, const uint8_t* const* images, const int32_t* image_width,
                             const int32_t* image_height, const int64_t* image_pitch, int32_t n_shots, const uint8_t* default_rgb,
                             int32_t inputs_on_device, int32_t device, void* stream, uint8_t* out_rgb, int64_t* out_record) {
    if (n_points < 0 || n_origins < 0 || n_shots < 0) return fail("negative count");
    if (!origin_offsets || (n_shots && (!images || !image_width || !image_height || !image_pitch)) || (n_points && !out_rgb) ||
        (n_origins && (!origin_shot || !origin_xy)))
        return fail("null argument");
    for (int s = 0; s < n_shots; ++s) {
        if (image_width[s] < 0 || image_height[s] < 0) return fail("image with a negative size");
        if (image_pitch[s] < 3 * (int64_t)image_width[s]) return fail("image pitch below 3 * width");
        if (!images[s] && image_width[s] && image_height[s]) return fail("null image");
    }
    if (n_origins && !n_points) return fail("origin records without a point");
    if (!inputs_on_device) {
        const char* bad = check_csr(origin_offsets, n_points, origin_shot, n_origins, n_shots);
        if (bad) return fail(bad);
    }
    if (n_points == 0) {   // no point: nothing is launched
        g_colorize_ms = 0.f;
        return SFMX_OK;
    }
    const int64_t n_blocks = (n_points + BLOCK - 1) / BLOCK;
    if (n_blocks > INT32_MAX) return fail("too many points");
    const uint8_t zero[3] = {0, 0, 0};
    const uint8_t* def = default_rgb ? default_rgb : zero;
    std::vector<int64_t> rec;      // the host gather's inputs: alive until F.finish has drained the stream
    std::vector<int32_t> px, py;
    DeviceCall F(stream, !inputs_on_device);
    const hipStream_t st = F.st;
    {
        const int orc = F.open(g_slot, device);
        if (orc != SFMX_OK) return orc;
    }
    Slot* const S = F.S;
    int rc = SFMX_OK;
    {
        // device block: [image table | result word | (host inputs: offsets, shots, positions, record, px, py)]
        const bool H = F.host;
        BlockLayout L;
        ImageD* imd;
        int64_t *resd, *od, *rd;
        double* qd;
        int32_t *sd, *pxd, *pyd;
        L.want(imd, n_shots, !H);
        L.want(resd, 1);
        const size_t b_tab = L.need;   // up to here: staged in pinned memory, one upload
        L.want(od, (size_t)n_points + 1, H);
        L.want(sd, n_origins, H);
        L.want(qd, 2 * (size_t)n_origins, H);
        L.want(rd, n_points, H);
        L.want(pxd, n_points, H);
        L.want(pyd, n_points, H);
        if ((rc = F.reserve(L, b_tab)) != SFMX_OK) goto done;
        if (!H) {
            ImageD* hi = F.pinned(imd);
            for (int s = 0; s < n_shots; ++s) hi[s] = ImageD{images[s], image_width[s], image_height[s], image_pitch[s]};
        }
        int64_t* hres = F.pinned(resd);
        hres[0] = 0;
        SFMX_HIP_CHK(F.upload(b_tab));   // table, result word = 0
        const int64_t* doff = F.in(origin_offsets, od, (size_t)n_points + 1);
        const int32_t* dsh = n_origins ? F.in(origin_shot, sd, n_origins) : nullptr;
        const double* dq = n_origins ? F.in(origin_xy, qd, 2 * (size_t)n_origins) : nullptr;
        SFMX_HIP_CHK(F.err);
        int64_t* drec = H ? rd : out_record;
        (void)hipEventRecord(S->e0, st);
        colorize_kernel<<<(unsigned)n_blocks, BLOCK, 0, st>>>(doff, dsh, reinterpret_cast<const double2*>(dq), n_points, n_origins,
                                                              n_shots, H ? nullptr : imd, def[0], def[1], def[2],
                                                              H ? nullptr : out_rgb, drec, pxd, pyd, resd);
        (void)hipEventRecord(S->e1, st);
        SFMX_HIP_CHK(hipGetLastError());
        SFMX_HIP_CHK(hipMemcpyAsync(hres, resd, sizeof(int64_t), hipMemcpyDeviceToHost, st));
        if (H) {
            rec.resize(n_points);
            px.resize(n_points);
            py.resize(n_points);
            SFMX_HIP_CHK(hipMemcpyAsync(rec.data(), rd, sizeof(int64_t) * n_points, hipMemcpyDeviceToHost, st));
            SFMX_HIP_CHK(hipMemcpyAsync(px.data(), pxd, sizeof(int32_t) * n_points, hipMemcpyDeviceToHost, st));
            SFMX_HIP_CHK(hipMemcpyAsync(py.data(), pyd, sizeof(int32_t) * n_points, hipMemcpyDeviceToHost, st));
            SFMX_HIP_CHK(hipStreamSynchronize(st));
            if (hres[0] == 0) {
                std::vector<reporthost::Image> im(n_shots);
                for (int s = 0; s < n_shots; ++s) im[s] = reporthost::Image{images[s], image_width[s], image_height[s], image_pitch[s]};
                reporthost::gather_colors(n_points, rec.data(), px.data(), py.data(), origin_shot, im.data(), def, out_rgb);
                if (out_record) std::memcpy(out_record, rec.data(), sizeof(int64_t) * n_points);
            }
        } else {
            SFMX_HIP_CHK(hipStreamSynchronize(st));
        }
        if (hres[0] != 0) { set_last_error("origin offsets or origin shot index out of range"); rc = SFMX_EINVAL; goto done; }
        float ms = -1.f;
        (void)hipEventElapsedTime(&ms, S->e0, S->e1);
        g_colorize_ms = ms;
    }
done:;
    return F.finish(rc, "sfmx_colorize_pointcloud");
}

// ---- host-only entry points: the writers of csrc/report_host.hpp ---------------------------------------

int sfmx_reprojection_write_stats_csv(const char* path, const sfmx_cloud_stats* s) {
    if (!path || !s) return fail("null argument");
    std::string err;
    const cloudhost::Stats hs{s->n_points, s->max, s->min, s->mean, s->median, s->variance, s->deviation};
    const int rc = cloudhost::write_file(path, reporthost::stats_csv(hs), err);
    return rc == cloudhost::OK ? SFMX_OK : fail(rc, err);
}

int sfmx_reprojection_write_hist_csv(const char* path, const double* key, const uint64_t* count, int64_t n) {
    if (!path || n < 0 || (n && (!key || !count))) return fail("null argument or negative count");
    std::string err;
    const int rc = cloudhost::write_file(path, reporthost::hist_csv(key, count, n), err);
    return rc == cloudhost::OK ? SFMX_OK : fail(rc, err);
}

int sfmx_write_pointcloud_ply(const char* path, const double* xyz, int64_t n_points, const uint8_t* rgb) {
    if (!path || n_points < 0 || (n_points && !xyz)) return fail("null argument or negative count");
    try {
        std::string err;
        const int rc = cloudhost::write_file(path, reporthost::pointcloud_ply(xyz, n_points, rgb), err);
        return rc == cloudhost::OK ? SFMX_OK : fail(rc, err);
    } catch (const std::bad_alloc&) {
        return fail(SFMX_ENOMEM, "out of host memory");
    }
}

int sfmx_write_cameras_ply(const char* path, const sfmx_mvs_camera* cameras, int32_t n_cameras, const sfmx_mvs_shot* shots,
                           int32_t n_shots, const uint8_t* color, int32_t only_recovered) {
    if (!path || n_cameras < 0 || n_shots < 0 || (n_cameras && !cameras) || (n_shots && !shots))
        return fail("null argument or negative count");
    try {
        std::vector<reporthost::Camera> cams(n_cameras);
        for (int c = 0; c < n_cameras; ++c)
            cams[c] = reporthost::Camera{cameras[c].width, cameras[c].height, cameras[c].K[0], cameras[c].K[4], cameras[c].K[2],
                                         cameras[c].K[5]};
        std::vector<reporthost::Shot> sh(n_shots);
        for (int i = 0; i < n_shots; ++i) {
            sh[i].camera = shots[i].camera;
            sh[i].recovered = shots[i].recovered;
            std::memcpy(sh[i].pose, shots[i].pose, sizeof(double) * 12);
        }
        std::string bytes, err;
        int rc = reporthost::cameras_ply(cams.data(), n_cameras, sh.data(), n_shots, color, only_recovered != 0, bytes, err);
        if (rc == cloudhost::OK) rc = cloudhost::write_file(path, bytes, err);
        return rc == cloudhost::OK ? SFMX_OK : fail(rc, err);
    } catch (const std::bad_alloc&) {
        return fail(SFMX_ENOMEM, "out of host memory");
    }
}

}  // extern "C"
