// The host-side call frame of the geometry rows (homography, triangulate, pose, pnp, cloud, report, scene, merge):
// a per-device slot kept between calls, the layout of its device block, the staging of host arguments, one error
// macro, one tail.  A row writes its validation, its host tables and its launches; everything around them is here.
// A block whose size is known only in mid-call (merge's link list) is a second slot array and a second DeviceCall
// on the same device and stream, always opened after the first.
//
//     DeviceCall F(stream, host_inputs);
//     if (<the call needs a device>) { const int orc = F.open(g_slot, device); if (orc != SFMX_OK) return orc; }
//     int rc = SFMX_OK;
//     {
//         BlockLayout L;
//         L.want(tab, n_tab);                        // tables first: staged in pinned memory, one upload
//         const size_t b_tab = L.need;
//         L.want(scratch, n);
//         L.want(xd, n, F.host);                     // staging copies: only with host arguments
//         if ((rc = F.reserve(L, b_tab)) != SFMX_OK) goto done;
//         ... fill F.pinned(tab) ...
//         SFMX_HIP_CHK(F.upload(b_tab));
//         x = F.in(x, xd, n);
//         SFMX_HIP_CHK(F.err);
//         double* dy = F.out(y, yd);
//         kernel<<<..., F.st>>>(tab, x, dy);
//         SFMX_HIP_CHK(F.back(y, yd, n));
//     done:;
//         rc = F.finish(rc, "sfmx_row");
//     }
//     return rc;
#pragma once
#include <algorithm>
#include <cstddef>
#include <vector>

namespace sfmx {

inline size_t r256(size_t b) { return (std::max<size_t>(b, 1) + 255) & ~(size_t)255; }

// The parts of one block, in request order, each rounded up to 256 bytes (an empty part still takes 256).  A part
// that is not needed takes no bytes and its pointer stays null.  Plain C++: tests/cpp/device_call_main.cpp.
struct BlockLayout {
    struct Part { void** where; size_t bytes; };
    std::vector<Part> parts;
    size_t need = 0;   // bytes of the parts requested so far
    template <class T> void want(T*& p, size_t count, bool needed = true) {   // p is set by commit()
        p = nullptr;
        const size_t bytes = needed ? r256(sizeof(T) * count) : 0;
        parts.push_back({reinterpret_cast<void**>(&p), bytes});
        need += bytes;
    }
    void commit(char* base) const {
        for (const Part& r : parts) {
            if (r.bytes) *r.where = base;
            base += r.bytes;
        }
    }
};

}  // namespace sfmx

#ifdef __HIPCC__
#include <cstring>
#include <mutex>
#include <string>

#include "../../include/sfmx.h"
#include "match_common.hpp"

namespace sfmx {

// Per device, kept between calls: the device check's result, one device block for the call's tables, scratch and
// staging copies (regrown with headroom), pinned staging for the small uploads and the result words, two timing
// events.  Every row has its own Slot g_slot[64]: rows run concurrently, calls of one row on one device do not.
struct Slot {
    bool checked = false;
    char* dev = nullptr;
    size_t dev_cap = 0;
    char* pin = nullptr;
    size_t pin_cap = 0;
    hipEvent_t e0 = nullptr, e1 = nullptr;
    std::mutex mu;   // one call per device at a time; calls on different devices run concurrently
};

#define SFMX_HIP_CHK(expr) do { if ((expr) != hipSuccess) { rc = SFMX_EDEVICE; goto done; } } while (0)

struct DeviceCall {
    const hipStream_t st;
    const bool host;              // the caller's arrays are host memory: inputs go up, outputs come back
    Slot* S = nullptr;            // null until open(): a call that needs no device touches none
    hipError_t err = hipSuccess;  // the first failed upload of in()
    int prev = -1;
    std::unique_lock<std::mutex> lock;

    DeviceCall(void* stream, bool host_args) : st((hipStream_t)stream), host(host_args) {}
    DeviceCall(const DeviceCall&) = delete;
    ~DeviceCall() { if (prev >= 0) (void)hipSetDevice(prev); }   // before the lock goes

    // the locked slot of `device`, checked for gfx950, the device selected; SFMX_OK or the error code
    int open(Slot* slots, int device) {
        int ndev = 0;
        if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0) { set_last_error("no HIP device visible"); return SFMX_EDEVICE; }
        if (device < 0 || device >= ndev || device >= 64) { set_last_error("device index out of range"); return SFMX_EINVAL; }
        lock = std::unique_lock<std::mutex>(slots[device].mu);
        if (!slots[device].checked) {
            hipDeviceProp_t prop;
            if (hipGetDeviceProperties(&prop, device) != hipSuccess || std::strncmp(prop.gcnArchName, "gfx950", 6) != 0) {
                set_last_error("sfmx kernels are built for gfx950 only");
                return SFMX_EDEVICE;
            }
            slots[device].checked = true;
        }
        S = &slots[device];
        (void)hipGetDevice(&prev);
        (void)hipSetDevice(device);
        return SFMX_OK;
    }

    // the device block for L (its pointers are set), `need_pin` pinned bytes and the two events
    int reserve(const BlockLayout& L, size_t need_pin) {
        if (S->dev_cap < L.need) {
            if (S->dev) (void)hipFree(S->dev);
            S->dev = nullptr;
            S->dev_cap = 0;
            if (hipMalloc(reinterpret_cast<void**>(&S->dev), L.need + L.need / 4) != hipSuccess) {
                S->dev = nullptr;
                (void)hipGetLastError();
                return SFMX_ENOMEM;
            }
            S->dev_cap = L.need + L.need / 4;
        }
        if (S->pin_cap < need_pin) {
            if (S->pin) (void)hipHostFree(S->pin);
            S->pin = nullptr;
            S->pin_cap = 0;
            if (hipHostMalloc(reinterpret_cast<void**>(&S->pin), need_pin + need_pin / 4, hipHostMallocDefault) != hipSuccess) {
                S->pin = nullptr;
                return SFMX_ENOMEM;
            }
            S->pin_cap = need_pin + need_pin / 4;
        }
        if (!S->e0) {   // both events or neither
            if (hipEventCreate(&S->e0) != hipSuccess) { S->e0 = nullptr; return SFMX_EDEVICE; }
            if (hipEventCreate(&S->e1) != hipSuccess) {
                (void)hipEventDestroy(S->e0);
                S->e0 = S->e1 = nullptr;
                return SFMX_EDEVICE;
            }
        }
        L.commit(S->dev);
        return SFMX_OK;
    }

    // the pinned twin of a part among the first `need_pin` bytes of the block
    template <class T> T* pinned(T* part) const { return reinterpret_cast<T*>(S->pin + (reinterpret_cast<char*>(part) - S->dev)); }
    // the block's first `bytes` (the tables, filled through pinned()) go up at once
    hipError_t upload(size_t bytes) const { return hipMemcpyAsync(S->dev, S->pin, bytes, hipMemcpyHostToDevice, st); }

    // what the kernels read for a caller's input: the caller's array, or `part` with the host array on its way up
    template <class T> const T* in(const T* arg, T* part, size_t count) {
        if (!host) return arg;
        if (err == hipSuccess) err = hipMemcpyAsync(part, arg, sizeof(T) * count, hipMemcpyHostToDevice, st);
        return part;
    }
    // what the kernels write for a caller's output, and the copy back to a host array once the count is known
    template <class T> T* out(T* arg, T* part) const { return host ? part : arg; }
    template <class T> hipError_t back(T* arg, const T* part, size_t count) const {
        return host ? hipMemcpyAsync(arg, part, sizeof(T) * count, hipMemcpyDeviceToHost, st) : hipSuccess;
    }

    // at `done:`, while the host arrays of the call's copies are alive: nothing stays in flight after an error
    int finish(int rc, const char* function) const {
        if (rc != SFMX_OK && S) (void)hipStreamSynchronize(st);
        if (rc == SFMX_EDEVICE) set_last_error((std::string("HIP error in ") + function).c_str());
        if (rc == SFMX_ENOMEM) set_last_error("device allocation failed");
        return rc;
    }
};

}  // namespace sfmx
#endif  // __HIPCC__
