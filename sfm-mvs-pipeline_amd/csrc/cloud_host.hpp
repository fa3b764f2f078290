// SPDX-License-Identifier: MIT
// sfmx — host side of the point-cloud neighbour statistics (include/sfmx_cloud.h): the statistics of
// MathUtils::calculateStatistics, the neighbour histogram, a PLY reader and the three writers of
// PclUtils::writeTo*.  Header only, no HIP: csrc/cloud.hip wraps it into the C ABI and
// tests/cpp/cloud_host_main.cpp builds it stand-alone under the host sanitizers.
//
// Every function returns 0 or a negative code (the values of sfmx.h) and leaves a text in `err`.
// Build the including file with -ffp-contract=off: the sums below are sequential double sums.
#pragma once
#include <algorithm>
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

namespace sfmx {
namespace cloudhost {

constexpr int OK = 0, E_INVAL = -1;   // SFMX_OK, SFMX_EINVAL of sfmx.h

struct Stats { int64_t n_points; double max, min, mean, median, variance, deviation; };

// MathUtils.h:53-90, bug for bug: min and max start at 0, the sums run in sorted order, the variance
// divides by size - 1 (NaN for one element).  pow(x - mean, 2) is the product (x - mean) * (x - mean).
// The part behind the sort, on a list that is already in order (csrc/report_host.hpp sorts its own).
inline Stats statistics_sorted(const std::vector<double>& v, int64_t n_points) {
    Stats s{n_points, 0, 0, 0, 0, 0, 0};
    const int64_t n = (int64_t)v.size();
    if (n <= 0) return s;
    double mn = 0, mx = 0, mean = 0, var = 0;
    for (double x : v) {
        mn = std::min(mn, x);
        mx = std::max(mx, x);
        mean += x;
    }
    mean /= (double)n;
    for (double x : v) {
        const double e = x - mean;
        var += e * e;
    }
    var /= ((double)n - 1.0);
    s.min = mn;
    s.max = mx;
    s.mean = mean;
    s.variance = var;
    s.deviation = std::sqrt(var);
    s.median = (n % 2 == 0) ? (v[n / 2] + v[n / 2 - 1]) / 2.0 : v[n / 2];
    return s;
}

// Ascending, NaNs behind the ordered values.  The reference's std::sort on a list with NaNs is undefined (its
// comparison is no strict weak order); a list without NaNs is sorted exactly as before.  Distances are never
// NaN; reprojection errors can be (include/sfmx_report.h).
inline void sort_nan_last(std::vector<double>& v) {
    const auto nan = std::partition(v.begin(), v.end(), [](double x) { return x == x; });
    std::sort(v.begin(), nan, [](double a, double b) { return a < b; });
}

inline Stats statistics(const double* d, int64_t n, int64_t n_points) {
    if (n <= 0) return Stats{n_points, 0, 0, 0, 0, 0, 0};
    std::vector<double> v(d, d + n);
    sort_nan_last(v);
    return statistics_sorted(v, n_points);
}

// PclUtils.cpp:313-328.  resolution < 0: the variance of the list.  Keys ascend; distinct as doubles.
// NaN keys (a NaN resolution: the variance of a one-element list) form one last row.
inline void histogram(const double* d, int64_t n, double resolution, std::vector<double>& key, std::vector<uint64_t>& count) {
    key.clear();
    count.clear();
    if (resolution < 0) resolution = statistics(d, n, n).variance;
    std::vector<double> k(n > 0 ? n : 0);
    int64_t nan = 0, m = 0;
    for (int64_t i = 0; i < n; ++i) {
        const double id = (resolution <= 0) ? d[i] : std::ceil(d[i] / resolution) * resolution;
        if (id != id) ++nan; else k[m++] = id;
    }
    std::sort(k.begin(), k.begin() + m);
    for (int64_t i = 0; i < m; ++i) {
        if (!key.empty() && key.back() == k[i]) ++count.back();
        else { key.push_back(k[i]); count.push_back(1); }
    }
    if (nan) { key.push_back(std::nan("")); count.push_back((uint64_t)nan); }
}

// ---- writers ----------------------------------------------------------------------------------------

inline int write_file(const char* path, const std::string& bytes, std::string& err) {
    FILE* f = path ? std::fopen(path, "wb") : nullptr;
    if (!f) { err = std::string("cannot open for writing: ") + (path ? path : "(null)"); return E_INVAL; }
    const bool ok = bytes.empty() || std::fwrite(bytes.data(), 1, bytes.size(), f) == bytes.size();
    if (std::fclose(f) != 0 || !ok) { err = std::string("write failed: ") + path; return E_INVAL; }
    return OK;
}

inline void put_f6(std::string& s, double v) {   // ostream << fixed: %.6f
    char b[400];
    std::snprintf(b, sizeof b, "%.6f", v);
    s += b;
}

inline std::string stats_csv(const Stats& s) {   // PclUtils.cpp:388-395
    std::string o = "N_Points,Max_Distance,Min_Distance,Avg_Distance,Median_Distance,Variance_Distance,Deviation_Distance\n";
    o += std::to_string((long long)s.n_points);
    for (double v : {s.max, s.min, s.mean, s.median, s.variance, s.deviation}) { o += ','; put_f6(o, v); }
    o += '\n';
    return o;
}

inline std::string neighbors_csv(const double* key, const uint64_t* count, int64_t n) {   // PclUtils.cpp:330-335
    std::string o = "Distance,Count\n";
    for (int64_t i = 0; i < n; ++i) {
        put_f6(o, key[i]);
        o += ',';
        o += std::to_string((unsigned long long)count[i]);
        o += '\n';
    }
    return o;
}

// double -> u_char as the reference's x86-64 build converts it: truncation to int32 (the "integer
// indefinite" 0x80000000 for a NaN or a value outside int32), then the low 8 bits.
inline uint8_t to_u8(double v) {
    if (!(v > -2147483649.0 && v < 2147483648.0)) return 0;
    return (uint8_t)(uint32_t)(int32_t)v;
}

template <class T> inline void put_raw(std::string& s, T v) { s.append(reinterpret_cast<const char*>(&v), sizeof(T)); }

// PclUtils.cpp:91-265 with binary = true on a little-endian host.  distances: n_distances = n_points of
// the cloud, or 0 (the reference's size > 1 guard); the vertex block has n_distances records.
inline std::string quality_ply(const float* xyz, const double* distances, int64_t n_distances, const int32_t* face_sizes,
                               int64_t n_faces, const int32_t* face_indices, double cutoff) {
    std::vector<double> dist(distances, distances + (n_distances > 0 ? n_distances : 0));
    double maxd = 0;
    for (double& d : dist) {
        if (cutoff > 0 && d > cutoff) d = cutoff;
        if (d > maxd) maxd = d;
    }
    std::string o = "ply\nformat binary_little_endian 1.0\nelement vertex " + std::to_string((long long)dist.size()) +
                    "\nproperty float x\nproperty float y\nproperty float z\nproperty uchar red\nproperty uchar green\n"
                    "property uchar blue\nproperty float quality\nelement face " + std::to_string((long long)n_faces) +
                    "\nproperty list uchar int vertex_indices\nproperty uchar red\nproperty uchar green\n"
                    "property uchar blue\nproperty float quality\nend_header\n";
    const bool flat = !(maxd > 0);   // maxDistance == 0: the ratio is NaN; r = b = 0
    for (size_t i = 0; i < dist.size(); ++i) {
        const double ratio = dist[i] / maxd;
        const uint8_t b = flat ? 0 : to_u8(255 * ratio), r = flat ? 0 : to_u8(255 * (1.0 - ratio));
        put_raw<float>(o, xyz[3 * i]);
        put_raw<float>(o, xyz[3 * i + 1]);
        put_raw<float>(o, xyz[3 * i + 2]);
        put_raw<uint8_t>(o, r);
        put_raw<uint8_t>(o, 0);
        put_raw<uint8_t>(o, b);
        put_raw<float>(o, (float)dist[i]);
    }
    int64_t at = 0;
    for (int64_t f = 0; f < n_faces; ++f) {
        const int64_t cnt = face_sizes[f];
        const int32_t* idx = face_indices + at;
        at += cnt > 0 ? cnt : 0;
        if (cnt > 255 || cnt <= 0) continue;   // oversized: skipped by the reference; empty: it divides by zero
        bool inside = true;
        for (int64_t k = 0; k < cnt; ++k) inside = inside && idx[k] >= 0 && (int64_t)idx[k] < (int64_t)dist.size();
        if (!inside) continue;                 // the reference reads out of bounds
        uint8_t r = 0, b = 0;
        float q = 0;
        for (int64_t k = 0; k < cnt; ++k) {
            const double d = dist[idx[k]];
            q = (float)((double)q + d);
            const double ratio = d / maxd;
            b = flat ? 0 : to_u8((double)b + 255 * ratio);
            r = flat ? 0 : to_u8((double)r + 255 * (1.0 - ratio));
        }
        q = q / (float)cnt;
        r = (uint8_t)(r / (int)cnt);
        b = (uint8_t)(b / (int)cnt);
        put_raw<uint8_t>(o, (uint8_t)cnt);
        for (int64_t k = 0; k < cnt; ++k) put_raw<int32_t>(o, idx[k]);
        put_raw<uint8_t>(o, r);
        put_raw<uint8_t>(o, 0);
        put_raw<uint8_t>(o, b);
        put_raw<float>(o, q);
    }
    return o;
}

// ---- PLY reader -------------------------------------------------------------------------------------

struct Ply {
    std::vector<float> xyz;             // 3 per vertex
    std::vector<int32_t> face_sizes;    // vertices per face
    std::vector<int32_t> face_indices;  // concatenated
    int64_t n_points = 0, n_faces = 0, n_indices = 0;
};

namespace detail {

inline int type_size(const std::string& t) {   // 0: not a PLY scalar type
    if (t == "char" || t == "uchar" || t == "int8" || t == "uint8") return 1;
    if (t == "short" || t == "ushort" || t == "int16" || t == "uint16") return 2;
    if (t == "int" || t == "uint" || t == "int32" || t == "uint32" || t == "float" || t == "float32") return 4;
    if (t == "double" || t == "float64") return 8;
    return 0;
}
inline bool is_float(const std::string& t) { return t == "float" || t == "float32"; }
inline bool is_uchar(const std::string& t) { return t == "uchar" || t == "uint8"; }
inline bool is_int(const std::string& t) { return t == "int" || t == "int32"; }
inline bool is_uint(const std::string& t) { return t == "uint" || t == "uint32"; }

struct Prop { std::string name, type, count_type; bool list = false; int size = 0; };
struct Elem { std::string name; int64_t count = 0; std::vector<Prop> props; };

inline std::vector<std::string> words(const std::string& line) {
    std::vector<std::string> w;
    size_t i = 0;
    while (i < line.size()) {
        while (i < line.size() && (line[i] == ' ' || line[i] == '\t' || line[i] == '\r')) ++i;
        size_t j = i;
        while (j < line.size() && line[j] != ' ' && line[j] != '\t' && line[j] != '\r') ++j;
        if (j > i) w.push_back(line.substr(i, j - i));
        i = j;
    }
    return w;
}

struct Cursor {            // the body; every read is checked against `end`
    const char* p;
    const char* end;
    bool token(const char*& b, const char*& e) {   // ascii: next whitespace-separated token
        while (p < end && (*p == ' ' || *p == '\n' || *p == '\r' || *p == '\t')) ++p;
        if (p >= end) return false;
        b = p;
        while (p < end && !(*p == ' ' || *p == '\n' || *p == '\r' || *p == '\t')) ++p;
        e = p;
        return true;
    }
};

inline bool parse_double(const char* b, const char* e, double& v) {
    char buf[64];
    const size_t n = (size_t)(e - b);
    if (n == 0 || n >= sizeof buf) return false;
    std::memcpy(buf, b, n);
    buf[n] = 0;
    char* stop = nullptr;
    v = std::strtod(buf, &stop);
    return stop == buf + n;
}

inline bool parse_int(const char* b, const char* e, long long& v) {
    char buf[32];
    const size_t n = (size_t)(e - b);
    if (n == 0 || n >= sizeof buf) return false;
    std::memcpy(buf, b, n);
    buf[n] = 0;
    char* stop = nullptr;
    v = std::strtoll(buf, &stop, 10);
    return stop == buf + n;
}

}  // namespace detail

// Reads `bytes` (a whole PLY file).  fill = false: only the three sizes are set.
inline int parse_ply(const char* data, size_t size, bool fill, Ply& out, std::string& err) {
    using namespace detail;
    out = Ply();
    const char* p = data;
    const char* const end = data + size;
    auto next_line = [&](std::string& line) -> bool {
        if (p >= end) return false;
        const char* nl = static_cast<const char*>(std::memchr(p, '\n', (size_t)(end - p)));
        if (!nl) return false;               // a header line always ends in a newline
        line.assign(p, nl);
        p = nl + 1;
        return true;
    };
    auto fail = [&](const std::string& m) { err = "PLY: " + m; return E_INVAL; };
    std::string line;
    if (!next_line(line) || words(line) != std::vector<std::string>{"ply"}) return fail("missing 'ply' magic");
    int format = -1;                         // 0 ascii, 1 binary_little_endian
    std::vector<Elem> elems;
    bool ended = false;
    while (next_line(line)) {
        const std::vector<std::string> w = words(line);
        if (w.empty() || w[0] == "comment" || w[0] == "obj_info") continue;
        if (w[0] == "end_header") { ended = true; break; }
        if (w[0] == "format") {
            if (w.size() < 2) return fail("bad format line");
            if (w[1] == "ascii") format = 0;
            else if (w[1] == "binary_little_endian") format = 1;
            else return fail("format '" + w[1] + "' is not supported (ascii, binary_little_endian)");
        } else if (w[0] == "element") {
            long long c = 0;
            if (w.size() != 3 || !parse_int(w[2].data(), w[2].data() + w[2].size(), c) || c < 0) return fail("bad element line");
            if (elems.size() >= 64) return fail("too many elements");
            Elem e;
            e.name = w[1];
            e.count = c;
            elems.push_back(e);
        } else if (w[0] == "property") {
            if (elems.empty()) return fail("property before any element");
            if (elems.back().props.size() >= 1024) return fail("too many properties");
            Prop pr;
            if (w.size() == 3) {
                pr.type = w[1];
                pr.name = w[2];
                pr.size = type_size(pr.type);
                if (!pr.size) return fail("unknown property type '" + pr.type + "'");
            } else if (w.size() == 5 && w[1] == "list") {
                pr.list = true;
                pr.count_type = w[2];
                pr.type = w[3];
                pr.name = w[4];
                if (!type_size(pr.count_type) || !type_size(pr.type)) return fail("unknown list type");
            } else {
                return fail("bad property line");
            }
            elems.back().props.push_back(pr);
        } else {
            return fail("unknown header line '" + w[0] + "'");
        }
    }
    if (!ended) return fail("header without end_header");
    if (format < 0) return fail("header without a format line");
    // what each element must look like
    int n_vertex = 0, n_face = 0;
    for (const Elem& e : elems) {
        int lists = 0;
        for (const Prop& pr : e.props) lists += pr.list;
        if (e.name == "vertex") {
            if (++n_vertex > 1) return fail("more than one vertex element");
            if (lists) return fail("list property in the vertex element");
            int have = 0;
            for (const Prop& pr : e.props)
                if (pr.name == "x" || pr.name == "y" || pr.name == "z") {
                    if (!is_float(pr.type)) return fail("vertex property " + pr.name + " is not float");
                    have |= pr.name == "x" ? 1 : pr.name == "y" ? 2 : 4;
                }
            if (have != 7) return fail("vertex element without float x, y, z");
            if (e.count > INT32_MAX) return fail("more than 2^31 - 1 vertices");
        } else if (e.name == "face") {
            if (++n_face > 1) return fail("more than one face element");
            if (lists > 1) return fail("second list property in the face element");
            for (const Prop& pr : e.props)
                if (pr.list) {
                    if (pr.name != "vertex_indices" && pr.name != "vertex_index") return fail("face list property '" + pr.name + "'");
                    if (!is_uchar(pr.count_type)) return fail("face list count type is not uchar");
                    if (!is_int(pr.type) && !is_uint(pr.type)) return fail("face list index type is not int or uint");
                }
            if (e.count && !lists) return fail("face element without a list property");
        } else if (lists) {
            return fail("list property in element '" + e.name + "'");
        }
    }
    if (!n_vertex) return fail("no vertex element");
    Cursor c{p, end};
    for (const Elem& e : elems) {
        const size_t np = e.props.size();
        if (e.count && np == 0) return fail("element '" + e.name + "' without properties");
        const bool is_v = e.name == "vertex", is_f = e.name == "face";
        size_t stride = 0;
        for (const Prop& pr : e.props) stride += pr.list ? 0 : (size_t)pr.size;
        const size_t left = (size_t)(c.end - c.p);
        if (!is_f) {       // scalars only: the size of the block is known before it is read
            if (format == 1) {
                if (stride && (uint64_t)e.count > left / stride) return fail("truncated body in element '" + e.name + "'");
            } else if (np && (uint64_t)e.count > left / (2 * np) + 1) {   // a token and its separator take two bytes
                return fail("truncated body in element '" + e.name + "'");
            }
        } else if ((uint64_t)e.count > left) {
            return fail("face count overruns the file");
        }
        if (is_v) {
            out.n_points = e.count;
            if (fill) out.xyz.resize(3 * (size_t)e.count);
            size_t off[3] = {0, 0, 0}, which[3] = {0, 0, 0}, o = 0;
            for (size_t k = 0; k < np; ++k) {
                const Prop& pr = e.props[k];
                const int a = pr.name == "x" ? 0 : pr.name == "y" ? 1 : pr.name == "z" ? 2 : -1;
                if (a >= 0) { off[a] = o; which[a] = k; }
                o += (size_t)pr.size;
            }
            if (format == 1) {
                if (fill)
                    for (int64_t i = 0; i < e.count; ++i)
                        for (int a = 0; a < 3; ++a) std::memcpy(&out.xyz[3 * i + a], c.p + (size_t)i * stride + off[a], 4);
                c.p += (size_t)e.count * stride;
            } else {
                for (int64_t i = 0; i < e.count; ++i)
                    for (size_t k = 0; k < np; ++k) {
                        const char *b, *t;
                        double v;
                        if (!c.token(b, t) || !parse_double(b, t, v)) return fail("truncated or malformed vertex " + std::to_string((long long)i));
                        if (fill)
                            for (int a = 0; a < 3; ++a)
                                if (which[a] == k) out.xyz[3 * i + a] = (float)v;
                    }
            }
        } else if (is_f) {
            out.n_faces = e.count;
            if (fill) out.face_sizes.reserve((size_t)e.count);
            for (int64_t i = 0; i < e.count; ++i)
                for (const Prop& pr : e.props) {
                    if (!pr.list) {
                        if (format == 1) {
                            if ((size_t)(c.end - c.p) < (size_t)pr.size) return fail("truncated face " + std::to_string((long long)i));
                            c.p += pr.size;
                        } else {
                            const char *b, *t;
                            double v;
                            if (!c.token(b, t) || !parse_double(b, t, v)) return fail("truncated or malformed face " + std::to_string((long long)i));
                        }
                        continue;
                    }
                    long long cnt = 0;
                    if (format == 1) {
                        if (c.end - c.p < 1) return fail("truncated face " + std::to_string((long long)i));
                        cnt = (uint8_t)*c.p++;
                        if ((size_t)(c.end - c.p) < (size_t)cnt * 4) return fail("face " + std::to_string((long long)i) + " overruns the file");
                        if (fill) {
                            const size_t at = out.face_indices.size();
                            out.face_indices.resize(at + (size_t)cnt);
                            if (cnt) std::memcpy(&out.face_indices[at], c.p, (size_t)cnt * 4);
                        }
                        c.p += cnt * 4;
                    } else {
                        const char *b, *t;
                        if (!c.token(b, t) || !parse_int(b, t, cnt)) return fail("truncated or malformed face " + std::to_string((long long)i));
                        if (cnt < 0) return fail("negative list count in face " + std::to_string((long long)i));
                        if (cnt > 255) return fail("list count above the uchar range in face " + std::to_string((long long)i));
                        for (long long k = 0; k < cnt; ++k) {
                            long long v = 0;
                            if (!c.token(b, t) || !parse_int(b, t, v)) return fail("face " + std::to_string((long long)i) + " overruns the file");
                            if (v < INT32_MIN || v > (long long)UINT32_MAX) return fail("face index outside 32 bits");
                            if (fill) out.face_indices.push_back((int32_t)(uint32_t)(v & 0xffffffffll));
                        }
                    }
                    if (fill) out.face_sizes.push_back((int32_t)cnt);
                    out.n_indices += cnt;
                }
        } else if (format == 1) {
            c.p += (size_t)e.count * stride;
        } else {
            for (int64_t i = 0; i < e.count; ++i)
                for (size_t k = 0; k < np; ++k) {
                    const char *b, *t;
                    if (!c.token(b, t)) return fail("truncated body in element '" + e.name + "'");
                }
        }
    }
    return OK;
}

inline int read_file(const char* path, std::vector<char>& bytes, std::string& err) {
    FILE* f = path ? std::fopen(path, "rb") : nullptr;
    if (!f) { err = std::string("cannot open ") + (path ? path : "(null)"); return E_INVAL; }
    bytes.clear();
    char buf[1 << 16];
    size_t got;
    while ((got = std::fread(buf, 1, sizeof buf, f)) > 0) bytes.insert(bytes.end(), buf, buf + got);
    const bool bad = std::ferror(f) != 0;
    std::fclose(f);
    if (bad) { err = std::string("read failed: ") + path; return E_INVAL; }
    return OK;
}

inline int read_ply(const char* path, bool fill, Ply& out, std::string& err) {
    std::vector<char> bytes;
    const int rc = read_file(path, bytes, err);
    if (rc != OK) return rc;
    return parse_ply(bytes.data(), bytes.size(), fill, out, err);
}

}  // namespace cloudhost
}  // namespace sfmx
