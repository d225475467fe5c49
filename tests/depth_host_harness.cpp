// A stand-alone host build of csrc/depth_pixel.h (behind the stub <hip/hip_runtime.h> of tests/toolchain.py): reads the records that
// tests/test_depth_clean_cpu.py wrote (inputs and the numpy restatement's outputs), recomputes every output with the header's functions by
// the plainest loops there are (one join after another through depth_link, one pixel after another; no tiles, no waves) and compares bit
// for bit. The atomics of the header are plain host functions here: one thread runs. Built plain and with -fsanitize=address,undefined;
// runs on the CPU only.
//   usage: depth_host_harness <file>       prints "ok <name>" or "DIFFERENT <name>" per record, then PASSED or FAILED
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#define IM_DEPTH_HOST_ATOMICS
static inline int depth_load(const int* p) { return *p; }
static inline void depth_store(int* p, int v) { *p = v; }
static inline int atomicMin(int* p, int v) { const int old = *p; if (v < old) *p = v; return old; }

#include "depth_pixel.h"

using namespace im;

static FILE* g_f;
template <typename T> static std::vector<T> rd(size_t n) {
    std::vector<T> v(n);
    if (n && fread(v.data(), sizeof(T), n, g_f) != n) { printf("MISSING data\n"); exit(2); }
    return v;
}
template <typename T> static bool same(const std::vector<T>& a, const std::vector<T>& b) {
    return a.size() == b.size() && (a.empty() || memcmp(a.data(), b.data(), a.size() * sizeof(T)) == 0);
}

// labels and sizes of one map; `backwards` takes the joins in the opposite order: the result may not depend on it
static void components(const std::vector<int16_t>& plane, int h, int w, int mode, int max_diff, bool backwards, std::vector<int>& label, std::vector<int>& size) {
    const int n = h * w;
    std::vector<int> parent(n), cnt(n, 0);
    for (int i = 0; i < n; ++i) parent[i] = i;
    for (int k = 0; k < n; ++k) {
        const int i = backwards ? n - 1 - k : k, x = i % w, y = i / w;
        if (x > 0 && depth_joined(plane[i], plane[i - 1], mode, max_diff)) depth_link(parent.data(), i, i - 1);
        if (y > 0 && depth_joined(plane[i], plane[i - w], mode, max_diff)) depth_link(parent.data(), i, i - w);
    }
    label.assign(n, -1);
    size.assign(n, 0);
    for (int i = 0; i < n; ++i)
        if (depth_member(plane[i], mode)) { label[i] = depth_find(parent.data(), i); ++cnt[label[i]]; }
    for (int i = 0; i < n; ++i)
        if (label[i] >= 0) size[i] = cnt[label[i]];
}

static bool label_record() {
    const auto m = rd<long long>(4);
    const int h = (int)m[0], w = (int)m[1], mode = (int)m[2], max_diff = (int)m[3];
    const size_t n = (size_t)h * w;
    const auto plane = rd<int16_t>(n);
    const auto e_label = rd<int>(n), e_size = rd<int>(n);
    bool ok = true;
    for (int backwards = 0; backwards < 2; ++backwards) {
        std::vector<int> label, size;
        components(plane, h, w, mode, max_diff, backwards != 0, label, size);
        ok = ok && same(label, e_label) && same(size, e_size);
    }
    return ok;
}

static bool drop_record() {
    const auto m = rd<long long>(5);
    const int h = (int)m[0], w = (int)m[1], min_size = (int)m[2], max_diff = (int)m[3];
    const long long e_count = m[4];
    const size_t n = (size_t)h * w;
    auto plane = rd<int16_t>(n);
    auto wm = rd<double>(n);
    auto score = rd<float>(n);
    const auto e_plane = rd<int16_t>(n);
    const auto e_w = rd<double>(n);
    const auto e_score = rd<float>(n);
    std::vector<int> label, size;
    components(plane, h, w, DEPTH_SURFACES, max_diff, false, label, size);
    long long count = 0;
    for (size_t i = 0; i < n; ++i)
        if (plane[i] >= 0 && size[i] < min_size) { plane[i] = -1; wm[i] = 0.0; score[i] = 0.0f; ++count; }
    return count == e_count && same(plane, e_plane) && same(wm, e_w) && same(score, e_score);
}

static bool fill_record() {
    const auto m = rd<long long>(6);
    const int h = (int)m[0], w = (int)m[1], max_hole = (int)m[2], max_diff = (int)m[3], D = (int)m[4];
    const long long e_count = m[5];
    const auto d = rd<double>(2);
    const size_t n = (size_t)h * w;
    const auto plane = rd<int16_t>(n);
    const auto wm = rd<double>(n);
    const auto score = rd<float>(n);
    const auto e_plane = rd<int16_t>(n);
    const auto e_w = rd<double>(n);
    const auto e_score = rd<float>(n);
    const auto e_filled = rd<uint8_t>(n);
    std::vector<int> label, size;
    components(plane, h, w, DEPTH_HOLES, 0, false, label, size);
    std::vector<int> lo(n, DEPTH_NO_RIM), hi(n, 0);
    for (int y = 0; y < h; ++y)
        for (int x = 0; x < w; ++x) {
            const size_t i = (size_t)y * w + x;
            if (label[i] < 0) continue;
            const int l = label[i];
            if (x == 0 || y == 0 || x == w - 1 || y == h - 1) { hi[l] |= DEPTH_BORDER; continue; }
            const int q[4] = {plane[i - 1], plane[i + 1], plane[i - w], plane[i + w]};
            for (int k = 0; k < 4; ++k)
                if (q[k] >= 0) { lo[l] = q[k] < lo[l] ? q[k] : lo[l]; hi[l] = q[k] > hi[l] ? q[k] : hi[l]; }      // atomicMin / atomicMax
        }
    auto o_plane = plane;
    auto o_w = wm;
    auto o_score = score;
    std::vector<uint8_t> filled(n, 0);
    long long count = 0;
    for (int y = 0; y < h; ++y)
        for (int x = 0; x < w; ++x) {
            const size_t i = (size_t)y * w + x;
            if (label[i] < 0 || !depth_hole_qualifies(size[i], lo[label[i]], hi[label[i]], max_hole, max_diff)) continue;
            int xl = x, xr = x, yu = y, yd = y;
            while (plane[(size_t)y * w + xl] < 0) --xl;
            while (plane[(size_t)y * w + xr] < 0) ++xr;
            while (plane[(size_t)yu * w + x] < 0) --yu;
            while (plane[(size_t)yd * w + x] < 0) ++yd;
            const double a = depth_between(wm[(size_t)y * w + xl], wm[(size_t)y * w + xr], x, xl, xr);
            const double b = depth_between(wm[(size_t)yu * w + x], wm[(size_t)yd * w + x], y, yu, yd);
            o_w[i] = depth_fill(a, b);
            o_plane[i] = (int16_t)depth_plane_of(o_w[i], d[0], d[1], D);
            o_score[i] = 0.0f;
            filled[i] = 1;
            ++count;
        }
    return count == e_count && same(o_plane, e_plane) && same(o_w, e_w) && same(o_score, e_score) && same(filled, e_filled);
}

int main(int argc, char** argv) {
    if (argc != 2 || !(g_f = fopen(argv[1], "rb"))) { printf("MISSING file\n"); return 2; }
    int bad = 0, count = 0;
    for (;;) {
        long long head[2];
        if (fread(head, sizeof(long long), 2, g_f) != 2) break;
        const auto name_bytes = rd<char>((size_t)head[1]);
        const std::string name(name_bytes.begin(), name_bytes.end());
        bool ok = false;
        if (head[0] == 1) ok = label_record();
        else if (head[0] == 2) ok = drop_record();
        else if (head[0] == 3) ok = fill_record();
        else { printf("MISSING kind %lld\n", head[0]); return 2; }
        printf("%s %s\n", ok ? "ok" : "DIFFERENT", name.c_str());
        bad += !ok; ++count;
    }
    fclose(g_f);
    printf("%d records\n%s\n", count, bad ? "FAILED" : "PASSED");
    return bad ? 1 : 0;
}
