// A stand-alone host build of csrc/dense_pixel.h (behind the stub <hip/hip_runtime.h> of tests/toolchain.py): reads the records that
// tests/test_dense_cpu.py wrote (inputs and the numpy restatement's outputs), recomputes every output with the header's functions by the
// plainest loops there are (a direct sum over every window; no tiles, no partials) and compares bit for bit. Built plain and with
// -fsanitize=address,undefined; runs on the CPU only.
//   usage: dense_host_harness <file>       prints "ok <name>" or "DIFFERENT <name> ..." per record, then PASSED or FAILED
//          dense_host_harness --scratch n  prints the bytes of DenseCloudScratch(n) (csrc/stage_scratch.h)
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "dense_pixel.h"
#include "stage_scratch.h"

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

static bool sweep_record() {
    const auto m = rd<long long>(7);
    const int h0 = (int)m[0], w0 = (int)m[1], h1 = (int)m[2], w1 = (int)m[3], D = (int)m[4], r = (int)m[5];
    const long long min_var = m[6];
    const auto d = rd<double>(21);
    const auto ref = rd<uint8_t>((size_t)h0 * w0), src = rd<uint8_t>((size_t)h1 * w1);
    const auto e_plane = rd<int16_t>((size_t)h0 * w0);
    const auto e_w = rd<double>((size_t)h0 * w0);
    const auto e_score = rd<float>((size_t)h0 * w0);
    const size_t N = (size_t)h0 * w0;
    std::vector<DenseBest> best(N);
    for (auto& b : best) dense_best_init(b);
    std::vector<int> bimg(N);
    std::vector<uint8_t> okimg(N);
    const long long n = (long long)(2 * r + 1) * (2 * r + 1);
    for (int k = 0; k < D; ++k) {
        double H[9];
        dense_plane(&d[0], &d[9], d[18], d[19], k, H);
        for (int v = 0; v < h0; ++v)
            for (int u = 0; u < w0; ++u) okimg[(size_t)v * w0 + u] = dense_sample(src.data(), h1, w1, H, u, v, bimg[(size_t)v * w0 + u]);
        for (int v = 0; v < h0; ++v)
            for (int u = 0; u < w0; ++u) {
                bool valid = u >= r && u < w0 - r && v >= r && v < h0 - r;
                double s = 0.0;
                if (valid) {
                    long long sa = 0, saa = 0, sb = 0, sbb = 0, sab = 0;
                    for (int dy = -r; dy <= r; ++dy)
                        for (int dx = -r; dx <= r; ++dx) {
                            const size_t i = (size_t)(v + dy) * w0 + (u + dx);
                            const long long a = ref[i], b = bimg[i];
                            valid = valid && okimg[i];
                            sa += a; saa += a * a; sb += b; sbb += b * b; sab += a * b;
                        }
                    valid = valid && dense_score(n, sa, saa, sb, sbb, sab, min_var, s);
                }
                dense_best_step(best[(size_t)v * w0 + u], k, valid, s);
            }
    }
    std::vector<int16_t> plane(N);
    std::vector<double> w(N);
    std::vector<float> score(N);
    for (size_t i = 0; i < N; ++i) dense_best_finish(best[i], D, d[18], d[19], d[20], plane[i], w[i], score[i]);
    return same(plane, e_plane) && same(w, e_w) && same(score, e_score);
}

static bool consistency_record() {
    const auto m = rd<long long>(5);
    const int h0 = (int)m[0], w0 = (int)m[1], h1 = (int)m[2], w1 = (int)m[3], check = (int)m[4];
    const auto d = rd<double>(31);
    const auto p0 = rd<int16_t>((size_t)h0 * w0);
    const auto w0m = rd<double>((size_t)h0 * w0);
    const auto p1 = rd<int16_t>((size_t)h1 * w1);
    const auto w1m = rd<double>((size_t)h1 * w1);
    const auto e_keep = rd<uint8_t>((size_t)h0 * w0);
    DensePose P;
    memcpy(&P, d.data(), sizeof(P));
    std::vector<uint8_t> keep((size_t)h0 * w0);
    for (int v = 0; v < h0; ++v)
        for (int u = 0; u < w0; ++u) {
            const size_t i = (size_t)v * w0 + u;
            bool k = p0[i] >= 0;
            if (k && check) k = dense_consistent(P, u, v, w0m[i], p1.data(), w1m.data(), h1, w1, d[30]);
            keep[i] = k ? 1 : 0;
        }
    return same(keep, e_keep);
}

static bool cloud_record() {
    const auto m = rd<long long>(4);
    const int h = (int)m[0], w = (int)m[1], channels = (int)m[2];
    const size_t n = (size_t)m[3], N = (size_t)h * w;
    const auto d = rd<double>(21);
    const auto keep = rd<uint8_t>(N);
    const auto wm = rd<double>(N);
    const auto sc = rd<float>(N);
    const auto img = rd<uint8_t>(N * channels);
    const auto e_xyz = rd<double>(3 * n);
    const auto e_rgb = rd<uint8_t>(3 * n);
    const auto e_nrm = rd<double>(3 * n);
    const auto e_conf = rd<float>(n);
    DenseCam cam;
    memcpy(&cam, d.data(), sizeof(cam));
    std::vector<double> xyz, nrm;
    std::vector<uint8_t> rgb;
    std::vector<float> conf;
    for (int v = 0; v < h; ++v)
        for (int u = 0; u < w; ++u) {
            const size_t i = (size_t)v * w + u;
            if (!keep[i]) continue;
            double W[3], Nn[3];
            dense_point(cam, keep.data(), wm.data(), h, w, u, v, W, Nn);
            for (int c = 0; c < 3; ++c) {
                xyz.push_back(W[c]); nrm.push_back(Nn[c]);
                rgb.push_back(channels == 3 ? img[3 * i + c] : img[i]);
            }
            conf.push_back(sc[i]);
        }
    return same(xyz, e_xyz) && same(rgb, e_rgb) && same(nrm, e_nrm) && same(conf, e_conf);
}

int main(int argc, char** argv) {
    if (argc == 3 && std::string(argv[1]) == "--scratch") {      // the bytes im_dense_cloud carves for n pixels
        printf("%zu\n", DenseCloudScratch(atoll(argv[2])).bytes);
        return 0;
    }
    if (argc != 2 || !(g_f = fopen(argv[1], "rb"))) { printf("MISSING file\n"); return 2; }
    int bad = 0, count = 0;
    for (;;) {
        long long head[2];
        if (fread(head, sizeof(long long), 2, g_f) != 2) break;
        const auto name_bytes = rd<char>((size_t)head[1]);
        const std::string name(name_bytes.begin(), name_bytes.end());
        bool ok = false;
        if (head[0] == 1) ok = sweep_record();
        else if (head[0] == 2) ok = consistency_record();
        else if (head[0] == 3) ok = cloud_record();
        else { printf("MISSING kind %lld\n", head[0]); return 2; }
        printf("%s %s\n", ok ? "ok" : "DIFFERENT", name.c_str());
        bad += !ok; ++count;
    }
    fclose(g_f);
    printf("%d records\n%s\n", count, bad ? "FAILED" : "PASSED");
    return bad ? 1 : 0;
}
