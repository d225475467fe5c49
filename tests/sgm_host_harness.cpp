// A stand-alone host build of csrc/sgm_pixel.h and csrc/dense_pixel.h (behind the stub <hip/hip_runtime.h> of tests/toolchain.py): reads the
// records that tests/test_sgm_cpu.py wrote (inputs and the numpy restatement's outputs), recomputes every output with the headers' functions
// by the plainest loops there are (a direct sum over every window, one pixel after another along every path, one plane after another in the
// choice; no tiles, no waves) and compares bit for bit. Built plain and with -fsanitize=address,undefined; runs on the CPU only.
//   usage: sgm_host_harness <file>       prints "ok <name>" or "DIFFERENT <name>" per record, then PASSED or FAILED
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "dense_pixel.h"
#include "sgm_pixel.h"

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

static bool cost_record() {
    const auto m = rd<long long>(7);
    const int h0 = (int)m[0], w0 = (int)m[1], h1 = (int)m[2], w1 = (int)m[3], D = (int)m[4], r = (int)m[5];
    const long long min_var = m[6];
    const auto d = rd<double>(20);
    const auto ref = rd<uint8_t>((size_t)h0 * w0), src = rd<uint8_t>((size_t)h1 * w1);
    const size_t N = (size_t)h0 * w0;
    const auto e_cost = rd<uint8_t>(N * D);
    std::vector<uint8_t> cost(N * D);
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
                cost[((size_t)v * w0 + u) * D + k] = (uint8_t)sgm_cost(valid, s);
            }
    }
    return same(cost, e_cost);
}

static bool aggregate_record() {
    const auto m = rd<long long>(6);
    const int h0 = (int)m[0], w0 = (int)m[1], D = (int)m[2], P1 = (int)m[3], P2 = (int)m[4], paths = (int)m[5];
    const size_t N = (size_t)h0 * w0;
    const auto cost = rd<uint8_t>(N * D);
    const auto e_sum = rd<uint16_t>(N * D);
    std::vector<int> total(N * D, 0), L(N * D);
    for (int p = 0; p < paths; ++p) {
        const int dy = SGM_DY[p], dx = SGM_DX[p];
        // every pixel after its predecessor: rows and columns in the sense of the direction
        for (int a = 0; a < h0; ++a)
            for (int b = 0; b < w0; ++b) {
                const int v = dy >= 0 ? a : h0 - 1 - a, u = dx >= 0 ? b : w0 - 1 - b;
                const int qv = v - dy, qu = u - dx;
                const size_t i = ((size_t)v * w0 + u) * D;
                if (qv < 0 || qv >= h0 || qu < 0 || qu >= w0) {
                    for (int k = 0; k < D; ++k) L[i + k] = cost[i + k];
                    continue;
                }
                const size_t q = ((size_t)qv * w0 + qu) * D;
                int mn = L[q];
                for (int k = 1; k < D; ++k) mn = L[q + k] < mn ? L[q + k] : mn;
                for (int k = 0; k < D; ++k)
                    L[i + k] = sgm_step(cost[i + k], L[q + k], k >= 1 ? L[q + k - 1] : SGM_FAR, k + 1 < D ? L[q + k + 1] : SGM_FAR, mn, P1, P2);
            }
        for (size_t i = 0; i < N * D; ++i) total[i] += L[i];
    }
    std::vector<uint16_t> sum(N * D);
    for (size_t i = 0; i < N * D; ++i) {
        if (total[i] < 0 || total[i] > 65535) return false;
        sum[i] = (uint16_t)total[i];
    }
    return same(sum, e_sum);
}

static bool choose_record() {
    const auto m = rd<long long>(3);
    const int h0 = (int)m[0], w0 = (int)m[1], D = (int)m[2];
    const auto d = rd<double>(3);
    const size_t N = (size_t)h0 * w0;
    const auto cost = rd<uint8_t>(N * D);
    const auto sum = rd<uint16_t>(N * D);
    const auto e_plane = rd<int16_t>(N);
    const auto e_w = rd<double>(N);
    const auto e_score = rd<float>(N);
    std::vector<int16_t> plane(N);
    std::vector<double> w(N);
    std::vector<float> score(N);
    for (size_t i = 0; i < N; ++i) {
        const uint8_t* c = &cost[i * D];
        const uint16_t* S = &sum[i * D];
        unsigned key = SGM_NO_KEY;
        for (int k = 0; k < D; ++k) {
            const unsigned q = sgm_key(c[k], S[k], k);
            key = q < key ? q : key;
        }
        int c0 = SGM_INVALID, cm = SGM_INVALID, cp = SGM_INVALID, Sm = 0, Sp = 0;
        if (key != SGM_NO_KEY) {
            const int k = (int)(key & 0xFFFFu);
            c0 = c[k];
            if (k >= 1 && k <= D - 2) { cm = c[k - 1]; cp = c[k + 1]; Sm = S[k - 1]; Sp = S[k + 1]; }
        }
        sgm_finish(key, D, c0, cm, cp, Sm, Sp, d[0], d[1], d[2], plane[i], w[i], score[i]);
    }
    return same(plane, e_plane) && same(w, e_w) && same(score, e_score);
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
        if (head[0] == 1) ok = cost_record();
        else if (head[0] == 2) ok = aggregate_record();
        else if (head[0] == 3) ok = choose_record();
        else { printf("MISSING kind %lld\n", head[0]); return 2; }
        printf("%s %s\n", ok ? "ok" : "DIFFERENT", name.c_str());
        bad += !ok; ++count;
    }
    fclose(g_f);
    printf("%d records\n%s\n", count, bad ? "FAILED" : "PASSED");
    return bad ? 1 : 0;
}
