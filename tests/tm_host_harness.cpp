// A stand-alone host build of csrc/tm_pair.h (behind the stub <hip/hip_runtime.h> of tests/toolchain.py): reads the records that
// tests/test_templatematch_host_cpu.py wrote (inputs and the numpy restatement's outputs), recomputes every output with the header's
// functions by the plainest loops there are (64 lanes one after another, every element of C through tm_corr_element) and compares bit
// for bit, a NaN equal to any NaN. Built plain and with -fsanitize=address,undefined; runs on the CPU only.
//   usage: tm_host_harness <file>     prints "ok <name>" or "DIFFERENT <name> ..." per record, then PASSED or FAILED
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "tm_pair.h"

using namespace im;

extern "C" {
float tm_h_fmaf(float a, float b, float c) { return fmaf(a, b, c); }
void tm_h_plan(int T, int S, int* out) {
    const TmPlan p = tm_plan(T, S);
    const int v[12] = {p.R, p.gy, p.gx, p.ks, p.ny, p.nx, p.kt, p.kx, p.pitch, p.brows, p.threads, p.lds_floats};
    memcpy(out, v, sizeof(v));
}
int tm_h_stage_floats(int T, int S) { return tm_stage_floats(tm_plan(T, S)); }
}

static FILE* g_f;
template <typename T> static std::vector<T> rd(size_t n) {
    std::vector<T> v(n);
    if (n && fread(v.data(), sizeof(T), n, g_f) != n) { printf("MISSING data\n"); exit(2); }
    return v;
}
template <typename T> static bool same(const std::vector<T>& a, const std::vector<T>& b) {
    return a.size() == b.size() && (a.empty() || memcmp(a.data(), b.data(), a.size() * sizeof(T)) == 0);
}
// bits equal, or both NaN
template <typename T> static bool same_fp(const std::vector<T>& a, const std::vector<T>& b, const char* what) {
    if (a.size() != b.size()) return false;
    for (size_t i = 0; i < a.size(); ++i) {
        if (a[i] != a[i] && b[i] != b[i]) continue;
        if (memcmp(&a[i], &b[i], sizeof(T)) != 0) {
            printf("  %s[%zu]: %.17g here, %.17g expected\n", what, i, (double)a[i], (double)b[i]);
            return false;
        }
    }
    return true;
}

static bool fma_record() {
    const size_t n = (size_t)rd<long long>(1)[0];
    const auto a = rd<float>(n), b = rd<float>(n), c = rd<float>(n), e = rd<float>(n);
    std::vector<float> got(n);
    for (size_t i = 0; i < n; ++i) got[i] = tm_h_fmaf(a[i], b[i], c[i]);
    return same_fp(got, e, "fma");
}

static bool plan_record() {
    const size_t n = (size_t)rd<long long>(1)[0];
    const auto T = rd<int>(n), S = rd<int>(n), e = rd<int>(12 * n);
    bool ok = true;
    for (size_t i = 0; i < n && ok; ++i) {
        int v[12];
        tm_h_plan(T[i], S[i], v);
        const TmPlan p = tm_plan(T[i], S[i]);
        if (memcmp(v, &e[12 * i], sizeof(v)) != 0) { printf("  plan(%d, %d) differs\n", T[i], S[i]); ok = false; }
        if (v[11] != std::max(tm_stage_floats(p), p.ks > 1 ? p.threads * TM_DX : 0)) ok = false;
    }
    return ok;
}

static bool window_record() {
    const auto m = rd<long long>(8);
    const size_t n = (size_t)m[0];
    const auto pairs = rd<double>(4 * n);
    const auto bidx = rd<int32_t>(n);
    const auto e_valid = rd<uint8_t>(n);
    const auto e_rows = rd<long long>(4 * n);
    const auto e_dbl = rd<double>(4 * n);
    std::vector<uint8_t> valid(n);
    std::vector<long long> rows(4 * n);
    std::vector<double> dbl(4 * n);
    for (size_t i = 0; i < n; ++i) {
        const PairWin w = pair_window(pairs.data(), bidx.data(), (int)m[1], (long)i, (int)m[2], (int)m[3], (int)m[4], (int)m[5], (int)m[6], (int)m[7]);
        valid[i] = w.valid;
        rows[4 * i] = w.arow; rows[4 * i + 1] = w.acol; rows[4 * i + 2] = w.brow; rows[4 * i + 3] = w.bcol;
        dbl[4 * i] = w.pu; dbl[4 * i + 1] = w.pv; dbl[4 * i + 2] = w.initdu; dbl[4 * i + 3] = w.initdv;
    }
    return same(valid, e_valid) && same(rows, e_rows) && same_fp(dbl, e_dbl, "window");
}

static bool forient_record() {
    const auto m = rd<long long>(4);
    const int dtype = (int)m[0], n = (int)m[1], h = (int)m[2], w = (int)m[3];
    const size_t N = (size_t)n * h * w;
    const auto img = rd<uint8_t>(N * (dtype == 0 ? 1 : 4));
    const auto e = rd<float>(2 * N);
    std::vector<float> got(2 * N);
    for (int k = 0; k < n; ++k)
        for (int y = 0; y < h; ++y)
            for (int x = 0; x < w; ++x) {
                const long base = (long)k * h * w;
                forient_pixel(img.data(), dtype, base, h, w, y, x, got[2 * (base + (long)y * w + x)], got[2 * (base + (long)y * w + x) + 1]);
            }
    return same_fp(got, e, "forient");
}

static bool corr_record() {
    const auto m = rd<long long>(3);
    const int T = (int)m[0], S = (int)m[1], R = S - T;
    const float isign = m[2] ? 1.f : -1.f;
    const auto Aw = rd<float>((size_t)2 * T * T), Bw = rd<float>((size_t)2 * S * S), e = rd<float>((size_t)R * R);
    const TmPlan p = tm_plan(T, S);
    std::vector<float> got((size_t)R * R);
    for (int i = 0; i < R; ++i)
        for (int j = 0; j < R; ++j) got[(size_t)i * R + j] = tm_corr_element(p, T, S, Aw.data(), T, Bw.data(), S, i, j, isign);
    return same_fp(got, e, "C");
}

static bool peak_record() {
    const int R = (int)rd<long long>(1)[0];
    const auto d = rd<double>(2);
    const auto C = rd<float>((size_t)R * R);
    const auto e_bi = rd<long long>(1);
    const auto e_best = rd<float>(1);
    const auto e_sabs = rd<double>(1);
    const auto e_out = rd<double>(4);
    float best[TM_WAVE];
    int bi[TM_WAVE];
    double sabs[TM_WAVE];
    for (int lane = 0; lane < TM_WAVE; ++lane) tm_lane_scan(C.data(), R * R, lane, best[lane], bi[lane], sabs[lane]);
    tm_wave_reduce(best, bi, sabs);
    std::vector<double> out(4);
    tm_peak_tail(C.data(), R, bi[0], best[0], sabs[0], d[0], d[1], out.data());
    if (bi[0] != e_bi[0]) { printf("  argmax %d here, %lld expected\n", bi[0], e_bi[0]); return false; }
    return same_fp(std::vector<float>{best[0]}, e_best, "best") && same_fp(std::vector<double>{sabs[0]}, e_sabs, "sabs") && same_fp(out, e_out, "out");
}

static bool finite_record() {
    const auto m = rd<long long>(5);
    const int side = (int)m[0], h = (int)m[1], w = (int)m[2];
    const auto map = rd<float>((size_t)2 * h * w);
    const auto e = rd<uint8_t>(1);
    bool bad = false;
    for (int lane = 0; lane < TM_WAVE; ++lane) bad = tm_window_not_finite(map.data(), (long)m[3], (long)m[4], w, side, lane) || bad;
    return (bad ? 1 : 0) == e[0];
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
        switch (head[0]) {
            case 1: ok = fma_record(); break;
            case 2: ok = plan_record(); break;
            case 3: ok = window_record(); break;
            case 4: ok = forient_record(); break;
            case 5: ok = corr_record(); break;
            case 6: ok = peak_record(); break;
            case 7: ok = finite_record(); break;
            default: printf("MISSING kind %lld\n", head[0]); return 2;
        }
        printf("%s %s\n", ok ? "ok" : "DIFFERENT", name.c_str());
        bad += !ok; ++count;
    }
    fclose(g_f);
    printf("%d records\n%s\n", count, bad ? "FAILED" : "PASSED");
    return bad ? 1 : 0;
}
