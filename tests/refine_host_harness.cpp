// A stand-alone host build of csrc/refine_pixel.h (behind the stub <hip/hip_runtime.h> of tests/toolchain.py): reads the records that
// tests/test_refine_cpu.py wrote (the inputs of a case and the numpy restatement's outputs), recomputes every output with the header's
// functions by the plainest loops there are (one pixel after another on the maps themselves, once forwards and once backwards: no tiles, no
// staging, and the result may not depend on the order) and compares bit for bit. Built plain and with -fsanitize=address,undefined; runs on
// the CPU only.
//   usage: refine_host_harness <file>       prints "ok <name>" or "DIFFERENT <name>" per record, then PASSED or FAILED
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "refine_pixel.h"

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

static bool refine_record() {
    // h0 w0 h1 w1 r min_var span sub R min_count
    const auto m = rd<long long>(10);
    const int h0 = (int)m[0], w0 = (int)m[1], h1 = (int)m[2], w1 = (int)m[3], r = (int)m[4], span = (int)m[6], sub = (int)m[7], R = (int)m[8], min_count = (int)m[9];
    const long long min_var = m[5];
    const auto d = rd<double>(20);                    // A, B, w_step, max_diff
    const double* A = d.data();
    const double* B = d.data() + 9;
    const double w_step = d[18], max_diff = d[19];
    const size_t n0 = (size_t)h0 * w0;
    const auto ref = rd<uint8_t>(n0);
    const auto src = rd<uint8_t>((size_t)h1 * w1);
    const auto plane = rd<int16_t>(n0);
    const auto w = rd<double>(n0);
    const auto score = rd<float>(n0);
    const auto e_slant = rd<double>(2 * n0);
    const auto e_fitted = rd<uint8_t>(n0);
    const auto e_w = rd<double>(n0);
    const auto e_score = rd<float>(n0);
    const auto e_taken = rd<uint8_t>(n0);
    std::vector<uint8_t> kept(n0);
    for (size_t i = 0; i < n0; ++i) kept[i] = plane[i] >= 0 ? 1 : 0;
    bool ok = true;
    for (int backwards = 0; backwards < 2; ++backwards) {
        std::vector<double> slant(2 * n0, -7.0), w_out(n0, -7.0);
        std::vector<uint8_t> fitted(n0, 7), taken(n0, 7);
        std::vector<float> score_out(n0, -7.0f);
        for (size_t k = 0; k < n0; ++k) {
            const size_t i = backwards ? n0 - 1 - k : k;
            const int u = (int)(i % w0), v = (int)(i / w0);
            double gu = 0.0, gv = 0.0;
            bool fit = false;
            if (kept[i])
                fit = slant_pixel(w.data() + i, kept.data() + i, w0, -std::min(R, u), std::min(R, w0 - 1 - u), -std::min(R, v), std::min(R, h0 - 1 - v), w_step,
                                  max_diff, min_count, gu, gv);
            slant[2 * i] = gu; slant[2 * i + 1] = gv; fitted[i] = fit ? 1 : 0;
        }
        // the refinement on the restatement's slant, so that a slant bug cannot hide a refinement bug (the slants above are compared too)
        for (size_t k = 0; k < n0; ++k) {
            const size_t i = backwards ? n0 - 1 - k : k;
            const int u = (int)(i % w0), v = (int)(i / w0);
            double wv = w[i];
            float sv = score[i];
            bool took = false;
            if (kept[i] && u >= r && u < w0 - r && v >= r && v < h0 - r)
                took = refine_pixel(ref.data() + i, w0, src.data(), h1, w1, A, B, u, v, r, w[i], score[i], e_slant[2 * i], e_slant[2 * i + 1], w_step, span, sub,
                                    min_var, wv, sv);
            w_out[i] = wv; score_out[i] = sv; taken[i] = took ? 1 : 0;
        }
        ok = ok && same(slant, e_slant) && same(fitted, e_fitted) && same(w_out, e_w) && same(score_out, e_score) && same(taken, e_taken);
    }
    return ok;
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
        if (head[0] == 1) ok = refine_record();
        else { printf("MISSING kind %lld\n", head[0]); return 2; }
        printf("%s %s\n", ok ? "ok" : "DIFFERENT", name.c_str());
        bad += !ok; ++count;
    }
    fclose(g_f);
    printf("%d records\n%s\n", count, bad ? "FAILED" : "PASSED");
    return bad ? 1 : 0;
}
