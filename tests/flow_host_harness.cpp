// A stand-alone host build of csrc/flow_pixel.h (behind the stub <hip/hip_runtime.h> of tests/toolchain.py): reads the records that
// tests/test_flow_cpu.py wrote (the inputs of a case and the numpy restatement's outputs), recomputes every output with the header's
// functions by the plainest loops there are (one pixel after another on the images and maps themselves, once forwards and once backwards:
// no tiles, no staging, and the result may not depend on the order) and compares bit for bit. Built plain and with
// -fsanitize=address,undefined; runs on the CPU only.
//   usage: flow_host_harness <file>       prints "ok <name>" or "DIFFERENT <name>" per record, then PASSED or FAILED
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "flow_pixel.h"

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

static bool match_record() {
    // h w r S pu pv min_var has_ask
    const auto m = rd<long long>(8);
    const int h = (int)m[0], w = (int)m[1], r = (int)m[2], S = (int)m[3], pu = (int)m[4], pv = (int)m[5];
    const long long min_var = m[6];
    const double min_score = rd<double>(1)[0];
    const size_t n = (size_t)h * w;
    const auto a = rd<uint8_t>(n);
    const auto b = rd<uint8_t>(n);
    const auto ask = rd<uint8_t>(m[7] ? n : 0);
    const auto e_du = rd<double>(n);
    const auto e_dv = rd<double>(n);
    const auto e_score = rd<float>(n);
    const auto e_valid = rd<uint8_t>(n);
    bool ok = true;
    for (int backwards = 0; backwards < 2; ++backwards) {
        std::vector<double> du(n, -7.0), dv(n, -7.0);
        std::vector<float> score(n, -7.0f);
        std::vector<uint8_t> valid(n, 7);
        for (size_t k = 0; k < n; ++k) {
            const size_t i = backwards ? n - 1 - k : k;
            double x = 0.0, y = 0.0;
            float s = 0.0f;
            bool v = false;
            if (ask.empty() || ask[i] != 0) v = flow_match_pixel(a.data(), b.data(), h, w, (int)(i % w), (int)(i / w), r, S, pu, pv, min_var, min_score, x, y, s);
            du[i] = x; dv[i] = y; score[i] = s; valid[i] = v ? 1 : 0;
        }
        ok = ok && same(du, e_du) && same(dv, e_dv) && same(score, e_score) && same(valid, e_valid);
    }
    return ok;
}

static bool check_record() {
    const auto m = rd<long long>(2);
    const int h = (int)m[0], w = (int)m[1];
    const double tol = rd<double>(1)[0];
    const size_t n = (size_t)h * w;
    const auto du = rd<double>(n);
    const auto dv = rd<double>(n);
    const auto valid = rd<uint8_t>(n);
    const auto du_b = rd<double>(n);
    const auto dv_b = rd<double>(n);
    const auto valid_b = rd<uint8_t>(n);
    const auto e_keep = rd<uint8_t>(n);
    bool ok = true;
    for (int backwards = 0; backwards < 2; ++backwards) {
        std::vector<uint8_t> keep(n, 7);
        for (size_t k = 0; k < n; ++k) {
            const size_t i = backwards ? n - 1 - k : k;
            keep[i] = valid[i] != 0 && flow_consistent((int)(i % w), (int)(i / w), du[i], dv[i], du_b.data(), dv_b.data(), valid_b.data(), h, w, tol) ? 1 : 0;
        }
        ok = ok && same(keep, e_keep);
    }
    return ok;
}

static bool lift_record() {
    const auto m = rd<long long>(4);
    const int h = (int)m[0], w = (int)m[1], hb = (int)m[2], wb = (int)m[3];
    const auto d = rd<double>(44);                    // cam_a, cam_b, w_step_b, max_diff
    DenseCam ca, cb;
    memcpy(&ca, d.data(), sizeof(DenseCam));
    memcpy(&cb, d.data() + 21, sizeof(DenseCam));
    const double span = d[43] * fabs(d[42]);          // as im_flow_lift forms it
    const size_t n = (size_t)h * w, nb = (size_t)hb * wb;
    const auto du = rd<double>(n);
    const auto dv = rd<double>(n);
    const auto valid = rd<uint8_t>(n);
    const auto keep = rd<uint8_t>(n);
    const auto plane_a = rd<int16_t>(n);
    const auto w_a = rd<double>(n);
    const auto plane_b = rd<int16_t>(nb);
    const auto w_b = rd<double>(nb);
    const auto keep_b = rd<uint8_t>(nb);
    const auto e_P = rd<double>(3 * n);
    const auto e_D = rd<double>(3 * n);
    const auto e_ok = rd<uint8_t>(n);
    bool ok = true;
    for (int backwards = 0; backwards < 2; ++backwards) {
        std::vector<double> P(3 * n, -7.0), D(3 * n, -7.0);
        std::vector<uint8_t> lifted(n, 7);
        for (size_t k = 0; k < n; ++k) {
            const size_t i = backwards ? n - 1 - k : k;
            double p[3] = {0.0, 0.0, 0.0}, q[3] = {0.0, 0.0, 0.0};
            bool l = false;
            if (keep[i] != 0 && plane_a[i] >= 0 && valid[i] != 0)
                l = flow_lift_pixel(ca, cb, (int)(i % w), (int)(i / w), w_a[i], du[i], dv[i], plane_b.data(), w_b.data(), keep_b.data(), hb, wb, span, p, q);
            for (int c = 0; c < 3; ++c) { P[3 * i + c] = p[c]; D[3 * i + c] = q[c]; }
            lifted[i] = l ? 1 : 0;
        }
        ok = ok && same(P, e_P) && same(D, e_D) && same(lifted, e_ok);
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
        if (head[0] == 1) ok = match_record();
        else if (head[0] == 2) ok = check_record();
        else if (head[0] == 3) ok = lift_record();
        else { printf("MISSING kind %lld\n", head[0]); return 2; }
        printf("%s %s\n", ok ? "ok" : "DIFFERENT", name.c_str());
        bad += !ok; ++count;
    }
    fclose(g_f);
    printf("%d records\n%s\n", count, bad ? "FAILED" : "PASSED");
    return bad ? 1 : 0;
}
