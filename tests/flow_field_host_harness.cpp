// A stand-alone host build of csrc/flow_field_pixel.h and csrc/flow_pixel.h (behind the stub <hip/hip_runtime.h> of tests/toolchain.py):
// reads the records that tests/test_pyrflow_cpu.py wrote (the inputs of a case and the numpy restatement's outputs), recomputes every
// output with the headers' functions by the plainest loops there are (one pixel after another, once forwards and once backwards: no
// tiles, no staging, and the result may not depend on the order) and compares bit for bit. Built plain and with
// -fsanitize=address,undefined; runs on the CPU only.
//   usage: flow_field_host_harness <file>       prints "ok <name>" or "DIFFERENT <name>" per record, then PASSED or FAILED
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "flow_field_pixel.h"

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

static bool prior_up_record() {
    // hc wc h w m min_count
    const auto m = rd<long long>(6);
    const int hc = (int)m[0], wc = (int)m[1], h = (int)m[2], w = (int)m[3], radius = (int)m[4], min_count = (int)m[5];
    const size_t nc = (size_t)hc * wc, n = (size_t)h * w;
    const auto du = rd<double>(nc);
    const auto dv = rd<double>(nc);
    const auto valid = rd<uint8_t>(nc);
    const auto e_pu = rd<int16_t>(n);
    const auto e_pv = rd<int16_t>(n);
    const auto e_have = rd<uint8_t>(n);
    bool ok = true;
    for (int backwards = 0; backwards < 2; ++backwards) {
        std::vector<int16_t> pu(n, -7), pv(n, -7);
        std::vector<uint8_t> have(n, 7);
        for (size_t k = 0; k < n; ++k) {
            const size_t i = backwards ? n - 1 - k : k;
            const int u = (int)(i % w), v = (int)(i / w);
            int x = 0, y = 0;
            bool got = false;
            if (radius == 0) got = flow_prior_up_pixel<0>(du.data(), dv.data(), valid.data(), hc, wc, u, v, min_count, x, y);
            else if (radius == 1) got = flow_prior_up_pixel<1>(du.data(), dv.data(), valid.data(), hc, wc, u, v, min_count, x, y);
            else got = flow_prior_up_pixel<2>(du.data(), dv.data(), valid.data(), hc, wc, u, v, min_count, x, y);
            pu[i] = (int16_t)x; pv[i] = (int16_t)y; have[i] = got ? 1 : 0;
        }
        ok = ok && same(pu, e_pu) && same(pv, e_pv) && same(have, e_have);
    }
    return ok;
}

static bool field_record() {
    // h w r S min_var has_ask
    const auto m = rd<long long>(6);
    const int h = (int)m[0], w = (int)m[1], r = (int)m[2], S = (int)m[3];
    const long long min_var = m[4];
    const double min_score = rd<double>(1)[0];
    const size_t n = (size_t)h * w;
    const auto a = rd<uint8_t>(n);
    const auto b = rd<uint8_t>(n);
    const auto pu = rd<int16_t>(n);
    const auto pv = rd<int16_t>(n);
    const auto have = rd<uint8_t>(n);
    const auto ask = rd<uint8_t>(m[5] ? n : 0);
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
            if (flow_field_wanted(have[i], ask.empty() ? 1 : ask[i], pu[i], pv[i]))
                v = flow_match_pixel(a.data(), b.data(), h, w, (int)(i % w), (int)(i / w), r, S, pu[i], pv[i], min_var, min_score, x, y, s);
            du[i] = x; dv[i] = y; score[i] = s; valid[i] = v ? 1 : 0;
        }
        ok = ok && same(du, e_du) && same(dv, e_dv) && same(score, e_score) && same(valid, e_valid);
    }
    return ok;
}

static bool spread_record() {
    // count, then per entry: r S E and the bytes of LDS of an E x E box on a 64 x 16 tile
    const long long count = rd<long long>(1)[0];
    const auto e = rd<long long>((size_t)count * 4);
    bool ok = true;
    for (long long k = 0; k < count; ++k) {
        const int r = (int)e[4 * k], S = (int)e[4 * k + 1];
        const int E = flow_field_spread(64, 16, r, S);
        ok = ok && E == e[4 * k + 2] && flow_field_lds_bytes(64, 16, r, S, E, E) == e[4 * k + 3] && flow_field_lds_bytes(64, 16, r, S, E, E) <= FLOW_FIELD_LDS_BUDGET;
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
        if (head[0] == 1) ok = prior_up_record();
        else if (head[0] == 2) ok = field_record();
        else if (head[0] == 3) ok = spread_record();
        else { printf("MISSING kind %lld\n", head[0]); return 2; }
        printf("%s %s\n", ok ? "ok" : "DIFFERENT", name.c_str());
        bad += !ok; ++count;
    }
    fclose(g_f);
    printf("%d records\n%s\n", count, bad ? "FAILED" : "PASSED");
    return bad ? 1 : 0;
}
