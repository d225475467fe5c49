// A stand-alone host build of csrc/fuse_pixel.h (behind the stub <hip/hip_runtime.h> of tests/toolchain.py): reads the records that
// tests/test_fuse_cpu.py wrote (the inputs of a case and the numpy restatement's outputs), recomputes every output with the header's
// functions by the plainest loops there are (one pixel after another, once forwards and once backwards: the result may not depend on the
// order) and compares bit for bit. Built plain and with -fsanitize=address,undefined; runs on the CPU only.
//   usage: fuse_host_harness <file>       prints "ok <name>" or "DIFFERENT <name>" per record, then PASSED or FAILED
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "fuse_pixel.h"

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

static bool fuse_record() {
    const auto m = rd<long long>(4);
    const int ha = (int)m[0], wa = (int)m[1], hb = (int)m[2], wb = (int)m[3];
    const auto d = rd<double>(62);
    DensePose ab, ba;
    memcpy(&ab, d.data(), sizeof(DensePose));
    memcpy(&ba, d.data() + 30, sizeof(DensePose));
    const double tol_b = d[60], tol_a = d[61];
    const size_t na = (size_t)ha * wa, nb = (size_t)hb * wb;
    const auto keep_a = rd<uint8_t>(na);
    const auto w_a = rd<double>(na);
    const auto score_a = rd<float>(na);
    const auto keep_b = rd<uint8_t>(nb);
    const auto w_b = rd<double>(nb);
    const auto score_b = rd<float>(nb);
    const auto e_link = rd<int>(na);
    const auto e_w = rd<double>(na);
    const auto e_score = rd<float>(na);
    const auto e_views = rd<uint8_t>(na);
    const auto e_claimed = rd<uint8_t>(nb);
    const auto e_rest = rd<uint8_t>(nb);
    bool ok = true;
    for (int backwards = 0; backwards < 2; ++backwards) {
        std::vector<int> link(na, -7);
        std::vector<double> w(na, -7.0);
        std::vector<float> score(na, -7.0f);
        std::vector<uint8_t> views(na, 7), claimed(nb, 0), rest(nb, 7);
        for (size_t k = 0; k < na; ++k) {
            const size_t i = backwards ? na - 1 - k : k;
            const FusedPixel o = fuse_pixel(ab, (int)(i % wa), (int)(i / wa), keep_a[i], w_a[i], score_a[i], keep_b.data(), w_b.data(), score_b.data(), hb, wb, tol_b);
            link[i] = o.link; w[i] = o.w; score[i] = o.score; views[i] = o.views;
            if (o.link >= 0) claimed.at((size_t)o.link) = 1;
        }
        for (size_t k = 0; k < nb; ++k) {
            const size_t i = backwards ? nb - 1 - k : k;
            rest[i] = fuse_rest(ba, (int)(i % wb), (int)(i / wb), keep_b[i], claimed[i], w_b[i], keep_a.data(), w_a.data(), ha, wa, tol_a) ? 1 : 0;
        }
        ok = ok && same(link, e_link) && same(w, e_w) && same(score, e_score) && same(views, e_views) && same(claimed, e_claimed) && same(rest, e_rest);
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
        if (head[0] == 1) ok = fuse_record();
        else { printf("MISSING kind %lld\n", head[0]); return 2; }
        printf("%s %s\n", ok ? "ok" : "DIFFERENT", name.c_str());
        bad += !ok; ++count;
    }
    fclose(g_f);
    printf("%d records\n%s\n", count, bad ? "FAILED" : "PASSED");
    return bad ? 1 : 0;
}
