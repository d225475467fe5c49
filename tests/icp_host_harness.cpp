// Host build of the arithmetic of csrc/icp.hip (csrc/icp_point.h) for tests/test_icp_cpu.py: the very text the kernels compile, behind a
// stub <hip/hip_runtime.h>. The rows, the solve, the update and the record are the header's functions. What the kernels do with wave
// shuffles and LDS is replayed here over an array of 256 thread sums: the butterfly v[lane] + v[lane ^ o] and icp_join_waves.
#include <hip/hip_runtime.h>

#include <vector>

#include "icp_point.h"
#include "stage_scratch.h"

namespace {

// the block's sum of every term from its 256 threads' sums, as icp_block_sum forms it
void block_sum(std::vector<double>& S, double* out) {
    std::vector<double> nv(im::ICP_BLOCK);
    for (int k = 0; k < im::ICP_TERMS; ++k) {
        for (int o = 1; o < 64; o <<= 1) {
            for (int t = 0; t < im::ICP_BLOCK; ++t) nv[t] = S[t * im::ICP_TERMS + k] + S[((t & ~63) | ((t & 63) ^ o)) * im::ICP_TERMS + k];
            for (int t = 0; t < im::ICP_BLOCK; ++t) S[t * im::ICP_TERMS + k] = nv[t];
        }
        out[k] = im::icp_join_waves(S[k], S[64 * im::ICP_TERMS + k], S[128 * im::ICP_TERMS + k], S[192 * im::ICP_TERMS + k]);
    }
}

}  // namespace

extern "C" int icp_host_chunk() { return im::ICP_CHUNK; }

extern "C" void icp_host_apply(const double* M, const double* in, double* out, long long n, int as_vectors) {
    for (long long i = 0; i < n; ++i) {
        double p[3];
        im::icp_apply(M, in[3 * i], in[3 * i + 1], in[3 * i + 2], as_vectors != 0, p);
        for (int a = 0; a < 3; ++a) out[3 * i + a] = p[a];
    }
}

// what one point alone adds to sums that start at +0.0: terms [n][32]
extern "C" void icp_host_terms(const double* src, long long n, const double* tgt, const double* nrm, long long n_tgt, const int* idx,
                               const double* d2, const double* c, int method, double* terms) {
    const double cc[3] = {c[0], c[1], c[2]};
    for (long long i = 0; i < n; ++i) {
        double S[im::ICP_TERMS];
        im::icp_zero(S);
        im::icp_point(S, src[3 * i], src[3 * i + 1], src[3 * i + 2], tgt, nrm, n_tgt, idx[i], d2[i], cc, method);
        for (int k = 0; k < im::ICP_TERMS; ++k) terms[i * im::ICP_TERMS + k] = S[k];
    }
}

// the partial of every chunk: parts [ceil(n / ICP_CHUNK)][32]
extern "C" void icp_host_partials(const double* src, long long n, const double* tgt, const double* nrm, long long n_tgt, const int* idx,
                                  const double* d2, const double* c, int method, double* parts) {
    const double cc[3] = {c[0], c[1], c[2]};
    std::vector<double> S(im::ICP_BLOCK * im::ICP_TERMS);
    for (long long first = 0, ch = 0; first < n; first += im::ICP_CHUNK, ++ch) {
        const long long end = first + im::ICP_CHUNK < n ? first + im::ICP_CHUNK : n;
        for (int t = 0; t < im::ICP_BLOCK; ++t) {
            double T[im::ICP_TERMS];
            im::icp_zero(T);
            for (long long i = first + t; i < end; i += im::ICP_BLOCK)
                im::icp_point(T, src[3 * i], src[3 * i + 1], src[3 * i + 2], tgt, nrm, n_tgt, idx[i], d2[i], cc, method);
            for (int k = 0; k < im::ICP_TERMS; ++k) S[t * im::ICP_TERMS + k] = T[k];
        }
        block_sum(S, parts + ch * im::ICP_TERMS);
    }
}

// the partials summed as icp_finish_kernel sums them: total [32]
extern "C" void icp_host_total(const double* parts, long long n_chunks, double* total) {
    std::vector<double> S(im::ICP_BLOCK * im::ICP_TERMS);
    for (int t = 0; t < im::ICP_BLOCK; ++t) {
        double T[im::ICP_TERMS];
        im::icp_zero(T);
        for (long long ch = t; ch < n_chunks; ch += im::ICP_BLOCK)
            for (int k = 0; k < im::ICP_SUMS; ++k) T[k] = T[k] + parts[ch * im::ICP_TERMS + k];
        for (int k = 0; k < im::ICP_TERMS; ++k) S[t * im::ICP_TERMS + k] = T[k];
    }
    block_sum(S, total);
}

extern "C" void icp_host_finish(const double* S, const double* M, const double* c, long long n, int solve, double* rec) {
    const double cc[3] = {c[0], c[1], c[2]};
    im::icp_finish(S, M, cc, n, solve != 0, rec);
}

extern "C" void icp_host_cayley(const double* w, double* R) {
    double out[9];
    im::icp_cayley(w[0], w[1], w[2], out);
    for (int k = 0; k < 9; ++k) R[k] = out[k];
}

// the bytes im_icp_accumulate asks its context for
extern "C" unsigned long long icp_host_scratch(long long chunks) { return im::IcpScratch(chunks).bytes; }
