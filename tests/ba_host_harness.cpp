// Host build of the arithmetic of csrc/ba.hip (csrc/ba_point.h) for tests/test_ba_cpu.py: the very text the kernels compile, behind a stub
// <hip/hip_runtime.h>. The factors, the terms, the solve, the steps and the decision are the header's functions; what the kernels do with
// blocks and LDS is replayed here as plain loops in the order the header states: a chunk's points ascending, then the chunks ascending.
#include <hip/hip_runtime.h>

#include <vector>

#include "ba_point.h"
#include "stage_scratch.h"

using namespace im;

extern "C" int ba_host_chunk() { return BA_CHUNK; }
extern "C" int ba_host_tile() { return BA_TILE; }
extern "C" int ba_host_fac() { return BA_FAC; }
extern "C" unsigned ba_host_default_mask() { return BA_MASK_DEFAULT; }
extern "C" unsigned long long ba_host_scratch(long long E, long long M) { return BaScratch(E, M).bytes; }

extern "C" void ba_host_project(const double* cam, const double* X, double* out) {
    const double x[3] = {X[0], X[1], X[2]};
    BaProj p;
    ba_project(cam, x, p);
    out[0] = p.u; out[1] = p.v; out[2] = p.Xc[2];
}

extern "C" void ba_host_factors(const double* cams, const double* pts, const double* obs, const double* sig, const double* prior, long long n,
                                double lambda, double* fac) {
    for (long long i = 0; i < n; ++i) {
        const double X[3] = {pts[3 * i], pts[3 * i + 1], pts[3 * i + 2]};
        ba_point_factors(cams, X, obs + 4 * i, sig[i], prior + 6 * i, lambda, fac + i * BA_FAC);
    }
}

// parts [ceil(n / BA_CHUNK)][448] from the factors
extern "C" void ba_host_partials(const double* fac, long long n, double* parts) {
    for (long long c0 = 0, ch = 0; c0 < n; c0 += BA_CHUNK, ++ch) {
        const long long end = c0 + BA_CHUNK < n ? c0 + BA_CHUNK : n;
        for (int e = 0; e < BA_TERMS; ++e) {
            int kind, a, b;
            ba_entry(e, kind, a, b);
            double s = 0.0;
            for (long long i = c0; i < end; ++i) s = s + ba_term(fac + i * BA_FAC, kind, a, b);
            parts[ch * BA_TERMS + e] = s;
        }
    }
}

extern "C" void ba_host_total(const double* parts, long long chunks, double* tot) {
    for (int e = 0; e < BA_TERMS; ++e) {
        double s = 0.0;
        for (long long ch = 0; ch < chunks; ++ch) s = s + parts[ch * BA_TERMS + e];
        tot[e] = s;
    }
}

extern "C" void ba_host_solve(const double* tot, const double* cams, const double* cprior, double lambda, unsigned mask, double* rec, double* cand) {
    std::vector<double> A(BA_DIM * BA_DIM), wk(5 * BA_DIM);
    ba_solve_epoch(tot, cams, cprior, lambda, mask, A.data(), wk.data(), rec, cand);
}

// the candidate points, their cost terms [n] and the chunk partials of the cost
extern "C" void ba_host_step_points(const double* fac, const double* x, const double* pts, const double* cand, const double* obs, const double* sig,
                                    const double* prior, long long n, double* out, double* terms, double* cparts) {
    for (long long i = 0; i < n; ++i) {
        const double* keep = fac + i * BA_FAC + BA_F_Y;
        const double X[3] = {pts[3 * i], pts[3 * i + 1], pts[3 * i + 2]};
        double Y[3];
        ba_point_step(keep, x, X, Y);
        for (int k = 0; k < 3; ++k) out[3 * i + k] = Y[k];
        terms[i] = ba_point_cost(cand, Y, obs + 4 * i, sig[i], prior + 6 * i, keep[BA_F_OK - BA_F_Y] != 0.0);
    }
    for (long long c0 = 0, ch = 0; c0 < n; c0 += BA_CHUNK, ++ch) {
        double s = 0.0;
        for (long long i = c0; i < c0 + BA_CHUNK; ++i) s = s + (i < n ? terms[i] : 0.0);
        cparts[ch] = s;
    }
}

extern "C" double ba_host_centre_cost(const double* cams, const double* cprior) { return ba_centre_cost(cams, cprior); }

extern "C" void ba_host_decide(const double* draft, double cost1, const double* opts, double* st, double* rec) { ba_decide(draft, cost1, opts, st, rec); }

extern "C" void ba_host_residuals(const double* cams, const double* pts, const double* obs, long long n, double* res) {
    for (long long i = 0; i < n; ++i) {
        const double X[3] = {pts[3 * i], pts[3 * i + 1], pts[3 * i + 2]};
        ba_point_residuals(cams, X, obs + 4 * i, res + 6 * i);
    }
}

// The whole loop of one epoch as the four kernels run it: cams [48] and pts [n][3] in and out, st [8] in and out, history [hist_rows][64].
extern "C" void ba_host_run(double* cams, double* pts, const double* obs, const double* sig, const double* prior, long long n, const double* cprior,
                            unsigned mask, const double* opts, double* st, double* history, long long hist_rows) {
    const long long chunks = (n + BA_CHUNK - 1) / BA_CHUNK;
    std::vector<double> fac((n > 0 ? n : 1) * BA_FAC), parts((chunks > 0 ? chunks : 1) * BA_TERMS), tot(BA_TERMS), draft(BA_RECORD), cand(BA_EPOCH),
        out(3 * (n > 0 ? n : 1)), terms(n > 0 ? n : 1), cparts(chunks > 0 ? chunks : 1), dummy(BA_RECORD);
    for (long long launch = 0; launch < hist_rows; ++launch) {
        if (st[BA_ST_DONE] != 0.0) break;
        ba_host_factors(cams, pts, obs, sig, prior, n, st[BA_ST_LAMBDA], fac.data());
        ba_host_partials(fac.data(), n, parts.data());
        ba_host_total(parts.data(), chunks, tot.data());
        ba_host_solve(tot.data(), cams, cprior, st[BA_ST_LAMBDA], mask, draft.data(), cand.data());
        ba_host_step_points(fac.data(), draft.data() + BA_REC_X, pts, cand.data(), obs, sig, prior, n, out.data(), terms.data(), cparts.data());
        double s = 0.0;
        for (long long ch = 0; ch < chunks; ++ch) s = s + cparts[ch];
        const double cost1 = s + ba_centre_cost(cand.data(), cprior);
        const double parity = st[BA_ST_PARITY];
        const long long it = (long long)st[BA_ST_ITER];
        ba_decide(draft.data(), cost1, opts, st, it < hist_rows ? history + it * BA_RECORD : dummy.data());
        if (st[BA_ST_PARITY] != parity) {
            for (int k = 0; k < BA_EPOCH; ++k) cams[k] = cand[k];
            for (long long k = 0; k < 3 * n; ++k) pts[k] = out[k];
        }
    }
}
