// extern "C" boundary of libicematch (see include/icematch.h): context, workspace (im_ctx_reserve), profiler, debug reads / clock probe
// and the stage entry points. The model forwards live in superpoint.hip / lightglue.hip / superglue.hip, weights in weights.hip,
// the IM_DEBUG_GUARDS entry points in guards.hip.
#include "block.h"
#include "ctx.h"
#include "lg_misc.h"
#include "sp_post.h"
#include "workspace.h"

#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <cstring>

using namespace im;

// Stage entry points that take host weights: uploads the N arrays, runs launch(d) on `st`, synchronises and frees on every path;
// the first error is the result
template <int N, typename F>
static hipError_t with_uploads(const float* const (&src)[N], const size_t (&sizes)[N], hipStream_t st, F&& launch) {
    float* d[N] = {};
    hipError_t e = hipSuccess;
    for (int i = 0; i < N && e == hipSuccess; ++i) {
        e = hipMalloc(&d[i], sizes[i] * sizeof(float));
        if (e == hipSuccess) e = hipMemcpy(d[i], src[i], sizes[i] * sizeof(float), hipMemcpyHostToDevice);
    }
    if (e == hipSuccess) e = launch(d);
    const hipError_t e2 = hipStreamSynchronize(st);
    for (int i = 0; i < N; ++i) hipFree(d[i]);
    return e != hipSuccess ? e : e2;
}

extern "C" {

int im_version(void) { return 100; }

int im_ctx_create(int device, im_ctx** out) {
    if (!out) return -1;
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || device < 0 || device >= ndev) return -2;
    if (hipSetDevice(device) != hipSuccess) return -3;
    im_ctx* c = new im_ctx();
    c->device = device;
    c->guards_on = env_is_1("IM_DEBUG_GUARDS");
    *out = c;
    return 0;
}

void im_ctx_destroy(im_ctx* ctx) {
    if (!ctx) return;
    hipSetDevice(ctx->device);
    ctx->free_all();
    delete ctx;
}

const char* im_last_error(im_ctx* ctx) { return ctx ? ctx->err.c_str() : "null context"; }

int im_ctx_reserve(im_ctx* ctx, int max_h, int max_w, int max_images, int max_kpts) {
    IM_CHECK_CTX(ctx);
    if (max_h < 8 || max_w < 8 || max_images < 1 || max_kpts < 1) return ctx->fail(-30, "im_ctx_reserve: bad sizes");
    // the kernels address one image / one score matrix through 32-bit buffer offsets (range-checked descriptors): fail loudly
    // instead of wrapping around. Larger inputs go through the tile modes of the matcher (`matchers.py:304-469`).
    // (16 rows of margin: halo rows below the image and the rows of a last, partial region are addressed too - past the descriptor's
    // range, where loads return zero and stores are dropped - and their offsets must not wrap either)
    if ((long)(max_h / 2 + 16) * (max_w / 2) * 64 * 4 >= (1L << 32))
        return ctx->fail(-33, "im_ctx_reserve: %d x %d exceeds 67 MP per image (32-bit offsets into the half-resolution activations): use a tile mode", max_h, max_w);
    if (max_kpts >= 32768)
        return ctx->fail(-34, "im_ctx_reserve: %d keypoints per image: the K x K score matrix is addressed with 32-bit byte offsets (K < 32768)", max_kpts);
    if (ctx->ws && max_h <= ctx->max_h && max_w <= ctx->max_w && max_images <= ctx->max_images && max_kpts <= ctx->max_kpts) return 0;
    IM_HIP(ctx, hipDeviceSynchronize());
    if (ctx->ws) {
        IM_GUARD_CHECK(ctx, nullptr, "the last use of the workspace that im_ctx_reserve replaces");
        for (void* p : ctx->ws->allocs) ctx->gfree(p);
        delete ctx->ws;
        ctx->ws = nullptr;
    }
    if (ctx->max_h > max_h) max_h = ctx->max_h;
    if (ctx->max_w > max_w) max_w = ctx->max_w;
    if (ctx->max_images > max_images) max_images = ctx->max_images;
    if (ctx->max_kpts > max_kpts) max_kpts = ctx->max_kpts;
    Workspace* ws = new Workspace();
    const long B = max_images;
    const long H8 = (max_h / 8) * 8, W8 = (max_w / 8) * 8, cells = (H8 / 8) * (W8 / 8), K = max_kpts;
    ws->smap_floats = (size_t)B * H8 * W8;
    bool ok = true;
    auto alloc_named = [&](auto*& p, size_t n, const char* name) {
        using T = std::remove_reference_t<decltype(*p)>;
        p = reinterpret_cast<T*>(ctx->galloc(n * sizeof(T), name, ws->allocs));
        if (!p) ok = false;
    };
#define A(ptr, n) alloc_named(ptr, n, #ptr)
    A(ws->act0, (size_t)B * (max_h / 2) * (max_w / 2) * 64);  // conv1a is fused: nothing is stored at full resolution
    A(ws->act1, (size_t)B * (max_h / 2) * (max_w / 2) * 64);
    A(ws->logits, (size_t)B * cells * 65);
    A(ws->dense, (size_t)B * cells * 256);
    A(ws->smap, ws->smap_floats);
    A(ws->nms, ws->smap_floats);
    A(ws->rest, ws->smap_floats);
    A(ws->mask, ws->smap_floats);
    A(ws->supp, ws->smap_floats);
    A(ws->kpsel.n_cand, (sel_state_bytes((int)B) + 3) / 4);
    A(ws->kpsel.keys, ws->smap_floats);
    ws->kpsel.ties_cap = (size_t)B * (H8 + 32) * (W8 + 64);      // whole 32 x 64 tiles per image: the candidate staging of the last NMS round
    A(ws->kpsel.ties, ws->kpsel.ties_cap);
    A(ws->kpsel.chosen, (size_t)B * K);
    // matcher buffers: NP pairs = 2 NP images side by side (batch over pairs: one launch serves every pair)
    const size_t NP = (size_t)(B + 1) / 2, NI = 2 * NP;
    for (int i = 0; i < 2; ++i) {
        A(ws->x[i], NI * K * 256);
        A(ws->cs[i], NI * K * 32);
        A(ws->sn[i], NI * K * 32);
        A(ws->ind[i], NI * K);
    }
    A(ws->q, NI * K * 256); A(ws->k, NI * K * 256); A(ws->v, NI * K * 256);
    A(ws->att, NI * K * 256); A(ws->msg, NI * K * 256); A(ws->h, NI * K * 512);
    A(ws->attn_part, attn_part_floats((int)K, (int)NI, 4)); A(ws->attn_cnt, attn_counter_ints((int)K, (int)NI, 4));
    A(ws->attn_planes, attn_planes_bytes((int)K, (int)NI, 4));
    A(ws->conf, NI * K); A(ws->msc, NI * K); A(ws->keep_idx, NI * K); A(ws->prune, NI * K);
    A(ws->md, NI * K * 256); A(ws->z, NI * K); A(ws->lz, NI * K);
    ws->sim_ps = (((size_t)K * K + (size_t)K + 4) + 3) & ~(size_t)3;     // floats between the score matrices of consecutive pairs
    ws->vec_ps = ((size_t)K + 4 + 3) & ~(size_t)3;
    ws->part_ps = (size_t)((K + 15) / 16 + 1) * (K + 4);
    A(ws->sim, NP * ws->sim_ps + (size_t)K + 8);
    A(ws->sim2, (size_t)1);
    A(ws->rmax, NP * ws->vec_ps); A(ws->rlog, NP * ws->vec_ps); A(ws->cmax, NP * ws->vec_ps); A(ws->clog, NP * ws->vec_ps);
    A(ws->part, NP * ws->part_ps);
    A(ws->ridx, NP * ws->vec_ps); A(ws->rval, NP * ws->vec_ps); A(ws->cbest, NP * ws->vec_ps);
    A(ws->st, NP); A(ws->sel, NP + 3);
    A(ws->uv, (size_t)4 * (K + 8));
#undef A
    ws->n_pairs = (int)NP;
    if (!ok) {
        for (void* p : ws->allocs) ctx->gfree(p);
        delete ws;
        ctx->max_h = ctx->max_w = ctx->max_images = ctx->max_kpts = 0;   // no workspace any more: the next call starts from its own sizes
        return ctx->fail(-31, "im_ctx_reserve: out of device memory (%d x %d, %d images, %d keypoints)", max_h, max_w, max_images, max_kpts);
    }
    ctx->ws = ws;
    ctx->max_h = max_h; ctx->max_w = max_w; ctx->max_images = max_images; ctx->max_kpts = max_kpts;
    IM_HIP(ctx, hipMemset(ws->st, 0, sizeof(LGState) * NP));
    IM_HIP(ctx, hipMemset(ws->sel, 0, (NP + 3) * sizeof(int)));
    IM_HIP(ctx, hipMemset(ws->attn_cnt, 0, attn_counter_ints((int)K, (int)NI, 4) * sizeof(int)));
    IM_HIP(ctx, hipDeviceSynchronize());
    return 0;
}

// ------------------------------------------------------------------------------------------------ profiler
int im_profile_begin(im_ctx* ctx) {
    IM_CHECK_CTX(ctx);
    IM_HIP(ctx, hipDeviceSynchronize());
    for (auto& e : ctx->prof) { ctx->prof_pool.push_back(e.e0); ctx->prof_pool.push_back(e.e1); }
    ctx->prof.clear();
    ctx->prof_on = true;
    return 0;
}

// Writes {"name": {"count": n, "total_ms": t}, ...} (aggregated over the launches since im_profile_begin).
int im_profile_end(im_ctx* ctx, char* buf, size_t cap) {
    IM_CHECK_CTX(ctx);
    ctx->prof_on = false;
    // calibration: an event pair with nothing in between still reads a few microseconds (each record is a packet the
    // command processor has to retire); measured here on the same stream and reported as "_empty_event_pair" so that
    // the caller can subtract it per launch
    constexpr int NCAL = 32;
    hipEvent_t cal[2 * NCAL];
    for (int i = 0; i < NCAL; ++i) {
        cal[2 * i] = ctx->prof_event(); cal[2 * i + 1] = ctx->prof_event();
        hipEventRecord(cal[2 * i], ctx->prof_stream);
        hipEventRecord(cal[2 * i + 1], ctx->prof_stream);
    }
    IM_HIP(ctx, hipDeviceSynchronize());
    std::map<std::string, std::pair<int, double>> agg;
    for (int i = 0; i < NCAL; ++i) {
        float ms = 0.f;
        if (hipEventElapsedTime(&ms, cal[2 * i], cal[2 * i + 1]) == hipSuccess) { agg["_empty_event_pair"].first += 1; agg["_empty_event_pair"].second += ms; }
        ctx->prof_pool.push_back(cal[2 * i]); ctx->prof_pool.push_back(cal[2 * i + 1]);
    }
    for (auto& e : ctx->prof) {
        float ms = 0.f;
        IM_HIP(ctx, hipEventElapsedTime(&ms, e.e0, e.e1));
        auto& a = agg[e.name];
        a.first += 1;
        a.second += ms;
    }
    std::string out = "{";
    bool first = true;
    for (auto& kv : agg) {
        char line[256];
        snprintf(line, sizeof(line), "%s\"%s\": {\"count\": %d, \"total_ms\": %.6f}", first ? "" : ", ", kv.first.c_str(),
                 kv.second.first, kv.second.second);
        out += line;
        first = false;
    }
    out += "}";
    if (!buf || out.size() + 1 > cap) return ctx->fail(-60, "im_profile_end: buffer too small (%zu needed)", out.size() + 1);
    memcpy(buf, out.c_str(), out.size() + 1);
    return 0;
}

// ------------------------------------------------------------------------------------------------ debug reads
// Copies an internal buffer of the last forward to d_dst (stage-level parity tests). Names: "lg_x" (descriptors after the
// last executed layer, [2][K][256]), "lg_cos" / "lg_sin" (rotary tables [2][K][32]), "sim" ([K][K] score matrix),
// "md" (projected matching descriptors [2][K][256]), "sp_smap" / "sp_nms" (SuperPoint score map before / after simple_nms of
// the last im_superpoint_forward, [n_images][H8][W8] densely packed for that call's size). Of the last assignment stage, pair 0, as
// raw 32-bit words: "rmax" / "rlog" / "cmax" / "clog" / "rval" (floats) and "ridx" (int32), one per row or column; "cbest" (the 64-bit
// column keys f2ord(score) << 32 | ~row, two words per column, low word first); "lz" (log-sigmoid certainties [2][K]). Of SuperGlue's
// Sinkhorn potentials: "u" (rows, then the dustbin), "v" (columns, then the dustbin; it starts (K + 4) & ~3 floats into the buffer)
// and "norm" (one float). Synchronises the stream.
int im_debug_read(im_ctx* ctx, const char* name, float* d_dst, size_t nfloats, void* stream) {
    IM_CHECK_CTX(ctx);
    Workspace* ws = ctx->ws;
    if (!ws || !name) return ctx->fail(-51, "im_debug_read: no workspace");
    const size_t K = (size_t)ctx->max_kpts;
    const std::string nm = name;
    const float* src = nullptr;
    size_t avail = 0;
    if (nm == "lg_x") { src = ws->x[ctx->dbg_cur]; avail = 2 * K * 256; }
    else if (nm == "lg_cos") { src = ws->cs[ctx->dbg_cur]; avail = 2 * K * 32; }
    else if (nm == "lg_sin") { src = ws->sn[ctx->dbg_cur]; avail = 2 * K * 32; }
    else if (nm == "sim") { src = ws->sim; avail = K * K; }   // pair 0
    else if (nm == "md") { src = ws->md; avail = 2 * K * 256; }
    else if (nm == "sp_smap") { src = ws->smap; avail = ws->smap_floats; }
    else if (nm == "sp_nms") { src = ws->nms; avail = ws->smap_floats; }
    else if (nm == "rmax") { src = ws->rmax; avail = ws->vec_ps; }
    else if (nm == "rlog") { src = ws->rlog; avail = ws->vec_ps; }
    else if (nm == "cmax") { src = ws->cmax; avail = ws->vec_ps; }
    else if (nm == "clog") { src = ws->clog; avail = ws->vec_ps; }
    else if (nm == "rval") { src = ws->rval; avail = ws->vec_ps; }
    else if (nm == "ridx") { src = reinterpret_cast<const float*>(ws->ridx); avail = ws->vec_ps; }
    else if (nm == "cbest") { src = reinterpret_cast<const float*>(ws->cbest); avail = 2 * ws->vec_ps; }
    else if (nm == "lz") { src = ws->lz; avail = 2 * K; }
    else if (nm == "u" || nm == "v" || nm == "norm") {
        const size_t voff = (K + 4) & ~(size_t)3;      // as im_superglue_forward lays ws->uv out
        src = ws->uv + (nm == "u" ? 0 : nm == "v" ? voff : 2 * voff);
        avail = nm == "norm" ? 1 : K + 1;
    }
    else return ctx->fail(-61, "im_debug_read: unknown buffer '%s'", name);
    if (nfloats > avail) return ctx->fail(-62, "im_debug_read: %zu floats requested, %zu available", nfloats, avail);
    IM_HIP(ctx, hipMemcpyAsync(d_dst, src, nfloats * sizeof(float), hipMemcpyDeviceToDevice, (hipStream_t)stream));
    IM_HIP(ctx, hipStreamSynchronize((hipStream_t)stream));
    return 0;
}

// Sustained shader clock of the two matrix-core kernel classes: arm = 1 allocates / clears the probe words and hands them to
// every attention (attention_bx.hip) and Winograd BX (conv_wino.hip) launch of this context until arm = 0; the kernels' first wave stores the
// shader cycles (s_memtime) and the 100 MHz reference ticks (s_memrealtime) spent in its main loop. Reading (arm = 0 or 2): the median over the
// blocks that wrote of cycles / ticks x 100 MHz, per class; h_out = {attention MHz, attention blocks, convolution MHz, convolution blocks}.
int im_debug_clock_probe(im_ctx* ctx, int arm, double* h_out, void* stream) {
    IM_CHECK_CTX(ctx);
    hipStream_t s = (hipStream_t)stream;
    const size_t bytes = (size_t)CLOCK_PROBE_SLOTS * 2 * sizeof(unsigned long long);
    if (arm == 1) {
        IM_GROW(ctx, ctx->grow(ctx->scratch.clock[0], bytes, "clock_probe_attention"), -22, "im_debug_clock_probe: allocation failed");
        IM_GROW(ctx, ctx->grow(ctx->scratch.clock[1], bytes, "clock_probe_convolution"), -22, "im_debug_clock_probe: allocation failed");
        IM_HIP(ctx, hipMemsetAsync(ctx->scratch.clock[0].p, 0, bytes, s));
        IM_HIP(ctx, hipMemsetAsync(ctx->scratch.clock[1].p, 0, bytes, s));
        IM_HIP(ctx, hipStreamSynchronize(s));
        ctx->clock_armed = true;
        return 0;
    }
    if (!ctx->scratch.clock[0].p || !h_out) return ctx->fail(-51, "im_debug_clock_probe: not armed");
    std::vector<unsigned long long> h((size_t)CLOCK_PROBE_SLOTS * 2);
    const void* src[2] = {ctx->scratch.clock[0].p, ctx->scratch.clock[1].p};
    for (int c = 0; c < 2; ++c) {
        IM_HIP(ctx, hipMemcpyAsync(h.data(), src[c], bytes, hipMemcpyDeviceToHost, s));
        IM_HIP(ctx, hipStreamSynchronize(s));
        std::vector<double> mhz;
        for (int i = 0; i < CLOCK_PROBE_SLOTS; ++i)
            if (h[2 * i + 1] > 0) mhz.push_back(100.0 * (double)h[2 * i] / (double)h[2 * i + 1]);
        std::sort(mhz.begin(), mhz.end());
        h_out[2 * c] = mhz.empty() ? 0.0 : mhz[mhz.size() / 2];
        h_out[2 * c + 1] = (double)mhz.size();
    }
    if (arm == 0) ctx->clock_armed = false;       // the buffers stay with the context (a graph captured while armed keeps writing into them, harmlessly)
    return 0;
}

// ------------------------------------------------------------------------------------------------ stage entry points
int im_gemm_nt(im_ctx* ctx, const float* d_a, const float* d_w, const float* d_bias, float* d_c, int m, int n, int k,
               float alpha, int big_tile, void* stream) {
    IM_CHECK_CTX(ctx);
    GemmArgs g;
    g.A = d_a; g.lda = k; g.W = d_w; g.ldw = k; g.bias = d_bias; g.N = n; g.K = k; g.m_max = m;
    g.C = d_c; g.ldc = n; g.alpha = alpha; g.epi = EPI_BIAS; g.big_tile = big_tile & 1; g.bx = (big_tile >> 1) & 1;
    IM_HIP(ctx, launch_gemm(g, (hipStream_t)stream));
    return 0;
}

int im_ffn_fused(im_ctx* ctx, int act, float* d_x, const float* d_att, const float* h_w0, const float* h_b0, const float* h_ln_g,
                   const float* h_ln_b, const float* h_w3, const float* h_b3, int n_images, int n_rows, const int32_t* d_n, void* stream) {
    IM_CHECK_CTX(ctx);
    if (n_images < 1 || n_rows < 1 || act < 0 || act > 1 || (act == 0 && (!h_ln_g || !h_ln_b))) return ctx->fail(-12, "im_ffn_fused: bad arguments");
    if (act == 1) h_ln_g = h_ln_b = h_b0;   // unused by the ReLU form
    const std::vector<float> p0 = pack_frag_weights(h_w0, 512, 512), p3 = pack_frag_weights(h_w3, 256, 512);
    const size_t sizes[6] = {p0.size(), 512, 512, 512, p3.size(), 256};
    const float* src[6] = {p0.data(), h_b0, h_ln_g, h_ln_b, p3.data(), h_b3};
    hipStream_t st = (hipStream_t)stream;
    IM_HIP(ctx, with_uploads(src, sizes, st, [&](float* const* d) {
        FfnArgs f;
        f.act = act; f.x = d_x; f.x_bstride = (long)n_rows * 256; f.att = d_att; f.att_bstride = (long)n_rows * 256;
        f.w0p = d[0]; f.b0 = d[1]; f.ln_g = d[2]; f.ln_b = d[3]; f.w3p = d[4]; f.b3 = d[5];
        f.m_max = n_rows; f.batch = n_images; f.m_ptr = d_n; f.pstride = 2;
        return ctx->timed("ffn_fused", st, [&] { return launch_ffn_fused(f, st); });
    }));
    return 0;
}

static int conv3x3_entry(im_ctx* ctx, bool wino, const float* d_in, const float* h_weight, const float* h_bias, float* d_out,
                         int b, int h, int w, int cin, int cout, int relu, int pool, void* stream) {
    IM_CHECK_CTX(ctx);
    if (cin % 16 || cout % 64) return ctx->fail(-10, "im_conv3x3: cin %% 16 and cout %% 64 must be 0");
    std::vector<float> packed = wino ? pack_conv3x3_wino(h_weight, cout, cin) : pack_conv3x3(h_weight, cout, cin);
    std::vector<float> planes = wino ? pack_conv3x3_wino_bx(h_weight, cout, cin) : std::vector<float>(1);   // the product form of the Winograd layer (IM_CONV_F32=1: the f32-input form)
    const size_t sizes[3] = {packed.size(), (size_t)cout, planes.size()};
    const float* src[3] = {packed.data(), h_bias, planes.data()};
    hipStream_t st = (hipStream_t)stream;
    IM_HIP(ctx, with_uploads(src, sizes, st, [&](float* const* d) {
        ConvArgs a;
        a.in = d_in; a.w = d[0]; a.bias = d[1]; a.out = d_out; a.B = b; a.H = h; a.W = w; a.Cin = cin; a.Cout = cout;
        a.relu = relu; a.pool = pool;
        if (wino) a.wx = d[2];
        return ctx->timed(wino ? "conv_wino" : "conv_direct", st, [&] { return wino ? launch_conv3x3_wino(a, st) : launch_conv3x3(a, st); });
    }));
    return 0;
}

int im_conv3x3(im_ctx* ctx, const float* d_in, const float* h_weight, const float* h_bias, float* d_out, int b, int h,
               int w, int cin, int cout, int relu, int pool, void* stream) {
    return conv3x3_entry(ctx, false, d_in, h_weight, h_bias, d_out, b, h, w, cin, cout, relu, pool, stream);
}

int im_conv3x3_winograd(im_ctx* ctx, const float* d_in, const float* h_weight, const float* h_bias, float* d_out, int b,
                        int h, int w, int cin, int cout, int relu, int pool, void* stream) {
    return conv3x3_entry(ctx, true, d_in, h_weight, h_bias, d_out, b, h, w, cin, cout, relu, pool, stream);
}

int im_flash_attn(im_ctx* ctx, const float* d_q, const float* d_k, const float* d_v, float* d_out, const int32_t* d_n,
                  int n_max, int batch, int heads, int cross, float scale, void* stream) {
    IM_CHECK_CTX(ctx);
    AttnArgs a;
    a.q = d_q; a.k = d_k; a.v = d_v; a.hstride = (long)n_max * 64; a.bstride = a.hstride * heads;
    a.out = d_out; a.ldo = heads * 64; a.out_bstride = (long)n_max * a.ldo;
    a.n_ptr = d_n; a.n_max = n_max; a.batch = batch; a.heads = heads; a.cross = cross & 1; a.f32_form = (cross >> 1) & 1; a.scale = scale;
    // split-KV scratch of the stage entry point (the model paths use the reserved workspace). Each of the three grows on its own (ADVICE r05:
    // growing both when either was short re-allocated on alternating shapes, and the planes were grown for calls that do not use them)
    im_ctx::StageScratch& sc = ctx->scratch;
    const bool wants_planes = !(cross & 4) && !a.f32_form;      // bit 2: K / V cut inside the attention kernel; the f32 form has no planes
    IM_GROW(ctx, ctx->grow(sc.attn_part, attn_part_floats(n_max, batch, heads) * sizeof(float), "stage_attn_part"), -11, "im_flash_attn: out of device memory");
    // the counters reset themselves, so only a new buffer needs zeroing - before it becomes the context's
    IM_GROW(ctx, ctx->grow(sc.attn_cnt, attn_counter_ints(n_max, batch, heads) * sizeof(int), "stage_attn_cnt", true), -11, "im_flash_attn: out of device memory");
    if (wants_planes) IM_GROW(ctx, ctx->grow(sc.attn_planes, attn_planes_bytes(n_max, batch, heads), "stage_attn_planes"), -11, "im_flash_attn: out of device memory");
    a.part = sc.attn_part.as<float>(); a.counters = sc.attn_cnt.as<int>(); a.planes = wants_planes ? sc.attn_planes.as<unsigned char>() : nullptr;
    IM_HIP(ctx, launch_attn_planes(a, (hipStream_t)stream));
    IM_HIP(ctx, launch_flash_attn(a, (hipStream_t)stream));
    IM_GUARD_CHECK(ctx, (hipStream_t)stream, "im_flash_attn");
    return 0;
}

int im_block_proj_attn(im_ctx* ctx, int cross, const float* d_x, const float* h_w, const float* h_bias, const float* d_cs, const float* d_sn, float alpha,
                       const int32_t* d_n, const int32_t* d_active, int n_pairs, int n_max, float* d_q, float* d_k, float* d_v, void* d_planes,
                       float* d_att, float scale, void* stream) {
    IM_CHECK_CTX(ctx);
    if (n_pairs < 1 || n_max < 1 || !d_x || !h_w || !h_bias || !d_q || !d_k || !d_v || !d_planes) return ctx->fail(-12, "im_block_proj_attn: bad arguments");
    const int N = cross ? 512 : 768, NI = 2 * n_pairs;
    const std::vector<float> packed = pack_frag_weights(h_w, N, 256);
    const size_t sizes[3] = {(size_t)N * 256, packed.size(), (size_t)N};
    const float* src[3] = {h_w, packed.data(), h_bias};
    hipStream_t st = (hipStream_t)stream;
    int rc = 0;
    IM_HIP(ctx, with_uploads(src, sizes, st, [&](float* const* d) {
        GemmArgs g;       // as lg_block builds them (lightglue.hip)
        g.m_max = n_max; g.m_ptr = d_n; g.active = d_active; g.pstride = 2; g.batch = NI; g.bx = 1; g.big_tile = NI >= 4;
        g.A = d_x; g.a_bstride = (long)n_max * 256; g.lda = 256; g.ldw = 256; g.K = 256; g.W = d[0]; g.bias = d[2]; g.N = N;
        g.q = d_q; g.v = d_v; g.head_bstride = (long)n_max * 256; g.head_stride = (long)n_max * 64;
        if (!cross) { g.epi = EPI_QKV_ROPE; g.k = d_k; g.cs = d_cs; g.sn = d_sn; g.enc_bstride = (long)n_max * 32; }
        else { g.epi = EPI_HEADS_QV; g.alpha = alpha; }
        AttnArgs at;
        at.q = d_q; at.k = cross ? d_q : d_k; at.v = d_v; at.hstride = (long)n_max * 64; at.bstride = (long)n_max * 256;
        at.out = d_att; at.out_bstride = (long)n_max * 256; at.ldo = 256; at.n_ptr = d_n; at.pstride = 2; at.n_max = n_max; at.batch = NI; at.heads = 4;
        at.cross = cross ? 1 : 0; at.active = d_active; at.planes = d_planes; at.scale = scale;
        bool planes_done = false;
        rc = launch_block_proj(ctx, st, "block_proj", g, d[1], 0, at, &planes_done);
        if (rc) return hipSuccess;
        if (!planes_done)
            if (hipError_t e = launch_attn_planes(at, st); e != hipSuccess) return e;
        return d_att ? launch_flash_attn(at, st) : hipSuccess;
    }));
    if (rc) return rc;
    IM_GUARD_CHECK(ctx, st, "im_block_proj_attn");
    return 0;
}

int im_nms(im_ctx* ctx, const float* d_scores, float* d_out, int n_images, int h, int w, int radius, void* stream) {
    IM_CHECK_CTX(ctx);
    Workspace* ws = ctx->ws;
    if (!ws || (long)n_images * h * w > (long)ws->smap_floats)
        return ctx->fail(-41, "im_nms: exceeds the reserved workspace");
    IM_HIP(ctx, launch_nms(d_scores, d_out, ws->mask, ws->supp, ws->rest, n_images, h, w, radius, (hipStream_t)stream));
    IM_GUARD_CHECK(ctx, (hipStream_t)stream, "im_nms");
    return 0;
}

int im_select_topk(im_ctx* ctx, const float* d_nms, int n_images, int h, int w, int border, float threshold, int max_kpts,
                   float* d_kpts, float* d_scores, int32_t* d_n, void* stream) {
    IM_CHECK_CTX(ctx);
    Workspace* ws = ctx->ws;
    if (!ws || (long)n_images * h * w > (long)ws->smap_floats)
        return ctx->fail(-41, "im_select_topk: exceeds the reserved workspace");
    IM_HIP(ctx, launch_select_topk(d_nms, n_images, h, w, border, threshold, max_kpts, ctx->max_kpts, ws->kpsel, d_kpts, d_scores, d_n,
                                   (hipStream_t)stream));
    IM_GUARD_CHECK(ctx, (hipStream_t)stream, "im_select_topk");
    return 0;
}

int im_sample_descriptors(im_ctx* ctx, const float* d_dense_raw, int n_images, int hc, int wc, const float* d_kpts,
                          const int32_t* d_n, float* d_desc, void* stream) {
    IM_CHECK_CTX(ctx);
    if (!ctx->ws) return ctx->fail(-51, "im_sample_descriptors: call im_ctx_reserve first");
    IM_HIP(ctx, launch_sample_desc(d_dense_raw, n_images, hc, wc, d_kpts, d_n, ctx->max_kpts, d_desc, (hipStream_t)stream));
    return 0;
}

int im_assign_from_sim(im_ctx* ctx, const float* d_sim, int m, int n, int ld, const float* d_z0, const float* d_z1,
                       float threshold, int32_t* d_m0, int32_t* d_m1, float* d_ms0, float* d_ms1, void* stream) {
    IM_CHECK_CTX(ctx);
    Workspace* ws = ctx->ws;
    const int K = ctx->max_kpts;
    if (!ws || m > K || n > K || m < 1 || n < 1) return ctx->fail(-41, "im_assign_from_sim: m, n must be 1..max_kpts");
    hipStream_t s = (hipStream_t)stream;
    // reuse the matcher state as the (m, n) holder
    const int mn[2] = {m, n};
    IM_HIP(ctx, hipMemcpyAsync(ws->st->n, mn, sizeof(mn), hipMemcpyHostToDevice, s));
    IM_HIP(ctx, hipStreamSynchronize(s));
    IM_HIP(ctx, hipMemcpyAsync(ws->z, d_z0, sizeof(float) * m, hipMemcpyDeviceToDevice, s));
    IM_HIP(ctx, hipMemcpyAsync(ws->z + K, d_z1, sizeof(float) * n, hipMemcpyDeviceToDevice, s));
    IM_HIP(ctx, launch_logsig(ws->z, K, ws->st, 2, K, ws->lz, s));
    AssignArgs a;
    a.sim = d_sim; a.ld = ld; a.m_ptr = &ws->st->n[0]; a.n_ptr = &ws->st->n[1]; a.m_max = m; a.n_max = n;
    a.lz0 = ws->lz; a.lz1 = ws->lz + K;
    a.rmax = ws->rmax; a.rlog = ws->rlog; a.cmax = ws->cmax; a.clog = ws->clog; a.part = ws->part;
    a.ridx = ws->ridx; a.rval = ws->rval; a.cbest = ws->cbest; a.threshold = threshold;
    a.out_m0 = d_m0; a.out_m1 = d_m1; a.out_s0 = d_ms0; a.out_s1 = d_ms1;
    a.n_pairs = 1;
    IM_HIP(ctx, launch_assign(a, s));
    IM_GUARD_CHECK(ctx, s, "im_assign_from_sim");
    return 0;
}

}  // extern "C"
