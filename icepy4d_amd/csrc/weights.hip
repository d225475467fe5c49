// Host-side weight handling: tensors arrive under their official state-dict key names (im_set_tensor),
// im_finalize_weights re-packs them for the kernels and uploads.
#include <cmath>
#include <cstring>
#include <string>

#include "bf16x3.h"
#include "ctx.h"

namespace im {

std::vector<float> pack_conv3x3(const float* w, int cout, int cin) {
    std::vector<float> p((size_t)cin * 9 * cout);
    for (int co = 0; co < cout; ++co)
        for (int ci = 0; ci < cin; ++ci)
            for (int tap = 0; tap < 9; ++tap)
                p[(((size_t)(ci / 16) * 9 + tap) * cout + co) * 16 + (ci % 16)] = w[((size_t)co * cin + ci) * 9 + tap];
    return p;
}

// U = G g G^T per (cout, cin), evaluated in double and rounded once; layout [cin/8][pos = 4 xi + nu][cout][cin % 8]
std::vector<float> pack_conv3x3_wino(const float* w, int cout, int cin) {
    static const double G[4][3] = {{1, 0, 0}, {0.5, 0.5, 0.5}, {0.5, -0.5, 0.5}, {0, 0, 1}};
    std::vector<float> p((size_t)cin * 16 * cout);
    for (int co = 0; co < cout; ++co)
        for (int ci = 0; ci < cin; ++ci) {
            const float* g = w + ((size_t)co * cin + ci) * 9;
            double t[4][3];
            for (int i = 0; i < 4; ++i)
                for (int j = 0; j < 3; ++j) t[i][j] = G[i][0] * g[0 * 3 + j] + G[i][1] * g[1 * 3 + j] + G[i][2] * g[2 * 3 + j];
            for (int i = 0; i < 4; ++i)
                for (int j = 0; j < 4; ++j) {
                    const double u = t[i][0] * G[j][0] + t[i][1] * G[j][1] + t[i][2] * G[j][2];
                    p[(((size_t)(ci / 8) * 16 + (i * 4 + j)) * cout + co) * 8 + (ci % 8)] = (float)u;
                }
        }
    return p;
}

// The same U values (pack_conv3x3_wino's: evaluated in double, rounded once to fp32) cut into three bf16 planes (bf16x3.h::cut3), in the fragment order of v_mfma_f32_32x32x16_bf16's B
// operand: [cin / 16][pos][cout / 32][plane][lane = (cin % 16 / 8) * 32 + cout % 32][cin % 8] bf16 - one plane of one (position, 32 output
// channels, 16 input channels) fragment is 1 KB, lane-linear 16 bytes per lane. Returned as floats holding the bytes (for im_ctx::upload).
std::vector<float> pack_conv3x3_wino_bx(const float* w, int cout, int cin) {
    const std::vector<float> u = pack_conv3x3_wino(w, cout, cin);      // [cin/8][16][cout][8]
    const size_t n16 = (size_t)cin * 16 * cout * 3;
    std::vector<float> out((n16 + 1) / 2);
    uint16_t* p = reinterpret_cast<uint16_t*>(out.data());
    const int nct = cout / 32;
    for (int ci = 0; ci < cin; ++ci)
        for (int pos = 0; pos < 16; ++pos)
            for (int co = 0; co < cout; ++co) {
                const float x = u[(((size_t)(ci / 8) * 16 + pos) * cout + co) * 8 + (ci % 8)];
                uint16_t h, m, l;
                cut3(x, h, m, l);
                const int lane = ((ci % 16) / 8) * 32 + (co % 32);
                const size_t base = ((((size_t)(ci / 16) * 16 + pos) * nct + co / 32) * 3) * 512 + (size_t)lane * 8 + (ci % 8);
                p[base] = h; p[base + 512] = m; p[base + 1024] = l;
            }
    return out;
}

// per layer: fragment order for proj_rows_kernel / ffn_fused_kernel. `src` = [layers][n][k] row-major
std::vector<float> pack_layers(const std::vector<float>& src, int n, int k) {
    std::vector<float> packed;
    packed.reserve(src.size() * 3 / 2);
    for (size_t off = 0; off < src.size(); off += (size_t)n * k) {
        const std::vector<float> one = pack_frag_weights(&src[off], n, k);
        packed.insert(packed.end(), one.begin(), one.end());
    }
    return packed;
}

// The 256 -> 256 output projection of the attention (LightGlue out_proj / to_out, SuperGlue merge) feeds only the second half of the first
// feed-forward layer (`lightglue.py:160-162, 212-216`, `superglue.py:104-116`: the message is used only as its input), so it is folded
// into columns 256..511 of that layer: W0([x | Wo a + bo]) + b0 = W0a x + (W0b Wo) a + (W0b bo + b0). Products accumulated in double;
// one 256 -> 256 GEMM launch and the `message` round trip through HBM less per block. One layer: Wo [256][256], bo [256], w0 [512][512], b0 [512].
void fold_out_proj_into_ffn0(const float* Wo, const float* bo, float* w0, float* b0) {
    std::vector<double> row(256);
    for (int n = 0; n < 512; ++n) {
        float* w0r = w0 + (size_t)n * 512 + 256;
        double bacc = b0[n];
        for (int k = 0; k < 256; ++k) row[k] = 0.0;
        for (int j = 0; j < 256; ++j) {
            const double wj = w0r[j];
            const float* wor = Wo + (size_t)j * 256;
            for (int k = 0; k < 256; ++k) row[k] += wj * (double)wor[k];
            bacc += wj * (double)bo[j];
        }
        for (int k = 0; k < 256; ++k) w0r[k] = (float)row[k];
        b0[n] = (float)bacc;
    }
}

}  // namespace im

using namespace im;

// ------------------------------------------------------------------------------------------------ host tensors
static const std::vector<float>* find_w(im_ctx* ctx, const std::string& model, const std::string& key, size_t numel) {
    auto it = ctx->host_w.find(model + "/" + key);
    if (it == ctx->host_w.end()) {
        ctx->fail(-20, "weights: missing tensor %s of model %s", key.c_str(), model.c_str());
        return nullptr;
    }
    if (it->second.size() != numel) {
        ctx->fail(-21, "weights: tensor %s has %zu elements, expected %zu", key.c_str(), it->second.size(), numel);
        return nullptr;
    }
    return &it->second;
}

#define GETW(var, model, key, numel)                           \
    const std::vector<float>* var = find_w(ctx, model, key, numel); \
    if (!var) return -20

// dst = the tensors fmt % 0 .. fmt % (count - 1) one behind the other
static int cat_layers(im_ctx* ctx, const char* model, const std::string& fmt, size_t numel, int count, std::vector<float>& dst) {
    dst.clear();
    for (int i = 0; i < count; ++i) {
        char key[160];
        snprintf(key, sizeof(key), fmt.c_str(), i);
        GETW(t, model, key, numel);
        dst.insert(dst.end(), t->begin(), t->end());
    }
    return 0;
}

// ------------------------------------------------------------------------------------------------ SuperPoint
static int finalize_superpoint(im_ctx* ctx) {
    SuperPointW& w = ctx->sp;
    {
        GETW(cw, "superpoint", "conv1a.weight", 64 * 9);
        GETW(cb, "superpoint", "conv1a.bias", 64);
        std::vector<float> p(9 * 64);
        for (int co = 0; co < 64; ++co)
            for (int t = 0; t < 9; ++t) p[t * 64 + co] = (*cw)[co * 9 + t];
        w.c1a_w = ctx->upload(p);
        w.c1a_b = ctx->upload(*cb);
        // contraction index k of the matrix form: 0 = bias (times the in-image mask), 1 + t = tap t; lane half hh supplies k = 2 s + hh
        std::vector<float> pq(64 * 2 * 8, 0.f);
        for (int co = 0; co < 64; ++co)
            for (int k = 0; k < 10; ++k) pq[((size_t)co * 2 + (k & 1)) * 8 + (k >> 1)] = k == 0 ? (*cb)[co] : (*cw)[co * 9 + (k - 1)];
        w.c1a_wq = ctx->upload(pq);
    }
    for (int i = 0; SP_CONV3[i]; ++i) {
        const std::string nm = SP_CONV3[i];
        GETW(cw, "superpoint", nm + ".weight", (size_t)SP_COUT[i] * SP_CIN[i] * 9);
        GETW(cb, "superpoint", nm + ".bias", (size_t)SP_COUT[i]);
        w.cw[i] = ctx->upload(pack_conv3x3(cw->data(), SP_COUT[i], SP_CIN[i]));
        w.cww[i] = ctx->upload(pack_conv3x3_wino(cw->data(), SP_COUT[i], SP_CIN[i]));
        w.cwx[i] = ctx->upload(pack_conv3x3_wino_bx(cw->data(), SP_COUT[i], SP_CIN[i]));
        w.cb[i] = ctx->upload(*cb);
        if (!w.cw[i] || !w.cww[i] || !w.cwx[i] || !w.cb[i]) return ctx->fail(-22, "weights: upload failed");
    }
    GETW(pbw, "superpoint", "convPb.weight", 65 * 256);
    GETW(pbb, "superpoint", "convPb.bias", 65);
    GETW(dbw, "superpoint", "convDb.weight", 256 * 256);
    GETW(dbb, "superpoint", "convDb.bias", 256);
    w.pb_w = ctx->upload(*pbw); w.pb_b = ctx->upload(*pbb);
    w.db_w = ctx->upload(*dbw); w.db_b = ctx->upload(*dbb);
    if (!w.pb_w || !w.pb_b || !w.db_w || !w.db_b || !w.c1a_w || !w.c1a_b) return ctx->fail(-22, "weights: upload failed");
    w.ready = true;
    return 0;
}

// ------------------------------------------------------------------------------------------------ LightGlue
// the feed-forward of the self (attn = "self_attn", out = "out_proj") or cross ("cross_attn", "to_out") blocks of all layers
static int finalize_lightglue_ffn(im_ctx* ctx, int L, const std::string& attn, const char* out, LightGlueW::Ffn& f) {
    const std::string p = "transformers.%d." + attn + ".";
    std::vector<float> o_w, o_b, f_w, f_b, buf;
    if (cat_layers(ctx, "lightglue", p + out + ".weight", 256 * 256, L, o_w) || cat_layers(ctx, "lightglue", p + out + ".bias", 256, L, o_b) ||
        cat_layers(ctx, "lightglue", p + "ffn.0.weight", 512 * 512, L, f_w) || cat_layers(ctx, "lightglue", p + "ffn.0.bias", 512, L, f_b))
        return -20;
    for (int l = 0; l < L; ++l) fold_out_proj_into_ffn0(&o_w[(size_t)l * 65536], &o_b[(size_t)l * 256], &f_w[(size_t)l * 512 * 512], &f_b[(size_t)l * 512]);
    f.w0 = ctx->upload(f_w);
    f.b0 = ctx->upload(f_b);
    f.w0p = ctx->upload(pack_layers(f_w, 512, 512));
    if (!f.w0 || !f.b0 || !f.w0p) return -22;
    if (cat_layers(ctx, "lightglue", p + "ffn.1.weight", 512, L, buf)) return -20;
    f.ln_g = ctx->upload(buf);
    if (cat_layers(ctx, "lightglue", p + "ffn.1.bias", 512, L, buf)) return -20;
    f.ln_b = ctx->upload(buf);
    if (cat_layers(ctx, "lightglue", p + "ffn.3.weight", 256 * 512, L, buf)) return -20;
    f.w3 = ctx->upload(buf);
    f.w3p = ctx->upload(pack_layers(buf, 256, 512));
    if (cat_layers(ctx, "lightglue", p + "ffn.3.bias", 256, L, buf)) return -20;
    f.b3 = ctx->upload(buf);
    return (f.ln_g && f.ln_b && f.w3 && f.w3p && f.b3) ? 0 : -22;
}

static int finalize_lightglue(im_ctx* ctx) {
    LightGlueW& w = ctx->lg;
    const int L = 9;
    std::vector<float> buf;
#define CAT_UP(dstptr, fmt, numel, count)                               \
    if (cat_layers(ctx, "lightglue", fmt, numel, count, buf)) return -20; \
    dstptr = ctx->upload(buf);                                          \
    if (!dstptr) return ctx->fail(-22, "weights: upload failed")

    {
        GETW(wr, "lightglue", "posenc.Wr.weight", 64);
        w.wr = ctx->upload(*wr);
    }
    // Wqkv rows: original index head*192 + d*3 + which  ->  which*256 + head*64 + d  (`lightglue.py:155`)
    {
        std::vector<float> qw, qb, pw((size_t)L * 768 * 256), pb((size_t)L * 768);
        if (cat_layers(ctx, "lightglue", "transformers.%d.self_attn.Wqkv.weight", 768 * 256, L, qw)) return -20;
        if (cat_layers(ctx, "lightglue", "transformers.%d.self_attn.Wqkv.bias", 768, L, qb)) return -20;
        for (int l = 0; l < L; ++l)
            for (int h = 0; h < 4; ++h)
                for (int d = 0; d < 64; ++d)
                    for (int which = 0; which < 3; ++which) {
                        const int src = h * 192 + d * 3 + which, dst = which * 256 + h * 64 + d;
                        memcpy(&pw[((size_t)l * 768 + dst) * 256], &qw[((size_t)l * 768 + src) * 256], 256 * sizeof(float));
                        pb[(size_t)l * 768 + dst] = qb[(size_t)l * 768 + src];
                    }
        w.qkv_w = ctx->upload(pw);
        w.qkv_b = ctx->upload(pb);
        w.qkv_wp = ctx->upload(pack_layers(pw, 768, 256));
    }
    if (int rc = finalize_lightglue_ffn(ctx, L, "self_attn", "out_proj", w.self_ffn))
        return rc == -22 ? ctx->fail(rc, "weights: upload failed (self ffn)") : rc;
    {   // [to_qk ; to_v] as one 256 -> 512 projection
        std::vector<float> qw, qb, vw, vb, pw((size_t)L * 512 * 256), pb((size_t)L * 512);
        if (cat_layers(ctx, "lightglue", "transformers.%d.cross_attn.to_qk.weight", 256 * 256, L, qw) ||
            cat_layers(ctx, "lightglue", "transformers.%d.cross_attn.to_qk.bias", 256, L, qb) ||
            cat_layers(ctx, "lightglue", "transformers.%d.cross_attn.to_v.weight", 256 * 256, L, vw) ||
            cat_layers(ctx, "lightglue", "transformers.%d.cross_attn.to_v.bias", 256, L, vb))
            return -20;
        for (int l = 0; l < L; ++l) {
            memcpy(&pw[(size_t)l * 512 * 256], &qw[(size_t)l * 65536], 65536 * sizeof(float));
            memcpy(&pw[(size_t)l * 512 * 256 + 65536], &vw[(size_t)l * 65536], 65536 * sizeof(float));
            memcpy(&pb[(size_t)l * 512], &qb[(size_t)l * 256], 256 * sizeof(float));
            memcpy(&pb[(size_t)l * 512 + 256], &vb[(size_t)l * 256], 256 * sizeof(float));
        }
        w.cqv_w = ctx->upload(pw);
        w.cqv_b = ctx->upload(pb);
        w.cqv_wp = ctx->upload(pack_layers(pw, 512, 256));
        if (!w.cqv_w || !w.cqv_b || !w.cqv_wp) return ctx->fail(-22, "weights: upload failed");
    }
    if (int rc = finalize_lightglue_ffn(ctx, L, "cross_attn", "to_out", w.cross_ffn))
        return rc == -22 ? ctx->fail(rc, "weights: upload failed (cross ffn)") : rc;
    CAT_UP(w.fp_w, "log_assignment.%d.final_proj.weight", 256 * 256, L);
    CAT_UP(w.fp_b, "log_assignment.%d.final_proj.bias", 256, L);
    CAT_UP(w.ma_w, "log_assignment.%d.matchability.weight", 256, L);
    CAT_UP(w.ma_b, "log_assignment.%d.matchability.bias", 1, L);
    CAT_UP(w.tc_w, "token_confidence.%d.token.0.weight", 256, L - 1);
    CAT_UP(w.tc_b, "token_confidence.%d.token.0.bias", 1, L - 1);
#undef CAT_UP
    if (ctx->host_w.count("lightglue/confidence_thresholds")) {
        GETW(thr, "lightglue", "confidence_thresholds", (size_t)L);
        for (int i = 0; i < L; ++i) w.thr[i] = (*thr)[i];
    } else {
        // a registered buffer the reference computes in __init__ and loads with strict=False (`lightglue.py:371-373, 392,
        // 558-561`): absent from a checkpoint saved without buffers. Same formula, double -> float32.
        for (int i = 0; i < L; ++i) {
            double t = 0.8 + 0.1 * std::exp(-4.0 * i / L);
            w.thr[i] = (float)(t < 0.0 ? 0.0 : (t > 1.0 ? 1.0 : t));
        }
    }
    if (!w.wr || !w.qkv_w || !w.qkv_b || !w.qkv_wp) return ctx->fail(-22, "weights: upload failed");
    w.ready = true;
    return 0;
}

// ------------------------------------------------------------------------------------------------ SuperGlue
// SuperGlue's head layout (channel c = d * 4 + head, `view(b, 64, 4, N)` `superglue.py:111-114`) is absorbed into the packed weights:
// projection rows and merge columns are permuted to head-major. BatchNorm (eval) is folded into the preceding 1x1 convolution.

// fold eval-mode BatchNorm1d (eps 1e-5) into the preceding 1x1 conv: y = g (Wx + b - mean) / sqrt(var + eps) + beta
static int fold_bn(im_ctx* ctx, const std::string& bn, int c, int in, std::vector<float>& w, std::vector<float>& b) {
    GETW(g, "superglue", bn + ".weight", c);
    GETW(be, "superglue", bn + ".bias", c);
    GETW(mu, "superglue", bn + ".running_mean", c);
    GETW(var, "superglue", bn + ".running_var", c);
    for (int o = 0; o < c; ++o) {
        const float sc = (*g)[o] / std::sqrt((*var)[o] + 1e-5f);
        for (int i = 0; i < in; ++i) w[(size_t)o * in + i] *= sc;
        b[o] = (b[o] - (*mu)[o]) * sc + (*be)[o];
    }
    return 0;
}

static int finalize_superglue(im_ctx* ctx) {
    SuperGlueW& W = ctx->sg;
    static const int dims[6] = {3, 32, 64, 128, 256, 256};
    for (int l = 0; l < 5; ++l) {
        const int in = dims[l], out = dims[l + 1], inp = l == 0 ? 32 : in;
        const std::string key = "kenc.encoder." + std::to_string(3 * l);
        GETW(w, "superglue", key + ".weight", (size_t)out * in);
        GETW(b, "superglue", key + ".bias", out);
        std::vector<float> ww(*w), bb(*b);
        if (l < 4 && fold_bn(ctx, "kenc.encoder." + std::to_string(3 * l + 1), out, in, ww, bb)) return -20;
        std::vector<float> wp((size_t)out * inp, 0.f);
        for (int o = 0; o < out; ++o)
            for (int i = 0; i < in; ++i) wp[(size_t)o * inp + i] = ww[(size_t)o * in + i];
        W.kenc_w[l] = ctx->upload(wp);
        W.kenc_b[l] = ctx->upload(bb);
    }
    const int L = 18;
    std::vector<float> qkv_w((size_t)L * 768 * 256), qkv_b((size_t)L * 768), mg_w(65536),
        m0_w((size_t)L * 512 * 512), m0_b((size_t)L * 512), m3_w((size_t)L * 256 * 512), m3_b((size_t)L * 256);
    for (int l = 0; l < L; ++l) {
        const std::string p = "gnn.layers." + std::to_string(l);
        for (int which = 0; which < 3; ++which) {
            GETW(w, "superglue", p + ".attn.proj." + std::to_string(which) + ".weight", 65536);
            GETW(b, "superglue", p + ".attn.proj." + std::to_string(which) + ".bias", 256);
            for (int h = 0; h < 4; ++h)
                for (int d = 0; d < 64; ++d) {
                    const int src = d * 4 + h, dst = which * 256 + h * 64 + d;
                    memcpy(&qkv_w[((size_t)l * 768 + dst) * 256], &(*w)[(size_t)src * 256], 256 * sizeof(float));
                    qkv_b[(size_t)l * 768 + dst] = (*b)[src];
                }
        }
        GETW(mw, "superglue", p + ".attn.merge.weight", 65536);
        GETW(mb, "superglue", p + ".attn.merge.bias", 256);
        for (int o = 0; o < 256; ++o)   // head-permuted merge weights [256 out][256 in (h * 64 + d)]
            for (int h = 0; h < 4; ++h)
                for (int d = 0; d < 64; ++d) mg_w[(size_t)o * 256 + h * 64 + d] = (*mw)[(size_t)o * 256 + d * 4 + h];
        GETW(w0, "superglue", p + ".mlp.0.weight", 512 * 512);
        GETW(b0, "superglue", p + ".mlp.0.bias", 512);
        GETW(w3, "superglue", p + ".mlp.3.weight", 256 * 512);
        GETW(b3, "superglue", p + ".mlp.3.bias", 256);
        std::vector<float> ww(*w0), bb(*b0);
        if (fold_bn(ctx, p + ".mlp.1", 512, 512, ww, bb)) return -20;
        fold_out_proj_into_ffn0(mg_w.data(), mb->data(), ww.data(), bb.data());   // `merge` into the (BatchNorm-folded) mlp.0
        memcpy(&m0_w[(size_t)l * 512 * 512], ww.data(), ww.size() * sizeof(float));
        memcpy(&m0_b[(size_t)l * 512], bb.data(), 512 * sizeof(float));
        memcpy(&m3_w[(size_t)l * 256 * 512], w3->data(), w3->size() * sizeof(float));
        memcpy(&m3_b[(size_t)l * 256], b3->data(), 256 * sizeof(float));
    }
    W.proj_w = ctx->upload(qkv_w); W.proj_b = ctx->upload(qkv_b);
    W.mlp0_w = ctx->upload(m0_w); W.mlp0_b = ctx->upload(m0_b);
    W.mlp3_w = ctx->upload(m3_w); W.mlp3_b = ctx->upload(m3_b);
    W.mlp0_wp = ctx->upload(pack_layers(m0_w, 512, 512));
    W.mlp3_wp = ctx->upload(pack_layers(m3_w, 256, 512));
    W.proj_wp = ctx->upload(pack_layers(qkv_w, 768, 256));
    if (!W.mlp0_wp || !W.mlp3_wp || !W.proj_wp) return ctx->fail(-22, "weights: upload failed");
    GETW(fw, "superglue", "final_proj.weight", 65536);
    GETW(fb, "superglue", "final_proj.bias", 256);
    GETW(bs, "superglue", "bin_score", 1);
    W.fp_w = ctx->upload(*fw); W.fp_b = ctx->upload(*fb);
    W.bin_score = (*bs)[0];
    if (!W.proj_w || !W.mlp0_w || !W.mlp3_w || !W.fp_w) return ctx->fail(-22, "weights: upload failed");
    W.ready = true;
    return 0;
}

// ------------------------------------------------------------------------------------------------ entry points
extern "C" {

int im_set_tensor(im_ctx* ctx, const char* model, const char* key, const float* h_data, size_t numel) {
    IM_CHECK_CTX(ctx);
    if (!model || !key || !h_data) return ctx->fail(-1, "im_set_tensor: null argument");
    ctx->host_w[std::string(model) + "/" + key].assign(h_data, h_data + numel);
    return 0;
}

int im_finalize_weights(im_ctx* ctx, const char* model) {
    IM_CHECK_CTX(ctx);
    const std::string m = model ? model : "";
    if (m != "superpoint" && m != "lightglue" && m != "superglue")
        return ctx->fail(-23, "im_finalize_weights: unknown model '%s'", m.c_str());
    IM_HIP(ctx, hipDeviceSynchronize());
    std::vector<void*>& mine = ctx->model_allocs[m];
    for (void* p : mine) ctx->gfree(p);   // a reload replaces the previous device copy of this model
    mine.clear();
    ctx->cur_model = &mine;
    int rc;
    if (m == "superpoint") rc = finalize_superpoint(ctx);
    else if (m == "lightglue") rc = finalize_lightglue(ctx);
    else rc = finalize_superglue(ctx);
    ctx->cur_model = nullptr;
    if (rc) return rc;
    IM_HIP(ctx, hipDeviceSynchronize());
    return 0;
}

}  // extern "C"
