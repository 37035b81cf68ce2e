// The frozen sentence-sentiment classifier of the RL rewards (sent_senti_cls.py:38-56 in eval mode), forward only:
// isc_sent_cls_fwd drives the library's own embed kernel, grouped GEMM and fused LSTM cell over a time-major workspace
// and adds the two kernels the library lacked - the squeeze-excite pooling and the k-way head with the reward rows.
#include <atomic>

#include "common.h"

static std::atomic<long long> g_sent_cls_launches{0};
extern "C" long long isc_sent_cls_launches(void) { return g_sent_cls_launches.load(); }

// ------------------------------------------------------------------ pooling
// One workgroup of four waves per caption.  Phase 1: wave v takes the steps t = v, v + 4, ... below the length; its 64
// lanes walk the H excitation outputs of (t, b) as float4, the lane sums are folded by the wave's butterfly - one fixed
// order - and w[t] = sum / H goes to LDS (the only thing phase 2 would otherwise have to re-read and re-reduce).
// Phase 2: thread x owns the float4 columns x, x + 256, ... of feats[b] and adds w[t] * out[t, b, :] for t ascending.
// Steps at or beyond the length are never loaded: what the LSTM wrote there cannot reach a sum.
__global__ __launch_bounds__(256) void sent_cls_pool_kernel(const float *e2, const float *out, const int32_t *lens,
                                                            int B, int L, int H, int T_out, float *weights,
                                                            float *feats) {
    extern __shared__ float w_lds[];                       // [L]
    const int b = blockIdx.x;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    int len = lens[b];
    len = len < 0 ? 0 : (len > L ? L : len);
    const int H4 = H >> 2;
    for (int t = wave; t < len; t += 4) {
        const float4 *row = reinterpret_cast<const float4 *>(e2 + ((long long)t * B + b) * H);
        float s = 0.f;
        for (int i = lane; i < H4; i += 64) {
            const float4 v = row[i];
            s += (1.f / (1.f + expf(-v.x)) + 1.f / (1.f + expf(-v.y))) +
                 (1.f / (1.f + expf(-v.z)) + 1.f / (1.f + expf(-v.w)));
        }
        s = wave_sum(s);
        if (lane == 0) w_lds[t] = s / (float)H;
    }
    __syncthreads();
    for (int t = threadIdx.x; t < T_out; t += 256) weights[(long long)b * T_out + t] = t < len ? w_lds[t] : 0.f;
    for (int i = threadIdx.x; i < H4; i += 256) {
        float4 acc = make_float4(0.f, 0.f, 0.f, 0.f);
        for (int t = 0; t < len; ++t) {
            const float w = w_lds[t];
            const float4 v = reinterpret_cast<const float4 *>(out + ((long long)t * B + b) * H)[i];
            acc.x += w * v.x; acc.y += w * v.y; acc.z += w * v.z; acc.w += w * v.w;
        }
        reinterpret_cast<float4 *>(feats + (long long)b * H)[i] = acc;
    }
}

// ------------------------------------------------------------------ head + reward
// The logits of one caption on one wave, and their arg-max (every lane returns the same values): the one place the head's
// summation order is written - the frozen forward's head and the training head (sent_cls_head_loss_kernel) share its bits.
__device__ __forceinline__ int sent_cls_logits_row(const float *hid, const float *Wc, const float *bc, long long b, int H,
                                                   int k, int lane, float (&z)[8]) {
    const int H4 = H >> 2;
    const float4 *x = reinterpret_cast<const float4 *>(hid + b * H);
    float acc[8];
#pragma unroll
    for (int j = 0; j < 8; ++j) acc[j] = 0.f;
    for (int i = lane; i < H4; i += 64) {
        const float4 v = x[i];
#pragma unroll
        for (int j = 0; j < 8; ++j)
            if (j < k) {
                const float4 w = reinterpret_cast<const float4 *>(Wc + (long long)j * H)[i];
                acc[j] += (v.x * w.x + v.y * w.y) + (v.z * w.z + v.w * w.w);
            }
    }
    float best = 0.f;
    int arg = 0;
#pragma unroll
    for (int j = 0; j < 8; ++j) {
        z[j] = 0.f;
        if (j < k) {
            const float s = wave_sum(acc[j]) + bc[j];
            z[j] = s;
            if (j == 0 || s > best) { best = s; arg = j; }
        }
    }
    return arg;
}

// One wave per caption: logits[b, j] = hid[b, :] . W[j, :] + bias[j] for the k <= 8 classes (lane l multiplies the float4
// columns l, l + 64, ... in ascending order, the butterfly folds the lanes: fixed order), arg-max with the lowest index on
// ties, and the caption's reward row = its weights row when the prediction equals the label, zeros otherwise (the weights
// row already carries the zeros behind the length and in the padding columns).
__global__ __launch_bounds__(256) void sent_cls_head_kernel(const float *hid, const float *Wc, const float *bc,
                                                            const int64_t *labels, const float *weights, int B, int H,
                                                            int k, int T_out, float *logits, int32_t *pred,
                                                            float *reward) {
    const int lane = threadIdx.x & 63;
    const int b = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (b >= B) return;
    float z[8];
    const int arg = sent_cls_logits_row(hid, Wc, bc, b, H, k, lane, z);
    if (lane == 0)
#pragma unroll
        for (int j = 0; j < 8; ++j)
            if (j < k) logits[(long long)b * k + j] = z[j];
    if (lane == 0) pred[b] = arg;
    if (reward) {
        const bool hit = (int64_t)arg == labels[b];
        for (int t = lane; t < T_out; t += 64)
            reward[(long long)b * T_out + t] = hit ? weights[(long long)b * T_out + t] : 0.f;
    }
}

// ------------------------------------------------------------------ driver
// Workspace, in floats (every block a multiple of 64 floats: 256-byte starts), time-major rows r = t * B + b:
//   x [L*B, W] | Xg [L*B, 4H] | out [L*B, H] | e1 [L*B, H] | e2 [L*B, H] | zero [B, H] | c [2, B, H] | feats [B, H] | hid [B, H]
namespace {
struct SentClsLayout {
    long long x, xg, out, e1, e2, zero, c, feats, hid, total;
};
long long up64(long long n) { return (n + 63) / 64 * 64; }
SentClsLayout sent_cls_layout(long long B, long long L, long long W, long long H) {
    SentClsLayout o;
    long long at = 0;
    o.x = at;     at += up64(L * B * W);
    o.xg = at;    at += up64(L * B * 4 * H);
    o.out = at;   at += up64(L * B * H);
    o.e1 = at;    at += up64(L * B * H);
    o.e2 = at;    at += up64(L * B * H);
    o.zero = at;  at += up64(B * H);
    o.c = at;     at += 2 * up64(B * H);
    o.feats = at; at += up64(B * H);
    o.hid = at;   at += up64(B * H);
    o.total = at;
    return o;
}
bool sent_cls_shape_ok(long long B, long long L, long long W, long long H) {
    return B >= 1 && L >= 1 && L <= 4096 && W >= 32 && H >= 32 && (W % 32) == 0 && (H % 32) == 0 &&
           L * B * 4 * H <= 0x7fffffffLL && L * B * W <= 0x7fffffffLL;      // (element counts of one tensor stay 32-bit)
}
isc_linear_problem sent_cls_linear(const float *A, int K, const float *Wt, const float *b0, const float *b1, int M, int N,
                                   int relu, float *C) {
    isc_linear_problem p = {};
    p.seg[0].A = A; p.seg[0].W = Wt; p.seg[0].lda = K; p.seg[0].ldw = K; p.seg[0].K = K;
    p.nseg = 1; p.M = M; p.N = N; p.relu = relu;
    p.bias0 = b0; p.bias1 = b1;
    p.mask_scale = 1.f; p.ldc = N; p.C = C;
    return p;
}
}  // namespace

extern "C" int64_t isc_sent_cls_workspace_bytes(int B, int L, int W, int H) {
    if (!sent_cls_shape_ok(B, L, W, H)) return 0;
    return sent_cls_layout(B, L, W, H).total * (int64_t)sizeof(float);
}

extern "C" int isc_sent_cls_fwd(const isc_sent_cls_problem *q, void *stream) {
    if (!q) return ISC_E_NULL;
    if (!q->tokens || !q->lens || !q->emb || !q->w_ih || !q->w_hh || !q->b_ih || !q->b_hh || !q->ex0_w || !q->ex0_b ||
        !q->ex2_w || !q->ex2_b || !q->cls0_w || !q->cls0_b || !q->cls3_w || !q->cls3_b || !q->workspace || !q->logits ||
        !q->weights || !q->pred)
        return ISC_E_NULL;
    if (q->reward && !q->labels) return ISC_E_NULL;
    const int B = q->B, L = q->L, W = q->W, H = q->H, k = q->k;
    if (!sent_cls_shape_ok(B, L, W, H) || q->V < 1 || k < 1 || k > 8 || q->T_out < L || q->tokens_ld < L)
        return ISC_E_SHAPE;
    const SentClsLayout lay = sent_cls_layout(B, L, W, H);
    if (q->workspace_bytes < lay.total * (int64_t)sizeof(float)) return ISC_E_WORKSPACE;
    if (!isc_aligned16(q->workspace) || !isc_aligned16(q->emb) || !isc_aligned16(q->cls3_w) ||
        (q->feats && !isc_aligned16(q->feats)))
        return ISC_E_ALIGN;
    hipStream_t st = (hipStream_t)stream;
    float *ws = static_cast<float *>(q->workspace);
    float *x = ws + lay.x, *xg = ws + lay.xg, *out = ws + lay.out, *e1 = ws + lay.e1, *e2 = ws + lay.e2;
    float *zero = ws + lay.zero, *c0 = ws + lay.c, *c1 = c0 + up64((long long)B * H);
    float *feats = q->feats ? q->feats : ws + lay.feats, *hid = ws + lay.hid;
    const int rows = L * B;
    long long launched = 0;

    // 1. x = relu(Emb[tokens]) for all L*B rows, time-major; the zero state (h and c in front of step 0) cleared
    int rc = isc_embed_relu_tm_(q->emb, q->V, W, q->tokens, q->tokens_ld, B, L, x, zero, (long long)B * H / 4, st);
    if (rc) return rc;
    ++launched;
    // 2. Xg = x W_ih^T + b_ih + b_hh: ONE GEMM over all rows
    isc_linear_problem p = sent_cls_linear(x, W, q->w_ih, q->b_ih, q->b_hh, rows, 4 * H, 0, xg);
    if ((rc = isc_linear_fwd(&p, 1, stream))) return rc;
    ++launched;
    // 3. the recurrence on the fused cell: gates = h_{t-1} W_hh^T + Xg[t]
    for (int t = 0; t < L; ++t) {
        isc_lstm_problem s = {};
        s.seg[0].A = t ? out + (long long)(t - 1) * B * H : zero;
        s.seg[0].W = q->w_hh; s.seg[0].lda = H; s.seg[0].ldw = H; s.seg[0].K = H;
        s.nseg = 1; s.M = B; s.H = H;
        s.c_prev = t ? ((t - 1) & 1 ? c1 : c0) : zero;
        s.h_out = out + (long long)t * B * H;
        s.c_out = (t & 1) ? c1 : c0;
        s.mask_scale = 1.f;
        s.pre = xg + (long long)t * B * 4 * H;
        if ((rc = isc_lstm_fwd(&s, stream))) return rc;
        ++launched;
    }
    // 4. excitation: e2 = ex2(relu(ex0(out))) (the sigmoid is the pooling kernel's)
    p = sent_cls_linear(out, H, q->ex0_w, q->ex0_b, nullptr, rows, H, 1, e1);
    if ((rc = isc_linear_fwd(&p, 1, stream))) return rc;
    p = sent_cls_linear(e1, H, q->ex2_w, q->ex2_b, nullptr, rows, H, 0, e2);
    if ((rc = isc_linear_fwd(&p, 1, stream))) return rc;
    launched += 2;
    // 5. token weights and pooled features
    hipLaunchKernelGGL(sent_cls_pool_kernel, dim3(B), dim3(256), (size_t)L * sizeof(float), st, e2, out, q->lens, B, L, H,
                       q->T_out, q->weights, feats);
    ISC_LAUNCH_CHECK();
    ++launched;
    // 6. head, hidden layer
    p = sent_cls_linear(feats, H, q->cls0_w, q->cls0_b, nullptr, B, H, 1, hid);
    if ((rc = isc_linear_fwd(&p, 1, stream))) return rc;
    ++launched;
    // 7. k-way logits, prediction, reward rows
    hipLaunchKernelGGL(sent_cls_head_kernel, dim3((B + 3) / 4), dim3(256), 0, st, hid, q->cls3_w, q->cls3_b, q->labels,
                       q->weights, B, H, k, q->T_out, q->logits, q->pred, q->reward);
    ISC_LAUNCH_CHECK();
    ++launched;
    g_sent_cls_launches += launched;
    return ISC_OK;
}

// =================================================================== training (train_sent_senti_cls_rnn.py:110-126)
static std::atomic<long long> g_sent_cls_bwd_launches{0};
extern "C" long long isc_sent_cls_bwd_launches(void) { return g_sent_cls_bwd_launches.load(); }

// ------------------------------------------------------------------ head + loss
// One wave per caption, as sent_cls_head_kernel (same logits, bit for bit).  Every lane holds the k logits; the loss row
// is (m - z[label]) + log(sum_j exp(z_j - m)) with m the largest logit - finite wherever the logits are -, dz_j =
// (softmax_j - [j == label]) * (g / B), and the lanes then share the float4 columns of dhid = sum_j dz_j W[j, :], j ascending.
__global__ __launch_bounds__(256) void sent_cls_head_loss_kernel(const float *hid, const float *Wc, const float *bc,
                                                                 const int64_t *labels, int B, int H, int k, float gB,
                                                                 float *logits, int32_t *pred, float *loss_rows,
                                                                 float *dz8, float *dhid) {
    const int lane = threadIdx.x & 63;
    const int b = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (b >= B) return;
    float z[8], d[8];
    const int arg = sent_cls_logits_row(hid, Wc, bc, b, H, k, lane, z);
    const long long lab = labels[b];
    const float m = z[arg];
    float se = 0.f, zl = 0.f;
#pragma unroll
    for (int j = 0; j < 8; ++j)
        if (j < k) {
            d[j] = expf(z[j] - m);
            se += d[j];
            if (j == lab) zl = z[j];
        }
    const float inv = 1.f / se;
#pragma unroll
    for (int j = 0; j < 8; ++j) d[j] = j < k ? (d[j] * inv - (j == lab ? 1.f : 0.f)) * gB : 0.f;
    if (lane == 0) {
#pragma unroll
        for (int j = 0; j < 8; ++j)
            if (j < k) logits[(long long)b * k + j] = z[j];
        pred[b] = arg;
        loss_rows[b] = (m - zl) + logf(se);
        float4 *o = reinterpret_cast<float4 *>(dz8 + (long long)b * 8);
        o[0] = make_float4(d[0], d[1], d[2], d[3]);
        o[1] = make_float4(d[4], d[5], d[6], d[7]);
    }
    const int H4 = H >> 2;
    float4 *g = reinterpret_cast<float4 *>(dhid + (long long)b * H);
    for (int i = lane; i < H4; i += 64) {
        float4 acc = make_float4(0.f, 0.f, 0.f, 0.f);
#pragma unroll
        for (int j = 0; j < 8; ++j)
            if (j < k) {
                const float4 w = reinterpret_cast<const float4 *>(Wc + (long long)j * H)[i];
                acc.x += d[j] * w.x; acc.y += d[j] * w.y; acc.z += d[j] * w.z; acc.w += d[j] * w.w;
            }
        g[i] = acc;
    }
}
// One thread per output element, each summing over the captions in ascending order: dW3 [k, H], db3 [k], the mean loss and
// the number of wrong predictions.
__global__ __launch_bounds__(256) void sent_cls_head_reduce_kernel(const float *hid, const float *dz8, const float *loss_rows,
                                                                   const int32_t *pred, const int64_t *labels, int B, int H,
                                                                   int k, float *dw3, float *db3, float *loss,
                                                                   int32_t *wrong) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    const int n = k * H;
    if (i < n) {
        const int j = i / H, h = i - j * H;
        float s = 0.f;
        for (int b = 0; b < B; ++b) s += dz8[(long long)b * 8 + j] * hid[(long long)b * H + h];
        dw3[i] = s;
    } else if (i < n + k) {
        const int j = i - n;
        float s = 0.f;
        for (int b = 0; b < B; ++b) s += dz8[(long long)b * 8 + j];
        db3[j] = s;
    } else if (i == n + k) {
        float s = 0.f;
        for (int b = 0; b < B; ++b) s += loss_rows[b];
        loss[0] = s / (float)B;
    } else if (i == n + k + 1) {
        int c = 0;
        for (int b = 0; b < B; ++b) c += (int64_t)pred[b] != labels[b];
        wrong[0] = c;
    }
}

extern "C" int isc_sent_cls_head_loss(const float *hid, const float *cls3_w, const float *cls3_b, const int64_t *labels, int B,
                                      int H, int k, float g, float *logits, int32_t *pred, float *loss_rows, float *dz8,
                                      float *dhid, float *dw3, float *db3, float *loss, int32_t *wrong, void *stream) {
    if (!hid || !cls3_w || !cls3_b || !labels || !logits || !pred || !loss_rows || !dz8 || !dhid || !dw3 || !db3 || !loss ||
        !wrong)
        return ISC_E_NULL;
    if (B < 1 || H < 4 || (H & 3) || k < 1 || k > 8 || (long long)B * H > 0x7fffffffLL) return ISC_E_SHAPE;
    if (!isc_aligned16(hid) || !isc_aligned16(cls3_w) || !isc_aligned16(dz8) || !isc_aligned16(dhid) || !isc_aligned16(dw3))
        return ISC_E_ALIGN;
    hipStream_t st = (hipStream_t)stream;
    const float gB = (float)((double)g / (double)B);
    hipLaunchKernelGGL(sent_cls_head_loss_kernel, dim3((B + 3) / 4), dim3(256), 0, st, hid, cls3_w, cls3_b, labels, B, H, k,
                       gB, logits, pred, loss_rows, dz8, dhid);
    ISC_LAUNCH_CHECK();
    hipLaunchKernelGGL(sent_cls_head_reduce_kernel, dim3((k * H + k + 2 + 255) / 256), dim3(256), 0, st, hid, dz8, loss_rows,
                       pred, labels, B, H, k, dw3, db3, loss, wrong);
    ISC_LAUNCH_CHECK();
    return ISC_OK;
}

// ------------------------------------------------------------------ pooling backward
// The geometry of sent_cls_pool_kernel: one workgroup of four waves per caption, wave v takes the steps v, v + 4, ... - ALL
// L of them.  Below the length: dw = dfeats[b] . o[t, b] (float4 columns per lane, the wave's butterfly: one fixed order),
// then the wave writes de2[t, b, :] = (dw / H) s (1 - s) and d_o[t, b, :] = w[b, t] dfeats[b].  At and behind the length it
// writes zeros into both rows: the sweep's contractions run over all L * B rows and need no masking after this.
__global__ __launch_bounds__(256) void sent_cls_pool_bwd_kernel(const float *dfeats, const float *e2, const float *o,
                                                                const float *weights, long long ldw, const int32_t *lens,
                                                                int B, int L, int H, float *de2, float *d_o, float *dw) {
    const int b = blockIdx.x;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    int len = lens[b];
    len = len < 0 ? 0 : (len > L ? L : len);
    const int H4 = H >> 2;
    const float4 *g = reinterpret_cast<const float4 *>(dfeats + (long long)b * H);
    for (int t = wave; t < L; t += 4) {
        const long long row = ((long long)t * B + b) * H;
        float4 *pe = reinterpret_cast<float4 *>(de2 + row), *po = reinterpret_cast<float4 *>(d_o + row);
        if (t < len) {
            const float4 *ro = reinterpret_cast<const float4 *>(o + row), *re = reinterpret_cast<const float4 *>(e2 + row);
            float s = 0.f;
            for (int i = lane; i < H4; i += 64) {
                const float4 q = g[i], v = ro[i];
                s += (q.x * v.x + q.y * v.y) + (q.z * v.z + q.w * v.w);
            }
            s = wave_sum(s);
            const float c = s / (float)H, w = weights[(long long)b * ldw + t];
            for (int i = lane; i < H4; i += 64) {
                const float4 q = g[i], e = re[i];
                const float sx = 1.f / (1.f + expf(-e.x)), sy = 1.f / (1.f + expf(-e.y));
                const float sz = 1.f / (1.f + expf(-e.z)), sw = 1.f / (1.f + expf(-e.w));
                pe[i] = make_float4(c * (sx * (1.f - sx)), c * (sy * (1.f - sy)), c * (sz * (1.f - sz)),
                                    c * (sw * (1.f - sw)));
                po[i] = make_float4(w * q.x, w * q.y, w * q.z, w * q.w);
            }
            if (dw && lane == 0) dw[(long long)b * L + t] = s;
        } else {
            const float4 zero = make_float4(0.f, 0.f, 0.f, 0.f);
            for (int i = lane; i < H4; i += 64) { pe[i] = zero; po[i] = zero; }
            if (dw && lane == 0) dw[(long long)b * L + t] = 0.f;
        }
    }
}

extern "C" int isc_sent_cls_pool_bwd(const float *dfeats, const float *e2, const float *o, const float *weights, int64_t ldw,
                                     const int32_t *lens, int B, int L, int H, float *de2, float *d_o, float *dw,
                                     void *stream) {
    if (!dfeats || !e2 || !o || !weights || !lens || !de2 || !d_o) return ISC_E_NULL;
    if (B < 1 || L < 1 || L > 4096 || H < 4 || (H & 3) || ldw < L || (long long)L * B * H > 0x7fffffffLL)
        return ISC_E_SHAPE;
    if (!isc_aligned16(dfeats) || !isc_aligned16(e2) || !isc_aligned16(o) || !isc_aligned16(de2) || !isc_aligned16(d_o))
        return ISC_E_ALIGN;
    hipLaunchKernelGGL(sent_cls_pool_bwd_kernel, dim3(B), dim3(256), 0, (hipStream_t)stream, dfeats, e2, o, weights,
                       (long long)ldw, lens, B, L, H, de2, d_o, dw);
    ISC_LAUNCH_CHECK();
    return ISC_OK;
}

// ------------------------------------------------------------------ saved-activation forward
// Saved activations, in floats (256-byte starts), time-major rows r = t * B + b:
//   x [L*B, W] | Xg [L*B, 4H] | gates [L*B, 4H] | c [L*B, H] | h [L*B, H] | o [L*B, H] | e1 | e2 [L*B, H] | zero [B, H] |
//   feats [B, H] | hid [B, H] | dhid [B, H] | dz8 [B, 8] | loss_rows [B]
namespace {
struct SentClsSaved {
    long long x, xg, gates, c, h, o, e1, e2, zero, feats, hid, dhid, dz8, loss_rows, total;
};
SentClsSaved sent_cls_saved(long long B, long long L, long long W, long long H) {
    SentClsSaved o;
    long long at = 0;
    o.x = at;         at += up64(L * B * W);
    o.xg = at;        at += up64(L * B * 4 * H);
    o.gates = at;     at += up64(L * B * 4 * H);
    o.c = at;         at += up64(L * B * H);
    o.h = at;         at += up64(L * B * H);
    o.o = at;         at += up64(L * B * H);
    o.e1 = at;        at += up64(L * B * H);
    o.e2 = at;        at += up64(L * B * H);
    o.zero = at;      at += up64(B * H);
    o.feats = at;     at += up64(B * H);
    o.hid = at;       at += up64(B * H);
    o.dhid = at;      at += up64(B * H);
    o.dz8 = at;       at += up64(B * 8);
    o.loss_rows = at; at += up64(B);
    o.total = at;
    return o;
}
// Workspace of the sweep, in floats:
//   dphid [B, H] | dfeats [B, H] | de2 | d_o | de1 [L*B, H] | dgates [L*B, 4H] | dx [L*B, W] | dh_rec [B, H] | dc [2, B, H] |
//   column-sum partials [64 * 7H] | time-major ids [L*B] int64 | the embedding gradient's position index
struct SentClsBwdWs {
    long long dphid, dfeats, de2, d_o, de1, dgates, dx, dhrec, dc, colsum, ids, embws, total;
    long long colsum_floats, embws_bytes;
};
SentClsBwdWs sent_cls_bwd_ws(long long B, long long L, long long W, long long H, long long V) {
    SentClsBwdWs o;
    long long at = 0;
    o.dphid = at;  at += up64(B * H);
    o.dfeats = at; at += up64(B * H);
    o.de2 = at;    at += up64(L * B * H);
    o.d_o = at;    at += up64(L * B * H);
    o.de1 = at;    at += up64(L * B * H);
    o.dgates = at; at += up64(L * B * 4 * H);
    o.dx = at;     at += up64(L * B * W);
    o.dhrec = at;  at += up64(B * H);
    o.dc = at;     at += 2 * up64(B * H);
    o.colsum_floats = 64 * 7 * H;
    o.colsum = at; at += up64(o.colsum_floats);
    o.ids = at;    at += up64(2 * L * B);
    o.embws_bytes = (4 * V + 64 + L * B) * (long long)sizeof(int);
    o.embws = at;  at += up64((o.embws_bytes + 3) / 4);
    o.total = at;
    return o;
}
bool sent_cls_train_shape_ok(const isc_sent_cls_train_problem *q) {
    return sent_cls_shape_ok(q->B, q->L, q->W, q->H) && q->W <= 1024 && q->V >= 1 && q->k >= 1 && q->k <= 8 &&
           q->T_out >= q->L && q->tokens_ld >= q->L && (long long)q->V * q->W <= 0x7fffffffLL;
}
bool sent_cls_train_params_null(const isc_sent_cls_train_problem *q) {
    return !q->tokens || !q->lens || !q->emb || !q->w_ih || !q->w_hh || !q->b_ih || !q->b_hh || !q->ex0_w || !q->ex0_b ||
           !q->ex2_w || !q->ex2_b || !q->cls0_w || !q->cls0_b || !q->cls3_w || !q->cls3_b || !q->labels || !q->saved ||
           !q->weights;
}
isc_linear_problem sent_cls_gemm(const float *A, int lda, const float *Wt, int ldw, int K, int M, int N, float *C,
                                 int accumulate) {
    isc_linear_problem p = {};
    p.seg[0].A = A; p.seg[0].W = Wt; p.seg[0].lda = lda; p.seg[0].ldw = ldw; p.seg[0].K = K;
    p.nseg = 1; p.M = M; p.N = N;
    p.mask_scale = 1.f; p.ldc = N; p.C = C; p.accumulate = accumulate;
    return p;
}
}  // namespace

extern "C" int64_t isc_sent_cls_train_saved_bytes(int B, int L, int W, int H) {
    if (!sent_cls_shape_ok(B, L, W, H)) return 0;
    return sent_cls_saved(B, L, W, H).total * (int64_t)sizeof(float);
}

extern "C" int64_t isc_sent_cls_bwd_workspace_bytes(int B, int L, int W, int H, int V) {
    if (!sent_cls_shape_ok(B, L, W, H) || V < 1) return 0;
    return sent_cls_bwd_ws(B, L, W, H, V).total * (int64_t)sizeof(float);
}

extern "C" int isc_sent_cls_train_fwd(const isc_sent_cls_train_problem *q, void *stream) {
    if (!q) return ISC_E_NULL;
    if (sent_cls_train_params_null(q) || !q->logits || !q->pred || !q->loss || !q->wrong || !q->d_cls3_w || !q->d_cls3_b)
        return ISC_E_NULL;
    if (!sent_cls_train_shape_ok(q)) return ISC_E_SHAPE;
    const int B = q->B, L = q->L, W = q->W, H = q->H, k = q->k;
    const SentClsSaved lay = sent_cls_saved(B, L, W, H);
    if (q->saved_bytes < lay.total * (int64_t)sizeof(float)) return ISC_E_WORKSPACE;
    if (!isc_aligned16(q->saved) || !isc_aligned16(q->emb) || !isc_aligned16(q->w_ih) || !isc_aligned16(q->w_hh) ||
        !isc_aligned16(q->ex0_w) || !isc_aligned16(q->ex2_w) || !isc_aligned16(q->cls0_w) || !isc_aligned16(q->cls3_w) ||
        !isc_aligned16(q->d_cls3_w))
        return ISC_E_ALIGN;                         // (what the nested GEMM / cell calls would refuse after the first launch)
    hipStream_t st = (hipStream_t)stream;
    float *sv = static_cast<float *>(q->saved);
    float *x = sv + lay.x, *xg = sv + lay.xg, *gates = sv + lay.gates, *c = sv + lay.c, *h = sv + lay.h;
    float *o = q->out_keep ? sv + lay.o : h, *e1 = sv + lay.e1, *e2 = sv + lay.e2, *zero = sv + lay.zero;
    float *feats = sv + lay.feats, *hid = sv + lay.hid;
    const int rows = L * B;
    const long long BH = (long long)B * H;

    // the launch sequence of isc_sent_cls_fwd, every intermediate kept
    int rc = isc_embed_relu_tm_(q->emb, q->V, W, q->tokens, q->tokens_ld, B, L, x, zero, BH / 4, st);
    if (rc) return rc;
    if (q->emb_keep && (rc = isc_relu_mask_bwd(x, nullptr, q->emb_keep, q->mask_scale, (int64_t)rows * W, x, stream)))
        return rc;                                  // (pointwise, in place: x *= keep * scale)
    isc_linear_problem p = sent_cls_linear(x, W, q->w_ih, q->b_ih, q->b_hh, rows, 4 * H, 0, xg);
    if ((rc = isc_linear_fwd(&p, 1, stream))) return rc;
    for (int t = 0; t < L; ++t) {
        isc_lstm_problem s = {};
        s.seg[0].A = t ? h + (t - 1) * BH : zero;
        s.seg[0].W = q->w_hh; s.seg[0].lda = H; s.seg[0].ldw = H; s.seg[0].K = H;
        s.nseg = 1; s.M = B; s.H = H;
        s.c_prev = t ? c + (t - 1) * BH : zero;
        s.h_out = h + t * BH;
        s.c_out = c + t * BH;
        s.gates_out = gates + t * BH * 4;
        s.mask_scale = 1.f;
        if (q->out_keep) {
            s.h_keep_mask = q->out_keep + t * BH;
            s.mask_scale = q->mask_scale;
            s.hdrop_out = o + t * BH;
        }
        s.pre = xg + t * BH * 4;
        if ((rc = isc_lstm_fwd(&s, stream))) return rc;
    }
    p = sent_cls_linear(o, H, q->ex0_w, q->ex0_b, nullptr, rows, H, 1, e1);
    if ((rc = isc_linear_fwd(&p, 1, stream))) return rc;
    p = sent_cls_linear(e1, H, q->ex2_w, q->ex2_b, nullptr, rows, H, 0, e2);
    if ((rc = isc_linear_fwd(&p, 1, stream))) return rc;
    hipLaunchKernelGGL(sent_cls_pool_kernel, dim3(B), dim3(256), (size_t)L * sizeof(float), st, e2, o, q->lens, B, L, H,
                       q->T_out, q->weights, feats);
    ISC_LAUNCH_CHECK();
    p = sent_cls_linear(feats, H, q->cls0_w, q->cls0_b, nullptr, B, H, 1, hid);
    if (q->hid_keep) { p.keep_mask = q->hid_keep; p.mask_scale = q->mask_scale; }
    if ((rc = isc_linear_fwd(&p, 1, stream))) return rc;
    return isc_sent_cls_head_loss(hid, q->cls3_w, q->cls3_b, q->labels, B, H, k, q->grad_scale, q->logits, q->pred,
                                  sv + lay.loss_rows, sv + lay.dz8, sv + lay.dhid, q->d_cls3_w, q->d_cls3_b, q->loss,
                                  q->wrong, stream);
}

// ------------------------------------------------------------------ reverse sweep
// d_emb = 0 (the embedding gradient adds into the rows of the ids that occur), the token ids time-major with <PAD> behind
// each caption's length (skipped: those rows' dx is zero anyway, and the tokens there then cannot even reorder a sum), and
// d_w_hh = 0 when there is no recurrent row (L == 1).  A kernel, not a memset: a captured memset node is not relied on.
__global__ __launch_bounds__(256) void sent_cls_bwd_prep_kernel(const int64_t *tokens, long long ld, const int32_t *lens,
                                                                int B, int L, int V, long long pad_id, int64_t *ids_tm,
                                                                float4 *demb4, long long n_emb4, float4 *dwhh4,
                                                                long long n_whh4) {
    const long long i0 = (long long)blockIdx.x * 256 + threadIdx.x, stride = (long long)gridDim.x * 256;
    const float4 zero = make_float4(0.f, 0.f, 0.f, 0.f);
    for (long long i = i0; i < n_emb4; i += stride) demb4[i] = zero;
    for (long long i = i0; i < n_whh4; i += stride) dwhh4[i] = zero;
    for (long long r = i0; r < (long long)L * B; r += stride) {
        const int t = (int)(r / B), b = (int)(r - (long long)t * B);
        int len = lens[b];
        len = len < 0 ? 0 : (len > L ? L : len);
        long long id = tokens[(long long)b * ld + t];
        id = id < 0 ? 0 : (id >= V ? V - 1 : id);
        ids_tm[r] = t < len ? id : pad_id;
    }
}

extern "C" int isc_sent_cls_bwd(const isc_sent_cls_train_problem *q, void *stream) {
    if (!q) return ISC_E_NULL;
    if (sent_cls_train_params_null(q) || !q->workspace || !q->d_emb || !q->d_w_ih || !q->d_w_hh || !q->d_b_ih ||
        !q->d_b_hh || !q->d_ex0_w || !q->d_ex0_b || !q->d_ex2_w || !q->d_ex2_b || !q->d_cls0_w || !q->d_cls0_b)
        return ISC_E_NULL;
    if (!sent_cls_train_shape_ok(q) || q->pad_id < -1 || q->pad_id >= q->V) return ISC_E_SHAPE;
    const int B = q->B, L = q->L, W = q->W, H = q->H, V = q->V;
    const SentClsSaved lay = sent_cls_saved(B, L, W, H);
    const SentClsBwdWs wl = sent_cls_bwd_ws(B, L, W, H, V);
    if (q->saved_bytes < lay.total * (int64_t)sizeof(float) || q->workspace_bytes < wl.total * (int64_t)sizeof(float))
        return ISC_E_WORKSPACE;
    if (!isc_aligned16(q->saved) || !isc_aligned16(q->workspace) || !isc_aligned16(q->emb) || !isc_aligned16(q->w_ih) ||
        !isc_aligned16(q->w_hh) || !isc_aligned16(q->ex0_w) || !isc_aligned16(q->ex2_w) || !isc_aligned16(q->cls0_w) ||
        !isc_aligned16(q->d_emb) || !isc_aligned16(q->d_w_ih) || !isc_aligned16(q->d_w_hh) || !isc_aligned16(q->d_ex0_w) ||
        !isc_aligned16(q->d_ex2_w) || !isc_aligned16(q->d_cls0_w))
        return ISC_E_ALIGN;
    hipStream_t st = (hipStream_t)stream;
    float *sv = static_cast<float *>(q->saved), *ws = static_cast<float *>(q->workspace);
    const float *x = sv + lay.x, *gates = sv + lay.gates, *c = sv + lay.c, *h = sv + lay.h;
    const float *o = q->out_keep ? sv + lay.o : h, *e1 = sv + lay.e1, *e2 = sv + lay.e2, *zero = sv + lay.zero;
    const float *feats = sv + lay.feats, *hid = sv + lay.hid, *dhid = sv + lay.dhid;
    float *dphid = ws + wl.dphid, *dfeats = ws + wl.dfeats, *de2 = ws + wl.de2, *d_o = ws + wl.d_o, *de1 = ws + wl.de1;
    float *dgates = ws + wl.dgates, *dx = ws + wl.dx, *dhrec = ws + wl.dhrec, *dc0 = ws + wl.dc;
    float *dc1 = dc0 + up64((long long)B * H);
    int64_t *ids_tm = reinterpret_cast<int64_t *>(ws + wl.ids);
    const int rows = L * B;
    const long long BH = (long long)B * H;
    long long launched = 0;
    int rc;
    // The dW contractions (TN) get the caller's workspace - the split-f16 route of isc_gemm_bwd builds its planes there; the
    // dX contractions (NN) get none and stay on the exact-fp32 tiles: one kernel each, also inside the step loop.
    auto gemm = [&](isc_linear_problem p, int layout) {
        if (layout == ISC_LAYOUT_TN && q->splitk_ws) {
            p.splitk_ws = q->splitk_ws;
            p.splitk_ws_floats = q->splitk_ws_floats;
        }
        ++launched;
        return isc_gemm_bwd(&p, 1, layout, stream);
    };

    // 1. prepare
    {
        const long long n_emb4 = (long long)V * W / 4, n_whh4 = L == 1 ? (long long)4 * H * H / 4 : 0;
        long long n = n_emb4 > n_whh4 ? n_emb4 : n_whh4;
        if (rows > n) n = rows;
        long long nb = (n + 255) / 256;
        if (nb > 2048) nb = 2048;
        hipLaunchKernelGGL(sent_cls_bwd_prep_kernel, dim3((unsigned)nb), dim3(256), 0, st, q->tokens,
                           (long long)q->tokens_ld, q->lens, B, L, V, (long long)q->pad_id, ids_tm,
                           reinterpret_cast<float4 *>(q->d_emb), n_emb4, reinterpret_cast<float4 *>(q->d_w_hh), n_whh4);
        ISC_LAUNCH_CHECK();
        ++launched;
    }
    // 2. head hidden layer: hid = relu(.) [* keep * scale] is positive exactly where both let through
    if ((rc = isc_relu_mask_bwd(dhid, hid, q->hid_keep, q->mask_scale, BH, dphid, stream))) return rc;
    ++launched;
    if ((rc = gemm(sent_cls_gemm(dphid, H, feats, H, B, H, H, q->d_cls0_w, 0), ISC_LAYOUT_TN))) return rc;
    if ((rc = gemm(sent_cls_gemm(dphid, H, q->cls0_w, H, H, B, H, dfeats, 0), ISC_LAYOUT_NN))) return rc;
    // 3. pooling: de2, d_o (zeros at and behind every length)
    if ((rc = isc_sent_cls_pool_bwd(dfeats, e2, o, q->weights, q->T_out, q->lens, B, L, H, de2, d_o, nullptr, stream)))
        return rc;
    ++launched;
    // 4. excitation
    if ((rc = gemm(sent_cls_gemm(de2, H, e1, H, rows, H, H, q->d_ex2_w, 0), ISC_LAYOUT_TN))) return rc;
    if ((rc = gemm(sent_cls_gemm(de2, H, q->ex2_w, H, H, rows, H, de1, 0), ISC_LAYOUT_NN))) return rc;
    if ((rc = isc_relu_mask_bwd(de1, e1, nullptr, 1.f, (int64_t)rows * H, de1, stream))) return rc;
    ++launched;
    if ((rc = gemm(sent_cls_gemm(de1, H, o, H, rows, H, H, q->d_ex0_w, 0), ISC_LAYOUT_TN))) return rc;
    if ((rc = gemm(sent_cls_gemm(de1, H, q->ex0_w, H, H, rows, H, d_o, 1), ISC_LAYOUT_NN))) return rc;
    // 5. the LSTM-output dropout: d_o becomes dh
    if (q->out_keep) {
        if ((rc = isc_relu_mask_bwd(d_o, nullptr, q->out_keep, q->mask_scale, (int64_t)rows * H, d_o, stream))) return rc;
        ++launched;
    }
    // 6. back through time
    for (int t = L - 1; t >= 0; --t) {
        const bool last = t == L - 1;
        float *dc_out = (t & 1) ? dc1 : dc0;
        const float *dc_in = last ? nullptr : ((t + 1) & 1) ? dc1 : dc0;
        if ((rc = isc_lstm_bwd(d_o + t * BH, last ? nullptr : dhrec, dc_in, gates + t * BH * 4, t ? c + (t - 1) * BH : zero,
                               c + t * BH, B, H, dgates + t * BH * 4, dc_out, nullptr, stream)))
            return rc;
        ++launched;
        if (t > 0) {
            if ((rc = gemm(sent_cls_gemm(dgates + t * BH * 4, 4 * H, q->w_hh, H, 4 * H, B, H, dhrec, 0), ISC_LAYOUT_NN))) return rc;
        }
    }
    // 7. the weight gradients of the LSTM, dx, the embedding, the biases
    if (L > 1) {
        if ((rc = gemm(sent_cls_gemm(dgates + BH * 4, 4 * H, h, H, (L - 1) * B, 4 * H, H, q->d_w_hh, 0), ISC_LAYOUT_TN))) return rc;
    }
    if ((rc = gemm(sent_cls_gemm(dgates, 4 * H, x, W, rows, 4 * H, W, q->d_w_ih, 0), ISC_LAYOUT_TN))) return rc;
    if ((rc = gemm(sent_cls_gemm(dgates, 4 * H, q->w_ih, W, 4 * H, rows, W, dx, 0), ISC_LAYOUT_NN))) return rc;
    if ((rc = isc_embed_relu_bwd_ws(q->emb, V, W, ids_tm, 1, rows, 1, 0, 0, dx, 1.f, q->emb_keep, q->mask_scale, q->d_emb,
                                    q->pad_id, ws + wl.embws, wl.embws_bytes, stream)))
        return rc;
    ++launched;
    isc_colsum_job jobs[4] = {};
    jobs[0].x = dgates; jobs[0].ld = 4 * H; jobs[0].M = rows; jobs[0].N = 4 * H;
    jobs[0].out[0] = q->d_b_ih; jobs[0].out[1] = q->d_b_hh; jobs[0].n_out = 2;
    jobs[1].x = de2; jobs[1].ld = H; jobs[1].M = rows; jobs[1].N = H; jobs[1].out[0] = q->d_ex2_b; jobs[1].n_out = 1;
    jobs[2].x = de1; jobs[2].ld = H; jobs[2].M = rows; jobs[2].N = H; jobs[2].out[0] = q->d_ex0_b; jobs[2].n_out = 1;
    jobs[3].x = dphid; jobs[3].ld = H; jobs[3].M = B; jobs[3].N = H; jobs[3].out[0] = q->d_cls0_b; jobs[3].n_out = 1;
    if ((rc = isc_colsum_multi(jobs, 4, ws + wl.colsum, wl.colsum_floats, stream))) return rc;
    ++launched;
    g_sent_cls_bwd_launches += launched;
    return ISC_OK;
}
