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
    const int H4 = H >> 2;
    const float4 *x = reinterpret_cast<const float4 *>(hid + (long long)b * H);
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
    for (int j = 0; j < 8; ++j)
        if (j < k) {
            const float s = wave_sum(acc[j]) + bc[j];
            if (lane == 0) logits[(long long)b * k + j] = s;
            if (j == 0 || s > best) { best = s; arg = j; }
        }
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
