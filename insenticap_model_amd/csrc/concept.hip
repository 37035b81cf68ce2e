// The concept detector (concept_detector.py, train_cpt.py, detect_concepts.py; preprocess.py:288-301) on the device:
//   isc_concept_head                 sigmoid, the `num` best concepts per image, their vocabulary ids, precision / recall counts
//   isc_concept_loss                 MultiLabelClsLoss from the LOGITS, and d loss / d logits in the same pass
//   isc_senti_words_from_concepts    the sentiment words of an image from its detected concepts
//   isc_concept_fwd                  the eval forward: three isc_linear_fwd launches and the head
// Form of cider_dev.hip: one wave64 per row, cross-lane reads, no atomics, every sum in one fixed order (two runs give
// the same bits), no host synchronisation and no allocation in an entry point (capturable).
//
// ORDER of the head's top-`num`: the larger LOGIT first; on equal logits the lower index first; -0.0 equals +0.0; +-inf
// are ordinary values; a NaN ranks below every number (NaNs among themselves: lower index first) and raises the numerics
// status word (ISC_STATUS_NONFINITE_STATS).  The reference sorts the fp32 PROBABILITIES with an unstable sort
// (concept_detector.py:28); sigmoid is monotone, so ordering by logit gives the reference's answer wherever that answer is
// defined (distinct probabilities) and a fixed one where probabilities saturate to 0 / 1 or tie.
//
// LOSS: -mean(t log s(z)) - mean((1 - t) log(1 - s(z))) with -log s(z) = softplus(-z), -log(1 - s(z)) = softplus(z),
// softplus(x) = max(x, 0) + log1p(exp(-|x|)): finite for every finite z.  The reference takes result.log() of a sigmoid
// that has saturated to 0 or 1 in fp32 (|z| > ~17 / ~88) and gets inf, or NaN from 0 * inf, there.
#include <atomic>

#include "common.h"

ISC_STATUS_DECL(cpt)

static std::atomic<long long> g_concept_launches{0};
extern "C" long long isc_concept_launches(void) { return g_concept_launches.load(); }

#define CPT_WAVES 4        // rows per workgroup

// ------------------------------------------------------------------ head
// The order above as ONE unsigned comparison: the logit's bits made monotone (NaN -> 0, below -inf; -0.0 -> +0.0) in the
// high word, ~index in the low word - larger = better, no two elements of a row compare equal.
__device__ __forceinline__ unsigned long long cpt_rank(float z, int i) {
    unsigned int k = 0u;
    if (z == z) {
        const unsigned int u = z == 0.f ? 0u : __float_as_uint(z);
        k = (u & 0x80000000u) ? ~u : (u | 0x80000000u);
    }
    return ((unsigned long long)k << 32) | (unsigned long long)(0xffffffffu - (unsigned int)i);
}
__device__ __forceinline__ unsigned long long cpt_wave_max(unsigned long long v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        const unsigned long long ov = __shfl_xor(v, o, 64);
        v = ov > v ? ov : v;
    }
    return v;
}
__device__ __forceinline__ int cpt_wave_sum(int v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;
}
__device__ __forceinline__ double cpt_wave_sum(double v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;
}
__device__ __forceinline__ float cpt_sigmoid(float z) { return 1.f / (1.f + expf(-z)); }

struct CptHeadArgs {
    const float *logits;        // [B, C], leading dimension ld
    long long ld;
    int B, C, num, tgt_i64;
    float *probs;               // [B, C] or null
    int64_t *idx;               // [B, num] or null
    float *scores;              // [B, num] or null
    const int64_t *concept_word;    // [C] or null
    int64_t *words;             // [B, num] or null
    const void *targets;        // [B, C] uint8 / int64, or null
    int32_t *hits, *n_true;     // [B] or null
};

// Pass k finds the best element that ranks strictly below pick k - 1: no list of taken elements, `num` walks over a row
// that stays in the cache (8 KB at C = 2000).  Pick k lives in lane k until the row's results are written.
__global__ __launch_bounds__(64 * CPT_WAVES) void concept_head_kernel(const CptHeadArgs a) {
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    const long long b = (long long)blockIdx.x * CPT_WAVES + wave;
    if (b >= a.B) return;                                  // (the whole wave leaves)
    const int C = a.C;
    const float *row = a.logits + b * a.ld;

    bool bad = false;
    for (int c = lane; c < C; c += 64) {
        const float z = row[c];
        bad |= z != z;
        if (a.probs) a.probs[b * C + c] = cpt_sigmoid(z);
    }
    if (__ballot(bad) != 0ull && lane == 0) isc_flag_cpt(ISC_STATUS_WORD_STATS);

    unsigned long long prev = ~0ull;
    int my = 0;
    const int n_pick = (a.idx || a.scores || a.words || a.targets) ? a.num : 0;     // probabilities alone: no selection
    for (int k = 0; k < n_pick; ++k) {
        unsigned long long best = 0ull;                    // (below every rank: an index is < 2^31)
        for (int c = lane; c < C; c += 64) {
            const unsigned long long r = cpt_rank(row[c], c);
            if (r < prev && r > best) best = r;
        }
        best = cpt_wave_max(best);
        prev = best;
        if (lane == k) my = (int)(0xffffffffu - (unsigned int)best);
    }
    const bool mine = lane < a.num;                         // num <= C: every pass found an element
    if (mine) {
        const long long o = b * a.num + lane;
        if (a.idx) a.idx[o] = my;
        if (a.scores) a.scores[o] = cpt_sigmoid(row[my]);
        if (a.words) a.words[o] = a.concept_word[my];
    }
    if (a.targets) {
        const uint8_t *t8 = static_cast<const uint8_t *>(a.targets) + b * C;
        const int64_t *t64 = static_cast<const int64_t *>(a.targets) + b * C;
        int n = 0;
        for (int c = lane; c < C; c += 64) n += (a.tgt_i64 ? t64[c] != 0 : t8[c] != 0) ? 1 : 0;
        n = cpt_wave_sum(n);
        const bool hit = mine && (a.tgt_i64 ? t64[my] != 0 : t8[my] != 0);
        const int h = __popcll(__ballot(hit));
        if (lane == 0) {
            if (a.hits) a.hits[b] = h;
            if (a.n_true) a.n_true[b] = n;
        }
    }
}

extern "C" int isc_concept_head(const float *logits, int64_t ld, int B, int C, int num, float *probs, int64_t *idx,
                                float *scores, const int64_t *concept_word, int64_t *words, const void *targets,
                                int targets_i64, int32_t *hits, int32_t *n_true, void *stream) {
    if (!logits) return ISC_E_NULL;
    if (words && !concept_word) return ISC_E_NULL;
    if ((hits || n_true) && !targets) return ISC_E_NULL;
    if (B < 1 || C < 1 || num < 1 || num > ISC_CONCEPT_MAX_NUM || num > C || ld < C) return ISC_E_SHAPE;
    CptHeadArgs a = {};
    a.logits = logits; a.ld = ld; a.B = B; a.C = C; a.num = num; a.tgt_i64 = targets_i64 != 0;
    a.probs = probs; a.idx = idx; a.scores = scores; a.concept_word = concept_word; a.words = words;
    a.targets = (hits || n_true) ? targets : nullptr; a.hits = hits; a.n_true = n_true;
    hipLaunchKernelGGL(concept_head_kernel, dim3((unsigned)((B + CPT_WAVES - 1) / CPT_WAVES)), dim3(64 * CPT_WAVES), 0,
                       (hipStream_t)stream, a);
    ISC_LAUNCH_CHECK();
    return ISC_OK;
}

// ------------------------------------------------------------------ loss
// One wave per row: lane l takes the columns l, l + 64, ... ascending, the elements in fp32 (softplus above), the sums
// in fp64; the butterfly folds the lanes.  row2[b] = { sum t softplus(-z), sum (1 - t) softplus(z) } of row b.
template <typename T>
__global__ __launch_bounds__(64 * CPT_WAVES) void concept_loss_rows_kernel(const float *logits, long long ld, int B, int C,
                                                                           const T *tgt, float scale, double *row2,
                                                                           float *dz) {
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    const long long b = (long long)blockIdx.x * CPT_WAVES + wave;
    if (b >= B) return;
    const float *row = logits + b * ld;
    const T *t = tgt + b * C;
    double s1 = 0.0, s2 = 0.0;
    for (int c = lane; c < C; c += 64) {
        const float z = row[c];
        const bool on = t[c] != 0;
        const float l = log1pf(expf(-fabsf(z)));
        const float sp = (on ? (z < 0.f ? -z : 0.f) : (z > 0.f ? z : 0.f)) + l;      // softplus(-z) / softplus(z)
        if (on) s1 += (double)sp; else s2 += (double)sp;
        if (dz) dz[b * C + c] = (cpt_sigmoid(z) - (on ? 1.f : 0.f)) * scale;
    }
    s1 = cpt_wave_sum(s1);
    s2 = cpt_wave_sum(s2);
    if (lane == 0) { row2[2 * b] = s1; row2[2 * b + 1] = s2; }
}
// One wave: lane l adds the rows l, l + 64, ... ascending, the butterfly folds the lanes; out3 = { term1, term2, loss }.
__global__ __launch_bounds__(64) void concept_loss_final_kernel(const double *row2, int B, double inv_n, float *out3) {
    const int lane = threadIdx.x;
    double s1 = 0.0, s2 = 0.0;
    for (int b = lane; b < B; b += 64) { s1 += row2[2 * b]; s2 += row2[2 * b + 1]; }
    s1 = cpt_wave_sum(s1) * inv_n;
    s2 = cpt_wave_sum(s2) * inv_n;
    if (lane == 0) { out3[0] = (float)s1; out3[1] = (float)s2; out3[2] = (float)(s1 + s2); }
}

extern "C" int64_t isc_concept_loss_workspace_bytes(int B) { return B < 1 ? 0 : (int64_t)B * 2 * sizeof(double); }

extern "C" int isc_concept_loss(const float *logits, int64_t ld, int B, int C, const void *targets, int targets_i64,
                                float g, void *workspace, int64_t workspace_bytes, float *out3, float *dz, void *stream) {
    if (!logits || !targets || !workspace || !out3) return ISC_E_NULL;
    if (B < 1 || C < 1 || ld < C || (long long)B * C > 0x7fffffffLL) return ISC_E_SHAPE;
    if (workspace_bytes < isc_concept_loss_workspace_bytes(B)) return ISC_E_WORKSPACE;
    if (((uintptr_t)workspace & 7u) != 0) return ISC_E_ALIGN;
    hipStream_t st = (hipStream_t)stream;
    double *row2 = static_cast<double *>(workspace);
    const double n = (double)B * (double)C;
    const float scale = (float)((double)g / n);
    const dim3 grid((unsigned)((B + CPT_WAVES - 1) / CPT_WAVES)), block(64 * CPT_WAVES);
    if (targets_i64)
        hipLaunchKernelGGL(concept_loss_rows_kernel<int64_t>, grid, block, 0, st, logits, (long long)ld, B, C,
                           static_cast<const int64_t *>(targets), scale, row2, dz);
    else
        hipLaunchKernelGGL(concept_loss_rows_kernel<uint8_t>, grid, block, 0, st, logits, (long long)ld, B, C,
                           static_cast<const uint8_t *>(targets), scale, row2, dz);
    ISC_LAUNCH_CHECK();
    hipLaunchKernelGGL(concept_loss_final_kernel, dim3(1), dim3(64), 0, st, row2, B, 1.0 / n, out3);
    ISC_LAUNCH_CHECK();
    return ISC_OK;
}

// ------------------------------------------------------------------ sentiment words
// preprocess.py:288-301 for one image per wave (one wave per workgroup, the candidates in LDS).  The (word, score) entries
// of the image's concepts are staged in concept order, then list order - the order in which the host extends its list.
// Candidate i is a word's first occurrence when no j < i holds the same word; its sum adds the scores of the positions
// j >= i that hold the word, ascending, in fp64 without contraction: the host's `tmp_sentis[w] += s` over the same
// sequence (0.0 + s is s), hence the host's bits.  Then n_out passes: the largest sum that ranks strictly behind the
// previous pick in (sum descending, first position ascending) - Python's stable sort over the dict's insertion order.
// CAP: an image stages at most ISC_SENTI_WORDS_CAP = 1024 candidates (16 KB of words and scores, 12 KB of sums and
// flags in LDS); the entry point refuses num * max_list > CAP, and the kernel stops staging at CAP whatever the table
// says (a table that lies about max_list cannot make it write past its arrays).
struct CptSwArgs {
    const int64_t *idx;         // [B, num], leading dimension idx_ld
    long long idx_ld;
    int B, num, C, n_out;
    const int32_t *off;         // [C + 1]
    const int64_t *word;        // [nnz]
    const double *score;        // [nnz]
    int64_t pad_id;
    int64_t *out;               // [B, n_out]
};
__global__ __launch_bounds__(64) void senti_words_kernel(const CptSwArgs a) {
#pragma clang fp contract(off)
    __shared__ int64_t s_word[ISC_SENTI_WORDS_CAP];
    __shared__ double s_score[ISC_SENTI_WORDS_CAP];
    __shared__ double s_sum[ISC_SENTI_WORDS_CAP];
    __shared__ int s_first[ISC_SENTI_WORDS_CAP];
    const int lane = threadIdx.x;
    const long long b = blockIdx.x;
    int n = 0;
    for (int j = 0; j < a.num; ++j) {
        const long long c = a.idx[b * a.idx_ld + j];
        if (c < 0 || c >= a.C) continue;                    // (uniform: every lane read the same id)
        const int e0 = a.off[c], e1 = a.off[c + 1];
        int len = e1 - e0;
        if (len < 0) len = 0;
        if (len > ISC_SENTI_WORDS_CAP - n) len = ISC_SENTI_WORDS_CAP - n;
        for (int e = lane; e < len; e += 64) {
            s_word[n + e] = a.word[e0 + e];
            s_score[n + e] = a.score[e0 + e];
        }
        n += len;
    }
    __syncthreads();
    for (int i = lane; i < n; i += 64) {
        const int64_t w = s_word[i];
        bool first = true;
        for (int j = 0; j < i; ++j) first = first && s_word[j] != w;
        double s = 0.0;
        if (first)
            for (int j = i; j < n; ++j)
                if (s_word[j] == w) s += s_score[j];
        s_first[i] = first;
        s_sum[i] = s;
    }
    __syncthreads();
    double p_sum = 0.0;
    int p_pos = -1;                                         // -1: no pick yet, everything ranks behind it
    for (int k = 0; k < a.n_out; ++k) {
        double v = 0.0;
        int at = 0x7fffffff;                                // none
        for (int i = lane; i < n; i += 64) {
            if (!s_first[i]) continue;
            const double s = s_sum[i];
            const bool behind = p_pos < 0 || s < p_sum || (s == p_sum && i > p_pos);
            if (behind && (at == 0x7fffffff || s > v || (s == v && i < at))) { v = s; at = i; }
        }
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) {
            const double ov = __shfl_xor(v, o, 64);
            const int oa = __shfl_xor(at, o, 64);
            if (oa != 0x7fffffff && (at == 0x7fffffff || ov > v || (ov == v && oa < at))) { v = ov; at = oa; }
        }
        if (at == 0x7fffffff) {                             // nothing left: the collate's fill_(pad_index)
            for (int q = k + lane; q < a.n_out; q += 64) a.out[b * a.n_out + q] = a.pad_id;
            break;
        }
        if (lane == 0) a.out[b * a.n_out + k] = s_word[at];
        p_sum = v;
        p_pos = at;
    }
}

extern "C" int isc_senti_words_cap(void) { return ISC_SENTI_WORDS_CAP; }

extern "C" int isc_senti_words_pack_check(const int32_t *off_host, int C, int num, int *max_list_out) {
    if (!off_host) return ISC_E_NULL;
    if (C < 1 || num < 1 || num > ISC_CONCEPT_MAX_NUM || off_host[0] != 0) return ISC_E_SHAPE;
    int longest = 0;
    for (int c = 0; c < C; ++c) {
        const long long len = (long long)off_host[c + 1] - off_host[c];
        if (len < 0) return ISC_E_SHAPE;
        if (len > longest) longest = (int)len;
    }
    if (max_list_out) *max_list_out = longest;
    return (long long)num * longest > ISC_SENTI_WORDS_CAP ? ISC_E_SHAPE : ISC_OK;
}

extern "C" int isc_senti_words_from_concepts(const int64_t *idx, int64_t idx_ld, int B, int num, int C,
                                             const int32_t *off, const int64_t *word, const double *score, int max_list,
                                             int n_out, int64_t pad_id, int64_t *out, void *stream) {
    if (!idx || !off || !out) return ISC_E_NULL;
    if (max_list > 0 && (!word || !score)) return ISC_E_NULL;
    if (B < 1 || C < 1 || num < 1 || num > ISC_CONCEPT_MAX_NUM || idx_ld < num || n_out < 1 ||
        n_out > ISC_SENTI_WORDS_MAX_OUT || max_list < 0 || (long long)num * max_list > ISC_SENTI_WORDS_CAP)
        return ISC_E_SHAPE;
    CptSwArgs a = {};
    a.idx = idx; a.idx_ld = idx_ld; a.B = B; a.num = num; a.C = C; a.n_out = n_out;
    a.off = off; a.word = word; a.score = score; a.pad_id = pad_id; a.out = out;
    hipLaunchKernelGGL(senti_words_kernel, dim3((unsigned)B), dim3(64), 0, (hipStream_t)stream, a);
    ISC_LAUNCH_CHECK();
    return ISC_OK;
}

// ------------------------------------------------------------------ eval forward
// Workspace, in floats (every block a multiple of 64 floats): feats32 [B, F] (used only for f16 features that the first
// launch does not read natively) | h1 [B, H] | h2 [B, H] | logits [B, C] (used only without q->logits).
namespace {
long long cpt_up64(long long n) { return (n + 63) / 64 * 64; }
struct CptLayout {
    long long f32, h1, h2, logits, total;
};
CptLayout cpt_layout(long long B, long long F, long long H, long long C) {
    CptLayout o;
    long long at = 0;
    o.f32 = at;    at += cpt_up64(B * F);
    o.h1 = at;     at += cpt_up64(B * H);
    o.h2 = at;     at += cpt_up64(B * H);
    o.logits = at; at += cpt_up64(B * C);
    o.total = at;
    return o;
}
// what isc_linear_fwd asks of a contraction length (gemm_f32.hip check_segs) and what keeps element counts 32-bit
bool cpt_shape_ok(long long B, long long F, long long H, long long C) {
    return B >= 1 && F >= 32 && H >= 32 && C >= 1 && (F % 32) == 0 && (H % 32) == 0 && B * F <= 0x7fffffffLL &&
           B * H <= 0x7fffffffLL && B * C <= 0x7fffffffLL;
}
isc_linear_problem cpt_linear(const void *A, long long lda, int a_f16, int K, const float *W, const float *bias, int M,
                              int N, int relu, float *C, float *ws, long long ws_floats) {
    isc_linear_problem p = {};
    p.seg[0].A = static_cast<const float *>(A); p.seg[0].W = W; p.seg[0].lda = (int32_t)lda; p.seg[0].ldw = K;
    p.seg[0].K = K; p.seg[0].a_f16 = a_f16;
    p.nseg = 1; p.M = M; p.N = N; p.relu = relu; p.bias0 = bias;
    p.mask_scale = 1.f; p.ldc = N; p.C = C;
    p.splitk_ws = ws; p.splitk_ws_floats = ws_floats;
    return p;
}
}  // namespace

extern "C" int64_t isc_concept_workspace_bytes(int B, int F, int H, int C) {
    if (!cpt_shape_ok(B, F, H, C)) return 0;
    return cpt_layout(B, F, H, C).total * (int64_t)sizeof(float);
}

extern "C" int isc_concept_fwd(const isc_concept_problem *q, void *stream) {
    if (!q) return ISC_E_NULL;
    if (!q->feats || !q->w0 || !q->b0 || !q->w2 || !q->b2 || !q->w5 || !q->b5 || !q->workspace) return ISC_E_NULL;
    if (q->words && !q->concept_word) return ISC_E_NULL;
    const int B = q->B, F = q->F, H = q->H, C = q->C, num = q->num;
    if (!cpt_shape_ok(B, F, H, C) || num < 1 || num > ISC_CONCEPT_MAX_NUM || num > C || q->feats_ld < F ||
        q->feats_ld > 0x7fffffffLL)
        return ISC_E_SHAPE;
    const CptLayout lay = cpt_layout(B, F, H, C);
    if (q->workspace_bytes < lay.total * (int64_t)sizeof(float)) return ISC_E_WORKSPACE;
    if (!isc_aligned16(q->workspace) || !isc_aligned16(q->feats) || (q->feats_ld & 3) ||
        (q->logits && !isc_aligned16(q->logits)))
        return ISC_E_ALIGN;
    float *ws = static_cast<float *>(q->workspace);
    float *h1 = ws + lay.h1, *h2 = ws + lay.h2, *logits = q->logits ? q->logits : ws + lay.logits;
    float *sk = q->splitk_ws;
    const long long skf = q->splitk_ws_floats;

    isc_linear_problem p = cpt_linear(q->feats, q->feats_ld, q->feats_f16 != 0, F, q->w0, q->b0, B, H, 1, h1, sk, skf);
    if (q->feats_f16 && !isc_linear_f16_native(&p, 1, stream)) {
        // float16 features on a launch that does not read them natively: one explicit fp32 copy (as ops.linear_fwd)
        const int rc = isc_f16_to_f32(q->feats, q->feats_ld, ws + lay.f32, F, B, F, stream);
        if (rc) return rc;
        p = cpt_linear(ws + lay.f32, F, 0, F, q->w0, q->b0, B, H, 1, h1, sk, skf);
    }
    int rc = isc_linear_fwd(&p, 1, stream);
    if (rc) return rc;
    p = cpt_linear(h1, H, 0, H, q->w2, q->b2, B, H, 1, h2, sk, skf);
    if ((rc = isc_linear_fwd(&p, 1, stream))) return rc;
    p = cpt_linear(h2, H, 0, H, q->w5, q->b5, B, C, 0, logits, sk, skf);
    if ((rc = isc_linear_fwd(&p, 1, stream))) return rc;
    rc = isc_concept_head(logits, C, B, C, num, q->probs, q->idx, q->scores, q->concept_word, q->words, nullptr, 0,
                          nullptr, nullptr, stream);
    if (rc) return rc;
    g_concept_launches += 4;
    return ISC_OK;
}
