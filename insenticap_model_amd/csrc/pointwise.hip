// Embedding gathers, roll-out bookkeeping, log-softmax finalisation, beam top-k and the
// masked-NLL criterion (captioner.py:170-172, 201-202, 307-311, 329-344, 394-408, 427-440).
#include <atomic>
#include <cstddef>

#include "common.h"
#include "flt_key.h"

// ------------------------------------------------------------------ embeddings
// TM (isc_sent_cls_fwd, sent_cls.hip): the ids are a [B, L] matrix read TIME-MAJOR - output row r = t * tm_B + b takes
// ids[b * ids_stride + t], clamped into the table - and the workgroups behind the last row clear `zero` (zero4 float4s:
// the zero state in front of the first recurrent step), so that the call needs no fill of its own.
template <bool TM>
__global__ __launch_bounds__(256) void embed_relu_kernel(const float *emb, int W, const int64_t *ids,
                                                         long long ids_stride, const float *add,
                                                         int B, float *out, int tm_B, int V, float *zero, long long zero4) {
    const int lane = threadIdx.x & 63;
    const int b = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (TM) {
        const int row_blocks = (B + 3) / 4;
        if ((int)blockIdx.x >= row_blocks) {
            const long long i = (long long)(blockIdx.x - row_blocks) * 256 + threadIdx.x;
            if (i < zero4) reinterpret_cast<float4 *>(zero)[i] = make_float4(0.f, 0.f, 0.f, 0.f);
            return;
        }
    }
    if (b >= B) return;
    long long id;
    if (TM) {
        id = ids[(long long)(b % tm_B) * ids_stride + b / tm_B];
        id = id < 0 ? 0 : (id >= V ? V - 1 : id);
    } else {
        id = ids[(long long)b * ids_stride];
    }
    const float4 *src = reinterpret_cast<const float4 *>(emb + id * W);
    const float4 *ad = add ? reinterpret_cast<const float4 *>(add + (long long)b * W) : nullptr;
    float4 *dst = reinterpret_cast<float4 *>(out + (long long)b * W);
    for (int i = lane; i < (W >> 2); i += 64) {
        float4 v = src[i];
        v.x = fmaxf(v.x, 0.f); v.y = fmaxf(v.y, 0.f); v.z = fmaxf(v.z, 0.f); v.w = fmaxf(v.w, 0.f);
        if (ad) { const float4 a = ad[i]; v.x += a.x; v.y += a.y; v.z += a.z; v.w += a.w; }
        dst[i] = v;
    }
}

// x[t * B + b, :] = relu(emb[tokens[b * ld + t], :]) for all L * B rows, and zero4 float4s at `zero` cleared: ONE launch.
int isc_embed_relu_tm_(const float *emb, int V, int W, const int64_t *tokens, int64_t ld, int B, int L, float *out,
                       float *zero, long long zero4, hipStream_t st) {
    const long long rows = (long long)B * L;
    const long long blocks = (rows + 3) / 4 + (zero4 + 255) / 256;
    if (blocks > 0x7fffffffLL) return ISC_E_SHAPE;
    hipLaunchKernelGGL(embed_relu_kernel<true>, dim3((unsigned)blocks), dim3(256), 0, st, emb, W, tokens, (long long)ld,
                       (const float *)nullptr, (int)rows, out, B, V, zero, zero4);
    ISC_LAUNCH_CHECK();
    return ISC_OK;
}

extern "C" int isc_embed_relu_fwd(const float *emb, int V, int W, const int64_t *ids,
                                  int64_t ids_stride, const float *add, int B, float *out,
                                  void *stream) {
    if (!emb || !ids || !out) return ISC_E_NULL;
    if (B <= 0 || V <= 0 || W <= 0 || (W & 3)) return ISC_E_SHAPE;
    // the kernel reads and writes rows as float4
    if (!isc_aligned16(emb) || !isc_aligned16(out) || (add && !isc_aligned16(add))) return ISC_E_ALIGN;
    hipLaunchKernelGGL(embed_relu_kernel<false>, dim3((B + 3) / 4), dim3(256), 0, (hipStream_t)stream, emb, W,
                       ids, (long long)ids_stride, add, B, out, 0, V, (float *)nullptr, 0LL);
    ISC_LAUNCH_CHECK();
    return ISC_OK;
}

__global__ __launch_bounds__(256) void embed_relu_mean_kernel(const float *emb, int W, const int64_t *ids,
                                                              int C, int B, float *out) {
    const int lane = threadIdx.x & 63;
    const int b = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (b >= B) return;
    if ((W & 3) == 0 && (((uintptr_t)emb | (uintptr_t)out) & 15) == 0) {
        // the ids of up to eight words first, then every word's row chunk in flight at once (the rows come from an 82 MB
        // table: one dependent round trip per word and chunk made this a 20-27 us kernel at B = 128 ... 208); the sum
        // runs over the words in ascending order, as before
        for (int i = lane * 4; i < W; i += 256) {
            float4 s = make_float4(0.f, 0.f, 0.f, 0.f);
            for (int c0 = 0; c0 < C; c0 += 8) {
                long long id[8];
                float4 x[8];
#pragma unroll
                for (int k = 0; k < 8; ++k) id[k] = ids[(long long)b * C + (c0 + k < C ? c0 + k : C - 1)];
#pragma unroll
                for (int k = 0; k < 8; ++k) x[k] = *reinterpret_cast<const float4 *>(emb + id[k] * W + i);
#pragma unroll
                for (int k = 0; k < 8; ++k)
                    if (c0 + k < C) {
                        s.x += fmaxf(x[k].x, 0.f); s.y += fmaxf(x[k].y, 0.f);
                        s.z += fmaxf(x[k].z, 0.f); s.w += fmaxf(x[k].w, 0.f);
                    }
            }
            const float n = (float)C;
            *reinterpret_cast<float4 *>(out + (long long)b * W + i) = make_float4(s.x / n, s.y / n, s.z / n, s.w / n);
        }
        return;
    }
    for (int i = lane; i < W; i += 64) {
        float s = 0.f;
        for (int c = 0; c < C; ++c) s += fmaxf(emb[ids[(long long)b * C + c] * W + i], 0.f);
        out[(long long)b * W + i] = s / (float)C;
    }
}

extern "C" int isc_embed_relu_mean_fwd(const float *emb, int V, int W, const int64_t *ids, int C,
                                       int B, float *out, void *stream) {
    if (!emb || !ids || !out) return ISC_E_NULL;
    if (B <= 0 || V <= 0 || W <= 0 || C <= 0) return ISC_E_SHAPE;
    hipLaunchKernelGGL(embed_relu_mean_kernel, dim3((B + 3) / 4), dim3(256), 0, (hipStream_t)stream,
                       emb, W, ids, C, B, out);
    ISC_LAUNCH_CHECK();
    return ISC_OK;
}

__global__ __launch_bounds__(256) void embed_senti_words_kernel(const float *emb, int W,
                                                                const int64_t *ids, int n_words,
                                                                long long pad_id, int B,
                                                                const uint8_t *mask, float scale,
                                                                float *out) {
    const int lane = threadIdx.x & 63;
    const int row = blockIdx.x * 4 + (threadIdx.x >> 6);  // row = b*(n_words+1) + m
    const int Mw = n_words + 1;
    if (row >= B * Mw) return;
    const int b = row / Mw, m = row % Mw;
    const long long id = (m == 0) ? pad_id : ids[(long long)b * n_words + (m - 1)];
    for (int i = lane; i < W; i += 64) {
        float v = fmaxf(emb[id * W + i], 0.f);
        if (mask) v = v * (float)mask[(long long)row * W + i] * scale;
        out[(long long)row * W + i] = v;
    }
}

extern "C" int isc_embed_senti_words_fwd(const float *emb, int V, int W, const int64_t *ids,
                                         int n_words, int64_t pad_id, int B,
                                         const uint8_t *keep_mask, float mask_scale, float *out,
                                         void *stream) {
    if (!emb || !ids || !out) return ISC_E_NULL;
    if (B <= 0 || V <= 0 || W <= 0 || n_words <= 0) return ISC_E_SHAPE;
    const int rows = B * (n_words + 1);
    hipLaunchKernelGGL(embed_senti_words_kernel, dim3((rows + 3) / 4), dim3(256), 0,
                       (hipStream_t)stream, emb, W, ids, n_words, (long long)pad_id, B, keep_mask,
                       mask_scale, out);
    ISC_LAUNCH_CHECK();
    return ISC_OK;
}

// ------------------------------------------------------------------ beam search: candidate merge on the device
// captioner.py:378-411 for every image of a batched search, without the per-step device->host->device round trip:
// one workgroup per image.  Candidates in the reference's insertion order (parents by rank; an ended parent carries
// itself, a live one contributes its `beam` children by rank), scores as fp64 sums of the fp32 log-probs (the
// reference adds Python floats), selection = the first `beam` of a STABLE descending sort:
//     rank(c) = #{ j : s_j > s_c } + #{ j < c : s_j == s_c }.
// State is double-buffered by the caller (in -> out).  gather[row] = source row of the new row inside
// [next-state rows ; current-state rows] (a stepped parent's new state, or a carried candidate's old one).
#define ISC_BEAM_MAX 8
__global__ __launch_bounds__(64) void beam_merge_kernel(const isc_beam_merge_args a) {
    __shared__ double cs[ISC_BEAM_MAX * ISC_BEAM_MAX];
    __shared__ long long ctok[ISC_BEAM_MAX * ISC_BEAM_MAX];
    __shared__ int cpar[ISC_BEAM_MAX * ISC_BEAM_MAX], ccar[ISC_BEAM_MAX * ISC_BEAM_MAX], coff[ISC_BEAM_MAX + 1];
    __shared__ int s_all_ended;
    const int i = blockIdx.x, tid = threadIdx.x, beam = a.beam, T = a.T, rows = a.n_img * beam, base = i * beam;
    if (a.done[i]) {                      // frozen image: state carried over unchanged, rows keep their old state
        for (int k = tid; k < beam; k += 64) {
            a.gather[base + k] = base + k + rows;
            a.last_out[base + k] = a.last_in[base + k];
            a.score_out[base + k] = a.score_in[base + k];
            a.len_out[base + k] = a.len_in[base + k];
        }
        for (int e = tid; e < beam * T; e += 64) a.words_out[(long long)base * T + e] = a.words_in[(long long)base * T + e];
        return;
    }
    const int ncand = a.t == 0 ? 1 : beam;
    if (tid == 0) {
        int off = 0, all_ended = 1;
        for (int k = 0; k < ncand; ++k) {
            coff[k] = off;
            const int ended = a.t > 0 && a.last_in[base + k] == a.eos_id;
            off += ended ? 1 : beam;
            all_ended &= ended;
        }
        coff[ncand] = off;
        s_all_ended = all_ended;
    }
    __syncthreads();
    const int n = coff[ncand];
    for (int e = tid; e < ncand * beam; e += 64) {
        const int k = e / beam, j = e % beam, row = base + k;
        const int ended = a.t > 0 && a.last_in[row] == a.eos_id;
        if (ended) {
            if (j == 0) { const int c = coff[k]; cs[c] = a.score_in[row]; ctok[c] = a.last_in[row]; cpar[c] = k; ccar[c] = 1; }
        } else {
            const int c = coff[k] + j;
            cs[c] = a.score_in[row] + (double)a.top_val[(long long)row * beam + j];
            ctok[c] = a.top_idx[(long long)row * beam + j];
            cpar[c] = k; ccar[c] = 0;
        }
    }
    __syncthreads();
    if (tid < n) {
        const double sc = cs[tid];
        int rank = 0;
        for (int j = 0; j < n; ++j) rank += (cs[j] > sc) || (cs[j] == sc && j < tid);
        if (rank < beam) {
            const int par = cpar[tid], car = ccar[tid], dst = base + rank, srow = base + par;
            a.score_out[dst] = sc;
            a.last_out[dst] = ctok[tid];
            a.gather[dst] = car ? srow + rows : srow;
            const int len = a.len_in[srow];
            for (int e = 0; e < T; ++e) a.words_out[(long long)dst * T + e] = a.words_in[(long long)srow * T + e];
            if (!car && len < T) a.words_out[(long long)dst * T + len] = ctok[tid];
            a.len_out[dst] = len + (car ? 0 : 1);
        }
    }
    if (tid == 0) {
        if (s_all_ended) a.done[i] = 1;
        else atomicAdd(&a.live[a.t + 1], 1);
    }
}

extern "C" int isc_beam_merge(const isc_beam_merge_args *args, void *stream) {
    if (!args) return ISC_E_NULL;
    const isc_beam_merge_args &a = *args;
    if (!a.top_val || !a.top_idx || !a.score_in || !a.score_out || !a.last_in || !a.last_out || !a.words_in ||
        !a.words_out || !a.len_in || !a.len_out || !a.done || !a.gather || !a.live)
        return ISC_E_NULL;
    if (a.n_img <= 0 || a.beam <= 0 || a.beam > ISC_BEAM_MAX || a.T <= 0 || a.t < 0 || a.t >= a.T) return ISC_E_SHAPE;
    hipLaunchKernelGGL(beam_merge_kernel, dim3(a.n_img), dim3(64), 0, (hipStream_t)stream, a);
    ISC_LAUNCH_CHECK();
    return ISC_OK;
}

// ------------------------------------------------------------------ diverse beam search: the merge, group by group
// The search's `beam` rows form `groups` groups of bp = beam / groups ranks; group g's candidates are those of its own
// parents (insertion order as above: a contiguous range of the candidate table), ranked by
//     key = (s_parent + (double)logp) - lambda * (double)c,    c = tokens appended by the winners of groups < g that equal
// the candidate's (a carried candidate: its score).  One add, one multiply, one subtract - never an FMA, so that the host
// restatement and both kernels agree in bits.  The stored score is the un-augmented sum.
__device__ __forceinline__ double beam_group_key(double s, double lambda, int c) {
#pragma clang fp contract(off)
    const double pen = lambda * (double)c;
    return s - pen;
}
static inline bool beam_groups_ok(int beam, int groups, double lambda) {
    return groups >= 1 && beam % groups == 0 && lambda >= 0.0 && lambda <= 1.79769313486231570e308;   // (NaN fails both)
}

__global__ __launch_bounds__(64) void beam_merge_groups_kernel(const isc_beam_merge_args a, const int groups,
                                                               const double lambda) {
    __shared__ double cs[ISC_BEAM_MAX * ISC_BEAM_MAX], ckey[ISC_BEAM_MAX * ISC_BEAM_MAX];
    __shared__ long long ctok[ISC_BEAM_MAX * ISC_BEAM_MAX], chosen[ISC_BEAM_MAX];    // chosen: appended token by rank, -1 = carried
    __shared__ int cpar[ISC_BEAM_MAX * ISC_BEAM_MAX], ccar[ISC_BEAM_MAX * ISC_BEAM_MAX], coff[ISC_BEAM_MAX + 1];
    __shared__ int s_all_ended;
    const int i = blockIdx.x, tid = threadIdx.x, beam = a.beam, T = a.T, rows = a.n_img * beam, base = i * beam;
    const int bp = beam / groups;
    if (a.done[i]) {                      // frozen image: as beam_merge_kernel
        for (int k = tid; k < beam; k += 64) {
            a.gather[base + k] = base + k + rows;
            a.last_out[base + k] = a.last_in[base + k];
            a.score_out[base + k] = a.score_in[base + k];
            a.len_out[base + k] = a.len_in[base + k];
        }
        for (int e = tid; e < beam * T; e += 64) a.words_out[(long long)base * T + e] = a.words_in[(long long)base * T + e];
        return;
    }
    // parents: every row; at t == 0 the first row of every group (the rows of a search all decode the same step 0)
    if (tid == 0) {
        int off = 0, all_ended = 1;
        for (int k = 0; k < beam; ++k) {
            coff[k] = off;
            if (a.t == 0 && k % bp != 0) continue;
            const int ended = a.t > 0 && a.last_in[base + k] == a.eos_id;
            off += ended ? 1 : beam;
            all_ended &= ended;
        }
        coff[beam] = off;
        s_all_ended = all_ended;
    }
    __syncthreads();
    for (int e = tid; e < beam * beam; e += 64) {
        const int k = e / beam, j = e % beam, row = base + k;
        if (a.t == 0 && k % bp != 0) continue;
        const int ended = a.t > 0 && a.last_in[row] == a.eos_id;
        if (ended) {
            if (j == 0) { const int c = coff[k]; cs[c] = a.score_in[row]; ctok[c] = a.last_in[row]; cpar[c] = k; ccar[c] = 1; }
        } else {
            const int c = coff[k] + j;
            cs[c] = a.score_in[row] + (double)a.top_val[(long long)row * beam + j];
            ctok[c] = a.top_idx[(long long)row * beam + j];
            cpar[c] = k; ccar[c] = 0;
        }
    }
    __syncthreads();
    for (int g = 0; g < groups; ++g) {
        const int lo = coff[g * bp], hi = coff[(g + 1) * bp], c = lo + tid;      // hi - lo <= bp * beam <= 32
        if (c < hi) {
            int cnt = 0;
            if (!ccar[c])
                for (int s = 0; s < g * bp; ++s) cnt += chosen[s] == ctok[c];
            ckey[c] = ccar[c] ? cs[c] : beam_group_key(cs[c], lambda, cnt);
        }
        __syncthreads();
        if (c < hi) {
            const double key = ckey[c];
            int rank = 0;
            for (int j = lo; j < hi; ++j) rank += (ckey[j] > key) || (ckey[j] == key && j < c);
            if (rank < bp) {
                const int par = cpar[c], car = ccar[c], dst = base + g * bp + rank, srow = base + par;
                chosen[g * bp + rank] = car ? -1 : ctok[c];
                a.score_out[dst] = cs[c];
                a.last_out[dst] = ctok[c];
                a.gather[dst] = car ? srow + rows : srow;
                const int len = a.len_in[srow];
                for (int e = 0; e < T; ++e) a.words_out[(long long)dst * T + e] = a.words_in[(long long)srow * T + e];
                if (!car && len < T) a.words_out[(long long)dst * T + len] = ctok[c];
                a.len_out[dst] = len + (car ? 0 : 1);
            }
        }
        __syncthreads();
    }
    if (tid == 0) {
        if (s_all_ended) a.done[i] = 1;
        else atomicAdd(&a.live[a.t + 1], 1);
    }
}

extern "C" int isc_beam_merge_groups(const isc_beam_merge_args *args, int groups, double lambda, void *stream) {
    if (!args) return ISC_E_NULL;
    const isc_beam_merge_args &a = *args;
    if (!a.top_val || !a.top_idx || !a.score_in || !a.score_out || !a.last_in || !a.last_out || !a.words_in ||
        !a.words_out || !a.len_in || !a.len_out || !a.done || !a.gather || !a.live)
        return ISC_E_NULL;
    if (a.n_img <= 0 || a.beam <= 0 || a.beam > ISC_BEAM_MAX || a.T <= 0 || a.t < 0 || a.t >= a.T) return ISC_E_SHAPE;
    if (!beam_groups_ok(a.beam, groups, lambda)) return ISC_E_SHAPE;
    hipLaunchKernelGGL(beam_merge_groups_kernel, dim3(a.n_img), dim3(64), 0, (hipStream_t)stream, a, groups, lambda);
    ISC_LAUNCH_CHECK();
    return ISC_OK;
}

// New recurrent state of every beam row: out[p, r, :] = (gather[r] < rows ? next : current)[p, gather[r] % rows, :]
// for the P = 4 planes (h|c x layer) of a [P, rows, H] state - one launch instead of a concatenation + index_select.
__global__ __launch_bounds__(256) void beam_gather_kernel(const float *nxt, const float *cur, const int64_t *gather,
                                                          float *out, int rows, int H) {
    const int r = blockIdx.x, p = blockIdx.y;
    const long long g = gather[r];
    const float *src = (g < rows ? nxt : cur) + ((long long)p * rows + (g < rows ? g : g - rows)) * H;
    float *dst = out + ((long long)p * rows + r) * H;
    for (int i = threadIdx.x; i < (H >> 2); i += 256)
        reinterpret_cast<float4 *>(dst)[i] = reinterpret_cast<const float4 *>(src)[i];
}

extern "C" int isc_beam_gather(const float *state_next, const float *state_cur, const int64_t *gather, float *out,
                               int planes, int rows, int H, void *stream) {
    if (!state_next || !state_cur || !gather || !out) return ISC_E_NULL;
    if (planes <= 0 || rows <= 0 || H <= 0 || (H & 3)) return ISC_E_SHAPE;
    if (!isc_aligned16(state_next) || !isc_aligned16(state_cur) || !isc_aligned16(out)) return ISC_E_ALIGN;
    hipLaunchKernelGGL(beam_gather_kernel, dim3(rows, planes), dim3(256), 0, (hipStream_t)stream, state_next, state_cur,
                       gather, out, rows, H);
    ISC_LAUNCH_CHECK();
    return ISC_OK;
}

// ------------------------------------------------------------------ beam search: ban lists (n-gram blocking, minimum length)
// isc_beam_ngram_ban: one wave64 per candidate row.  The row's last n - 1 words (`pre`) sit in registers; lane l of
// chunk c tests position j = 64 c + l: does the (n - 1)-gram in front of w[j] equal `pre`?  The ballot of a chunk
// and the population count of the lanes below place every match at its rank, so the list is in ascending j with
// duplicates kept - the order the host restatement produces - without atomics or LDS.
__global__ __launch_bounds__(64) void beam_ngram_ban_kernel(const isc_beam_ngram_ban_args a) {
    if (a.live_in != nullptr && *a.live_in == 0) return;      // (uniform: the search has ended)
    const int row = blockIdx.x, lane = threadIdx.x, n = a.no_repeat_ngram, T = a.T;
    const int64_t *w = a.words + (long long)row * T;
    int64_t *out = a.ban_ids + (long long)row * a.ban_ld;
    int L = a.len[row];
    L = L < 0 ? 0 : L;
    L = L > a.t ? a.t : L;                                    // (t < T: every index below stays inside the row)
    int cnt = 0;
    if (n >= 1 && L >= n - 1) {
        int64_t pre[3] = {0, 0, 0};                           // pre[k] = w[L - 1 - k], k < n - 1
#pragma unroll
        for (int k = 0; k < 3; ++k)
            if (k < n - 1) pre[k] = w[L - 1 - k];
        for (int j0 = 0; j0 < L; j0 += 64) {
            const int j = j0 + lane;
            bool match = j >= n - 1 && j < L;
            int64_t wj = 0;
            if (match) {
                wj = w[j];
#pragma unroll
                for (int k = 0; k < 3; ++k)
                    if (k < n - 1) match = match && (w[j - 1 - k] == pre[k]);
            }
            const unsigned long long bal = __ballot(match);
            const int pos = cnt + __popcll(bal & ((1ull << lane) - 1ull));
            if (match && pos < a.ban_ld) out[pos] = wj;
            cnt += __popcll(bal);
        }
    }
    if (a.t < a.min_len) {
        if (lane == 0 && cnt < a.ban_ld) out[cnt] = a.eos_id;
        ++cnt;
    }
    if (lane == 0) a.ban_cnt[row] = cnt < a.ban_ld ? cnt : (int)a.ban_ld;
}

extern "C" int isc_beam_ngram_ban(const isc_beam_ngram_ban_args *args, void *stream) {
    if (!args) return ISC_E_NULL;
    const isc_beam_ngram_ban_args &a = *args;
    if (!a.words || !a.len || !a.ban_ids || !a.ban_cnt) return ISC_E_NULL;
    if (a.rows <= 0 || a.T <= 0 || a.T > 256 || a.t < 0 || a.t >= a.T || a.no_repeat_ngram < 0 || a.no_repeat_ngram > 4 ||
        a.min_len < 0 || a.min_len > a.T || a.ban_ld < a.T)
        return ISC_E_SHAPE;
    hipLaunchKernelGGL(beam_ngram_ban_kernel, dim3(a.rows), dim3(64), 0, (hipStream_t)stream, a);
    ISC_LAUNCH_CHECK();
    return ISC_OK;
}

// ------------------------------------------------------------------ row statistics helper
// Folds the per-tile (max, sumexp, argmax) triples of one row: returns the global max, its
// vocabulary index (smallest index on ties) and S = sum exp(x - gmax).  All 64 lanes get
// the result.
// Numerics status (isc_status, include/insenticap_hip.h): word 0 = a row of vocabulary statistics held a non-finite
// maximum or sum.  Every decode path folds the step's tile statistics through fold_row_stats (roll-out finalize,
// scheduled sampling, the log-softmax passes, beam top-k), so whatever went non-finite upstream in the step - an operand
// beyond the split-f16 domain |x| < 65504 whose hi plane became inf, a NaN feature (ReLU lets NaN through: isc_relu) -
// is flagged within the same step at no measurable cost (one compare per row) instead of surfacing as garbage tokens.
ISC_STATUS_DECL(pw)

__device__ __forceinline__ void fold_row_stats(const float *pmax, const float *psum, const int *pidx,
                                               int n_tile, int lane, float &gmax, int &gidx, float &S) {
    if (fold_row_stats_impl(pmax, psum, pidx, n_tile, lane, gmax, gidx, S) && lane == 0)
        isc_flag_pw(ISC_STATUS_WORD_STATS);
}

// ------------------------------------------------------------------ roll-out step
struct DevRollout {
    int B, V, T, t, n_tile, W;
    const float *part_max, *part_sum;
    const int *part_idx;
    const float *logits;
    long long ld_logits;
    const int64_t *forced;
    const float *sample_u;
    long long eos_id;
    int64_t *seq;
    float *seq_logprobs, *seq_masks;
    int *unfinished, *alive;
    int64_t *raw_tokens;
    const float *emb, *xt_add;
    float *xt_next;
};

// Inverse-CDF sampling from softmax over one row, in vocabulary order, by one wavefront.  Two levels: the
// vocabulary kernel already left sum exp(x - tile max) per 128-column tile, so the tile holding the target
// mass is found by a prefix over n_tile values and only its 128 columns are exponentiated (4 wave-prefix
// rounds per row instead of V/64 = 157: 300 us -> ~12 us per roll-out step at B=512).
// Element mass = exp(x[i] - shift) * scale: (gmax, 1) for raw logits, (0, S) for log-probabilities, so that
// both agree with the tile masses psum[j] * exp(pmax[j] - gmax) and with target = u * S.
// Returns the drawn id, or -1 when rounding put the target past the total mass.
// (tile_w(j) = the mass of tile j, skip(i) = column i may not be drawn: the constrained finalize hands in corrected tile
// masses and its banned ids; sample_two_level below is the plain form.)
template <class TileW, class Skip>
__device__ __forceinline__ int sample_two_level_t(const float *x, float shift, float scale, TileW tile_w, Skip skip,
                                                  int n_tile, int V, float target, int lane) {
    auto wave_incl = [&](float v) __attribute__((always_inline)) {
#pragma unroll
        for (int o = 1; o < 64; o <<= 1) {
            const float n = __shfl_up(v, o, 64);
            if (lane >= o) v += n;
        }
        return v;
    };
    float run = 0.f;
    int tile = -1;
    for (int base = 0; base < n_tile && tile < 0; base += 64) {
        const int j = base + lane;
        const float w = (j < n_tile) ? tile_w(j) : 0.f;
        const float incl = wave_incl(w);
        const unsigned long long hit = __ballot((run + incl > target) && j < n_tile);
        if (hit) {
            const int l = __ffsll((long long)hit) - 1;
            tile = base + l;
            run += __shfl(incl - w, l, 64);       // mass in front of the tile
        } else {
            run += __shfl(incl, 63, 64);
        }
    }
    if (tile < 0) return -1;
    int pick = -1;
    for (int c = 0; c < 2 && pick < 0; ++c) {
        const int i = tile * 128 + c * 64 + lane;
        const float e = (i < V && !skip(i)) ? expf(x[i] - shift) * scale : 0.f;
        const float incl = wave_incl(e);
        const unsigned long long hit = __ballot((run + incl > target) && i < V && !skip(i));
        if (hit) pick = tile * 128 + c * 64 + __ffsll((long long)hit) - 1;
        run += __shfl(incl, 63, 64);
    }
    for (int c = 1; c >= 0 && pick < 0; --c) {    // the tile's own sum rounded differently: its last column that may be
        const int i = tile * 128 + c * 64 + lane; // drawn (nothing skipped: min(tile * 128 + 127, V - 1))
        const unsigned long long ok = __ballot(i < V && !skip(i));
        if (ok) pick = tile * 128 + c * 64 + 63 - __clzll((long long)ok);
    }
    return pick;
}

__device__ __forceinline__ int sample_two_level(const float *x, float shift, float scale, const float *pm,
                                                const float *ps, int n_tile, int V, float gmax, float target,
                                                int lane) {
    return sample_two_level_t(x, shift, scale, [&](int j) { return ps[j] * expf(pm[j] - gmax); },
                              [](int) { return false; }, n_tile, V, target, lane);
}

// The commit stage of a decode step, the one place where every form of the finalize writes what the step decided: the
// NT threads that worked on row b hand in its chosen token `it`, its log-probability `lp` (thread 0's counts) and the
// row's `unfinished` flag as it was read before the step.  Thread 0 stores seq / seq_masks / seq_logprobs / raw_tokens /
// unfinished, all NT threads stream xt_next = relu(emb[fed token]) (+ xt_add) as float4s.  Returns the row's next flag.
template <int NT>
__device__ __forceinline__ int finalize_commit(const DevRollout &R, int b, long long it, float lp, int unf, int tid) {
    long long itm;
    const int u2 = finalize_advance(unf, it, R.eos_id, itm);
    if (tid == 0) {
        const long long o = (long long)b * R.T + R.t;
        R.seq_masks[o] = (float)unf;
        R.seq[o] = itm;
        R.seq_logprobs[o] = lp;
        if (R.raw_tokens) R.raw_tokens[o] = it;
        R.unfinished[b] = u2;
    }
    if (R.xt_next) {
        const float4 *src = reinterpret_cast<const float4 *>(R.emb + itm * R.W);
        const float4 *ad = R.xt_add ? reinterpret_cast<const float4 *>(R.xt_add + (long long)b * R.W) : nullptr;
        float4 *dst = reinterpret_cast<float4 *>(R.xt_next + (long long)b * R.W);
        for (int i = tid; i < (R.W >> 2); i += NT) {
            float4 v = src[i];
            v.x = fmaxf(v.x, 0.f); v.y = fmaxf(v.y, 0.f); v.z = fmaxf(v.z, 0.f); v.w = fmaxf(v.w, 0.f);
            if (ad) { const float4 a = ad[i]; v.x += a.x; v.y += a.y; v.z += a.z; v.w += a.w; }
            dst[i] = v;
        }
    }
    return u2;
}

// The plain choice of row b by one wavefront: the forced token, a draw against sample_u, or the arg-max, and the
// model's log-probability of it.  Stores nothing.
__device__ __forceinline__ void rollout_choose_row(const DevRollout &R, int b, int lane, long long &it, float &lp) {
    float gmax, S;
    int gidx;
    fold_row_stats(R.part_max + (long long)b * R.n_tile, R.part_sum + (long long)b * R.n_tile,
                   R.part_idx + (long long)b * R.n_tile, R.n_tile, lane, gmax, gidx, S);
    const float logS = logf(S);
    if (R.forced) {
        it = R.forced[(long long)b * R.T + R.t];
        lp = (R.logits[(long long)b * R.ld_logits + it] - gmax) - logS;
    } else if (R.sample_u) {
        const float *x = R.logits + (long long)b * R.ld_logits;
        int pick = sample_two_level(x, gmax, 1.0f, R.part_max + (long long)b * R.n_tile,
                                    R.part_sum + (long long)b * R.n_tile, R.n_tile, R.V, gmax,
                                    R.sample_u[(long long)b * R.T + R.t] * S, lane);
        if (pick < 0) pick = gidx;  // target == S after rounding
        it = pick;
        lp = (x[it] - gmax) - logS;
    } else {
        it = gidx;
        lp = -logS;  // log_softmax at the arg-max: (x_max - x_max) - log S
    }
}

// ------------------------------------------------------------------ token constraints (the beam's rules in the roll-out)
// At most ISC_CON_MAX ids of a row may not be chosen at a step: the caller's ban list (with <EOS> appended while
// t < min_len; unused slots -1) and, under no_repeat, the token fed into the step - seq[b, t-1], first_id at t = 0.
// Duplicates are fine.  The tile statistics know nothing of them, and subtracting a banned mass from the row sum would
// cancel to noise under a dominant banned token: the (max, arg-max, sum-exp) of every 128-column tile that holds a banned
// id - at most ISC_CON_MAX tiles - are recomputed over its allowed columns, and the fold and the two-level draw run on the
// corrected statistics.  A tile without an allowed column has maximum -inf and mass 0.
struct DevCons {
    int ban[ISC_CON_MAX - 1];
    int no_repeat, first_id;
};

// the row's banned ids (-1: unused slot)
__device__ __forceinline__ void con_row_ids(const DevRollout &R, const DevCons &C, int b, int (&ids)[ISC_CON_MAX]) {
#pragma unroll
    for (int k = 0; k < ISC_CON_MAX - 1; ++k) ids[k] = C.ban[k];
    ids[ISC_CON_MAX - 1] = !C.no_repeat ? -1 : R.t == 0 ? C.first_id : (int)R.seq[(long long)b * R.T + R.t - 1];
}

__device__ __forceinline__ bool con_banned(const int (&ids)[ISC_CON_MAX], int i) {
    bool hit = false;
#pragma unroll
    for (int k = 0; k < ISC_CON_MAX; ++k) hit |= ids[k] == i;
    return hit;
}

// The constrained choice of row b by one wavefront: the arg-max, or a draw against sample_u, over the allowed ids, and
// the model's log-probability of it.  Stores nothing.
__device__ __forceinline__ void rollout_choose_con_row(const DevRollout &R, const DevCons &C, int b, int lane,
                                                       long long &it, float &lp) {
    const float *pm = R.part_max + (long long)b * R.n_tile, *ps = R.part_sum + (long long)b * R.n_tile;
    const int *pi = R.part_idx + (long long)b * R.n_tile;
    const float *x = R.logits + (long long)b * R.ld_logits;
    float gmax, S;                          // the full row: seq_logprobs stays the MODEL's log_softmax(x)[token]
    int gidx;
    fold_row_stats(pm, ps, pi, R.n_tile, lane, gmax, gidx, S);
    int ids[ISC_CON_MAX], ct[ISC_CON_MAX], ci[ISC_CON_MAX];
    float cm[ISC_CON_MAX], cs[ISC_CON_MAX];
    con_row_ids(R, C, b, ids);
    // ---- the tiles that hold a banned id, each once: their statistics over the allowed columns (wave-uniform)
#pragma unroll
    for (int k = 0; k < ISC_CON_MAX; ++k) {
        int tl = ids[k] >= 0 ? ids[k] >> 7 : -1;
#pragma unroll
        for (int j = 0; j < k; ++j)
            if (ct[j] == tl) tl = -1;
        ct[k] = tl; cm[k] = -INFINITY; cs[k] = 0.f; ci[k] = 0;
        if (tl < 0) continue;
        const int i0 = tl * 128 + lane, i1 = i0 + 64;
        const bool ok0 = i0 < R.V && !con_banned(ids, i0), ok1 = i1 < R.V && !con_banned(ids, i1);
        const float x0 = ok0 ? x[i0] : -INFINITY, x1 = ok1 ? x[i1] : -INFINITY;
        float mx = -INFINITY;
        int ix = 0x7fffffff;
        if (ok0) { mx = x0; ix = i0; }
        if (ok1 && (x1 > mx || ix == 0x7fffffff)) { mx = x1; ix = i1; }       // (equal values: i0 < i1 stays)
        full_argmax(mx, ix);
        if (ix != 0x7fffffff) {             // (uniform) else: every column of the tile is banned - it contributes nothing
            cm[k] = mx; cs[k] = full_sum((ok0 ? expf(x0 - mx) : 0.f) + (ok1 ? expf(x1 - mx) : 0.f)); ci[k] = ix;
        }
    }
    auto tile = [&](int j, float &m, float &s, int &id) __attribute__((always_inline)) {
        m = pm[j]; s = ps[j]; id = pi[j];
#pragma unroll
        for (int k = 0; k < ISC_CON_MAX; ++k)
            if (ct[k] == j) { m = cm[k]; s = cs[k]; id = cs[k] > 0.f ? ci[k] : 0x7fffffff; }
    };
    // ---- the fold of fold_row_stats_impl over the corrected statistics: (amax, aidx, A) of the allowed ids
    float amax = -INFINITY, A = 0.f;
    int aidx = 0x7fffffff;
    for (int j = lane; j < R.n_tile; j += 64) {
        float m, s;
        int id;
        tile(j, m, s, id);
        if (m > amax || (m == amax && id < aidx)) { amax = m; aidx = id; }
    }
    full_argmax(amax, aidx);
    for (int j = lane; j < R.n_tile; j += 64) {
        float m, s;
        int id;
        tile(j, m, s, id);
        if (s > 0.f) A += s * expf(m - amax);
    }
    A = full_sum(A);
    if (aidx == 0x7fffffff) aidx = gidx;    // (a non-finite row: flagged by the fold above)
    it = aidx;                              // arg-max over the allowed ids, ties to the smaller id
    if (R.sample_u) {
        const int pick = sample_two_level_t(
            x, amax, 1.0f,
            [&](int j) { float m, s; int id; tile(j, m, s, id); return s > 0.f ? s * expf(m - amax) : 0.f; },
            [&](int i) { return con_banned(ids, i); }, R.n_tile, R.V,
            R.sample_u[(long long)b * R.T + R.t] * A, lane);
        if (pick >= 0) it = pick;           // (else: target == A after rounding)
    }
    lp = (x[it] - gmax) - logf(S);
}

// The launch skeleton of the wave-per-row finalize, plain or constrained (CON): ONE row per wave - every row's dependent
// chain (two strided sweeps, a dozen cross-lane steps, logf, stores) runs at the same time as all the others - and the
// count of still-unfinished rows reduced inside the workgroup, so that the `alive` counter sees one atomic per WAVES rows
// (one per row, 4096 same-address atomics used to dominate this kernel).  Two launch shapes: WAVES = 4 up to 1024 rows,
// 16 (the wide one) beyond.
template <int WAVES, bool CON>
__device__ __forceinline__ void rollout_finalize_body(const DevRollout &R, const DevCons &C) {
    __shared__ int cnt[WAVES];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    // the reference `break`s once no row is unfinished (captioner.py:343-344): later steps
    // leave seq / seq_logprobs / seq_masks at their zero initialisation
    if (R.alive[R.t] == 0) return;          // block-uniform
    const int b = blockIdx.x * WAVES + wave;
    int alive = 0;
    if (b < R.B) {
        long long it;
        float lp;
        if (CON) rollout_choose_con_row(R, C, b, lane, it, lp);
        else rollout_choose_row(R, b, lane, it, lp);
        alive = finalize_commit<64>(R, b, it, lp, R.unfinished[b], lane);
    }
    if (lane == 0) cnt[wave] = alive;
    __syncthreads();
    if (threadIdx.x == 0) {
        int tot = 0;
#pragma unroll
        for (int w = 0; w < WAVES; ++w) tot += cnt[w];
        if (tot) atomicAdd(&R.alive[R.t + 1], tot);
    }
}

__global__ __launch_bounds__(256) void rollout_finalize_kernel(const DevRollout R) {
    rollout_finalize_body<4, false>(R, DevCons());
}

__global__ __launch_bounds__(1024) void rollout_finalize_wide_kernel(const DevRollout R) {
    rollout_finalize_body<16, false>(R, DevCons());
}

template <int WAVES>
__global__ __launch_bounds__(WAVES * 64) void rollout_finalize_con_kernel(const DevRollout R, const DevCons C) {
    rollout_finalize_body<WAVES, true>(R, C);
}

static std::atomic<long long> g_finalize_launches{0};
extern "C" long long isc_rollout_finalize_launches(void) { return g_finalize_launches.load(); }

static DevRollout dev_rollout(const isc_rollout_step *s) {
    DevRollout R;
    R.B = s->B; R.V = s->V; R.T = s->T; R.t = s->t; R.n_tile = s->n_tile; R.W = s->W;
    R.part_max = s->part_max; R.part_sum = s->part_sum; R.part_idx = s->part_idx;
    R.logits = s->logits; R.ld_logits = s->ld_logits; R.forced = s->forced; R.sample_u = s->sample_u;
    R.eos_id = s->eos_id; R.seq = s->seq; R.seq_logprobs = s->seq_logprobs; R.seq_masks = s->seq_masks;
    R.unfinished = s->unfinished; R.alive = s->alive; R.raw_tokens = s->raw_tokens;
    R.emb = s->emb; R.xt_add = s->xt_add; R.xt_next = s->xt_next;
    return R;
}

// What every finalize entry asks of its (non-null) isc_rollout_step, refused in the order the entries have always used: a
// missing pointer (ISC_E_NULL), then a size (ISC_E_SHAPE), then alignment (ISC_E_ALIGN).  `own_null` / `own_shape`: the
// calling entry's own conditions of the first two kinds, so that they keep their place in that order.
static int rollout_step_check(const isc_rollout_step *s, bool own_null, bool own_shape) {
    if (own_null || !s->part_max || !s->part_sum || !s->part_idx || !s->seq || !s->seq_logprobs || !s->seq_masks ||
        !s->unfinished || !s->alive || !s->emb)
        return ISC_E_NULL;
    if (own_shape || s->B <= 0 || s->T <= 0 || s->t < 0 || s->t >= s->T || (s->W & 3)) return ISC_E_SHAPE;
    // xt_next = relu(emb[token]) (+ xt_add) moves float4s (finalize_commit)
    if (s->xt_next && (!isc_aligned16(s->emb) || !isc_aligned16(s->xt_next) || (s->xt_add && !isc_aligned16(s->xt_add))))
        return ISC_E_ALIGN;
    return ISC_OK;
}

// (any n_tile: the few-row path keeps its statistics per rows_stats_tile(V) <= 64 columns; greedy reads no logits)
extern "C" int isc_rollout_finalize(const isc_rollout_step *s, void *stream) {
    if (!s) return ISC_E_NULL;
    if (const int rc = rollout_step_check(s, (s->forced || s->sample_u) && !s->logits, false)) return rc;
    const DevRollout R = dev_rollout(s);
    if (s->B > 1024)
        hipLaunchKernelGGL(rollout_finalize_wide_kernel, dim3((s->B + 15) / 16), dim3(1024), 0, (hipStream_t)stream, R);
    else
        hipLaunchKernelGGL(rollout_finalize_kernel, dim3((s->B + 3) / 4), dim3(256), 0, (hipStream_t)stream, R);
    ISC_LAUNCH_CHECK();
    ++g_finalize_launches;
    return ISC_OK;
}

// ------------------------------------------------------------------ filtered sampling: temperature, top-k, top-p
// The sampled roll-out's finalize with a per-row decision, on the device, of WHICH tokens may be drawn.  Ranking is by raw
// logit (largest first, ties to the smaller id): one 64-bit key K = (descending image of x : id), all distinct, ascending
// K = rank order.  The kept set is a rank prefix, i.e. {K <= K*}; K* is found by SELECTION, never by sorting the row:
//   1. a 256-bucket histogram (integer counts, integer masses) over buckets LINEAR in (max - x) - monotone in x, so a
//      bucket is a rank interval - and a scan over the buckets find the bucket that holds the boundary;
//   2. that bucket's few elements are ranked against each other (all pairs) - or, when it holds more than 256 (rows of
//      tied logits), by a radix descent over the bits of K, eight levels of 256 buckets.
// Top-k selects by count; top-p then selects by mass among the survivors, against top_p * (their summed mass).
// Masses are FIXED POINT: w = exp((x - max) / T) in (0, 1] scaled to 2^32 in a 64-bit sum.  Integer adds commute, so the
// LDS atomics of the histograms and every reduction give the same bits on every run; an element's rounding error is
// 2^-33 of the row's largest mass (V = 20000: <= 2.3e-6 of the total if every error had one sign, ~1e-8 as they fall).
// The draw is the inverse CDF over the kept set in vocabulary order, against u * (kept mass), in the same integers.
// One 256-thread workgroup per row, the row staged in LDS once (V <= ISC_FLT_STAGE_MAX; longer rows are re-read from
// L2); a workgroup walks rows blockIdx.x, + gridDim.x, ... so that `alive` sees one atomic per workgroup.
#define ISC_FLT_STAGE_MAX 12288
#define ISC_FLT_MAX_GRID 768            // 3 workgroups of ~47 KB LDS per CU
#define ISC_FLT_MASS_SPAN 23.0f         // exp(-23) * 2^32 < 1/2: beyond (max - x) / T = 23 a mass rounds to zero

struct DevFilter {
    float c_exp;       // log2(e) / temperature
    float tau;
    int top_k;         // 0: off
    float top_p;       // >= 1: off
    float *slp;        // optional [B,T]: log-probability under the sampled distribution
    int staged;        // row in LDS
    // isc_rollout_finalize_saved (all or none; ban optional): what the backward of `slp` reads, per (b, t)
    long long *sv_kstar;
    float *sv_gmax, *sv_logz;
    int *sv_ban;       // [B,T,ISC_CON_MAX]
};

// (flt_key: flt_key.h - shared with the backward)

__device__ __forceinline__ unsigned flt_mass(float x, float gmax, float c_exp) {
    const float e = __builtin_amdgcn_exp2f(fminf((x - gmax) * c_exp, 0.f)) * 4294967296.0f;
    return (unsigned)__builtin_rintf(fminf(e, 4294967040.0f));       // NaN -> 0
}

__device__ __forceinline__ int flt_bucket(float x, float gmax, float cb) {
    return (int)fminf(fmaxf((gmax - x) * cb, 0.f), 255.f);           // NaN -> 0
}

// exclusive prefix of (c, m) over the 256 threads of the workgroup, in thread order
__device__ __forceinline__ void flt_scan(unsigned &c, isc_u64 &m, unsigned *s32, isc_u64 *s64, int tid) {
    const int lane = tid & 63, wave = tid >> 6;
    unsigned ci = c;
    isc_u64 mi = m;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
        const unsigned nc = __shfl_up(ci, o, 64);
        const isc_u64 nm = __shfl_up(mi, o, 64);
        if (lane >= o) { ci += nc; mi += nm; }
    }
    __syncthreads();                      // (the scratch words may still be read from the previous use)
    if (lane == 63) { s32[wave] = ci; s64[wave] = mi; }
    __syncthreads();
    unsigned bc = 0;
    isc_u64 bm = 0;
    for (int w = 0; w < wave; ++w) { bc += s32[w]; bm += s64[w]; }
    c = bc + ci - c;
    m = bm + mi - m;
}

// CON (isc_rollout_finalize_constrained): the row's banned ids read as -inf - written over the staged row in LDS, or
// replaced as the unstaged row is read.  The selection starts from Kstar = the last finite key instead of "every token",
// so that they are out of the ranking, the histograms, the kept mass and the draw; the masses are taken relative to the
// largest ALLOWED logit (an extra pass over the row finds it, with its id), seq_logprobs relative to the full row's.
#define ISC_FLT_KEY_FINITE 0xff7fffffffffffffull
template <bool CON>
__device__ __forceinline__ void rollout_finalize_filtered_body(const DevRollout &R, const DevFilter &F, const DevCons &C) {
    extern __shared__ float flt_row[];
    __shared__ isc_u64 h_mass[256], c_key[256], c_mass[256], s64[4], sh64[4];
    __shared__ unsigned h_cnt[256], s32[4];
    __shared__ int shi[4];
    __shared__ float shf[4];
    if (R.alive[R.t] == 0) return;          // block-uniform
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, V = R.V;
    int alive = 0;
    for (int b = blockIdx.x; b < R.B; b += gridDim.x) {
        const float *xg = R.logits + (long long)b * R.ld_logits;
        const float *xs_ = F.staged ? flt_row : xg;
        int ids[ISC_CON_MAX];
        if (CON) con_row_ids(R, C, b, ids);
        // (the unstaged constrained row: a banned id reads as -inf)
        auto xs = [&](int i) __attribute__((always_inline)) {
            return CON && !F.staged && con_banned(ids, i) ? -INFINITY : xs_[i];
        };
        const int unf = R.unfinished[b];    // (thread 0 rewrites it behind the barriers below)
        float gmax, S;
        int gidx;
        fold_row_stats(R.part_max + (long long)b * R.n_tile, R.part_sum + (long long)b * R.n_tile,
                       R.part_idx + (long long)b * R.n_tile, R.n_tile, lane, gmax, gidx, S);
        const float lp_max = gmax;          // the full row's: seq_logprobs is the MODEL's log-probability
        unsigned n_ban = 0;
        if (CON) {
            if (F.staged) {
                for (int i = tid; i < V; i += 256) flt_row[i] = xg[i];
                __syncthreads();
#pragma unroll
                for (int k = 0; k < ISC_CON_MAX; ++k)
                    if (tid == k && ids[k] >= 0) flt_row[ids[k]] = -INFINITY;
                __syncthreads();
            }
#pragma unroll
            for (int k = 0; k < ISC_CON_MAX; ++k) {      // distinct banned ids
                bool fresh = ids[k] >= 0;
#pragma unroll
                for (int j = 0; j < k; ++j) fresh &= ids[j] != ids[k];
                n_ban += fresh;
            }
            // the largest allowed logit and its id (ties to the smaller id): the smallest key
            isc_u64 kb = ~0ull;
            for (int i = tid; i < V; i += 256) {
                const isc_u64 K = flt_key(xs(i), i);
                kb = K < kb ? K : kb;
            }
#pragma unroll
            for (int o = 32; o > 0; o >>= 1) {
                const isc_u64 K = __shfl_xor(kb, o, 64);
                kb = K < kb ? K : kb;
            }
            if (lane == 0) sh64[wave] = kb;
            __syncthreads();
            for (int w = 0; w < 4; ++w) kb = sh64[w] < kb ? sh64[w] : kb;
            gidx = (int)(unsigned)kb;
            gmax = xs(gidx);
            __syncthreads();                // (sh64 is the selection's below)
        }
        // ---- pass 1: stage the row, its minimum, its total mass
        isc_u64 wsum = 0;
        float mn = INFINITY;
        if (CON) {
            for (int i = tid; i < V; i += 256) {
                const float x = xs(i);
                if (x > -INFINITY) mn = fminf(mn, x);
                wsum += flt_mass(x, gmax, F.c_exp);
            }
        } else if (F.staged && !(R.ld_logits & 3) && !(V & 3) && !((uintptr_t)R.logits & 15)) {
            for (int i = tid * 4; i < V; i += 1024) {
                const float4 v = *reinterpret_cast<const float4 *>(xg + i);
                *reinterpret_cast<float4 *>(flt_row + i) = v;
                mn = fminf(fminf(mn, fminf(v.x, v.y)), fminf(v.z, v.w));
                wsum += (isc_u64)flt_mass(v.x, gmax, F.c_exp) + flt_mass(v.y, gmax, F.c_exp);
                wsum += (isc_u64)flt_mass(v.z, gmax, F.c_exp) + flt_mass(v.w, gmax, F.c_exp);
            }
        } else {
            for (int i = tid; i < V; i += 256) {
                const float x = xg[i];
                if (F.staged) flt_row[i] = x;
                mn = fminf(mn, x);
                wsum += flt_mass(x, gmax, F.c_exp);
            }
        }
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) {
            wsum += __shfl_xor(wsum, o, 64);
            mn = fminf(mn, __shfl_xor(mn, o, 64));
        }
        if (lane == 0) { s64[wave] = wsum; shf[wave] = mn; }
        __syncthreads();
        isc_u64 Wk = s64[0] + s64[1] + s64[2] + s64[3];            // mass of the survivors so far: every token
        const float xmin = fminf(fminf(shf[0], shf[1]), fminf(shf[2], shf[3]));
        unsigned Nk = (unsigned)V - n_ban;
        isc_u64 Kstar = CON ? ISC_FLT_KEY_FINITE : ~0ull;           // kept = {K <= Kstar}: every (allowed) token
        // ---- selection: pass 0 by count (top-k), pass 1 by mass (top-p) among pass 0's survivors
        for (int mode = 0; mode < 2; ++mode) {
            if (mode == 0 ? !(F.top_k > 0 && F.top_k < V) : !(F.top_p < 1.0f)) continue;      // uniform
            const isc_u64 Klim = Kstar, Wtot = Wk;
            const unsigned Ntot = Nk, klim = (unsigned)F.top_k;
            isc_u64 Mlim = (isc_u64)((double)F.top_p * (double)Wtot);
            if (Mlim < 1) Mlim = 1;                                 // rank 0 is always kept
            const float span = gmax - xmin;
            const float rr = mode == 0 ? span : fminf(span, ISC_FLT_MASS_SPAN * F.tau);
            const float cb = rr > 1e-30f ? 256.0f / rr : 0.f;
#define FLT_COND(C, M) (mode == 0 ? (C) < klim : (M) < Mlim)
            __syncthreads();
            h_cnt[tid] = 0; h_mass[tid] = 0;
            if (tid == 0) { shi[0] = -1; shi[1] = 0; shi[2] = 0; sh64[0] = 0; sh64[1] = 0; }
            __syncthreads();
            // bucket 255 takes everything beyond the span (by mass: the zero-mass tail): it gets no atomics, its count and
            // mass are what the others leave of the totals
            for (int i = tid; i < V; i += 256) {
                const float x = xs(i);
                if (flt_key(x, i) > Klim) continue;
                const int bk = flt_bucket(x, gmax, cb);
                if (bk < 255) {
                    atomicAdd(&h_cnt[bk], 1u);
                    atomicAdd(&h_mass[bk], (isc_u64)flt_mass(x, gmax, F.c_exp));
                }
            }
            __syncthreads();
            unsigned n = tid < 255 ? h_cnt[tid] : 0u, C = n;
            isc_u64 m = tid < 255 ? h_mass[tid] : 0ull, M = m;
            flt_scan(C, M, s32, s64, tid);
            if (tid == 255) { n = Ntot - C; m = Wtot - M; }
            if (n > 0 && FLT_COND(C, M)) atomicMax(&shi[0], tid);
            __syncthreads();
            const int bstar = shi[0];
            if (bstar < 0) continue;                                // (no survivor at all: a row of NaN keys) uniform
            __syncthreads();
            if (tid == bstar) { s32[0] = C; s32[1] = n; s64[0] = M; }
            __syncthreads();
            unsigned Cb = s32[0];
            const unsigned nstar = s32[1];
            isc_u64 Mb = s64[0];
            if (nstar <= 256) {
                // the boundary bucket's elements, ranked against each other
                for (int i = tid; i < V; i += 256) {
                    const float x = xs(i);
                    const isc_u64 K = flt_key(x, i);
                    if (K <= Klim && flt_bucket(x, gmax, cb) == bstar) {
                        const int slot = atomicAdd(&shi[1], 1);
                        if (slot < 256) { c_key[slot] = K; c_mass[slot] = flt_mass(x, gmax, F.c_exp); }
                    }
                }
                __syncthreads();
                if (tid < (int)nstar) {
                    const isc_u64 myK = c_key[tid], myM = c_mass[tid];
                    unsigned cnt = Cb;
                    isc_u64 ms = Mb;
                    for (int j = 0; j < (int)nstar; ++j) {
                        const isc_u64 kj = c_key[j], mj = c_mass[j];
                        if (kj < myK) { ++cnt; ms += mj; }
                    }
                    if (FLT_COND(cnt, ms)) {
                        atomicMax(&sh64[0], myK);
                        atomicAdd(&sh64[1], myM);
                        atomicAdd(&shi[2], 1);
                    }
                }
                __syncthreads();
                Kstar = sh64[0]; Wk = Mb + sh64[1]; Nk = Cb + (unsigned)shi[2];
            } else {
                // many elements in one bucket (tied logits): radix descent over the bits of K, most significant first
                isc_u64 prefix = 0, lastm = 0;
                for (int shift = 56; shift >= 0; shift -= 8) {
                    __syncthreads();
                    h_cnt[tid] = 0; h_mass[tid] = 0;
                    if (tid == 0) shi[0] = -1;
                    __syncthreads();
                    for (int i = tid; i < V; i += 256) {
                        const float x = xs(i);
                        const isc_u64 K = flt_key(x, i);
                        if (K <= Klim && flt_bucket(x, gmax, cb) == bstar && (shift == 56 || (K >> (shift + 8)) == prefix)) {
                            const int d = (int)((K >> shift) & 255);
                            atomicAdd(&h_cnt[d], 1u);
                            atomicAdd(&h_mass[d], (isc_u64)flt_mass(x, gmax, F.c_exp));
                        }
                    }
                    __syncthreads();
                    const unsigned nd = h_cnt[tid];
                    const isc_u64 md = h_mass[tid];
                    unsigned Cd = nd;
                    isc_u64 Md = md;
                    flt_scan(Cd, Md, s32, s64, tid);
                    if (nd > 0 && FLT_COND(Cb + Cd, Mb + Md)) atomicMax(&shi[0], tid);
                    __syncthreads();
                    const int dstar = shi[0] < 0 ? 0 : shi[0];
                    if (tid == dstar) { s32[0] = Cd; s64[0] = Md; s64[1] = md; }
                    __syncthreads();
                    Cb += s32[0]; Mb += s64[0]; lastm = s64[1];
                    prefix = (prefix << 8) | (unsigned)dstar;
                }
                Kstar = prefix; Wk = Mb + lastm; Nk = Cb + 1;
            }
#undef FLT_COND
        }
        // ---- draw: inverse CDF over the kept set in vocabulary order; thread t owns ids [t * chunk, (t + 1) * chunk)
        // (chunk odd: the threads' LDS reads fall on different banks)
        const int chunk = ((V + 255) >> 8) | 1;
        const int i0 = tid * chunk < V ? tid * chunk : V, i1 = i0 + chunk < V ? i0 + chunk : V;
        isc_u64 own = 0;
        for (int i = i0; i < i1; ++i) {
            const float x = xs(i);
            if (flt_key(x, i) <= Kstar) own += flt_mass(x, gmax, F.c_exp);
        }
        unsigned c0 = 0;
        isc_u64 ex = own;
        __syncthreads();
        if (tid == 0) shi[3] = -1;
        flt_scan(c0, ex, s32, s64, tid);
        const isc_u64 target = (isc_u64)((double)R.sample_u[(long long)b * R.T + R.t] * (double)Wk);
        if (own > 0 && ex <= target && target < ex + own) {          // exactly one thread (the masses sum to Wk > target)
            isc_u64 run = ex;
            int pick = i1 - 1;
            for (int i = i0; i < i1; ++i) {
                const float x = xs(i);
                if (flt_key(x, i) <= Kstar) run += flt_mass(x, gmax, F.c_exp);
                if (run > target) { pick = i; break; }
            }
            shi[3] = pick;
        }
        __syncthreads();
        const int pk = shi[3];
        const long long it = pk < 0 ? gidx : pk;                    // (a row without any mass: non-finite, flagged)
        // ---- the step's outputs (thread 0 alone holds the log-probabilities: it is the one that stores them)
        float lp = 0.f;
        if (tid == 0) {
            const float xi = xs_[it];
            lp = (xi - lp_max) - logf(S);                            // the MODEL's log-probability of the token
            const double logz = F.slp || F.sv_kstar ? log((double)Wk * (1.0 / 4294967296.0)) : 0.0;
            if (F.slp) F.slp[(long long)b * R.T + R.t] = (float)(((double)xi - (double)gmax) / (double)F.tau - logz);
            if (F.sv_kstar) {
                const long long o = (long long)b * R.T + R.t;
                F.sv_kstar[o] = (long long)Kstar; F.sv_gmax[o] = gmax; F.sv_logz[o] = (float)logz;
                if (CON && F.sv_ban) {
#pragma unroll
                    for (int k = 0; k < ISC_CON_MAX; ++k) F.sv_ban[o * ISC_CON_MAX + k] = ids[k];
                }
            }
        }
        const int u2 = finalize_commit<256>(R, b, it, lp, unf, tid);
        if (tid == 0) alive += u2;
        __syncthreads();                    // the row in LDS and the scratch words are the next row's
    }
    if (tid == 0 && alive) atomicAdd(&R.alive[R.t + 1], alive);
}

__global__ __launch_bounds__(256) void rollout_finalize_filtered_kernel(const DevRollout R, const DevFilter F) {
    rollout_finalize_filtered_body<false>(R, F, DevCons());
}

__global__ __launch_bounds__(256) void rollout_finalize_filtered_con_kernel(const DevRollout R, const DevFilter F,
                                                                            const DevCons C) {
    rollout_finalize_filtered_body<true>(R, F, C);
}

static bool flt_params_ok(const isc_sample_filter *f) {
    return f->temperature > 0.f && f->temperature <= 3.0e38f && f->top_k >= 0 && f->top_p > 0.f;     // NaN fails
}

// the filtered launch: a workgroup per row up to ISC_FLT_MAX_GRID, the staged row (if it is staged) as dynamic LDS
static dim3 flt_grid(const isc_rollout_step *s) { return dim3(s->B < ISC_FLT_MAX_GRID ? s->B : ISC_FLT_MAX_GRID); }
static size_t flt_lds(const isc_rollout_step *s) {
    return s->V <= ISC_FLT_STAGE_MAX ? (size_t)((s->V + 3) & ~3) * sizeof(float) : 0;
}

static DevFilter dev_filter(const isc_rollout_step *s, const isc_sample_filter *f, const isc_filter_saved *sv) {
    DevFilter F;
    F.c_exp = (float)(1.4426950408889634 / (double)f->temperature);
    F.tau = f->temperature; F.top_k = f->top_k; F.top_p = f->top_p; F.slp = f->sampling_logprobs;
    F.staged = flt_lds(s) != 0;
    F.sv_kstar = sv ? (long long *)sv->kstar : nullptr;
    F.sv_gmax = sv ? sv->gmax : nullptr; F.sv_logz = sv ? sv->logz : nullptr; F.sv_ban = sv ? sv->ban : nullptr;
    return F;
}

static int finalize_filtered(const isc_rollout_step *s, const isc_sample_filter *f, const isc_filter_saved *sv,
                             void *stream) {
    if (!s || !f) return ISC_E_NULL;
    if (const int rc = rollout_step_check(s, !s->logits || !s->sample_u,
                                          !flt_params_ok(f) || s->V <= 0 || s->n_tile <= 0 || s->ld_logits < s->V || s->forced))
        return rc;
    hipLaunchKernelGGL(rollout_finalize_filtered_kernel, flt_grid(s), dim3(256), flt_lds(s), (hipStream_t)stream,
                       dev_rollout(s), dev_filter(s, f, sv));
    ISC_LAUNCH_CHECK();
    ++g_finalize_launches;
    return ISC_OK;
}

extern "C" int isc_rollout_finalize_filtered(const isc_rollout_step *s, const isc_sample_filter *f, void *stream) {
    return finalize_filtered(s, f, nullptr, stream);
}

// The roll-out's finalize under token constraints (include/insenticap_hip.h: isc_decode_constraints).  `f` NULL: the
// plain finalize's choice (arg-max, or sample_u) over the allowed ids; given: the filtered one's.  A step at which
// nothing is banned IS the unconstrained step: it goes to the two entry points above, bit for bit.
static int finalize_constrained(const isc_rollout_step *s, const isc_sample_filter *f, const isc_decode_constraints *c,
                                const isc_filter_saved *sv, void *stream) {
    if (!s || !c) return ISC_E_NULL;
    if (c->n_ban < 0 || c->n_ban > 8 || c->min_len < 0 || c->min_len > s->T) return ISC_E_SHAPE;
    const bool any = c->n_ban > 0 || c->no_repeat || c->min_len > 0;
    if (any) {
        // (every constrained form reads the logits; forced tokens leave nothing to choose)
        if (!s->logits) return ISC_E_NULL;
        if (s->forced || s->V <= c->n_ban + 2) return ISC_E_SHAPE;
        for (int k = 0; k < c->n_ban; ++k)
            if (c->ban_ids[k] < 0 || c->ban_ids[k] >= s->V) return ISC_E_SHAPE;
        if (c->no_repeat && (c->first_id < 0 || c->first_id >= s->V)) return ISC_E_SHAPE;
        if (c->min_len > 0 && (s->eos_id < 0 || s->eos_id >= s->V)) return ISC_E_SHAPE;
    }
    DevCons C;
    int n = 0;
    for (; n < c->n_ban; ++n) C.ban[n] = (int)c->ban_ids[n];
    if (s->t >= 0 && s->t < c->min_len) C.ban[n++] = (int)s->eos_id;
    C.no_repeat = c->no_repeat != 0; C.first_id = (int)c->first_id;
    if (n == 0 && !C.no_repeat) return f ? finalize_filtered(s, f, sv, stream) : isc_rollout_finalize(s, stream);
    for (; n < ISC_CON_MAX - 1; ++n) C.ban[n] = -1;
    if (const int rc = rollout_step_check(s, f && !s->sample_u,
                                          (f && !flt_params_ok(f)) || s->V <= 0 || s->n_tile != (s->V + 127) / 128 ||
                                              s->ld_logits < s->V))
        return rc;
    const DevRollout R = dev_rollout(s);
    if (f) {
        hipLaunchKernelGGL(rollout_finalize_filtered_con_kernel, flt_grid(s), dim3(256), flt_lds(s), (hipStream_t)stream, R,
                           dev_filter(s, f, sv), C);
    } else if (s->B > 1024) {
        hipLaunchKernelGGL(rollout_finalize_con_kernel<16>, dim3((s->B + 15) / 16), dim3(1024), 0, (hipStream_t)stream, R, C);
    } else {
        hipLaunchKernelGGL(rollout_finalize_con_kernel<4>, dim3((s->B + 3) / 4), dim3(256), 0, (hipStream_t)stream, R, C);
    }
    ISC_LAUNCH_CHECK();
    ++g_finalize_launches;
    return ISC_OK;
}

extern "C" int isc_rollout_finalize_constrained(const isc_rollout_step *s, const isc_sample_filter *f,
                                                const isc_decode_constraints *c, void *stream) {
    return finalize_constrained(s, f, c, nullptr, stream);
}

// The filtered finalize (c NULL) or the constrained filtered one, additionally keeping per (b, t) what the backward of
// the sampling log-probability reads (isc_logsoftmax_bwd_raw_filtered): the boundary key K*, the largest allowed logit,
// log(kept mass) and - under constraints - the row's banned ids.  Same kernels, same choice, same outputs; a step the
// early break skips (alive[t] == 0) writes nothing: the caller zero-fills (ban: -1) up front.
extern "C" int isc_rollout_finalize_saved(const isc_rollout_step *s, const isc_sample_filter *f,
                                          const isc_decode_constraints *c, const isc_filter_saved *sv, void *stream) {
    if (!s || !f || !sv || !sv->kstar || !sv->gmax || !sv->logz) return ISC_E_NULL;
    return c ? finalize_constrained(s, f, c, sv, stream) : finalize_filtered(s, f, sv, stream);
}

// ------------------------------------------------------------------ scheduled sampling (captioner.py:219-228)
// out[b] = (u_select[b] < ss_prob) ? draw from exp(logp[b, :]) with uniform u_draw[b] : base[b].
// One launch and no host decision in place of rand / `if mask.sum() == 0` / multinomial / index_copy_:
// the reference's host test costs a device->host sync at every step.
// RAW: `logp` holds the raw logits of the row (the statistics describe them): the draw is then the roll-out's
// (exp(x - max) against tile masses psum * exp(pmax - max)) and a teacher-forced unroll with scheduled sampling can turn
// its logits into log-probs ONCE, after the last step, instead of step by step.
template <bool RAW>
__global__ __launch_bounds__(256) void sched_sample_kernel(const float *logp, long long ld, int M, int V,
                                                           const float *pmax, const float *psum, const int *pidx,
                                                           int n_tile, const float *u_select, const float *u_draw,
                                                           float ss_prob, const int64_t *base, long long base_stride,
                                                           int64_t *out) {
    const int lane = threadIdx.x & 63;
    const int b = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (b >= M) return;
    long long it = base[(long long)b * base_stride];
    if (u_select[b] < ss_prob) {                  // wave-uniform
        float gmax, S;
        int gidx;
        fold_row_stats(pmax + (long long)b * n_tile, psum + (long long)b * n_tile, pidx + (long long)b * n_tile,
                       n_tile, lane, gmax, gidx, S);
        const int pick = sample_two_level(logp + (long long)b * ld, RAW ? gmax : 0.f, RAW ? 1.0f : S,
                                          pmax + (long long)b * n_tile, psum + (long long)b * n_tile, n_tile, V, gmax,
                                          u_draw[b] * S, lane);
        it = pick < 0 ? gidx : pick;
    }
    if (lane == 0) out[b] = it;
}

static int sched_sample_launch(bool raw, const float *logp, int64_t ld, int M, int V, const float *part_max,
                               const float *part_sum, const int32_t *part_idx, const float *u_select,
                               const float *u_draw, float ss_prob, const int64_t *base_ids, int64_t base_stride,
                               int64_t *out_ids, void *stream) {
    if (!logp || !part_max || !part_sum || !part_idx || !u_select || !u_draw || !base_ids || !out_ids)
        return ISC_E_NULL;
    if (M <= 0 || V <= 0) return ISC_E_SHAPE;
    if (raw)
        hipLaunchKernelGGL(sched_sample_kernel<true>, dim3((M + 3) / 4), dim3(256), 0, (hipStream_t)stream, logp,
                           (long long)ld, M, V, part_max, part_sum, part_idx, (V + 127) / 128, u_select, u_draw, ss_prob,
                           base_ids, (long long)base_stride, out_ids);
    else
        hipLaunchKernelGGL(sched_sample_kernel<false>, dim3((M + 3) / 4), dim3(256), 0, (hipStream_t)stream, logp,
                           (long long)ld, M, V, part_max, part_sum, part_idx, (V + 127) / 128, u_select, u_draw, ss_prob,
                           base_ids, (long long)base_stride, out_ids);
    ISC_LAUNCH_CHECK();
    return ISC_OK;
}

extern "C" int isc_sched_sample(const float *logp, int64_t ld, int M, int V, const float *part_max,
                                const float *part_sum, const int32_t *part_idx, const float *u_select,
                                const float *u_draw, float ss_prob, const int64_t *base_ids, int64_t base_stride,
                                int64_t *out_ids, void *stream) {
    return sched_sample_launch(false, logp, ld, M, V, part_max, part_sum, part_idx, u_select, u_draw, ss_prob, base_ids,
                               base_stride, out_ids, stream);
}

extern "C" int isc_sched_sample_raw(const float *logits, int64_t ld, int M, int V, const float *part_max,
                                    const float *part_sum, const int32_t *part_idx, const float *u_select,
                                    const float *u_draw, float ss_prob, const int64_t *base_ids, int64_t base_stride,
                                    int64_t *out_ids, void *stream) {
    return sched_sample_launch(true, logits, ld, M, V, part_max, part_sum, part_idx, u_select, u_draw, ss_prob, base_ids,
                               base_stride, out_ids, stream);
}

// ------------------------------------------------------------------ several small device-to-device copies, one launch
// (the input copies in front of a graph replay: fc / att features, word ids, labels of one image are 300 KB in four
// tensors of two dtypes - torch._foreach_copy_ is one 17 us + one 4.5 us launch for them)
struct DevCopyMulti {
    unsigned char *dst[ISC_COPY_MULTI_MAX];
    const unsigned char *src[ISC_COPY_MULTI_MAX];
    long long bytes[ISC_COPY_MULTI_MAX];
    int first_block[ISC_COPY_MULTI_MAX + 1];      // blocks of 16 KB, prefix over the entries
    int n;
};
__global__ __launch_bounds__(256) void copy_multi_kernel(const DevCopyMulti a) {
    int e = 0;
#pragma unroll
    for (int i = 1; i < ISC_COPY_MULTI_MAX; ++i) e += (i < a.n && (int)blockIdx.x >= a.first_block[i]) ? 1 : 0;
    unsigned char *dst = a.dst[0];
    const unsigned char *src = a.src[0];
    long long nb = a.bytes[0];
    int fb = a.first_block[0];
#pragma unroll
    for (int i = 1; i < ISC_COPY_MULTI_MAX; ++i)
        if (e == i) { dst = a.dst[i]; src = a.src[i]; nb = a.bytes[i]; fb = a.first_block[i]; }
    const long long off = (long long)((int)blockIdx.x - fb) * 16384;
    const long long end = off + 16384 < nb ? off + 16384 : nb;
    if ((((uintptr_t)dst | (uintptr_t)src) & 15) == 0) {
        for (long long o = off + (long long)threadIdx.x * 16; o < end; o += 256 * 16) {
            if (o + 16 <= end) {
                *reinterpret_cast<float4 *>(dst + o) = *reinterpret_cast<const float4 *>(src + o);
            } else {
                for (long long q = o; q < end; ++q) dst[q] = src[q];
            }
        }
    } else {
        for (long long o = off + threadIdx.x; o < end; o += 256) dst[o] = src[o];
    }
}

extern "C" int isc_copy_multi(void *const *dst, const void *const *src, const int64_t *bytes, int n, void *stream) {
    if (!dst || !src || !bytes) return ISC_E_NULL;
    if (n < 1 || n > ISC_COPY_MULTI_MAX) return ISC_E_SHAPE;
    DevCopyMulti a = {};
    a.n = n;
    int blocks = 0;
    for (int i = 0; i < n; ++i) {
        if (bytes[i] < 0) return ISC_E_SHAPE;
        if (bytes[i] > 0 && (!dst[i] || !src[i])) return ISC_E_NULL;
        a.dst[i] = static_cast<unsigned char *>(dst[i]);
        a.src[i] = static_cast<const unsigned char *>(src[i]);
        a.bytes[i] = bytes[i];
        a.first_block[i] = blocks;
        if (bytes[i] > (1LL << 34)) return ISC_E_SHAPE;
        blocks += (int)((bytes[i] + 16383) / 16384);
    }
    for (int i = n; i <= ISC_COPY_MULTI_MAX; ++i) a.first_block[i] = blocks;
    if (blocks == 0) return ISC_OK;
    hipLaunchKernelGGL(copy_multi_kernel, dim3(blocks), dim3(256), 0, (hipStream_t)stream, a);
    ISC_LAUNCH_CHECK();
    return ISC_OK;
}

// ------------------------------------------------------------------ f16 -> fp32 rows
// What a consumer that cannot read f16 features gets (isc_seg.a_f16): one thread per 8 consecutive columns of a row
// (one 16-byte load, two 16-byte stores) when pointers and leading dimensions allow, else one thread per element.
static std::atomic<long long> g_f16_convert_launches{0};
extern "C" long long isc_f16_convert_launches(void) { return g_f16_convert_launches.load(); }

template <bool VEC>
__global__ __launch_bounds__(256) void f16_to_f32_kernel(const _Float16 *src, long long ld_src, float *dst, long long ld_dst,
                                                         long long rows, long long cols) {
    typedef _Float16 h8v __attribute__((ext_vector_type(8)));
    const long long per_row = VEC ? cols >> 3 : cols;
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    if (i >= rows * per_row) return;
    const long long r = i / per_row, c = i - r * per_row;
    if (VEC) {
        const h8v v = *reinterpret_cast<const h8v *>(src + r * ld_src + c * 8);
        float *o = dst + r * ld_dst + c * 8;
        *reinterpret_cast<float4 *>(o) = make_float4((float)v[0], (float)v[1], (float)v[2], (float)v[3]);
        *reinterpret_cast<float4 *>(o + 4) = make_float4((float)v[4], (float)v[5], (float)v[6], (float)v[7]);
    } else {
        dst[r * ld_dst + c] = (float)src[r * ld_src + c];
    }
}

extern "C" int isc_f16_to_f32(const void *src, int64_t ld_src, float *dst, int64_t ld_dst, int64_t rows, int64_t cols,
                              void *stream) {
    if (!src || !dst) return ISC_E_NULL;
    if (rows <= 0 || cols <= 0 || ld_src < cols || ld_dst < cols) return ISC_E_SHAPE;
    const bool vec = (cols & 7) == 0 && (ld_src & 7) == 0 && (ld_dst & 3) == 0 && isc_aligned16(src) && isc_aligned16(dst);
    const long long n = rows * (vec ? cols >> 3 : cols);
    if (n > (1LL << 31) * 255) return ISC_E_SHAPE;
    const dim3 grid((unsigned)((n + 255) / 256));
    const _Float16 *s = static_cast<const _Float16 *>(src);
    if (vec) hipLaunchKernelGGL(f16_to_f32_kernel<true>, grid, dim3(256), 0, (hipStream_t)stream, s, ld_src, dst, ld_dst, rows, cols);
    else hipLaunchKernelGGL(f16_to_f32_kernel<false>, grid, dim3(256), 0, (hipStream_t)stream, s, ld_src, dst, ld_dst, rows, cols);
    ISC_LAUNCH_CHECK();
    ++g_f16_convert_launches;
    return ISC_OK;
}

// ------------------------------------------------------------------ log-softmax apply
__global__ __launch_bounds__(256) void logsoftmax_apply_kernel(float *logits, long long ld, int M, int V,
                                                               const float *pmax, const float *psum,
                                                               int n_tile, float *lse_out) {
    __shared__ float sh[2];
    const int m = blockIdx.x;
    const int tid = threadIdx.x;
    if (tid < 64) {
        float gmax, S;
        int gi;
        fold_row_stats(pmax + (long long)m * n_tile, psum + (long long)m * n_tile, nullptr, n_tile, tid,
                       gmax, gi, S);
        if (tid == 0) {
            sh[0] = gmax;
            sh[1] = logf(S);
            if (lse_out) lse_out[m] = gmax + sh[1];
        }
    }
    __syncthreads();
    const float gmax = sh[0], logS = sh[1];
    float *x = logits + (long long)m * ld;
    for (int i = blockIdx.y * 256 + tid; i < V; i += gridDim.y * 256) x[i] = (x[i] - gmax) - logS;
}

extern "C" int isc_logsoftmax_apply(float *logits, int64_t ld_logits, int M, int V,
                                    const float *part_max, const float *part_sum, float *lse_out,
                                    void *stream) {
    if (!logits || !part_max || !part_sum) return ISC_E_NULL;
    if (M <= 0 || V <= 0) return ISC_E_SHAPE;
    const int n_tile = (V + 127) / 128;
    int gy = (V + 2047) / 2048;
    if (gy < 1) gy = 1;
    hipLaunchKernelGGL(logsoftmax_apply_kernel, dim3(M, gy), dim3(256), 0, (hipStream_t)stream, logits,
                       (long long)ld_logits, M, V, part_max, part_sum, n_tile, lse_out);
    ISC_LAUNCH_CHECK();
    return ISC_OK;
}

// The same for ALL T steps of a teacher-forced unroll in one launch: logits [B,T,V] (row (b,t) at b*ld_b + t*ld_t), tile
// statistics stacked per step [T,B,n_tile].  With every fed token known up front nothing reads a step's log-probs
// before the unroll ends, so the T per-step launches (38 of the ~750 of an XE iteration at B = 128) become one.
__global__ __launch_bounds__(256) void logsoftmax_apply_steps_kernel(float *logits, long long ld_b, long long ld_t,
                                                                     int B, int V, const float *pmax,
                                                                     const float *psum, int n_tile,
                                                                     const float *src, int step_rows) {
    __shared__ float sh[2];
    const int mi = blockIdx.x;                // = t * B + b
    // row of (t, b) in the per-step stacks: step_rows rows per step (>= B: the stacks of a merged unroll hold the rows
    // of both branches per step; statistics / src then point at this branch's first row)
    const long long m = (long long)(mi / B) * step_rows + (mi % B);
    const int tid = threadIdx.x;
    if (tid < 64) {
        float gmax, S;
        int gi;
        fold_row_stats(pmax + m * n_tile, psum + m * n_tile, nullptr, n_tile, tid,
                       gmax, gi, S);
        if (tid == 0) {
            sh[0] = gmax;
            sh[1] = logf(S);
        }
    }
    __syncthreads();
    const float gmax = sh[0], logS = sh[1];
    float *x = logits + (long long)(mi % B) * ld_b + (long long)(mi / B) * ld_t;
    const float *y = src ? src + m * V : x;       // src: raw logits stacked per step, [T*step_rows, V]
    for (int i = blockIdx.y * 256 + tid; i < V; i += gridDim.y * 256) x[i] = (y[i] - gmax) - logS;
}

extern "C" int isc_logsoftmax_apply_steps(float *logits, int64_t ld_b, int64_t ld_t, int B, int T, int V,
                                          const float *part_max, const float *part_sum, const float *src,
                                          int step_rows, void *stream) {
    if (!logits || !part_max || !part_sum) return ISC_E_NULL;
    if (B <= 0 || T <= 0 || V <= 0 || (long long)B * T > 2147483647LL) return ISC_E_SHAPE;
    if (step_rows == 0) step_rows = B;
    if (step_rows < B) return ISC_E_SHAPE;
    const int n_tile = (V + 127) / 128;
    int gy = (V + 2047) / 2048;
    if (gy < 1) gy = 1;
    hipLaunchKernelGGL(logsoftmax_apply_steps_kernel, dim3(B * T, gy), dim3(256), 0, (hipStream_t)stream, logits,
                       (long long)ld_b, (long long)ld_t, B, V, part_max, part_sum, n_tile, src, step_rows);
    ISC_LAUNCH_CHECK();
    return ISC_OK;
}

// ------------------------------------------------------------------ beam top-k
// Form for beam <= 8 over the tile statistics the classifier already produced: the top-`beam` masked log-probs can
// only sit in column tiles whose maximum is among the (beam + 4) largest tile maxima - at most 4 words are masked
// (<PAD>, <SOS>, <UNK>, the repeated last word), so at least `beam` unmasked entries reach that threshold and nothing
// below it can be selected.  Those ~9 of 79 tiles are swept once, every thread keeping its best 8 in registers, then
// `beam` rounds of a block-wide arg-max over the threads' list heads.  Same values and order as the kernel below
// (descending value, ties to the smaller word id, masked entries as -inf): [5 x 10000] 78 us -> ~10 us, which was
// 40 % of a one-image search.
// BAN (isc_beam_topk_banned): the row's ban list (at most 256 ids) is staged in LDS and masks like the specials; a row
// with c listed ids admits c more tiles, since up to 4 + c of the words above the threshold may be masked.
// (the instantiations without a list take an empty argument: their code and kernarg layout are what they were)
template <bool BAN>
struct BeamBan {
    const int64_t *ids;
    const int32_t *cnt;
    long long ld;
};
template <>
struct BeamBan<false> {};
#define ISC_BAN_MAX 256
template <bool BAN>
__global__ __launch_bounds__(256) void beam_topk8_kernel(const float *logits, long long ld,
                                                         const float *pmax, const float *psum, int n_tile,
                                                         int V, int beam, const int64_t *last_word,
                                                         long long pad_id, long long sos_id,
                                                         long long unk_id, int mask_special, int cons,
                                                         float *top_val, int64_t *top_idx, const int *gate,
                                                         const BeamBan<BAN> ban) {
    if (gate != nullptr && *gate == 0) return;      // (uniform; isc_set_stream_gate: the search has ended)
    constexpr int K = 8;
    __shared__ int sban[BAN ? ISC_BAN_MAX : 1];
    int nban = 0;
    if constexpr (BAN) {
        nban = ban.cnt[blockIdx.x];
        nban = nban < 0 ? 0 : (nban > ISC_BAN_MAX ? ISC_BAN_MAX : nban);
        nban = nban > ban.ld ? (int)ban.ld : nban;
        if ((int)threadIdx.x < nban) {
            const long long b = ban.ids[(long long)blockIdx.x * ban.ld + threadIdx.x];
            sban[threadIdx.x] = (b >= 0 && b < V) ? (int)b : -1;
        }
    }
    __shared__ float sv[2][4];
    __shared__ int si[2][4];
    __shared__ float sh[2];
    __shared__ int sel[256];               // selected tile ids (n_tile <= 256 on this path)
    __shared__ float spm[256];             // this row's tile maxima
    __shared__ int nsel;
    const int row = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    if (tid == 0) nsel = 0;
    if (tid >= 64 && tid - 64 < n_tile) spm[tid - 64] = pmax[(long long)row * n_tile + tid - 64];   // (waves 1-3 idle here)
    if (tid < 64) {
        if (n_tile > 192) for (int j = 192 + tid; j < n_tile; j += 64) spm[j] = pmax[(long long)row * n_tile + j];
        float gmax, S;
        int gi;
        fold_row_stats(pmax + (long long)row * n_tile, psum + (long long)row * n_tile, nullptr, n_tile,
                       tid, gmax, gi, S);
        if (tid == 0) { sh[0] = gmax; sh[1] = logf(S); }
    }
    __syncthreads();
    const float gmax = sh[0], logS = sh[1];
    // tile selection: rank of this thread's tile among the tile maxima (ties by tile id); tiles tied with the last
    // admitted maximum are admitted as well because the comparison below is on values, not ranks
    const int want = beam + 4 + nban;
    if (tid < n_tile) {
        const float mine = spm[tid];
        int larger = 0;
        for (int j = 0; j < n_tile; ++j) larger += spm[j] > mine;     // LDS broadcasts (was n_tile global loads)
        if (larger < want) sel[atomicAdd(&nsel, 1)] = tid;     // order of `sel` is irrelevant: ids break ties later
    }
    __syncthreads();
    const int ns = nsel;
    const float *x = logits + (long long)row * ld;
    const long long last = last_word[row];
    float tv[K];
    int ti[K];
#pragma unroll
    for (int k = 0; k < K; ++k) { tv[k] = -INFINITY; ti[k] = 0x7fffffff; }
    auto offer = [&](float raw, int i) __attribute__((always_inline)) {
        bool banned = false;
        if (mask_special && (i == pad_id || i == sos_id || i == unk_id)) banned = true;
        if (cons && i == last) banned = true;
        if constexpr (BAN)
            for (int b = 0; b < nban; ++b) banned |= (sban[b] == i);
        float v = banned ? -INFINITY : (raw - gmax) - logS;
        int id = i;
#pragma unroll
        for (int k = 0; k < K; ++k) {      // insertion into the sorted list (best first)
            const bool better = v > tv[k] || (v == tv[k] && id < ti[k]);
            const float ov = tv[k];
            const int oi = ti[k];
            tv[k] = better ? v : ov;
            ti[k] = better ? id : oi;
            v = better ? ov : v;
            id = better ? oi : id;
        }
    };
    // two selected tiles per pass: thread t takes column (t & 127) of tile sel[2*pass + (t >> 7)]; the loads of four
    // passes are issued together (the ~9 selected tiles used to be five dependent-looking L2 round trips)
    for (int s0 = 0; s0 < ns; s0 += 8) {
        float xv[4];
        int xi[4];
        bool ok[4];
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            const int si2 = s0 + 2 * u + (tid >> 7);
            ok[u] = si2 < ns;
            xi[u] = ok[u] ? sel[si2] * 128 + (tid & 127) : 0;
            ok[u] = ok[u] && xi[u] < V;
            xv[u] = x[ok[u] ? xi[u] : 0];
        }
#pragma unroll
        for (int u = 0; u < 4; ++u)
            if (ok[u]) offer(xv[u], xi[u]);
    }
    for (int k = 0; k < beam; ++k) {
        float mx = tv[0];
        int ix = ti[0];
        wave_argmax(mx, ix);
        if (lane == 0) { sv[k & 1][wave] = mx; si[k & 1][wave] = ix; }
        __syncthreads();
        float bm = sv[k & 1][0];
        int bi = si[k & 1][0];
#pragma unroll
        for (int w = 1; w < 4; ++w) {
            const float wv2 = sv[k & 1][w];
            const int wi = si[k & 1][w];
            if (wv2 > bm || (wv2 == bm && wi < bi)) { bm = wv2; bi = wi; }
        }
        if (ti[0] == bi) {                 // this thread's head won: pop it (word ids are unique)
#pragma unroll
            for (int j = 0; j + 1 < K; ++j) { tv[j] = tv[j + 1]; ti[j] = ti[j + 1]; }
            tv[K - 1] = -INFINITY; ti[K - 1] = 0x7fffffff;
        }
        if (tid == 0) {
            top_val[(long long)row * beam + k] = bm;
            top_idx[(long long)row * beam + k] = (unsigned)bi < (unsigned)V ? bi : 0;      // (NaN rows: sentinel -> <PAD>)
        }
    }
}

// One workgroup per live beam row; `beam` rounds of a block-wide arg-max over the masked
// log-probabilities (rows are few: images x beam).  Ties resolve to the smaller word id.
template <bool BAN>
__global__ __launch_bounds__(256) void beam_topk_kernel(const float *logits, long long ld,
                                                        const float *pmax, const float *psum, int n_tile,
                                                        int V, int beam, const int64_t *last_word,
                                                        long long pad_id, long long sos_id,
                                                        long long unk_id, int mask_special, int cons,
                                                        float *top_val, int64_t *top_idx, const int *gate,
                                                        const BeamBan<BAN> ban) {
    if (gate != nullptr && *gate == 0) return;      // (uniform; isc_set_stream_gate: the search has ended)
    __shared__ int sban[BAN ? ISC_BAN_MAX : 1];
    int nban = 0;
    if constexpr (BAN) {
        nban = ban.cnt[blockIdx.x];
        nban = nban < 0 ? 0 : (nban > ISC_BAN_MAX ? ISC_BAN_MAX : nban);
        nban = nban > ban.ld ? (int)ban.ld : nban;
        if ((int)threadIdx.x < nban) {
            const long long b = ban.ids[(long long)blockIdx.x * ban.ld + threadIdx.x];
            sban[threadIdx.x] = (b >= 0 && b < V) ? (int)b : -1;
        }
    }
    __shared__ float sv[4];
    __shared__ int si[4];
    __shared__ float sh[2];
    __shared__ int chosen[16];
    const int row = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    if (tid < 64) {
        float gmax, S;
        int gi;
        fold_row_stats(pmax + (long long)row * n_tile, psum + (long long)row * n_tile, nullptr, n_tile,
                       tid, gmax, gi, S);
        if (tid == 0) { sh[0] = gmax; sh[1] = logf(S); }
    }
    __syncthreads();
    const float gmax = sh[0], logS = sh[1];
    const float *x = logits + (long long)row * ld;
    const long long last = last_word[row];
    for (int k = 0; k < beam; ++k) {
        float mx = -INFINITY;
        int ix = 0x7fffffff;
        for (int i = tid; i < V; i += 256) {
            bool banned = false;
            if (mask_special && (i == pad_id || i == sos_id || i == unk_id)) banned = true;
            if (cons && i == last) banned = true;
            for (int j = 0; j < k; ++j) banned |= (chosen[j] == i);
            if constexpr (BAN)
                for (int b = 0; b < nban; ++b) banned |= (sban[b] == i);
            const float v = banned ? -INFINITY : (x[i] - gmax) - logS;
            // banned entries still take part as -inf (torch.sort keeps them, at the tail)
            if (v > mx || (v == mx && i < ix)) { mx = v; ix = i; }
        }
        wave_argmax(mx, ix);
        if (lane == 0) { sv[wave] = mx; si[wave] = ix; }
        __syncthreads();
        if (tid == 0) {
            float bm = sv[0];
            int bi = si[0];
            for (int w = 1; w < 4; ++w)
                if (sv[w] > bm || (sv[w] == bm && si[w] < bi)) { bm = sv[w]; bi = si[w]; }
            chosen[k] = bi;
            top_val[(long long)row * beam + k] = bm;
            top_idx[(long long)row * beam + k] = (unsigned)bi < (unsigned)V ? bi : 0;      // (NaN rows: sentinel -> <PAD>)
        }
        __syncthreads();
    }
}

template <bool BAN>
static int beam_topk_launch(const float *logits, int64_t ld_logits, const float *part_max, const float *part_sum,
                            int n_tile, int rows, int V, int beam, const int64_t *last_word, int64_t pad_id,
                            int64_t sos_id, int64_t unk_id, int mask_special, int decoding_constraint, const BeamBan<BAN> ban,
                            float *top_val, int64_t *top_idx, void *stream) {
    if (!logits || !part_max || !part_sum || !last_word || !top_val || !top_idx) return ISC_E_NULL;
    if (rows <= 0 || V <= 0 || beam <= 0 || beam > 16 || beam > V) return ISC_E_SHAPE;
    const int *gate = isc_stream_gate_(stream);
    if (beam <= 8 && n_tile <= 256 && V >= (beam + 4) * 128)
        hipLaunchKernelGGL(beam_topk8_kernel<BAN>, dim3(rows), dim3(256), 0, (hipStream_t)stream, logits,
                           (long long)ld_logits, part_max, part_sum, n_tile, V, beam, last_word,
                           (long long)pad_id, (long long)sos_id, (long long)unk_id, mask_special,
                           decoding_constraint, top_val, top_idx, gate, ban);
    else
        hipLaunchKernelGGL(beam_topk_kernel<BAN>, dim3(rows), dim3(256), 0, (hipStream_t)stream, logits,
                           (long long)ld_logits, part_max, part_sum, n_tile, V, beam, last_word,
                           (long long)pad_id, (long long)sos_id, (long long)unk_id, mask_special,
                           decoding_constraint, top_val, top_idx, gate, ban);
    ISC_LAUNCH_CHECK();
    return ISC_OK;
}

extern "C" int isc_beam_topk(const float *logits, int64_t ld_logits, const float *part_max,
                             const float *part_sum, int n_tile, int rows, int V, int beam,
                             const int64_t *last_word, int64_t pad_id, int64_t sos_id, int64_t unk_id,
                             int mask_special, int decoding_constraint, float *top_val,
                             int64_t *top_idx, void *stream) {
    return beam_topk_launch<false>(logits, ld_logits, part_max, part_sum, n_tile, rows, V, beam, last_word, pad_id, sos_id,
                                   unk_id, mask_special, decoding_constraint, BeamBan<false>{}, top_val, top_idx,
                                   stream);
}

extern "C" int isc_beam_topk_banned(const float *logits, int64_t ld_logits, const float *part_max,
                                    const float *part_sum, int n_tile, int rows, int V, int beam,
                                    const int64_t *last_word, int64_t pad_id, int64_t sos_id, int64_t unk_id,
                                    int mask_special, int decoding_constraint, const int64_t *ban_ids,
                                    const int32_t *ban_cnt, int64_t ban_ld, float *top_val, int64_t *top_idx,
                                    void *stream) {
    if (!ban_ids || !ban_cnt) return ISC_E_NULL;
    if (ban_ld < 1) return ISC_E_SHAPE;
    return beam_topk_launch<true>(logits, ld_logits, part_max, part_sum, n_tile, rows, V, beam, last_word, pad_id, sos_id,
                                  unk_id, mask_special, decoding_constraint, BeamBan<true>{ban_ids, ban_cnt, (long long)ban_ld},
                                  top_val, top_idx, stream);
}

// ------------------------------------------------------------------ beam step tail in one launch
// isc_beam_select: what isc_beam_topk + isc_beam_merge + isc_beam_gather do in three launches, from the tile
// statistics and per-tile sorted candidate lists the few-row classifier (rows.hip) leaves.  One workgroup per image.  A
// lone wave retires an instruction every ~6-8 cycles here (and a launch that returns at once already takes 4.6 us:
// tools/select_lab.py), so the launch is as long as the LONGEST dependent instruction chain of any wave.  The chain is
// merge -> scores -> rank -> new rows; everything that is not on it runs beside it on waves of its own:
//   merge wave r (one per beam row): the row's tile candidates (value, id) [n_tile][8] - a lane owns tiles lane,
//     lane + 64, ... and holds their lists in registers - and a `beam`-round k-way merge over the lists' heads: ONE 32-bit
//     DPP maximum per round, ties by ballots and scalar bit scans (value descending, then tile ascending = word id
//     ascending: tiles are column ranges, lists are sorted), the winner's list moves up one place, round k's winner
//     stays in lane k's registers;  barrier;  parent r's candidates scored in fp64 by lanes 0..beam-1 (captioner.py:
//     378-411, beam_merge_kernel's rules: the parents' bookkeeping sits in lanes 0..7 of every wave, no staging) -> LDS;
//     barrier;  stable descending rank with EIGHT lanes per candidate (each counts an eighth of the others), ranks
//     < beam write the new rows' bookkeeping;  barrier;  new row r's word list;
//   side wave r (one per beam row): row r's normaliser from (pmax, psum) - fold_row_stats, as every decode path - and its
//     word list -> LDS, row r's planes of the recurrent state -> LDS by LDS-DMA (when the state is re-ordered here), all
//     while the merges run; winners known: new row r's planes from its parent's LDS image.
// Word ids, log-probs ((x - max) - log(sum), the expression of beam_topk8_kernel) and tie order are those of the
// three-launch path on the same logits and statistics.
#define ISC_SEL_TILES_PER_LANE 4
#if ROWS_STAMP
#define RSTAMP_KID 5
RSTAMP_SETTER(isc_pw_set_stamp)
#endif
// Wave-wide maximum / sum that never leave the VALU: four DPP steps leave every 16-lane row holding its reduction, the
// four row values then meet through row_bcast15 / row_bcast31 (maximum) or four v_readlane (sum: the association of
// common.h's full_sum, so the normaliser keeps its bits).  The ds_swizzle / ds_bpermute steps these replace are
// LDS round trips (~100+ cycles each) - in a kernel that is ONE dependent chain they were a third of its time.
__device__ __forceinline__ float sel_wave_fmax(float v) {               // -> the wave's maximum, wave-uniform (NaNs are dropped)
    // v_max_f32 with the DPP operand folded in (the compiler keeps v_mov_dpp + a canonicalising v_max + v_max per step);
    // s_nop 1 = the two wait states a DPP read needs behind the VALU write of its source.  row_bcast15 / 31 write rows
    // 1, 3 / 2, 3 only (row_mask), the other rows keep their value.
    asm volatile("s_nop 1\n\tv_max_f32_dpp %0, %0, %0 quad_perm:[1,0,3,2] row_mask:0xf bank_mask:0xf\n\t"
                 "s_nop 1\n\tv_max_f32_dpp %0, %0, %0 quad_perm:[2,3,0,1] row_mask:0xf bank_mask:0xf\n\t"
                 "s_nop 1\n\tv_max_f32_dpp %0, %0, %0 row_half_mirror row_mask:0xf bank_mask:0xf\n\t"
                 "s_nop 1\n\tv_max_f32_dpp %0, %0, %0 row_mirror row_mask:0xf bank_mask:0xf\n\t"
                 "s_nop 1\n\tv_max_f32_dpp %0, %0, %0 row_bcast:15 row_mask:0xa bank_mask:0xf\n\t"
                 "s_nop 1\n\tv_max_f32_dpp %0, %0, %0 row_bcast:31 row_mask:0xc bank_mask:0xf\n\t"
                 "s_nop 1" : "+v"(v));
    return __int_as_float(__builtin_amdgcn_readlane(__float_as_int(v), 63));
}
__device__ __forceinline__ float sel_wave_sum(float v) {                // == full_sum(v), bit for bit
    v += isc_dpp<ISC_DPP_XOR1>(v);
    v += isc_dpp<ISC_DPP_XOR2>(v);
    v += isc_dpp<ISC_DPP_HALF_MIRROR>(v);
    v += isc_dpp<ISC_DPP_MIRROR>(v);
    const int b = __float_as_int(v);
    const float r0 = __int_as_float(__builtin_amdgcn_readlane(b, 0)), r1 = __int_as_float(__builtin_amdgcn_readlane(b, 16));
    const float r2 = __int_as_float(__builtin_amdgcn_readlane(b, 32)), r3 = __int_as_float(__builtin_amdgcn_readlane(b, 48));
    return (r0 + r1) + (r2 + r3);
}
// The winner's list (list Q of lane wl, both wave-uniform) moves up one place in its lane - static register indices,
// position 0 is always the head.  Branch-free: each list shifts under its own lane mask (empty for the three lists that did
// not win) - four copies under scalar branches cost more in the register copies that rejoin them than the idle selects do.
// A search pops at most `beam` <= 8 entries and a list holds 8, so no list runs dry before the last round; positions past
// the fifth are only ever heads for beam > 5.
#define SEL_SHIFT(Q, LO, HI)                                                                \
    _Pragma("unroll") for (int s_ = LO; s_ < HI; ++s_) {                                    \
        cvv[Q][s_] = me##Q ? cvv[Q][s_ + 1] : cvv[Q][s_];                                   \
        cid[Q][s_] = me##Q ? cid[Q][s_ + 1] : cid[Q][s_];                                   \
    }

// GR: the diverse search's group-sequential rank phase (isc_beam_select_groups; `groups` groups of bp = beam / groups
// ranks, beam_group_key's keys) - everything in front of the candidates and behind the winners is the plain search's.
struct sel_groups { int groups; double lambda; };
__device__ __forceinline__ sel_groups sel_groups_of() { return sel_groups{1, 0.0}; }
__device__ __forceinline__ sel_groups sel_groups_of(const sel_groups q) { return q; }
// (GQ: empty for the plain search, whose kernel keeps its one argument; one sel_groups for the diverse one)
template <bool GR, typename... GQ>
__global__ __launch_bounds__(1024) void beam_select_kernel(const isc_beam_select_args a, const GQ... gq) {
    const int groups = sel_groups_of(gq...).groups;
    const double lambda = sel_groups_of(gq...).lambda;
    extern __shared__ __attribute__((aligned(16))) unsigned char sel_smem[];
    __shared__ double cs[64];                          // the image's candidates (<= beam x beam): score,
    __shared__ long long ctk[64];                      //   token
    __shared__ float nrm[ISC_BEAM_MAX][2];             // per row: max, log(sum)
    __shared__ int w_par[ISC_BEAM_MAX], w_car[ISC_BEAM_MAX], w_len[ISC_BEAM_MAX];     // winners by rank
    __shared__ long long w_tok[ISC_BEAM_MAX];
    __shared__ int cpen[GR ? 64 : 1], w_pen[GR ? ISC_BEAM_MAX : 1];     // GR: appended token of a candidate (-1: carried) / winner (-2)
    rows_kernarg_warm<ROWS_KERNARG_LINES(isc_beam_select_args)>();
    const int i = blockIdx.x, tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int beam = a.beam, T = a.T, base = i * beam, n_tile = a.n_tile;
    const bool merger = wave < beam;                  // (wave-uniform) else: a side wave
    const int wrow = merger ? wave : wave - beam;     // the beam row this wave serves
    RSTAMP(0);
    // ---- the two block-uniform switches first (their round trip runs under everything requested behind them; without
    // live_in the same load reads this launch's own `beam` > 0 out of the argument block - no branch in front of a load)
    typedef const __attribute__((address_space(1))) int *sel_gint_p;      // (global, not flat: counted in order with the rest)
    const sel_gint_p gop = a.live_in ? (sel_gint_p)(unsigned long long)a.live_in
                                     : (sel_gint_p)((unsigned long long)__builtin_amdgcn_kernarg_segment_ptr() +
                                                    offsetof(isc_beam_select_args, beam));
    const int done_v = a.done[i];
    const int go_v = *gop;
    const int row = base + wrow;
    float cvv[ISC_SEL_TILES_PER_LANE][8];
    int cid[ISC_SEL_TILES_PER_LANE][8];
    float pm[ISC_SEL_TILES_PER_LANE], ps[ISC_SEL_TILES_PER_LANE];
    long long wv[4];                                  // the row's word list, positions lane, lane + 64, ..
    long long *wl = reinterpret_cast<long long *>(sel_smem);                                              // [row][T]
    float *st_lds = reinterpret_cast<float *>(sel_smem + (((size_t)beam * T * 8 + 15) & ~(size_t)15));   // [plane][row][H]
    const int rows_all = a.n_img * beam;
    // parents' bookkeeping: lane l of EVERY wave holds parent min(l & 7, beam - 1)
    const int pk = (lane & 7) < beam ? (lane & 7) : beam - 1;
    double my_score = 0.0;
    int my_len = 0;
    if (merger) {
        const float *cvp = a.cand_val + (long long)row * n_tile * 8;        // (wave-uniform bases, 32-bit lane offsets)
        const int *cip = a.cand_idx + (long long)row * n_tile * 8;
#pragma unroll
        for (int q = 0; q < ISC_SEL_TILES_PER_LANE; ++q) {
            const unsigned tl = lane + 64 * q, tc = tl < (unsigned)n_tile ? tl : (unsigned)n_tile - 1u;
            const float4 *gv = reinterpret_cast<const float4 *>(cvp + tc * 8u);
            const int4 *gi = reinterpret_cast<const int4 *>(cip + tc * 8u);
            const float4 v0 = gv[0], v1 = gv[1];
            const int4 i0 = gi[0], i1 = gi[1];
            cvv[q][0] = v0.x; cvv[q][1] = v0.y; cvv[q][2] = v0.z; cvv[q][3] = v0.w;
            cvv[q][4] = v1.x; cvv[q][5] = v1.y; cvv[q][6] = v1.z; cvv[q][7] = v1.w;
            cid[q][0] = i0.x; cid[q][1] = i0.y; cid[q][2] = i0.z; cid[q][3] = i0.w;
            cid[q][4] = i1.x; cid[q][5] = i1.y; cid[q][6] = i1.z; cid[q][7] = i1.w;
        }
        my_score = a.score_in[base + pk];
        my_len = a.len_in[base + pk];
    }
    const long long my_last = a.last_in[base + pk];
    if (!merger) {
        const float *pmp = a.part_max + (long long)row * n_tile, *psp = a.part_sum + (long long)row * n_tile;
#pragma unroll
        for (int q = 0; q < ISC_SEL_TILES_PER_LANE; ++q) {
            const unsigned tl = lane + 64 * q, tc = tl < (unsigned)n_tile ? tl : (unsigned)n_tile - 1u;
            pm[q] = pmp[tc];
            ps[q] = psp[tc];
        }
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            const int pos = lane + 64 * q;
            wv[q] = a.words_in[(long long)row * T + (pos < T ? pos : T - 1)];
        }
        if (a.state_out) {
            // this row's planes -> LDS image [plane][row][H], on their way while the merges run
            const unsigned lds0 = (unsigned)(size_t)st_lds;
            for (int pl = 0; pl < a.state_planes; ++pl) {
                const float *srow = a.state_in + ((long long)pl * rows_all + row) * a.H;
                const int pr = pl * beam + wrow;
                if ((a.H & 255) == 0) {
                    for (int c0 = 0; c0 < a.H; c0 += 256) {     // one 1 KB LDS-DMA per 256 floats
                        const unsigned dst = __builtin_amdgcn_readfirstlane(lds0 + (unsigned)(pr * a.H + c0) * 4u);
                        asm volatile("s_mov_b32 m0, %0\n\ts_nop 0\n\tglobal_load_lds_dwordx4 %1, off" :: "s"(dst), "v"(srow + c0 + lane * 4) : "memory");
                    }
                } else {                                        // small / odd widths: through registers
                    for (int c = lane * 4; c < a.H; c += 256)
                        *reinterpret_cast<float4 *>(st_lds + pr * a.H + c) = *reinterpret_cast<const float4 *>(srow + c);
                }
            }
        }
    }
    RSTAMP(1);
    if (__builtin_amdgcn_readfirstlane(go_v) == 0) {             // the search has ended (block-uniform)
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");         // (no LDS-DMA may land after the workgroup has gone)
        return;
    }
    if (__builtin_amdgcn_readfirstlane(done_v)) {                // frozen image: everything carried over unchanged (block-uniform)
        if (merger) {
            if (wave == 0 && lane < beam) {
                a.src_row[base + lane] = base + lane;
                a.last_out[base + lane] = my_last;
                a.score_out[base + lane] = my_score;
                a.len_out[base + lane] = my_len;
            }
        } else {
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                const int pos = lane + 64 * q;
                if (pos < T) a.words_out[(long long)row * T + pos] = wv[q];
            }
            asm volatile("s_waitcnt vmcnt(0)" ::: "memory");          // (a wave reads back only what it fetched itself)
            if (a.state_out)
                for (int pl = 0; pl < a.state_planes; ++pl)
                    for (int c = lane * 4; c < a.H; c += 256)
                        *reinterpret_cast<float4 *>(a.state_out + ((long long)pl * rows_all + row) * a.H + c) =
                            *reinterpret_cast<const float4 *>(st_lds + (pl * beam + wrow) * a.H + c);
        }
        return;
    }
    // ---- which parents have ended, where each parent's candidates start, how many there are: scalar work on one ballot
    const int ncand = a.t == 0 ? 1 : beam;
    const unsigned endm = a.t > 0 ? (unsigned)__ballot(my_last == a.eos_id) & ((1u << beam) - 1u) : 0u;
    // (GR: the parents are every row, at t == 0 the first row of every group - actm; candidates in front of parent p: gck(p))
    const int bp = GR ? beam / groups : beam;
    unsigned actm = (1u << ncand) - 1u;
    if constexpr (GR) {
        actm = (1u << beam) - 1u;
        if (a.t == 0) {
            actm = 0u;
            for (int g = 0; g < groups; ++g) actm |= 1u << (g * bp);
        }
    }
    auto gck = [&](int p) {
        const unsigned below = (1u << p) - 1u;
        return beam * __builtin_popcount(actm & below) - (beam - 1) * __builtin_popcount(endm & actm & below);
    };
    const int n = GR ? gck(beam) : ncand * beam - (beam - 1) * __builtin_popcount(endm & ((1u << ncand) - 1u));
    const int nrow = GR ? beam : n < beam ? n : beam;             // (t == 0: one live parent still yields `beam` rows)
    float myraw = -INFINITY;              // lane k < beam of a merge wave: the row's k-th best (raw logit, word id)
    int myid = 0;
    if (merger) {
#pragma unroll
        for (int q = 0; q < ISC_SEL_TILES_PER_LANE; ++q)
            if (lane + 64 * q >= n_tile) {
#pragma unroll
                for (int s_ = 0; s_ < 8; ++s_) cvv[q][s_] = -INFINITY;
            }
        // ---- k-way merge over the tiles' list heads: per round ONE 32-bit wave maximum of the lanes' best heads; ties
        // (equal values) go to the smaller word id = the smaller tile index = the first q with a lane at the maximum, then
        // its lowest lane - four ballots and scalar bit scans, no 64-bit keys in the lanes
        unsigned long long own[ISC_SEL_TILES_PER_LANE];         // lanes whose tile q exists (wave-uniform)
#pragma unroll
        for (int q = 0; q < ISC_SEL_TILES_PER_LANE; ++q) own[q] = __ballot(lane + 64 * q < n_tile);
        RSTAMP(2);
        for (int k = 0; k < beam; ++k) {
            const float mx = sel_wave_fmax(fmaxf(fmaxf(cvv[0][0], cvv[1][0]), fmaxf(cvv[2][0], cvv[3][0])));
            const unsigned long long h0 = __ballot(cvv[0][0] == mx) & own[0], h1 = __ballot(cvv[1][0] == mx) & own[1];
            const unsigned long long h2 = __ballot(cvv[2][0] == mx) & own[2], h3 = __ballot(cvv[3][0] == mx) & own[3];
            // the winning list as four lane masks, three of them empty (all empty: a NaN maximum - nothing moves)
            const unsigned long long f0 = h0, f1 = h0 ? 0 : h1, f2 = (h0 | h1) ? 0 : h2, f3 = (h0 | h1 | h2) ? 0 : h3;
            const unsigned long long fa = f0 | f1 | f2 | f3;
            const int wl = fa ? __builtin_ctzll(fa) : 0;        // its lowest lane
            const bool mel = lane == wl;
            const bool me0 = mel & (f0 != 0), me1 = mel & (f1 != 0), me2 = mel & (f2 != 0), me3 = mel & (f3 != 0);
            const int hidv = me0 ? cid[0][0] : me1 ? cid[1][0] : me2 ? cid[2][0] : cid[3][0];
            const int wid = fa ? __builtin_amdgcn_readlane(hidv, wl) : 0;
            SEL_SHIFT(0, 0, 4) SEL_SHIFT(1, 0, 4) SEL_SHIFT(2, 0, 4) SEL_SHIFT(3, 0, 4)
            if (beam > 5) {
                SEL_SHIFT(0, 4, 7) SEL_SHIFT(1, 4, 7) SEL_SHIFT(2, 4, 7) SEL_SHIFT(3, 4, 7)
                cvv[0][7] = me0 ? -INFINITY : cvv[0][7]; cvv[1][7] = me1 ? -INFINITY : cvv[1][7];
                cvv[2][7] = me2 ? -INFINITY : cvv[2][7]; cvv[3][7] = me3 ? -INFINITY : cvv[3][7];
            }
            myraw = lane == k ? (fa ? mx : -INFINITY) : myraw;
            myid = lane == k ? wid : myid;
        }
        RSTAMP(3);
    } else {
        // ---- side wave: the row's normaliser - max over the tile maxima, sum of the rescaled tile sums - and its word
        // list -> LDS
#pragma unroll
        for (int q = 0; q < ISC_SEL_TILES_PER_LANE; ++q)
            if (lane + 64 * q >= n_tile) { pm[q] = -INFINITY; ps[q] = 0.f; }
        const float gmax = sel_wave_fmax(fmaxf(fmaxf(pm[0], pm[1]), fmaxf(pm[2], pm[3])));
        float ssum = 0.f;
#pragma unroll
        for (int q = 0; q < ISC_SEL_TILES_PER_LANE; ++q) ssum += ps[q] * expf(pm[q] - gmax);
        ssum = sel_wave_sum(ssum);
        if (lane == 0) {
            if (!(fabsf(gmax) <= 3.0e38f && ssum <= 3.0e38f)) isc_flag_pw(ISC_STATUS_WORD_STATS);     // NaN fails both
            nrm[wrow][0] = gmax;
            nrm[wrow][1] = logf(ssum);
        }
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            const int pos = lane + 64 * q;
            if (pos < T) wl[wrow * T + pos] = wv[q];
        }
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");          // this wave's share of the state image has landed
    }
    __syncthreads();                                              // normalisers, word lists, state image
    if (merger) {
        const float myv = (myraw - nrm[wave][0]) - nrm[wave][1];  // (-inf stays -inf)
        if (a.top_val && lane < beam) {
            a.top_val[(long long)row * beam + lane] = myv;
            a.top_idx[(long long)row * beam + lane] = (unsigned)myid < (unsigned)a.V ? myid : 0;
        }
        // ---- parent `wave`'s candidates (captioner.py:378-411; beam_merge_kernel's rules): an ended parent is carried as
        // ONE candidate with its score, a live one expands into its `beam` best words
        if (GR ? (actm >> wave) & 1u : wave < ncand) {
            const int ended = (endm >> wave) & 1u;
            const int ck = GR ? gck(wave) : wave * beam - (beam - 1) * __builtin_popcount(endm & ((1u << wave) - 1u));
            const double sc_k = __hiloint2double(__builtin_amdgcn_readlane(__double2hiint(my_score), wave),
                                                 __builtin_amdgcn_readlane(__double2loint(my_score), wave));
            if (lane < (ended ? 1 : beam)) {
                cs[ck + lane] = ended ? sc_k : sc_k + (double)myv;
                ctk[ck + lane] = ended ? a.eos_id : (long long)((unsigned)myid < (unsigned)a.V ? myid : 0);
                if constexpr (GR) cpen[ck + lane] = ended ? -1 : ((unsigned)myid < (unsigned)a.V ? myid : 0);
            }
        }
    }
    RSTAMP(4);
    __syncthreads();                                              // candidates
    RSTAMP(5);
    if constexpr (GR) {
        // ---- group-sequential rank: round g is the plain rank over group g's candidates [lo, hi) (<= bp x beam <= 32: four
        // per lane, eight lanes per candidate) by their keys; a key is formed where it is compared - the score, the
        // candidate's appended token against the g x bp winners' in front of it (w_pen).  One barrier between rounds: the
        // next group's waves read this round's w_pen.
        const int wgrp = wave / bp;                       // (merge waves: the group of parent `wave`)
        for (int g = 0; g < groups; ++g) {
            if (merger && wgrp == g && ((actm >> wave) & 1u)) {
                const int ended = (endm >> wave) & 1u;
                const int ck = gck(wave), lo = gck(g * bp), hi = gck((g + 1) * bp), nch = g * bp;
                const int j = lane >> 3, s_ = lane & 7, c = ck + j;
                const bool mine_ok = j < (ended ? 1 : beam);
                auto key_of = [&](int it) {
                    const int pen = cpen[it];
                    int cn = 0;
                    for (int s = 0; s < nch; ++s) cn += w_pen[s] == pen;
                    return pen < 0 ? cs[it] : beam_group_key(cs[it], lambda, cn);
                };
                const double mine = key_of(mine_ok ? c : lo);
                int cnt = 0;
#pragma unroll
                for (int u = 0; u < 4; ++u) {
                    const int it = lo + s_ + 8 * u;
                    const double o = key_of(it < hi ? it : lo);
                    cnt += (it < hi) & ((int)(o > mine) | ((int)(o == mine) & (int)(it < c)));
                }
                cnt += isc_dpp<ISC_DPP_XOR1>(cnt);
                cnt += isc_dpp<ISC_DPP_XOR2>(cnt);
                cnt += isc_dpp<ISC_DPP_HALF_MIRROR>(cnt);
                if (s_ == 0 && mine_ok && cnt < bp) {
                    const int len = __builtin_amdgcn_readlane(my_len, wave);
                    const int slot = nch + cnt, dst = base + slot;
                    const long long tok = ctk[c];
                    w_par[slot] = wave; w_car[slot] = ended; w_len[slot] = len; w_tok[slot] = tok;
                    w_pen[slot] = ended ? -2 : cpen[c];
                    a.score_out[dst] = cs[c];                   // the model's log-probability: un-augmented
                    a.last_out[dst] = tok;
                    a.src_row[dst] = base + wave;
                    a.len_out[dst] = len + (ended ? 0 : 1);
                }
            }
            if (g + 1 < groups) __syncthreads();
        }
        if (tid == 0) {
            if ((endm & actm) == actm) a.done[i] = 1;
            else atomicAdd(&a.live[a.t + 1], 1);
        }
    } else if (merger) {
        if (wave < ncand) {
            // stable descending rank of candidate c = ck + j: lanes 8 j .. 8 j + 7 each count an eighth of the others
            const int ended = (endm >> wave) & 1u;
            const int ck = wave * beam - (beam - 1) * __builtin_popcount(endm & ((1u << wave) - 1u));
            const int j = lane >> 3, s_ = lane & 7, c = ck + j;
            const bool mine_ok = j < (ended ? 1 : beam);
            const double mine = cs[mine_ok ? c : 0];
            int cnt = 0;
#pragma unroll
            for (int u = 0; u < 8; ++u) {
                const int it = s_ + 8 * u;
                const double o = cs[it];                        // (it < 64: inside the array; counted only below n)
                cnt += (it < n) & ((int)(o > mine) | ((int)(o == mine) & (int)(it < c)));
            }
            cnt += isc_dpp<ISC_DPP_XOR1>(cnt);
            cnt += isc_dpp<ISC_DPP_XOR2>(cnt);
            cnt += isc_dpp<ISC_DPP_HALF_MIRROR>(cnt);
            if (s_ == 0 && mine_ok && cnt < beam) {
                const int len = __builtin_amdgcn_readlane(my_len, wave);
                const int dst = base + cnt;
                const long long tok = ctk[c];
                w_par[cnt] = wave; w_car[cnt] = ended; w_len[cnt] = len; w_tok[cnt] = tok;
                a.score_out[dst] = mine;
                a.last_out[dst] = tok;
                a.src_row[dst] = base + wave;
                a.len_out[dst] = len + (ended ? 0 : 1);
            }
        }
        if (tid == 0) {
            const unsigned all = (1u << ncand) - 1u;
            if ((endm & all) == all) a.done[i] = 1;
            else atomicAdd(&a.live[a.t + 1], 1);
        }
    }
    __syncthreads();                                              // winners
    RSTAMP(6);
    if (wrow >= nrow) return;
    const int par = w_par[wrow];
    if (merger) {
        // ---- new row `wave`'s word list: its parent's, with the new token at the parent's length
        const int car = w_car[wrow], len = w_len[wrow];
        const long long tok = w_tok[wrow];
        for (int pos = lane; pos < T; pos += 64)
            a.words_out[(long long)row * T + pos] = (!car && pos == len) ? tok : wl[par * T + pos];
    } else if (a.state_out) {
        // ---- the recurrent state follows the candidates: new row r continues its parent's
        for (int pl = 0; pl < a.state_planes; ++pl)
            for (int c = lane * 4; c < a.H; c += 256)
                *reinterpret_cast<float4 *>(a.state_out + ((long long)pl * rows_all + row) * a.H + c) =
                    *reinterpret_cast<const float4 *>(st_lds + (pl * beam + par) * a.H + c);
    }
    RSTAMP(7);
}
#undef SEL_SHIFT

// The argument checks of both entry points; *lds_out = the launch's dynamic LDS.
static int beam_select_check(const isc_beam_select_args &a, size_t *lds_out) {
    if (!a.part_max || !a.part_sum || !a.cand_val || !a.cand_idx || !a.score_in || !a.score_out || !a.last_in ||
        !a.last_out || !a.words_in || !a.words_out || !a.len_in || !a.len_out || !a.done || !a.src_row || !a.live)
        return ISC_E_NULL;
    if ((a.top_val == nullptr) != (a.top_idx == nullptr)) return ISC_E_NULL;
    if ((a.state_in == nullptr) != (a.state_out == nullptr)) return ISC_E_NULL;
    if (a.state_out && (a.state_planes <= 0 || a.H <= 0 || (a.H & 3) || a.state_in == a.state_out)) return ISC_E_SHAPE;
    if (a.state_out && (!isc_aligned16(a.state_in) || !isc_aligned16(a.state_out))) return ISC_E_ALIGN;
    if (a.n_img <= 0 || a.beam <= 0 || a.beam > ISC_BEAM_MAX || a.T <= 0 || a.t < 0 || a.t >= a.T || a.V <= 0)
        return ISC_E_SHAPE;
    if (a.n_tile < 1 || a.n_tile > 64 * ISC_SEL_TILES_PER_LANE) return ISC_E_SHAPE;
    if (!isc_aligned16(a.cand_val) || !isc_aligned16(a.cand_idx)) return ISC_E_ALIGN;
    size_t lds = (((size_t)a.beam * a.T * 8 + 15) & ~(size_t)15);                // the parents' word lists
    if (a.state_out) lds += (size_t)a.state_planes * a.beam * a.H * 4 + 1024;    // + the image's rows of the state (whole 1 KB pieces)
    if (lds > 150000) return ISC_E_SHAPE;
    if (a.T > 256) return ISC_E_SHAPE;
    *lds_out = lds;
    return ISC_OK;
}

extern "C" int isc_beam_select(const isc_beam_select_args *args, void *stream) {
    if (!args) return ISC_E_NULL;
    const isc_beam_select_args &a = *args;
    size_t lds = 0;
    const int rc = beam_select_check(a, &lds);
    if (rc != ISC_OK) return rc;
    static std::atomic<bool> attr_set{false};
    if (!attr_set.load()) {
        hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void *>(&beam_select_kernel<false>),
                                           hipFuncAttributeMaxDynamicSharedMemorySize, 150000);
        if (e != hipSuccess) return (int)e;
        attr_set.store(true);
    }
    // one merge wave + one side wave per beam row
    hipLaunchKernelGGL(beam_select_kernel<false>, dim3(a.n_img), dim3(128 * a.beam), lds, (hipStream_t)stream, a);
    ISC_LAUNCH_CHECK();
    return ISC_OK;
}

extern "C" int isc_beam_select_groups(const isc_beam_select_args *args, int groups, double lambda, void *stream) {
    if (!args) return ISC_E_NULL;
    const isc_beam_select_args &a = *args;
    size_t lds = 0;
    const int rc = beam_select_check(a, &lds);
    if (rc != ISC_OK) return rc;
    if (!beam_groups_ok(a.beam, groups, lambda)) return ISC_E_SHAPE;
    // one group is the plain search for any lambda (no candidate is penalised): the plain kernel.  The group rounds below
    // rank at most 32 candidates (four per lane), which holds for groups >= 2 only: bp x beam <= (beam / 2) x beam <= 32.
    if (groups == 1) return isc_beam_select(args, stream);
    static std::atomic<bool> attr_set{false};
    if (!attr_set.load()) {
        hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void *>(&beam_select_kernel<true, sel_groups>),
                                           hipFuncAttributeMaxDynamicSharedMemorySize, 150000);
        if (e != hipSuccess) return (int)e;
        attr_set.store(true);
    }
    hipLaunchKernelGGL((beam_select_kernel<true, sel_groups>), dim3(a.n_img), dim3(128 * a.beam), lds, (hipStream_t)stream, a,
                       sel_groups{groups, lambda});
    ISC_LAUNCH_CHECK();
    return ISC_OK;
}

// ------------------------------------------------------------------ XECriterion
// Single workgroup, fixed reduction order => bitwise reproducible loss.
__global__ __launch_bounds__(256) void xe_loss_kernel(const float *logp, const int64_t *target,
                                                      const int *lengths, int B, int T, int V,
                                                      float *out2) {
    __shared__ float ss[4], sn[4];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    float s = 0.f, n = 0.f;
    for (int i = tid; i < B * T; i += 256) {
        const int b = i / T, t = i % T;
        if (t < lengths[b]) {
            s -= logp[(long long)i * V + target[i]];
            n += 1.f;
        }
    }
    s = wave_sum(s);
    n = wave_sum(n);
    if (lane == 0) { ss[wave] = s; sn[wave] = n; }
    __syncthreads();
    if (tid == 0) {
        out2[0] = (ss[0] + ss[1]) + (ss[2] + ss[3]);
        out2[1] = (sn[0] + sn[1]) + (sn[2] + sn[3]);
    }
}

extern "C" int isc_xe_loss_fwd(const float *logp, const int64_t *target, const int32_t *lengths,
                               int B, int T, int V, float *out2, void *stream) {
    if (!logp || !target || !lengths || !out2) return ISC_E_NULL;
    if (B <= 0 || T <= 0 || V <= 0) return ISC_E_SHAPE;
    hipLaunchKernelGGL(xe_loss_kernel, dim3(1), dim3(256), 0, (hipStream_t)stream, logp, target, lengths,
                       B, T, V, out2);
    ISC_LAUNCH_CHECK();
    return ISC_OK;
}

// ------------------------------------------------------------------ criteria on RAW logits (training: no [B,T,V] log-probs)
// The criteria of this path read ONE column per (caption, step) row - XECriterion the target (captioner.py:427-440), the
// REINFORCE term the drawn token (captioner.py:336).  log p(id) = (x[id] - max) - log(sum exp) comes straight from the raw
// logits and the classifier's tile statistics: the [B,T,V] log-prob tensor (F.log_softmax at captioner.py:183 over every
// step) is then never written or read in a training iteration (0.56 ms of a 15.6 ms iteration at B = 1024).  Same
// expression as logsoftmax_apply_steps_kernel: the values are the bits that tensor would have held.
// One wave per row; rows in [B,T] order (ids / out), logits row (b,t) at b*ld_b + t*ld_t, statistics row t*step_rows + b.
__global__ __launch_bounds__(256) void gather_logp_raw_kernel(const float *raw, long long ld_b, long long ld_t, int B, int T,
                                                              const float *pmax, const float *psum, int n_tile,
                                                              int step_rows, const int64_t *ids, const float *live,
                                                              float *out) {
    const int lane = threadIdx.x & 63;
    const int mi = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (mi >= B * T) return;
    const int b = mi / T, t = mi - b * T;
    const long long ms = (long long)t * step_rows + b;
    float gmax, S;
    int gi;
    fold_row_stats(pmax + ms * n_tile, psum + ms * n_tile, nullptr, n_tile, lane, gmax, gi, S);
    if (lane == 0) {
        const float x = raw[(long long)b * ld_b + (long long)t * ld_t + ids[mi]];
        const float lp = (x - gmax) - logf(S);
        out[mi] = live ? lp * live[t] : lp;
    }
}

extern "C" int isc_gather_logp_raw(const float *raw, int64_t ld_b, int64_t ld_t, int B, int T, int V, const float *part_max,
                                   const float *part_sum, int step_rows, const int64_t *ids, const float *live, float *out,
                                   void *stream) {
    if (!raw || !part_max || !part_sum || !ids || !out) return ISC_E_NULL;
    if (B <= 0 || T <= 0 || V <= 0 || (long long)B * T > 2147483647LL) return ISC_E_SHAPE;
    if (step_rows == 0) step_rows = B;
    if (step_rows < B) return ISC_E_SHAPE;
    hipLaunchKernelGGL(gather_logp_raw_kernel, dim3((unsigned)((B * T + 3) / 4)), dim3(256), 0, (hipStream_t)stream, raw,
                       (long long)ld_b, (long long)ld_t, B, T, part_max, part_sum, (V + 127) / 128, step_rows, ids, live, out);
    ISC_LAUNCH_CHECK();
    return ISC_OK;
}

// XECriterion on per-token log-probs tlp [B,T] = log p(target): out2 = { -sum_{t < len_b} tlp, count }.  The summation
// order of xe_loss_kernel (single workgroup, thread-strided) - the same loss bits.
__global__ __launch_bounds__(256) void xe_loss_tokens_kernel(const float *tlp, const int *lengths, int B, int T, float *out2) {
    __shared__ float ss[4], sn[4];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    float s = 0.f, n = 0.f;
    for (int i = tid; i < B * T; i += 256) {
        const int b = i / T, t = i % T;
        if (t < lengths[b]) {
            s -= tlp[i];
            n += 1.f;
        }
    }
    s = wave_sum(s);
    n = wave_sum(n);
    if (lane == 0) { ss[wave] = s; sn[wave] = n; }
    __syncthreads();
    if (tid == 0) {
        out2[0] = (ss[0] + ss[1]) + (ss[2] + ss[3]);
        out2[1] = (sn[0] + sn[1]) + (sn[2] + sn[3]);
    }
}

extern "C" int isc_xe_loss_tokens_fwd(const float *tlp, const int32_t *lengths, int B, int T, float *out2, void *stream) {
    if (!tlp || !lengths || !out2) return ISC_E_NULL;
    if (B <= 0 || T <= 0) return ISC_E_SHAPE;
    hipLaunchKernelGGL(xe_loss_tokens_kernel, dim3(1), dim3(256), 0, (hipStream_t)stream, tlp, lengths, B, T, out2);
    ISC_LAUNCH_CHECK();
    return ISC_OK;
}

extern "C" int isc_abi_version(void) { return 2; }
extern "C" const char *isc_target_arch(void) { return "gfx950"; }
