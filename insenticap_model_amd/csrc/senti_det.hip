// The frozen image-sentiment detector (sentiment_detector.py:30-60 in eval mode), forward only: isc_senti_det_fwd.
//   x = conv3x3_{n-1}( ... conv3x3_0(features) ... )   (padding 1, cross-correlation, NO non-linearity in between)
//   r = relu(x);  m[j, p] = bs[j] + r[p, :] . Ws[j, :];  z = FC_{f-1}( ... FC_0(mean_p m) ... );  prob = softmax(z)
//   map[p] = sum_j prob_j m[j, p];  score = max prob;  label = first arg-max, neu_idx when score < threshold.
// The 3x3 convolutions are implicit GEMMs on the split-f16 engine (common.h: x = hi + lo 2^-11; three MFMA terms, the
// 2^-11 weight applied once): output row m = (b h + y) w + x, contraction over 9 taps x Cin in tap-major order, the A
// row of tap (dy, dx) = input pixel (b, y + dy, x + dx) read where it lies (channels-last: the features as they are, no
// im2col buffer, no padded copy) - or the workspace's zero line when the pixel is outside the image's own grid.
#include <atomic>

#include "common.h"

ISC_STATUS_DECL(sdet)

static std::atomic<long long> g_sdet_launches[ISC_SENTI_DET_KINDS];
extern "C" long long isc_senti_det_launches(int kind) {
    return kind >= 0 && kind < ISC_SENTI_DET_KINDS ? g_sdet_launches[kind].load() : -1;
}

typedef _Float16 sd_h8 __attribute__((ext_vector_type(8)));
typedef float sd_f4 __attribute__((ext_vector_type(4)));

// ------------------------------------------------------------------ weight pack
// w [N, Cin, 3, 3] fp32 -> planes of the K-concatenated matrix [N, 9 Cin], k = (ky 3 + kx) Cin + ci, in the plane layout
// of common.h (per row and 32-deep k-block: 32 hi halfs, then 32 lo halfs).  One thread per (n, k); runs once per weight
// version.
__global__ __launch_bounds__(256) void senti_det_pack_kernel(const float *w, int N, int Cin, _Float16 *planes) {
    const int K9 = 9 * Cin;
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    if (i >= (long long)N * K9) return;
    const int n = (int)(i / K9), k = (int)(i - (long long)n * K9);
    const int tap = k / Cin, ci = k - tap * Cin;
    _Float16 hi, lo;
    isc_split_f16(w[((long long)n * Cin + ci) * 9 + tap], hi, lo);
    const long long o = plane_index(n, k, K9);
    planes[o] = hi;
    planes[o + 32] = lo;
}

// ------------------------------------------------------------------ implicit-GEMM 3x3 convolution
// Tile 64 rows x 128 columns, four waves as 2 x 2, a wave = 32 x 64 = 2 row blocks x 4 column blocks of
// v_mfma_f32_16x16x32_f16.  Per 32-deep chunk (a tap and 32 of its channels) the workgroup stages A hi / A lo [64][32]
// and W hi / W lo [128][32] halfs in LDS, rows 80 bytes apart (16 rows x 16 bytes of one k-octet then fall on 16
// disjoint groups of four banks).  Global loads go to registers first, into two register sets: chunks c + 1 and c + 2
// are in flight while chunk c multiplies (one set: 5.9 ms at 512 images of 6 x 6 x 2048; two: 4.4 ms); two LDS buffers,
// one barrier per chunk (the buffer a wave writes in iteration c + 1 was last read in iteration c - 1, in front of the
// barrier of iteration c).
// Thread t stages k-octet (t & 3) of A row (t >> 2): eight fp32 values, split here (once per value, not once per
// fragment read), or eight halfs that are their own hi (AF16: lo is zero, no lo image, no al x bh MFMA - the fp32
// form on the up-cast values adds exact zeros there, so the bits are the same).
// An out-of-grid tap (and a row at or beyond M) reads the zero line: exact zeros, whatever the neighbouring image holds.
struct SdConvArgs {
    const void *A;              // [B h w, Cin] fp32 or halfs
    const void *zero;           // >= 32 zero bytes
    const _Float16 *W;          // planes [N, 2 * 9 Cin]
    const float *bias;          // [N]
    float *out;                 // ksplit == 1: [M, N]; else slabs [ksplit][M][N] of raw partial sums
    int h, w, Cin, N, M, relu, ksplit, _pad;
};
#define SD_BM 64
#define SD_BN 128
#define SD_LD 40                // halfs per LDS row: 32 + 8 of padding
#define SD_BUF (2 * SD_BM * SD_LD + 2 * SD_BN * SD_LD)      // halfs per buffer: A hi | A lo | W hi | W lo

// what a thread holds of one chunk between its global loads and its LDS stores
struct SdStageF16 {
    sd_h8 a0;                   // the eight halfs of the A octet
    uint4 w0, w1, w2, w3;
};
struct SdStageF32 {
    float4 a0, a1;              // the eight fp32 values of the A octet
    uint4 w0, w1, w2, w3;
};
template <bool AF16> struct SdStage { typedef SdStageF32 type; };
template <> struct SdStage<true> { typedef SdStageF16 type; };

template <bool AF16>
__global__ __launch_bounds__(256) void senti_det_conv_kernel(const SdConvArgs a) {
    __shared__ __attribute__((aligned(16))) _Float16 lds[2 * SD_BUF];
    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6, wm = wv >> 1, wn = wv & 1;
    const int row0 = blockIdx.y * SD_BM, col0 = blockIdx.x * SD_BN, ks = blockIdx.z;
    const int h = a.h, w = a.w, Cin = a.Cin, N = a.N, M = a.M;
    const int cpt = Cin >> 5, nchunks = 9 * cpt;                 // chunks per tap, chunks in all
    const int c_lo = (int)((long long)nchunks * ks / a.ksplit), c_hi = (int)((long long)nchunks * (ks + 1) / a.ksplit);

    // this thread's A row: pixel (b, y, x) of output row m
    const int ar = tid >> 2, aoct = tid & 3;
    const int m = row0 + ar;
    const bool m_ok = m < M;
    const int hw = h * w;
    const int mb = m_ok ? m / hw : 0, mrem = m_ok ? m - mb * hw : 0, my = mrem / w, mx = mrem - my * w;
    const int esz = AF16 ? 2 : 4;
    const char *Abase = static_cast<const char *>(a.A);
    const char *zrow = static_cast<const char *>(a.zero);
    // this thread's four 16-byte pieces of the W image: piece p = tid + 256 i -> row p >> 3, part p & 7 (0-3: hi octets,
    // 4-7: lo octets) = halfs [part * 8, + 8) of the row's 64-half k-block
    const _Float16 *wsrc[4];
    int wdst[4];
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const int p = tid + 256 * i, r = p >> 3, part = p & 7;
        const int gn = col0 + r < N ? col0 + r : N - 1;
        wsrc[i] = a.W + (long long)gn * 18 * Cin + part * 8;
        wdst[i] = 2 * SD_BM * SD_LD + (part >> 2) * SD_BN * SD_LD + r * SD_LD + (part & 3) * 8;
    }

    // two register sets: chunk c + 2 is requested while chunk c multiplies and chunk c + 1 waits in the other set
    typename SdStage<AF16>::type st0, st1;
    typedef typename SdStage<AF16>::type Stage;
    auto load = [&](int c, Stage &s) __attribute__((always_inline)) {
        const int tap = c / cpt, kc = c - tap * cpt;
        const int yy = my + tap / 3 - 1, xx = mx + tap % 3 - 1;
        const bool in = m_ok && yy >= 0 && yy < h && xx >= 0 && xx < w;
        const char *src = in ? Abase + ((((long long)mb * h + yy) * w + xx) * Cin + kc * 32 + aoct * 8) * esz : zrow;
        if constexpr (AF16) {
            s.a0 = *reinterpret_cast<const sd_h8 *>(src);
        } else {
            s.a0 = *reinterpret_cast<const float4 *>(src);
            s.a1 = *reinterpret_cast<const float4 *>(src + 16);
        }
        s.w0 = *reinterpret_cast<const uint4 *>(wsrc[0] + (long long)c * 64);
        s.w1 = *reinterpret_cast<const uint4 *>(wsrc[1] + (long long)c * 64);
        s.w2 = *reinterpret_cast<const uint4 *>(wsrc[2] + (long long)c * 64);
        s.w3 = *reinterpret_cast<const uint4 *>(wsrc[3] + (long long)c * 64);
    };
    auto store = [&](const Stage &s, int S) __attribute__((always_inline)) {     // set S -> LDS buffer S
        _Float16 *b = lds + S * SD_BUF;
        if constexpr (AF16) {
            *reinterpret_cast<sd_h8 *>(b + ar * SD_LD + aoct * 8) = s.a0;
        } else {
            const float x[8] = {s.a0.x, s.a0.y, s.a0.z, s.a0.w, s.a1.x, s.a1.y, s.a1.z, s.a1.w};
            sd_h8 hi, lo;
#pragma unroll
            for (int e = 0; e < 8; ++e) {
                _Float16 hh, ll;
                isc_split_f16(x[e], hh, ll);
                hi[e] = hh;
                lo[e] = ll;
            }
            *reinterpret_cast<sd_h8 *>(b + ar * SD_LD + aoct * 8) = hi;
            *reinterpret_cast<sd_h8 *>(b + SD_BM * SD_LD + ar * SD_LD + aoct * 8) = lo;
        }
        *reinterpret_cast<uint4 *>(b + wdst[0]) = s.w0;
        *reinterpret_cast<uint4 *>(b + wdst[1]) = s.w1;
        *reinterpret_cast<uint4 *>(b + wdst[2]) = s.w2;
        *reinterpret_cast<uint4 *>(b + wdst[3]) = s.w3;
    };

    sd_f4 acc0[2][4], acc1[2][4];
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int j = 0; j < 4; ++j)
#pragma unroll
            for (int r = 0; r < 4; ++r) { acc0[i][j][r] = 0.f; acc1[i][j][r] = 0.f; }

    const int fr = lane & 15, fq = lane >> 4;
    auto step = [&](int c, Stage &s, int S) __attribute__((always_inline)) {
        store(s, S);
        __syncthreads();
        if (c + 2 < c_hi) load(c + 2, s);
        const _Float16 *b = lds + S * SD_BUF;
        sd_h8 ah[2], al[2];
#pragma unroll
        for (int i = 0; i < 2; ++i) {
            const int o = (wm * 32 + i * 16 + fr) * SD_LD + fq * 8;
            ah[i] = *reinterpret_cast<const sd_h8 *>(b + o);
            if constexpr (!AF16) al[i] = *reinterpret_cast<const sd_h8 *>(b + SD_BM * SD_LD + o);
        }
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const int o = 2 * SD_BM * SD_LD + (wn * 64 + j * 16 + fr) * SD_LD + fq * 8;
            const sd_h8 bh = *reinterpret_cast<const sd_h8 *>(b + o);
            const sd_h8 bl = *reinterpret_cast<const sd_h8 *>(b + SD_BN * SD_LD + o);
#pragma unroll
            for (int i = 0; i < 2; ++i) {
                acc0[i][j] = __builtin_amdgcn_mfma_f32_16x16x32_f16(ah[i], bh, acc0[i][j], 0, 0, 0);
                acc1[i][j] = __builtin_amdgcn_mfma_f32_16x16x32_f16(ah[i], bl, acc1[i][j], 0, 0, 0);
                if constexpr (!AF16)
                    acc1[i][j] = __builtin_amdgcn_mfma_f32_16x16x32_f16(al[i], bh, acc1[i][j], 0, 0, 0);
            }
        }
    };
    if (c_lo < c_hi) load(c_lo, st0);
    if (c_lo + 1 < c_hi) load(c_lo + 1, st1);
    for (int c = c_lo; c < c_hi; c += 2) {
        step(c, st0, 0);
        if (c + 1 < c_hi) step(c + 1, st1, 1);
    }

    // C/D layout: register r of block (i, j) = tile row wm 32 + i 16 + 4 (lane >> 4) + r, column wn 64 + j 16 + (lane & 15)
    float *out = a.out + (a.ksplit > 1 ? (long long)ks * M * N : 0);
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        const int gn = col0 + wn * 64 + j * 16 + fr;
        if (gn >= N) continue;
        const float bv = a.ksplit > 1 ? 0.f : a.bias[gn];
#pragma unroll
        for (int i = 0; i < 2; ++i)
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int gm = row0 + wm * 32 + i * 16 + 4 * fq + r;
                if (gm >= M) continue;
                float v = fmaf(acc1[i][j][r], ISC_SPLIT_LO_WEIGHT, acc0[i][j][r]);
                if (a.ksplit == 1) {
                    v += bv;
                    if (a.relu) v = isc_relu(v);
                }
                out[(long long)gm * N + gn] = v;
            }
    }
}

// out[m, n] = (relu)(slab_0 + slab_1 + ... + slab_{S-1} + bias[n]): slabs ascending, then the bias - one fixed order.
__global__ __launch_bounds__(256) void senti_det_reduce_kernel(const float *slabs, int S, long long MN, int N,
                                                               const float *bias, int relu, float *out) {
    const long long i4 = ((long long)blockIdx.x * 256 + threadIdx.x) * 4;     // (N % 16 == 0: a float4 stays in its row)
    if (i4 >= MN) return;
    float4 s = *reinterpret_cast<const float4 *>(slabs + i4);
    for (int k = 1; k < S; ++k) {
        const float4 v = *reinterpret_cast<const float4 *>(slabs + (long long)k * MN + i4);
        s.x += v.x; s.y += v.y; s.z += v.z; s.w += v.w;
    }
    const float4 b = *reinterpret_cast<const float4 *>(bias + (int)(i4 % N));
    s.x += b.x; s.y += b.y; s.z += b.z; s.w += b.w;
    if (relu) { s.x = isc_relu(s.x); s.y = isc_relu(s.y); s.z = isc_relu(s.z); s.w = isc_relu(s.w); }
    *reinterpret_cast<float4 *>(out + i4) = s;
}

// ------------------------------------------------------------------ tail
// One workgroup of four waves per image.  Wave v takes the pixels p = v, v + 4, ...; its lanes walk the CL channels of
// r[p, :] (lane l: channels l, l + 64, ... ascending), the butterfly folds the lanes - one fixed order - and the k map
// values of the pixel go to LDS.  Thread j < k then sums map j over p ascending; thread 0 runs the FC layers, the
// softmax and the decision; all threads write map[p] = sum_j prob_j m[j, p] (j ascending).
struct SdTailArgs {
    const float *r;             // [B, hw, CL] post-ReLU
    const float *Ws, *bs;       // [k, CL], [k]
    const float *fc_w[ISC_SENTI_DET_MAX_FCS], *fc_b[ISC_SENTI_DET_MAX_FCS];
    int hw, CL, k, n_fcs, neu_idx;
    float threshold;
    float *logits, *maps, *scores;
    int64_t *labels;
};
__global__ __launch_bounds__(256) void senti_det_tail_kernel(const SdTailArgs a) {
    extern __shared__ float sd_m[];                 // [8][hw] maps, then 8 probabilities
    const int b = blockIdx.x, lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int hw = a.hw, CL = a.CL, k = a.k;
    float *prob = sd_m + 8 * hw;
    for (int p = wave; p < hw; p += 4) {
        const float *row = a.r + ((long long)b * hw + p) * CL;
        float acc[8];
#pragma unroll
        for (int j = 0; j < 8; ++j) acc[j] = 0.f;
        for (int c = lane; c < CL; c += 64) {
            const float v = row[c];
#pragma unroll
            for (int j = 0; j < 8; ++j)
                if (j < k) acc[j] += v * a.Ws[(long long)j * CL + c];
        }
#pragma unroll
        for (int j = 0; j < 8; ++j)
            if (j < k) {
                const float s = wave_sum(acc[j]) + a.bs[j];
                if (lane == 0) sd_m[j * hw + p] = s;
            }
    }
    __syncthreads();
    if (threadIdx.x < k) {
        float s = 0.f;
        for (int p = 0; p < hw; ++p) s += sd_m[threadIdx.x * hw + p];
        prob[threadIdx.x] = s / (float)hw;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        float z[8], t[8];
        for (int j = 0; j < k; ++j) z[j] = prob[j];
        for (int l = 0; l < a.n_fcs; ++l) {
            for (int i = 0; i < k; ++i) {
                float s = 0.f;
                for (int j = 0; j < k; ++j) s += z[j] * a.fc_w[l][i * k + j];
                t[i] = s + a.fc_b[l][i];
            }
            for (int i = 0; i < k; ++i) z[i] = t[i];
        }
        bool bad = false;
        float mxz = z[0];
        for (int j = 0; j < k; ++j) {
            a.logits[(long long)b * k + j] = z[j];
            bad |= !(fabsf(z[j]) <= 3.0e38f);
            if (z[j] > mxz) mxz = z[j];
        }
        float sum = 0.f;
        for (int j = 0; j < k; ++j) { t[j] = expf(z[j] - mxz); sum += t[j]; }
        float best = 0.f;
        int arg = 0;
        for (int j = 0; j < k; ++j) {
            t[j] = t[j] / sum;
            prob[j] = t[j];
            if (j == 0 || t[j] > best) { best = t[j]; arg = j; }
        }
        if (bad) {
            isc_flag_sdet(ISC_STATUS_WORD_STATS);
            arg = a.neu_idx;
        } else if (best < a.threshold) {
            arg = a.neu_idx;
        }
        a.scores[b] = best;
        a.labels[b] = arg;
    }
    __syncthreads();
    for (int p = threadIdx.x; p < hw; p += 256) {
        float s = 0.f;
        for (int j = 0; j < k; ++j) s += prob[j] * sd_m[j * hw + p];
        a.maps[(long long)b * hw + p] = s;
    }
}

// ------------------------------------------------------------------ driver
namespace {
long long sd_up64(long long n) { return (n + 63) / 64 * 64; }
// every conv's Cin = C >> i a multiple of 32 (the last Cout is then a multiple of 16)
bool sd_shape_ok(long long B, long long h, long long w, long long C, int n_convs) {
    if (B < 1 || h < 1 || w < 1 || h * w > ISC_SENTI_DET_MAX_HW || B * h * w > (1LL << 22) || C < 32 || C > 65536 ||
        n_convs < 1 || n_convs > ISC_SENTI_DET_MAX_CONVS)
        return false;
    for (int i = 0; i < n_convs; ++i)
        if (((C >> i) % 32) != 0) return false;
    return true;
}
// Route of one conv layer: 1 = one workgroup per tile with the epilogue in the kernel; n > 1 = the contraction split
// over n workgroups per tile, raw partial tiles to slabs, a reduce kernel behind them.  Auto: launches of fewer than
// 128 tiles (half the chip's 256 CUs) split until about 256 workgroups run, 32 at the most, every share >= 2 chunks.
int sd_ksplit(long long M, int N, int Cin, int want) {
    const int nchunks = 9 * (Cin / 32);
    int s = want;
    if (s <= 0) {
        const long long tiles = ((M + SD_BM - 1) / SD_BM) * ((N + SD_BN - 1) / SD_BN);
        if (tiles >= 128) return 1;
        s = (int)((256 + tiles - 1) / tiles);
        if (s > 32) s = 32;
        if (s > nchunks / 2) s = nchunks / 2;
    }
    if (s > nchunks) s = nchunks;
    return s < 1 ? 1 : s;
}
struct SdLayout {
    long long zero, act[2], slabs, total;       // in floats
};
SdLayout sd_layout(long long B, long long h, long long w, long long C, int n_convs, int ksplit) {
    SdLayout o;
    const long long M = B * h * w;
    long long at = 0, slab = 0;
    o.zero = at;   at += 64;
    o.act[0] = at; at += sd_up64(M * (C / 2));
    o.act[1] = at; at += n_convs > 1 ? sd_up64(M * (C / 4)) : 0;
    for (int i = 0; i < n_convs; ++i) {
        const int Cin = (int)(C >> i), N = Cin / 2, s = sd_ksplit(M, N, Cin, ksplit);
        if (s > 1 && s * M * N > slab) slab = s * M * N;
    }
    o.slabs = at;  at += sd_up64(slab);
    o.total = at;
    return o;
}
}  // namespace

extern "C" int64_t isc_senti_det_pack_bytes(int C, int n_convs) {
    if (!sd_shape_ok(1, 1, 1, C, n_convs)) return 0;
    long long halfs = 0;
    for (int i = 0; i < n_convs; ++i) halfs += (long long)((C >> i) / 2) * 18 * (C >> i);
    return halfs * 2;
}

extern "C" int isc_senti_det_pack(const float *const *conv_w_host, int C, int n_convs, void *packed, void *stream) {
    if (!conv_w_host || !packed) return ISC_E_NULL;
    if (!sd_shape_ok(1, 1, 1, C, n_convs)) return ISC_E_SHAPE;
    for (int i = 0; i < n_convs; ++i)
        if (!conv_w_host[i]) return ISC_E_NULL;
    if (!isc_aligned16(packed)) return ISC_E_ALIGN;
    _Float16 *dst = static_cast<_Float16 *>(packed);
    for (int i = 0; i < n_convs; ++i) {
        const int Cin = C >> i, N = Cin / 2;
        const long long n = (long long)N * 9 * Cin;
        hipLaunchKernelGGL(senti_det_pack_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, (hipStream_t)stream,
                           conv_w_host[i], N, Cin, dst);
        ISC_LAUNCH_CHECK();
        ++g_sdet_launches[ISC_SENTI_DET_KIND_PACK];
        dst += 2 * n;
    }
    return ISC_OK;
}

extern "C" int64_t isc_senti_det_workspace_bytes(int B, int h, int w, int C, int n_convs, int ksplit) {
    if (!sd_shape_ok(B, h, w, C, n_convs) || ksplit < 0) return 0;
    return sd_layout(B, h, w, C, n_convs, ksplit).total * (int64_t)sizeof(float);
}

extern "C" int isc_senti_det_fwd(const isc_senti_det_problem *q, void *stream) {
    if (!q) return ISC_E_NULL;
    if (!q->feats || !q->packed || !q->senti_w || !q->senti_b || !q->workspace || !q->logits || !q->maps || !q->labels ||
        !q->scores)
        return ISC_E_NULL;
    const int B = q->B, h = q->h, w = q->w, C = q->C, n_convs = q->n_convs, n_fcs = q->n_fcs, k = q->k;
    if (!sd_shape_ok(B, h, w, C, n_convs) || n_fcs < 0 || n_fcs > ISC_SENTI_DET_MAX_FCS || k < 1 || k > 8 ||
        q->ksplit < 0 || q->neu_idx < 0 || q->neu_idx >= k)
        return ISC_E_SHAPE;
    for (int i = 0; i < n_convs; ++i)
        if (!q->conv_b[i]) return ISC_E_NULL;
    for (int i = 0; i < n_fcs; ++i)
        if (!q->fc_w[i] || !q->fc_b[i]) return ISC_E_NULL;
    const SdLayout lay = sd_layout(B, h, w, C, n_convs, q->ksplit);
    if (q->workspace_bytes < lay.total * (int64_t)sizeof(float)) return ISC_E_WORKSPACE;
    if (!isc_aligned16(q->workspace) || !isc_aligned16(q->feats) || !isc_aligned16(q->packed) ||
        (q->conv_out && !isc_aligned16(q->conv_out)))
        return ISC_E_ALIGN;
    for (int i = 0; i < n_convs; ++i)
        if (!isc_aligned16(q->conv_b[i])) return ISC_E_ALIGN;
    hipStream_t st = (hipStream_t)stream;
    float *ws = static_cast<float *>(q->workspace);
    const int M = B * h * w;
    long long n_kind[ISC_SENTI_DET_KINDS] = {};

    if (hipMemsetAsync(ws + lay.zero, 0, 64 * sizeof(float), st) != hipSuccess) return (int)hipGetLastError();
    const void *A = q->feats;
    bool a_f16 = q->feats_f16 != 0;
    const _Float16 *Wp = static_cast<const _Float16 *>(q->packed);
    for (int i = 0; i < n_convs; ++i) {
        const int Cin = C >> i, N = Cin / 2;
        const bool last = i == n_convs - 1;
        float *dst = last && q->conv_out ? q->conv_out : ws + lay.act[i & 1];
        const int s = sd_ksplit(M, N, Cin, q->ksplit);
        SdConvArgs a = {};
        a.A = A; a.zero = ws + lay.zero; a.W = Wp; a.bias = q->conv_b[i];
        a.out = s > 1 ? ws + lay.slabs : dst;
        a.h = h; a.w = w; a.Cin = Cin; a.N = N; a.M = M; a.relu = last; a.ksplit = s;
        const dim3 grid((N + SD_BN - 1) / SD_BN, (M + SD_BM - 1) / SD_BM, s);
        if (a_f16) hipLaunchKernelGGL(senti_det_conv_kernel<true>, grid, dim3(256), 0, st, a);
        else hipLaunchKernelGGL(senti_det_conv_kernel<false>, grid, dim3(256), 0, st, a);
        ISC_LAUNCH_CHECK();
        ++n_kind[s > 1 ? ISC_SENTI_DET_KIND_SPLIT : ISC_SENTI_DET_KIND_DIRECT];
        if (a_f16) ++n_kind[ISC_SENTI_DET_KIND_F16];
        if (s > 1) {
            const long long MN = (long long)M * N;
            hipLaunchKernelGGL(senti_det_reduce_kernel, dim3((unsigned)((MN / 4 + 255) / 256)), dim3(256), 0, st,
                               ws + lay.slabs, s, MN, N, q->conv_b[i], (int)last, dst);
            ISC_LAUNCH_CHECK();
            ++n_kind[ISC_SENTI_DET_KIND_REDUCE];
        }
        A = dst;
        a_f16 = false;
        Wp += (long long)N * 18 * Cin;
    }
    SdTailArgs t = {};
    t.r = static_cast<const float *>(A); t.Ws = q->senti_w; t.bs = q->senti_b;
    for (int i = 0; i < n_fcs; ++i) { t.fc_w[i] = q->fc_w[i]; t.fc_b[i] = q->fc_b[i]; }
    t.hw = h * w; t.CL = C >> n_convs; t.k = k; t.n_fcs = n_fcs; t.neu_idx = q->neu_idx; t.threshold = q->threshold;
    t.logits = q->logits; t.maps = q->maps; t.scores = q->scores; t.labels = q->labels;
    hipLaunchKernelGGL(senti_det_tail_kernel, dim3(B), dim3(256), (size_t)(8 * h * w + 8) * sizeof(float), st, t);
    ISC_LAUNCH_CHECK();
    ++n_kind[ISC_SENTI_DET_KIND_TAIL];
    for (int i = 0; i < ISC_SENTI_DET_KINDS; ++i) g_sdet_launches[i] += n_kind[i];
    return ISC_OK;
}
