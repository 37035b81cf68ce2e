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
    float *sv_acts;             // TRAIN: pooled means and every FC output [n_fcs + 1][B][8]
    const int64_t *tr_labels;   // TRAIN: the image's category; dz [B][8] = (softmax - onehot) tr_scale / B and the
    float tr_scale;             //        image's cross-entropy term [B], both from the double-precision logits
    float *sv_dz, *sv_lrow;
};
// TRAIN: the training forward - the same arithmetic in the same order, the intermediates kept, no decision.
template <bool TRAIN>
__global__ __launch_bounds__(256) void senti_det_tail_kernel(const SdTailArgs a) {
    extern __shared__ float sd_m[];                 // [8][hw] maps, then 8 probabilities
    const int b = blockIdx.x, lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int hw = a.hw, CL = a.CL, k = a.k;
    float *prob = sd_m + 8 * hw;
    __shared__ double pool64[TRAIN ? 8 : 1];        // (TRAIN only)
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
    const long long B8 = (long long)gridDim.x * 8;
    if (threadIdx.x < k) {
        float s = 0.f;
        for (int p = 0; p < hw; ++p) s += sd_m[threadIdx.x * hw + p];
        prob[threadIdx.x] = s / (float)hw;
        if constexpr (TRAIN) {
            // What the backward reads - the pooled means, the FC outputs and the logits the loss and dz are formed from -
            // is a second evaluation of the same maps with the sums in double: the fp32 sum over p above runs
            // sequentially over up to 1024 like-signed values (about 3 ulp of the mean at h w = 196), and that error
            // times |pooled| would stand in every FC gradient.  The logits and maps handed out keep the frozen bits.
            double s64 = 0.0;
            for (int p = 0; p < hw; ++p) s64 += (double)sd_m[threadIdx.x * hw + p];
            pool64[threadIdx.x] = s64 / (double)hw;
            a.sv_acts[(long long)b * 8 + threadIdx.x] = (float)pool64[threadIdx.x];
        }
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
        if constexpr (TRAIN) {
            double z64[8], t64[8];
            for (int j = 0; j < k; ++j) z64[j] = pool64[j];
            for (int l = 0; l < a.n_fcs; ++l) {
                for (int i = 0; i < k; ++i) {
                    double s64 = 0.0;
                    for (int j = 0; j < k; ++j) s64 += z64[j] * (double)a.fc_w[l][i * k + j];
                    t64[i] = s64 + (double)a.fc_b[l][i];
                }
                for (int i = 0; i < k; ++i) {
                    z64[i] = t64[i];
                    a.sv_acts[(l + 1) * B8 + (long long)b * 8 + i] = (float)t64[i];
                }
            }
            // the image's loss term in the stable form, log sum_j exp(z_j - max) - (z_y - max), and dz: formed here, from
            // the logits before they are rounded to fp32 (at B = 1 half an ulp of a logit of 5 is the loss's whole bound)
            // (a label outside [0, k) - torch raises there - poisons the image's loss term and dz with NaN)
            long long y = a.tr_labels[b];
            const bool y_bad = y < 0 || y >= k;
            if (y_bad) y = 0;
            double mx64 = z64[0], sum64 = 0.0;
            for (int j = 1; j < k; ++j) mx64 = z64[j] > mx64 ? z64[j] : mx64;
            for (int j = 0; j < k; ++j) { t64[j] = exp(z64[j] - mx64); sum64 += t64[j]; }
            const double g64 = (double)a.tr_scale / (double)gridDim.x;
            for (int j = 0; j < k; ++j)
                a.sv_dz[(long long)b * 8 + j] = y_bad ? NAN : (float)((t64[j] / sum64 - (j == y ? 1.0 : 0.0)) * g64);
            a.sv_lrow[b] = y_bad ? NAN : (float)(log(sum64) - (z64[y] - mx64));
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
        if constexpr (!TRAIN) {
            a.scores[b] = best;
            a.labels[b] = arg;
        }
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
// One conv layer on its route (sd_ksplit): the direct kernel, or the split kernel and its reduce; n_kind counts per
// ISC_SENTI_DET_KIND_*.
int sd_launch_conv(const void *A, bool a_f16, const float *zero, const _Float16 *Wp, const float *bias, float *dst,
                   float *slabs, int h, int w, int Cin, int N, int M, int relu, int ksplit_want, hipStream_t st,
                   long long *n_kind) {
    const int s = sd_ksplit(M, N, Cin, ksplit_want);
    SdConvArgs a = {};
    a.A = A; a.zero = zero; a.W = Wp; a.bias = bias;
    a.out = s > 1 ? slabs : dst;
    a.h = h; a.w = w; a.Cin = Cin; a.N = N; a.M = M; a.relu = relu; a.ksplit = s;
    const dim3 grid((N + SD_BN - 1) / SD_BN, (M + SD_BM - 1) / SD_BM, s);
    if (a_f16) hipLaunchKernelGGL(senti_det_conv_kernel<true>, grid, dim3(256), 0, st, a);
    else hipLaunchKernelGGL(senti_det_conv_kernel<false>, grid, dim3(256), 0, st, a);
    ISC_LAUNCH_CHECK();
    ++n_kind[s > 1 ? ISC_SENTI_DET_KIND_SPLIT : ISC_SENTI_DET_KIND_DIRECT];
    if (a_f16) ++n_kind[ISC_SENTI_DET_KIND_F16];
    if (s > 1) {
        const long long MN = (long long)M * N;
        hipLaunchKernelGGL(senti_det_reduce_kernel, dim3((unsigned)((MN / 4 + 255) / 256)), dim3(256), 0, st, slabs, s, MN,
                           N, bias, relu, dst);
        ISC_LAUNCH_CHECK();
        ++n_kind[ISC_SENTI_DET_KIND_REDUCE];
    }
    return ISC_OK;
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
        const int rc = sd_launch_conv(A, a_f16, ws + lay.zero, Wp, q->conv_b[i], dst, ws + lay.slabs, h, w, Cin, N, M,
                                      (int)last, q->ksplit, st, n_kind);
        if (rc != ISC_OK) return rc;
        A = dst;
        a_f16 = false;
        Wp += (long long)N * 18 * Cin;
    }
    SdTailArgs t = {};
    t.r = static_cast<const float *>(A); t.Ws = q->senti_w; t.bs = q->senti_b;
    for (int i = 0; i < n_fcs; ++i) { t.fc_w[i] = q->fc_w[i]; t.fc_b[i] = q->fc_b[i]; }
    t.hw = h * w; t.CL = C >> n_convs; t.k = k; t.n_fcs = n_fcs; t.neu_idx = q->neu_idx; t.threshold = q->threshold;
    t.logits = q->logits; t.maps = q->maps; t.scores = q->scores; t.labels = q->labels;
    hipLaunchKernelGGL(senti_det_tail_kernel<false>, dim3(B), dim3(256), (size_t)(8 * h * w + 8) * sizeof(float), st, t);
    ISC_LAUNCH_CHECK();
    ++n_kind[ISC_SENTI_DET_KIND_TAIL];
    for (int i = 0; i < ISC_SENTI_DET_KINDS; ++i) g_sdet_launches[i] += n_kind[i];
    return ISC_OK;
}

// ====================================================================== training (isc_senti_det_train_fwd / _bwd)
static std::atomic<long long> g_sdet_train_launches[ISC_SENTI_DET_TRAIN_KINDS];
extern "C" long long isc_senti_det_bwd_launches(int kind) {
    return kind >= 0 && kind < ISC_SENTI_DET_TRAIN_KINDS ? g_sdet_train_launches[kind].load() : -1;
}

// r = relu(keep x2 mask_scale); keep null: r = relu(x2) - the bits the frozen forward's conv epilogue leaves
__global__ __launch_bounds__(256) void senti_det_drop_relu_kernel(const float *x2, const uint8_t *keep, float ms,
                                                                  long long n, float *r) {
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    float v = x2[i];
    if (keep) v = keep[i] ? v * ms : 0.f;
    r[i] = isc_relu(v);
}

// loss = scale mean_b lrow[b]: the per-image cross-entropy terms the training tail left (with dz), summed in double.  One
// workgroup: thread t takes the rows t, t + 256, ... ascending, the 256 partial sums fold in a fixed tree.
__global__ __launch_bounds__(256) void senti_det_loss_kernel(const float *lrow, int B, float scale, float *loss) {
    __shared__ double part[256];
    double s = 0.0;
    for (int b = threadIdx.x; b < B; b += 256) s += (double)lrow[b];
    part[threadIdx.x] = s;
    __syncthreads();
    for (int o = 128; o > 0; o >>= 1) {
        if ((int)threadIdx.x < o) part[threadIdx.x] += part[threadIdx.x + o];
        __syncthreads();
    }
    if (threadIdx.x == 0) loss[0] = (float)(part[0] / (double)B * (double)scale);
}

// 2^-floor(log2 mx) for a normal mx (mx e in [1, 2)); 2^126 for zero and denormals, 1 for what is not finite
__device__ __forceinline__ float sd_pow2_inv(float mx) {
    unsigned ex = (__float_as_uint(mx) >> 23) & 0xffu;
    if (ex >= 254u) return 1.f;
    if (ex < 1u) ex = 1u;
    return __uint_as_float((254u - ex) << 23);
}

// Per image: dz back through the FCs (thread 0: k <= 8), then thread c of the CL channels: rsum[b, c] = sum_p r[b, p, c]
// (p ascending), dr[b, c] = sum_j (dpool[b, j] / hw) Ws[j, c] (j ascending); eb[b] = the image's power-of-two scale.
struct SdTailBwdArgs {
    const float *dz, *r, *Ws;
    const float *fc_w[ISC_SENTI_DET_MAX_FCS];
    int B, hw, CL, k, n_fcs, _pad;
    float *g;                   // [n_fcs][B][8]: d loss / d (output of FC l)
    float *dpool;               // [B][8]
    float *rsum, *dr;           // [B, CL]
    float *eb;                  // [B]
};
__global__ __launch_bounds__(256) void senti_det_tail_bwd_kernel(const SdTailBwdArgs a) {
    __shared__ float dp[8];
    __shared__ float red[256];
    const int b = blockIdx.x, k = a.k, hw = a.hw, CL = a.CL;
    if (threadIdx.x == 0) {
        float g[8], t[8];
        for (int j = 0; j < k; ++j) g[j] = a.dz[(long long)b * 8 + j];
        for (int l = a.n_fcs - 1; l >= 0; --l) {
            for (int i = 0; i < k; ++i) a.g[((long long)l * a.B + b) * 8 + i] = g[i];
            for (int j = 0; j < k; ++j) {
                float s = 0.f;
                for (int i = 0; i < k; ++i) s += a.fc_w[l][i * k + j] * g[i];
                t[j] = s;
            }
            for (int j = 0; j < k; ++j) g[j] = t[j];
        }
        for (int j = 0; j < k; ++j) {
            a.dpool[(long long)b * 8 + j] = g[j];
            dp[j] = g[j] / (float)hw;
        }
    }
    __syncthreads();
    float mx = 0.f;
    for (int c = threadIdx.x; c < CL; c += 256) {
        const float *rp = a.r + (long long)b * hw * CL + c;
        float s = 0.f;
        for (int p = 0; p < hw; ++p) s += rp[(long long)p * CL];
        a.rsum[(long long)b * CL + c] = s;
        float d = 0.f;
        for (int j = 0; j < k; ++j) d += dp[j] * a.Ws[(long long)j * CL + c];
        a.dr[(long long)b * CL + c] = d;
        mx = fmaxf(mx, fabsf(d));
    }
    red[threadIdx.x] = mx;
    __syncthreads();
    for (int o = 128; o > 0; o >>= 1) {
        if ((int)threadIdx.x < o) red[threadIdx.x] = fmaxf(red[threadIdx.x], red[threadIdx.x + o]);
        __syncthreads();
    }
    if (threadIdx.x == 0) a.eb[b] = sd_pow2_inv(red[0]);
}

// The sums over the images, b ascending.  Workgroups 0 .. n-2: d senti_conv.weight, one thread per channel; the last
// workgroup: d senti_conv.bias, the FC gradients, and the scales (E = min_b eb: ratio = E / eb, inv_e = 1 / eb, 1 / E).
struct SdTailRedArgs {
    const float *dpool, *rsum, *g, *acts, *eb;
    int B, hw, CL, k, n_fcs, _pad;
    float *d_ws, *d_bs;
    float *d_fc_w[ISC_SENTI_DET_MAX_FCS], *d_fc_b[ISC_SENTI_DET_MAX_FCS];
    float *ratio, *inv_e, *unscale;
};
__global__ __launch_bounds__(256) void senti_det_tail_reduce_kernel(const SdTailRedArgs a) {
    __shared__ float red[256];
    const int B = a.B, k = a.k, CL = a.CL, t = threadIdx.x;
    if (blockIdx.x + 1 < gridDim.x) {
        const int c = blockIdx.x * 256 + t;
        if (c >= CL) return;
        for (int j = 0; j < k; ++j) {
            float s = 0.f;
            for (int b = 0; b < B; ++b) s += (a.dpool[(long long)b * 8 + j] / (float)a.hw) * a.rsum[(long long)b * CL + c];
            a.d_ws[(long long)j * CL + c] = s;
        }
        return;
    }
    if (t < k) {
        float s = 0.f;
        for (int b = 0; b < B; ++b) s += a.dpool[(long long)b * 8 + t];
        a.d_bs[t] = s;
    }
    for (int e = t; e < a.n_fcs * k * k; e += 256) {
        const int l = e / (k * k), i = (e - l * k * k) / k, j = e % k;
        const float *g = a.g + (long long)l * B * 8, *x = a.acts + (long long)l * B * 8;
        float s = 0.f;
        for (int b = 0; b < B; ++b) s += g[(long long)b * 8 + i] * x[(long long)b * 8 + j];
        a.d_fc_w[l][i * k + j] = s;
    }
    for (int e = t; e < a.n_fcs * k; e += 256) {
        const int l = e / k, i = e - l * k;
        const float *g = a.g + (long long)l * B * 8;
        float s = 0.f;
        for (int b = 0; b < B; ++b) s += g[(long long)b * 8 + i];
        a.d_fc_b[l][i] = s;
    }
    float mn = 3.0e38f;
    for (int b = t; b < B; b += 256) mn = fminf(mn, a.eb[b]);
    red[t] = mn;
    __syncthreads();
    for (int o = 128; o > 0; o >>= 1) {
        if (t < o) red[t] = fminf(red[t], red[t + o]);
        __syncthreads();
    }
    const float E = red[0];
    for (int b = t; b < B; b += 256) {
        a.ratio[b] = E / a.eb[b];
        a.inv_e[b] = 1.f / a.eb[b];
    }
    if (t == 0) a.unscale[0] = 1.f / E;
}

// dx2[m, c] = dr[b, c] eb[b] [x2 keep > 0] keep mask_scale into rows of ld >= CL floats (the padding: zeros)
__global__ __launch_bounds__(256) void senti_det_dx2_kernel(const float *x2, const uint8_t *keep, const float *dr,
                                                            const float *eb, float ms, long long M, int hw, int CL, int ld,
                                                            float *dx2) {
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    if (i >= M * ld) return;
    const long long m = i / ld;
    const int c = (int)(i - m * ld);
    float v = 0.f;
    if (c < CL) {
        const long long b = m / hw;
        const bool kp = keep ? keep[m * CL + c] != 0 : true;
        if (kp && x2[m * CL + c] > 0.f) {
            v = dr[b * CL + c] * eb[b];
            if (keep) v *= ms;
        }
    }
    dx2[i] = v;
}

// out[n] = unscale sum_m dy[m, n] ratio[b(m)]: 64 columns x 16 row groups per workgroup, a group sums its contiguous share
// of the rows ascending, the 16 partial sums fold ascending.
__global__ __launch_bounds__(1024) void senti_det_colsum_kernel(const float *dy, int ld, int M, int N, int hw,
                                                                const float *ratio, const float *unscale, float *out) {
    __shared__ float part[16][64];
    const int cl = threadIdx.x & 63, g = threadIdx.x >> 6, col = blockIdx.x * 64 + cl;
    const int Q = (M + 15) / 16, m0 = g * Q, m1 = m0 + Q < M ? m0 + Q : M;
    float s = 0.f;
    if (col < N)
        for (int m = m0; m < m1; ++m) s += dy[(long long)m * ld + col] * ratio[m / hw];
    part[g][cl] = s;
    __syncthreads();
    if (g == 0 && col < N) {
        float tot = 0.f;
        for (int q = 0; q < 16; ++q) tot += part[q][cl];
        out[col] = tot * unscale[0];
    }
}

// out[m, n] = dx[m, n] inv_e[b(m)] (tests: the unscaled gradient of conv_0's output)
__global__ __launch_bounds__(256) void senti_det_unscale_kernel(const float *dx, long long MN, int N, int hw,
                                                                const float *inv_e, float *out) {
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    if (i >= MN) return;
    out[i] = dx[i] * inv_e[(i / N) / hw];
}

// Planes of W'[ci, (2-ky, 2-kx), co] = w[co, ci, ky, kx]: the matrix [Cin, 9 Cp] (Cp = Cout rounded up to 32, zeros in the
// padding) the convolution kernel contracts dY's rows with - with padding 1 the transposed convolution is the same
// convolution on the flipped, transposed weights.
__global__ __launch_bounds__(256) void senti_det_pack_flipped_kernel(const float *w, int Cout, int Cin, int Cp,
                                                                     _Float16 *planes) {
    const int K9 = 9 * Cp;
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    if (i >= (long long)Cin * K9) return;
    const int n = (int)(i / K9), kk = (int)(i - (long long)n * K9);
    const int tap = kk / Cp, co = kk - tap * Cp;
    _Float16 hi, lo;
    isc_split_f16(co < Cout ? w[((long long)co * Cin + n) * 9 + (8 - tap)] : 0.f, hi, lo);
    const long long o = plane_index(n, kk, K9);
    planes[o] = hi;
    planes[o + 32] = lo;
}

// ------------------------------------------------------------------ weight gradient: the implicit TN contraction
// dw[co, ci, ky, kx] = unscale sum_m dy[m, co] ratio[b(m)] x[pixel(m) + (ky - 1, kx - 1), ci]  over the M = B h w rows.
// Output matrix [Cout, 9 Cin], column = tap Cin + ci; tile 64 (co) x 128 (columns), four waves as 2 x 2, the MFMA
// arrangement of the forward kernel with the roles  A = dy^T, B = x^T  and the contraction running over m, 32 rows a chunk.
// Both operands lie [m][channel] in memory and the MFMA wants eight consecutive m per lane, so they are staged through
// LDS transposed: thread t takes the row pair (t >> 4) of the chunk and, of each row, four channels of dy (quad t & 15)
// and four channels of each half of the x tile; it splits the values (once per value) and writes one 32-bit word - the
// two rows' halfs - per channel and plane to [channel][m], rows 80 bytes apart.  x is read where it lies, at the pixel
// the column's tap points to; a tap outside the image's own grid, a row at or beyond M and a column beyond the matrix
// contribute exact zeros.  Two register sets and two LDS buffers: chunks c + 1 and c + 2 are in flight while chunk c
// multiplies, one barrier per chunk (as in the forward kernel).  No atomics; one workgroup owns a tile and walks m
// ascending: two calls give the same bits.
struct SdDwArgs {
    const float *dy, *x, *ratio, *unscale;
    float *dw;
    int ldy, h, w, Cin, Cout, M, tapfast, _pad;
};
#define DW_BM 64
#define DW_BN 128
#define DW_LD 40
#define DW_BUF ((2 * DW_BM + 2 * DW_BN) * DW_LD)        // halfs per buffer: A hi | A lo | B hi | B lo
typedef _Float16 sd_h2 __attribute__((ext_vector_type(2)));
struct SdDwStage {
    float4 y[2], xa[2], xb[2];  // rows m, m + 1: the dy quad, the quad of the tile's first and of its second 64 columns
};

__device__ __forceinline__ void sd_dw_put(_Float16 *hi, _Float16 *lo, const float4 &r0, const float4 &r1) {
    const float v0[4] = {r0.x, r0.y, r0.z, r0.w}, v1[4] = {r1.x, r1.y, r1.z, r1.w};
#pragma unroll
    for (int e = 0; e < 4; ++e) {
        _Float16 h0, l0, h1, l1;
        isc_split_f16(v0[e], h0, l0);
        isc_split_f16(v1[e], h1, l1);
        sd_h2 ph, pl;
        ph[0] = h0; ph[1] = h1;
        pl[0] = l0; pl[1] = l1;
        *reinterpret_cast<sd_h2 *>(hi + e * DW_LD) = ph;
        *reinterpret_cast<sd_h2 *>(lo + e * DW_LD) = pl;
    }
}

__global__ __launch_bounds__(256) void senti_det_dw_kernel(const SdDwArgs a) {
    __shared__ __attribute__((aligned(16))) _Float16 lds[2 * DW_BUF];
    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6, wm = wv >> 1, wn = wv & 1;
    const int h = a.h, w = a.w, Cin = a.Cin, Cout = a.Cout, M = a.M, hw = h * w, K9 = 9 * Cin;
    // (tapfast, Cin % 128 == 0: the nine taps of one channel block are neighbours in launch order - they write the same lines)
    const int col0 = a.tapfast ? (int)(blockIdx.x % 9) * Cin + (int)(blockIdx.x / 9) * DW_BN : (int)blockIdx.x * DW_BN;
    const int co0 = blockIdx.y * DW_BM;
    const int rp = tid >> 4, q = tid & 15;
    const int yco = co0 + q * 4;
    const bool y_ok = yco < Cout;                               // (Cout % 16 == 0: a quad is inside or outside)
    // the two x quads of this thread: columns col0 + q 4 and col0 + 64 + q 4 (each inside one tap: Cin % 32 == 0)
    const int colA = col0 + q * 4, colB = colA + 64;
    const bool okA = colA < K9, okB = colB < K9;
    const int tapA = okA ? colA / Cin : 0, tapB = okB ? colB / Cin : 0;
    const int ciA = okA ? colA - tapA * Cin : 0, ciB = okB ? colB - tapB * Cin : 0;
    const int dyA = tapA / 3 - 1, dxA = tapA % 3 - 1, dyB = tapB / 3 - 1, dxB = tapB % 3 - 1;
    const int nchunks = (M + 31) / 32;
    const float4 z4 = make_float4(0.f, 0.f, 0.f, 0.f);

    SdDwStage st0, st1;
    auto load = [&](int c, SdDwStage &s) __attribute__((always_inline)) {
        int m = c * 32 + rp * 2;
        int b = m / hw, rem = m - b * hw, y = rem / w, x = rem - y * w;
#pragma unroll
        for (int r = 0; r < 2; ++r) {
            const bool ok = m < M;
            float4 yv = z4;
            if (ok && y_ok) {
                yv = *reinterpret_cast<const float4 *>(a.dy + (long long)m * a.ldy + yco);
                if (a.ratio) {
                    const float rt = a.ratio[b];
                    yv.x *= rt; yv.y *= rt; yv.z *= rt; yv.w *= rt;
                }
            }
            s.y[r] = yv;
            {
                const int yy = y + dyA, xx = x + dxA;
                const bool in = ok && okA && yy >= 0 && yy < h && xx >= 0 && xx < w;
                s.xa[r] = in ? *reinterpret_cast<const float4 *>(a.x + (((long long)b * h + yy) * w + xx) * Cin + ciA) : z4;
            }
            {
                const int yy = y + dyB, xx = x + dxB;
                const bool in = ok && okB && yy >= 0 && yy < h && xx >= 0 && xx < w;
                s.xb[r] = in ? *reinterpret_cast<const float4 *>(a.x + (((long long)b * h + yy) * w + xx) * Cin + ciB) : z4;
            }
            ++m;
            if (++x == w) { x = 0; if (++y == h) { y = 0; ++b; } }
        }
    };
    auto store = [&](const SdDwStage &s, int S) __attribute__((always_inline)) {
        _Float16 *bf = lds + S * DW_BUF;
        const int o = q * 4 * DW_LD + rp * 2;
        sd_dw_put(bf + o, bf + DW_BM * DW_LD + o, s.y[0], s.y[1]);
        _Float16 *xb = bf + 2 * DW_BM * DW_LD;
        sd_dw_put(xb + o, xb + DW_BN * DW_LD + o, s.xa[0], s.xa[1]);
        sd_dw_put(xb + 64 * DW_LD + o, xb + DW_BN * DW_LD + 64 * DW_LD + o, s.xb[0], s.xb[1]);
    };

    sd_f4 acc0[2][4], acc1[2][4];
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int j = 0; j < 4; ++j)
#pragma unroll
            for (int r = 0; r < 4; ++r) { acc0[i][j][r] = 0.f; acc1[i][j][r] = 0.f; }

    const int fr = lane & 15, fq = lane >> 4;
    auto step = [&](int c, SdDwStage &s, int S) __attribute__((always_inline)) {
        store(s, S);
        __syncthreads();
        if (c + 2 < nchunks) load(c + 2, s);
        const _Float16 *bf = lds + S * DW_BUF;
        sd_h8 ah[2], al[2];
#pragma unroll
        for (int i = 0; i < 2; ++i) {
            const int o = (wm * 32 + i * 16 + fr) * DW_LD + fq * 8;
            ah[i] = *reinterpret_cast<const sd_h8 *>(bf + o);
            al[i] = *reinterpret_cast<const sd_h8 *>(bf + DW_BM * DW_LD + o);
        }
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const int o = 2 * DW_BM * DW_LD + (wn * 64 + j * 16 + fr) * DW_LD + fq * 8;
            const sd_h8 bh = *reinterpret_cast<const sd_h8 *>(bf + o);
            const sd_h8 bl = *reinterpret_cast<const sd_h8 *>(bf + DW_BN * DW_LD + o);
#pragma unroll
            for (int i = 0; i < 2; ++i) {
                acc0[i][j] = __builtin_amdgcn_mfma_f32_16x16x32_f16(ah[i], bh, acc0[i][j], 0, 0, 0);
                acc1[i][j] = __builtin_amdgcn_mfma_f32_16x16x32_f16(ah[i], bl, acc1[i][j], 0, 0, 0);
                acc1[i][j] = __builtin_amdgcn_mfma_f32_16x16x32_f16(al[i], bh, acc1[i][j], 0, 0, 0);
            }
        }
    };
    load(0, st0);
    if (1 < nchunks) load(1, st1);
    for (int c = 0; c < nchunks; c += 2) {
        step(c, st0, 0);
        if (c + 1 < nchunks) step(c + 1, st1, 1);
    }

    // C/D layout: register r of block (i, j) = tile row wm 32 + i 16 + 4 (lane >> 4) + r, column wn 64 + j 16 + (lane & 15)
    const float us = a.unscale ? a.unscale[0] : 1.f;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        const int gcol = col0 + wn * 64 + j * 16 + fr;
        if (gcol >= K9) continue;
        const int tap = gcol / Cin, ci = gcol - tap * Cin;
#pragma unroll
        for (int i = 0; i < 2; ++i)
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int gco = co0 + wm * 32 + i * 16 + 4 * fq + r;
                if (gco >= Cout) continue;
                a.dw[((long long)gco * Cin + ci) * 9 + tap] = fmaf(acc1[i][j][r], ISC_SPLIT_LO_WEIGHT, acc0[i][j][r]) * us;
            }
    }
}

namespace {
long long sd_up32(long long n) { return (n + 31) / 32 * 32; }
int sd_launch_dw(const float *dy, int ldy, const float *x, int h, int w, int Cin, int Cout, int M, const float *ratio,
                 const float *unscale, float *dw, hipStream_t st) {
    SdDwArgs a = {};
    a.dy = dy; a.x = x; a.ratio = ratio; a.unscale = unscale; a.dw = dw;
    a.ldy = ldy; a.h = h; a.w = w; a.Cin = Cin; a.Cout = Cout; a.M = M; a.tapfast = Cin % DW_BN == 0;
    hipLaunchKernelGGL(senti_det_dw_kernel, dim3((9 * Cin + DW_BN - 1) / DW_BN, (Cout + DW_BM - 1) / DW_BM), dim3(256), 0,
                       st, a);
    ISC_LAUNCH_CHECK();
    return ISC_OK;
}
int sd_launch_pack_flipped(const float *w, int Cout, int Cin, _Float16 *planes, hipStream_t st) {
    const int Cp = (int)sd_up32(Cout);
    const long long n = (long long)Cin * 9 * Cp;
    hipLaunchKernelGGL(senti_det_pack_flipped_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, w, Cout, Cin,
                       Cp, planes);
    ISC_LAUNCH_CHECK();
    return ISC_OK;
}

// saved (floats): zero line | packed conv weights | slabs | x_i = conv_i's output (the last one: x2, with its bias, before
// dropout and ReLU) | r | pooled means and FC outputs [n_fcs + 1][B][8] | dz [B][8] | loss terms [B]
struct SdTrainLayout {
    long long zero, packed, slabs, x[ISC_SENTI_DET_MAX_CONVS], r, acts, dz, lrow, total;
};
SdTrainLayout sd_train_layout(long long B, long long h, long long w, long long C, int n_convs, int n_fcs) {
    SdTrainLayout o = {};
    const long long M = B * h * w;
    long long at = 0, slab = 0;
    o.zero = at;   at += 64;
    o.packed = at; at += sd_up64(isc_senti_det_pack_bytes((int)C, n_convs) / 4);
    for (int i = 0; i < n_convs; ++i) {
        const int Cin = (int)(C >> i), N = Cin / 2, s = sd_ksplit(M, N, Cin, 0);
        if (s > 1 && s * M * N > slab) slab = s * M * N;
    }
    o.slabs = at;  at += sd_up64(slab);
    for (int i = 0; i < n_convs; ++i) { o.x[i] = at; at += sd_up64(M * (C >> (i + 1))); }
    o.r = at;      at += sd_up64(M * (C >> n_convs));
    o.acts = at;   at += sd_up64((n_fcs + 1) * B * 8);
    o.dz = at;     at += sd_up64(B * 8);
    o.lrow = at;   at += sd_up64(B);
    o.total = at;
    return o;
}
// workspace of the backward (floats): zero line and a zero bias [C] (one memset) | g | dpool | rsum | dr | eb | ratio |
// inv_e | 1 / E | two gradient buffers [M, up32(C / 2)] | flipped planes | slabs of the dX convolutions
struct SdBwdLayout {
    long long zero, zbias, g, dpool, rsum, dr, eb, ratio, inv_e, unscale, dx[2], planes, slabs, total;
};
SdBwdLayout sd_bwd_layout(long long B, long long h, long long w, long long C, int n_convs) {
    SdBwdLayout o = {};
    const long long M = B * h * w, CL = C >> n_convs;
    long long at = 0, slab = 0, planes = 0;
    o.zero = at;    at += 64;
    o.zbias = at;   at += sd_up64(C);
    o.g = at;       at += sd_up64(ISC_SENTI_DET_MAX_FCS * B * 8);
    o.dpool = at;   at += sd_up64(B * 8);
    o.rsum = at;    at += sd_up64(B * CL);
    o.dr = at;      at += sd_up64(B * CL);
    o.eb = at;      at += sd_up64(B);
    o.ratio = at;   at += sd_up64(B);
    o.inv_e = at;   at += sd_up64(B);
    o.unscale = at; at += 64;
    o.dx[0] = at;   at += sd_up64(M * sd_up32(C / 2));
    o.dx[1] = at;   at += n_convs > 1 ? sd_up64(M * sd_up32(C / 2)) : 0;
    for (int i = 1; i < n_convs; ++i) {
        const long long Cin = C >> i, Cp = sd_up32(Cin / 2);
        const int s = sd_ksplit(M, (int)Cin, (int)Cp, 0);
        if (s > 1 && s * M * Cin > slab) slab = s * M * Cin;
        if (Cin * 9 * Cp > planes) planes = Cin * 9 * Cp;
    }
    o.planes = at;  at += sd_up64(planes);
    o.slabs = at;   at += sd_up64(slab);
    o.total = at;
    return o;
}
// the checks both calls share; *bwd: the gradients and the workspace as well
int sd_train_check(const isc_senti_det_train_problem *q, bool bwd) {
    if (!q) return ISC_E_NULL;
    if (!q->feats || !q->senti_w || !q->senti_b || !q->labels || !q->saved || !q->logits || !q->maps || !q->loss)
        return ISC_E_NULL;
    const int n_convs = q->n_convs, n_fcs = q->n_fcs, k = q->k;
    if (!sd_shape_ok(q->B, q->h, q->w, q->C, n_convs) || n_fcs < 0 || n_fcs > ISC_SENTI_DET_MAX_FCS || k < 1 || k > 8)
        return ISC_E_SHAPE;
    for (int i = 0; i < n_convs; ++i)
        if (!q->conv_w[i] || !q->conv_b[i] || (bwd && (!q->d_conv_w[i] || !q->d_conv_b[i]))) return ISC_E_NULL;
    for (int i = 0; i < n_fcs; ++i)
        if (!q->fc_w[i] || !q->fc_b[i] || (bwd && (!q->d_fc_w[i] || !q->d_fc_b[i]))) return ISC_E_NULL;
    if (bwd && (!q->workspace || !q->d_senti_w || !q->d_senti_b)) return ISC_E_NULL;
    if (bwd && q->dx_out && n_convs < 2) return ISC_E_SHAPE;
    if (q->saved_bytes < sd_train_layout(q->B, q->h, q->w, q->C, n_convs, n_fcs).total * (int64_t)sizeof(float))
        return ISC_E_WORKSPACE;
    if (bwd && q->workspace_bytes < sd_bwd_layout(q->B, q->h, q->w, q->C, n_convs).total * (int64_t)sizeof(float))
        return ISC_E_WORKSPACE;
    if (!isc_aligned16(q->feats) || !isc_aligned16(q->saved) || (bwd && !isc_aligned16(q->workspace)) ||
        (bwd && q->dx_out && !isc_aligned16(q->dx_out)))
        return ISC_E_ALIGN;
    for (int i = 0; i < n_convs; ++i)
        if (!isc_aligned16(q->conv_b[i])) return ISC_E_ALIGN;
    return ISC_OK;
}
}  // namespace

extern "C" int64_t isc_senti_det_train_saved_bytes(int B, int h, int w, int C, int n_convs, int n_fcs) {
    if (!sd_shape_ok(B, h, w, C, n_convs) || n_fcs < 0 || n_fcs > ISC_SENTI_DET_MAX_FCS) return 0;
    return sd_train_layout(B, h, w, C, n_convs, n_fcs).total * (int64_t)sizeof(float);
}
extern "C" int64_t isc_senti_det_bwd_workspace_bytes(int B, int h, int w, int C, int n_convs) {
    if (!sd_shape_ok(B, h, w, C, n_convs)) return 0;
    return sd_bwd_layout(B, h, w, C, n_convs).total * (int64_t)sizeof(float);
}

extern "C" int isc_senti_det_bwd_tail_offsets(int B, int h, int w, int C, int n_convs, int64_t *out6) {
    if (!out6) return ISC_E_NULL;
    if (!sd_shape_ok(B, h, w, C, n_convs)) return ISC_E_SHAPE;
    const SdBwdLayout lay = sd_bwd_layout(B, h, w, C, n_convs);
    const long long o[6] = {lay.g, lay.dpool, lay.rsum, lay.dr, lay.eb, lay.ratio};
    for (int i = 0; i < 6; ++i) out6[i] = o[i];
    return ISC_OK;
}

extern "C" int isc_senti_det_dw(const float *dy, int ldy, const float *x, int B, int h, int w, int Cin, int Cout,
                                const float *ratio, const float *unscale, float *dw, void *stream) {
    if (!dy || !x || !dw) return ISC_E_NULL;
    if (B < 1 || h < 1 || w < 1 || (long long)B * h * w > (1LL << 22) || Cin < 32 || Cin % 32 || Cin > 65536 || Cout < 16 ||
        Cout % 16 || Cout > 65536 || ldy < Cout || ldy % 4)
        return ISC_E_SHAPE;
    if (!isc_aligned16(dy) || !isc_aligned16(x)) return ISC_E_ALIGN;
    return sd_launch_dw(dy, ldy, x, h, w, Cin, Cout, B * h * w, ratio, unscale, dw, (hipStream_t)stream);
}
extern "C" int isc_senti_det_pack_flipped(const float *w, int Cout, int Cin, void *planes, void *stream) {
    if (!w || !planes) return ISC_E_NULL;
    if (Cin < 32 || Cin % 32 || Cin > 65536 || Cout < 16 || Cout % 16 || Cout > 65536) return ISC_E_SHAPE;
    if (!isc_aligned16(planes)) return ISC_E_ALIGN;
    return sd_launch_pack_flipped(w, Cout, Cin, static_cast<_Float16 *>(planes), (hipStream_t)stream);
}

extern "C" int isc_senti_det_train_fwd(const isc_senti_det_train_problem *q, void *stream) {
    const int rc0 = sd_train_check(q, false);
    if (rc0 != ISC_OK) return rc0;
    const int B = q->B, h = q->h, w = q->w, C = q->C, n_convs = q->n_convs, n_fcs = q->n_fcs, k = q->k;
    const SdTrainLayout lay = sd_train_layout(B, h, w, C, n_convs, n_fcs);
    hipStream_t st = (hipStream_t)stream;
    float *sv = static_cast<float *>(q->saved);
    const int M = B * h * w, CL = C >> n_convs;
    long long n_kind[ISC_SENTI_DET_KINDS] = {}, n = 0;

    if (hipMemsetAsync(sv + lay.zero, 0, 64 * sizeof(float), st) != hipSuccess) return (int)hipGetLastError();
    _Float16 *planes = reinterpret_cast<_Float16 *>(sv + lay.packed);
    {
        _Float16 *dst = planes;
        for (int i = 0; i < n_convs; ++i) {
            const int Cin = C >> i, N = Cin / 2;
            const long long np = (long long)N * 9 * Cin;
            hipLaunchKernelGGL(senti_det_pack_kernel, dim3((unsigned)((np + 255) / 256)), dim3(256), 0, st, q->conv_w[i],
                               N, Cin, dst);
            ISC_LAUNCH_CHECK();
            ++n;
            dst += 2 * np;
        }
    }
    const void *A = q->feats;
    const _Float16 *Wp = planes;
    for (int i = 0; i < n_convs; ++i) {
        const int Cin = C >> i, N = Cin / 2;
        const int rc = sd_launch_conv(A, false, sv + lay.zero, Wp, q->conv_b[i], sv + lay.x[i], sv + lay.slabs, h, w, Cin,
                                      N, M, 0, 0, st, n_kind);
        if (rc != ISC_OK) return rc;
        A = sv + lay.x[i];
        Wp += (long long)N * 18 * Cin;
    }
    const long long reduces = n_kind[ISC_SENTI_DET_KIND_REDUCE];
    n += n_kind[ISC_SENTI_DET_KIND_DIRECT] + n_kind[ISC_SENTI_DET_KIND_SPLIT] + reduces;
    const long long MC = (long long)M * CL;
    hipLaunchKernelGGL(senti_det_drop_relu_kernel, dim3((unsigned)((MC + 255) / 256)), dim3(256), 0, st,
                       sv + lay.x[n_convs - 1], q->keep, q->mask_scale, MC, sv + lay.r);
    ISC_LAUNCH_CHECK();
    SdTailArgs t = {};
    t.r = sv + lay.r; t.Ws = q->senti_w; t.bs = q->senti_b;
    for (int i = 0; i < n_fcs; ++i) { t.fc_w[i] = q->fc_w[i]; t.fc_b[i] = q->fc_b[i]; }
    t.hw = h * w; t.CL = CL; t.k = k; t.n_fcs = n_fcs; t.neu_idx = 0; t.threshold = 0.f;
    t.logits = q->logits; t.maps = q->maps; t.sv_acts = sv + lay.acts;
    t.tr_labels = q->labels; t.tr_scale = q->scale; t.sv_dz = sv + lay.dz; t.sv_lrow = sv + lay.lrow;
    hipLaunchKernelGGL(senti_det_tail_kernel<true>, dim3(B), dim3(256), (size_t)(8 * h * w + 8) * sizeof(float), st, t);
    ISC_LAUNCH_CHECK();
    hipLaunchKernelGGL(senti_det_loss_kernel, dim3(1), dim3(256), 0, st, sv + lay.lrow, B, q->scale, q->loss);
    ISC_LAUNCH_CHECK();
    n += 3;
    g_sdet_train_launches[ISC_SENTI_DET_TRAIN_KIND_FWD] += n;
    g_sdet_train_launches[ISC_SENTI_DET_TRAIN_KIND_REDUCE] += reduces;
    return ISC_OK;
}

extern "C" int isc_senti_det_bwd(const isc_senti_det_train_problem *q, void *stream) {
    const int rc0 = sd_train_check(q, true);
    if (rc0 != ISC_OK) return rc0;
    const int B = q->B, h = q->h, w = q->w, C = q->C, n_convs = q->n_convs, n_fcs = q->n_fcs, k = q->k;
    const SdTrainLayout sl = sd_train_layout(B, h, w, C, n_convs, n_fcs);
    const SdBwdLayout lay = sd_bwd_layout(B, h, w, C, n_convs);
    hipStream_t st = (hipStream_t)stream;
    float *sv = static_cast<float *>(q->saved), *ws = static_cast<float *>(q->workspace);
    const int M = B * h * w, CL = C >> n_convs, hw = h * w;
    long long n_kind[ISC_SENTI_DET_KINDS] = {}, n = 0;

    if (hipMemsetAsync(ws + lay.zero, 0, (size_t)(lay.g - lay.zero) * sizeof(float), st) != hipSuccess)
        return (int)hipGetLastError();
    SdTailBwdArgs tb = {};
    tb.dz = sv + sl.dz; tb.r = sv + sl.r; tb.Ws = q->senti_w;
    for (int i = 0; i < n_fcs; ++i) tb.fc_w[i] = q->fc_w[i];
    tb.B = B; tb.hw = hw; tb.CL = CL; tb.k = k; tb.n_fcs = n_fcs;
    tb.g = ws + lay.g; tb.dpool = ws + lay.dpool; tb.rsum = ws + lay.rsum; tb.dr = ws + lay.dr; tb.eb = ws + lay.eb;
    hipLaunchKernelGGL(senti_det_tail_bwd_kernel, dim3(B), dim3(256), 0, st, tb);
    ISC_LAUNCH_CHECK();
    SdTailRedArgs tr = {};
    tr.dpool = ws + lay.dpool; tr.rsum = ws + lay.rsum; tr.g = ws + lay.g; tr.acts = sv + sl.acts; tr.eb = ws + lay.eb;
    tr.B = B; tr.hw = hw; tr.CL = CL; tr.k = k; tr.n_fcs = n_fcs;
    tr.d_ws = q->d_senti_w; tr.d_bs = q->d_senti_b;
    for (int i = 0; i < n_fcs; ++i) { tr.d_fc_w[i] = q->d_fc_w[i]; tr.d_fc_b[i] = q->d_fc_b[i]; }
    tr.ratio = ws + lay.ratio; tr.inv_e = ws + lay.inv_e; tr.unscale = ws + lay.unscale;
    hipLaunchKernelGGL(senti_det_tail_reduce_kernel, dim3((CL + 255) / 256 + 1), dim3(256), 0, st, tr);
    ISC_LAUNCH_CHECK();
    int ld = (int)sd_up32(CL);
    float *dy = ws + lay.dx[0];
    const long long Ml = (long long)M * ld;
    hipLaunchKernelGGL(senti_det_dx2_kernel, dim3((unsigned)((Ml + 255) / 256)), dim3(256), 0, st, sv + sl.x[n_convs - 1],
                       q->keep, ws + lay.dr, ws + lay.eb, q->mask_scale, (long long)M, hw, CL, ld, dy);
    ISC_LAUNCH_CHECK();
    n += 3;
    for (int i = n_convs - 1; i >= 0; --i) {
        const int Cin = C >> i, N = Cin / 2;
        const float *X = i > 0 ? sv + sl.x[i - 1] : q->feats;
        hipLaunchKernelGGL(senti_det_colsum_kernel, dim3((N + 63) / 64), dim3(1024), 0, st, dy, ld, M, N, hw,
                           ws + lay.ratio, ws + lay.unscale, q->d_conv_b[i]);
        ISC_LAUNCH_CHECK();
        int rc = sd_launch_dw(dy, ld, X, h, w, Cin, N, M, ws + lay.ratio, ws + lay.unscale, q->d_conv_w[i], st);
        if (rc != ISC_OK) return rc;
        n += 2;
        if (i > 0) {
            // dX = conv3x3(dY [M, ld], W'): Cin rows of 9 ld columns, the padding channels of dY and of W' both zero
            _Float16 *planes = reinterpret_cast<_Float16 *>(ws + lay.planes);
            rc = sd_launch_pack_flipped(q->conv_w[i], N, Cin, planes, st);
            if (rc != ISC_OK) return rc;
            float *dx = ws + lay.dx[dy == ws + lay.dx[0] ? 1 : 0];
            rc = sd_launch_conv(dy, false, ws + lay.zero, planes, ws + lay.zbias, dx, ws + lay.slabs, h, w, ld, Cin, M, 0, 0,
                                st, n_kind);
            if (rc != ISC_OK) return rc;
            n += 2;
            dy = dx;
            ld = Cin;
        }
    }
    if (q->dx_out) {
        const long long MN = (long long)M * (C / 2);
        hipLaunchKernelGGL(senti_det_unscale_kernel, dim3((unsigned)((MN + 255) / 256)), dim3(256), 0, st, dy, MN, C / 2,
                           hw, ws + lay.inv_e, q->dx_out);
        ISC_LAUNCH_CHECK();
        ++n;
    }
    n += n_kind[ISC_SENTI_DET_KIND_REDUCE];
    g_sdet_train_launches[ISC_SENTI_DET_TRAIN_KIND_BWD] += n;
    g_sdet_train_launches[ISC_SENTI_DET_TRAIN_KIND_REDUCE] += n_kind[ISC_SENTI_DET_KIND_REDUCE];
    return ISC_OK;
}
