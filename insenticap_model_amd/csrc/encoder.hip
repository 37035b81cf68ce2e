// The image encoder (the reference's models/encoder.py in eval mode): a bottleneck ResNet from pixels to the pooled
// feature vector fc [C] and the region grid att [a, a, C], forward only, every batch norm folded into the convolution in
// front of it.  Activations are channels-last fp32 [B, h, w, C], viewed as rows [B h w, C].
//   stem:  7x7 / 2, pad 3, 3 -> C0, + bias, ReLU on fp32 FMAs (K = 147 is no multiple of the engine's 32-deep chunk and
//          the layer holds under 2 % of the network's FLOPs); uint8 pixels are normalised as the taps load
//   pool:  3x3 / 2, pad 0, ceil mode (overhanging windows are clipped)
//   convs: 1x1 (stride 1 or 2) and 3x3 (stride 1, pad 1) as implicit GEMMs on the split-f16 engine - the tile design of
//          senti_det.hip's senti_det_conv_kernel (64 x 128 tile, two register sets, two LDS buffers, the zero line for
//          out-of-grid taps, K-split with a fixed-order slab reduce), generalised by the tap geometry and a residual
//          epilogue.  The tile body is duplicated on purpose: senti_det.hip's kernels are pinned to exact bits by their
//          own tests and stay as they are (DESIGN.md lists the shared tile header as a follow-up).
//   tail:  fc = mean over w, then over h; att = adaptive average pool to a x a; optional float16 copies
// No atomics anywhere: two runs give the same bits.
#include <atomic>

#include "common.h"

static std::atomic<long long> g_enc_launches[ISC_ENCODER_KINDS];
extern "C" long long isc_encoder_launches(int kind) {
    return kind >= 0 && kind < ISC_ENCODER_KINDS ? g_enc_launches[kind].load() : -1;
}

typedef _Float16 ec_h8 __attribute__((ext_vector_type(8)));
typedef float ec_f4 __attribute__((ext_vector_type(4)));

// ------------------------------------------------------------------ weight pack
// s[n] = gamma / sqrt(var + eps), w' = w s, b' = beta - mean s: in double, rounded once to fp32 (gamma null: w' = w, no
// bias written).  One thread per (n, k).
__device__ __forceinline__ double ec_bn_scale(const float *gamma, const float *var, int n) {
    return (double)gamma[n] / sqrt((double)var[n] + 1e-5);
}
// w [N, Cin, R, R] -> planes [N, 2 R R Cin], k = tap Cin + ci, in the plane layout of common.h
__global__ __launch_bounds__(256) void encoder_pack_kernel(const float *w, const float *gamma, const float *beta,
                                                           const float *mean, const float *var, int N, int Cin, int RR,
                                                           _Float16 *planes, float *bias) {
    const int K = RR * Cin;
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    if (i >= (long long)N * K) return;
    const int n = (int)(i / K), k = (int)(i - (long long)n * K);
    const int tap = k / Cin, ci = k - tap * Cin;
    float v = w[((long long)n * Cin + ci) * RR + tap];
    if (gamma) {
        const double s = ec_bn_scale(gamma, var, n);
        v = (float)__dmul_rn((double)v, s);
        if (k == 0) bias[n] = (float)__dsub_rn((double)beta[n], __dmul_rn((double)mean[n], s));     // (no contraction)
    }
    _Float16 hi, lo;
    isc_split_f16(v, hi, lo);
    const long long o = plane_index(n, k, K);
    planes[o] = hi;
    planes[o + 32] = lo;
}
// the stem: w [C0, 3, 7, 7] -> wk [147, C0] fp32, k = (ky 7 + kx) 3 + c
__global__ __launch_bounds__(256) void encoder_stem_pack_kernel(const float *w, const float *gamma, const float *beta,
                                                                const float *mean, const float *var, int C0, float *wk,
                                                                float *bias) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= 147 * C0) return;
    const int k = i / C0, n = i - k * C0, tap = k / 3, c = k - tap * 3;
    float v = w[(n * 3 + c) * 49 + tap];
    if (gamma) {
        const double s = ec_bn_scale(gamma, var, n);
        v = (float)__dmul_rn((double)v, s);
        if (k == 0) bias[n] = (float)__dsub_rn((double)beta[n], __dmul_rn((double)mean[n], s));     // (no contraction)
    }
    wk[i] = v;
}

// ------------------------------------------------------------------ stem
// A workgroup takes EC_ST_PIX consecutive output pixels: the folded weights [147][C0] and the pixels' 7 x 7 x 3 patches
// (normalised here for uint8 input, zero outside the image) go to LDS; a thread then owns one channel of four pixels and
// runs the 147 FMAs in k order.
#define EC_ST_PIX 32
struct EcStemArgs {
    const void *img;            // [B, H, W, 3] uint8 or fp32
    const float *wk, *bias;     // [147, C0], [C0]
    float *out;                 // [B, Ho, Wo, C0]
    int H, W, Ho, Wo, C0, M;
};
template <bool U8>
__global__ __launch_bounds__(256) void encoder_stem_kernel(const EcStemArgs a) {
    extern __shared__ float ec_st[];
    const int C0 = a.C0, tid = threadIdx.x;
    float *wk = ec_st, *patch = ec_st + 147 * C0;
    for (int i = tid; i < 147 * C0; i += 256) wk[i] = a.wk[i];
    const int m0 = blockIdx.x * EC_ST_PIX, HoWo = a.Ho * a.Wo;
    for (int i = tid; i < EC_ST_PIX * 147; i += 256) {
        const int p = i / 147, k = i - p * 147, tap = k / 3, c = k - tap * 3, ky = tap / 7, kx = tap - ky * 7;
        const int m = m0 + p;
        float v = 0.f;
        if (m < a.M) {
            const int b = m / HoWo, r = m - b * HoWo, y = r / a.Wo, x = r - y * a.Wo;
            const int iy = 2 * y + ky - 3, ix = 2 * x + kx - 3;
            if (iy >= 0 && iy < a.H && ix >= 0 && ix < a.W) {
                const long long o = (((long long)b * a.H + iy) * a.W + ix) * 3 + c;
                if constexpr (U8) {
                    const float mean = c == 0 ? 0.485f : c == 1 ? 0.456f : 0.406f;
                    const float sd = c == 0 ? 0.229f : c == 1 ? 0.224f : 0.225f;
                    v = ((float)static_cast<const uint8_t *>(a.img)[o] / 255.0f - mean) / sd;
                } else {
                    v = static_cast<const float *>(a.img)[o];
                }
            }
        }
        patch[i] = v;
    }
    __syncthreads();
    for (int item = tid; item < (EC_ST_PIX / 4) * C0; item += 256) {
        const int g = item / C0, c = item - g * C0;
        const float *p0 = patch + (4 * g) * 147;
        float acc[4] = {0.f, 0.f, 0.f, 0.f};
        for (int k = 0; k < 147; ++k) {
            const float wv = wk[k * C0 + c];
#pragma unroll
            for (int j = 0; j < 4; ++j) acc[j] = fmaf(p0[j * 147 + k], wv, acc[j]);
        }
        const float bv = a.bias[c];
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const int m = m0 + 4 * g + j;
            if (m < a.M) a.out[(long long)m * C0 + c] = isc_relu(acc[j] + bv);
        }
    }
}

// ------------------------------------------------------------------ max-pool 3x3 / 2, pad 0, ceil mode
// One thread per output pixel and channel quad; a window is clipped to the grid (NaN propagates, as torch's does).
__global__ __launch_bounds__(256) void encoder_maxpool_kernel(const float *x, int h, int w, int ho, int wo, int C,
                                                              long long n4, float *out) {
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    if (i >= n4) return;
    const int C4 = C >> 2, c4 = (int)(i % C4);
    const long long m = i / C4;
    const int ox = (int)(m % wo), oy = (int)((m / wo) % ho);
    const long long b = m / ((long long)wo * ho);
    const int y1 = min(2 * oy + 3, h), x1 = min(2 * ox + 3, w);
    float4 best = make_float4(-INFINITY, -INFINITY, -INFINITY, -INFINITY);
    for (int y = 2 * oy; y < y1; ++y)
        for (int xx = 2 * ox; xx < x1; ++xx) {
            const float4 v = *reinterpret_cast<const float4 *>(x + ((b * h + y) * w + xx) * C + c4 * 4);
            if (v.x > best.x || v.x != v.x) best.x = v.x;
            if (v.y > best.y || v.y != v.y) best.y = v.y;
            if (v.z > best.z || v.z != v.z) best.z = v.z;
            if (v.w > best.w || v.w != v.w) best.w = v.w;
        }
    *reinterpret_cast<float4 *>(out + m * C + c4 * 4) = best;
}

// ------------------------------------------------------------------ implicit-GEMM convolution, R = 1 or 3
// Output row m = (b ho + y) wo + x.  R3: the nine taps of input pixel (y + dy - 1, x + dx - 1) in tap-major order, the
// zero line for a tap outside the image's own grid (input grid = output grid).  R = 1: the one tap (y stride, x stride),
// always inside the grid (ho = (hi - 1) / stride + 1).  A row at or beyond M reads the zero line.
// Epilogue (ksplit == 1): + bias[n], + residual[m, n] when given, ReLU when asked - in this order; ksplit > 1: the raw
// partial tile to slab blockIdx.z, the epilogue in encoder_reduce_kernel.
struct EcConvArgs {
    const float *A;             // [B hi wi, Cin]
    const float *zero;          // >= 32 zero bytes
    const _Float16 *W;          // planes [N, 2 K], K = R R Cin
    const float *bias;          // [N]
    const float *res;           // [M, N] or null
    float *out;                 // ksplit == 1: [M, N]; else slabs [ksplit][M][N]
    int hi, wi, ho, wo, Cin, N, M, stride, relu, ksplit;
};
#define EC_BM 64
#define EC_BN 128
#define EC_LD 40                // halfs per LDS row: 32 + 8 of padding
#define EC_BUF (2 * EC_BM * EC_LD + 2 * EC_BN * EC_LD)      // halfs per buffer: A hi | A lo | W hi | W lo
struct EcStage {
    float4 a0, a1;              // the eight fp32 values of the A octet
    uint4 w0, w1, w2, w3;
};

template <bool R3>
__global__ __launch_bounds__(256) void encoder_conv_kernel(const EcConvArgs a) {
    __shared__ __attribute__((aligned(16))) _Float16 lds[2 * EC_BUF];
    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6, wm = wv >> 1, wn = wv & 1;
    const int row0 = blockIdx.y * EC_BM, col0 = blockIdx.x * EC_BN, ks = blockIdx.z;
    const int hi_ = a.hi, wi_ = a.wi, Cin = a.Cin, N = a.N, M = a.M;
    const int cpt = Cin >> 5, nchunks = (R3 ? 9 : 1) * cpt;
    const int K2 = 2 * (R3 ? 9 : 1) * Cin;                       // halfs per W row
    const int c_lo = (int)((long long)nchunks * ks / a.ksplit), c_hi = (int)((long long)nchunks * (ks + 1) / a.ksplit);

    // this thread's A row: output pixel (b, y, x) of row m
    const int ar = tid >> 2, aoct = tid & 3;
    const int m = row0 + ar;
    const bool m_ok = m < M;
    const int howo = a.ho * a.wo;
    const int mb = m_ok ? m / howo : 0, mrem = m_ok ? m - mb * howo : 0, my = mrem / a.wo, mx = mrem - my * a.wo;
    const float *zrow = a.zero;
    // this thread's four 16-byte pieces of the W image: piece p = tid + 256 i -> row p >> 3, part p & 7 (0-3: hi octets,
    // 4-7: lo octets) of the row's 64-half k-block; a column at or beyond N re-reads row N - 1 (never stored)
    const _Float16 *wsrc[4];
    int wdst[4];
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const int p = tid + 256 * i, r = p >> 3, part = p & 7;
        const int gn = col0 + r < N ? col0 + r : N - 1;
        wsrc[i] = a.W + (long long)gn * K2 + part * 8;
        wdst[i] = 2 * EC_BM * EC_LD + (part >> 2) * EC_BN * EC_LD + r * EC_LD + (part & 3) * 8;
    }

    EcStage st0, st1;
    auto load = [&](int c, EcStage &s) __attribute__((always_inline)) {
        int kc, yy, xx;
        bool in;
        if constexpr (R3) {
            const int tap = c / cpt;
            kc = c - tap * cpt;
            yy = my + tap / 3 - 1;
            xx = mx + tap % 3 - 1;
            in = m_ok && yy >= 0 && yy < hi_ && xx >= 0 && xx < wi_;
        } else {
            kc = c;
            yy = my * a.stride;
            xx = mx * a.stride;
            in = m_ok;
        }
        const float *src = in ? a.A + (((long long)mb * hi_ + yy) * wi_ + xx) * Cin + kc * 32 + aoct * 8 : zrow;
        s.a0 = *reinterpret_cast<const float4 *>(src);
        s.a1 = *reinterpret_cast<const float4 *>(src + 4);
        s.w0 = *reinterpret_cast<const uint4 *>(wsrc[0] + (long long)c * 64);
        s.w1 = *reinterpret_cast<const uint4 *>(wsrc[1] + (long long)c * 64);
        s.w2 = *reinterpret_cast<const uint4 *>(wsrc[2] + (long long)c * 64);
        s.w3 = *reinterpret_cast<const uint4 *>(wsrc[3] + (long long)c * 64);
    };
    auto store = [&](const EcStage &s, int S) __attribute__((always_inline)) {     // set S -> LDS buffer S
        _Float16 *b = lds + S * EC_BUF;
        const float x[8] = {s.a0.x, s.a0.y, s.a0.z, s.a0.w, s.a1.x, s.a1.y, s.a1.z, s.a1.w};
        ec_h8 hi, lo;
#pragma unroll
        for (int e = 0; e < 8; ++e) {
            _Float16 hh, ll;
            isc_split_f16(x[e], hh, ll);
            hi[e] = hh;
            lo[e] = ll;
        }
        *reinterpret_cast<ec_h8 *>(b + ar * EC_LD + aoct * 8) = hi;
        *reinterpret_cast<ec_h8 *>(b + EC_BM * EC_LD + ar * EC_LD + aoct * 8) = lo;
        *reinterpret_cast<uint4 *>(b + wdst[0]) = s.w0;
        *reinterpret_cast<uint4 *>(b + wdst[1]) = s.w1;
        *reinterpret_cast<uint4 *>(b + wdst[2]) = s.w2;
        *reinterpret_cast<uint4 *>(b + wdst[3]) = s.w3;
    };

    ec_f4 acc0[2][4], acc1[2][4];
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int j = 0; j < 4; ++j)
#pragma unroll
            for (int r = 0; r < 4; ++r) { acc0[i][j][r] = 0.f; acc1[i][j][r] = 0.f; }

    const int fr = lane & 15, fq = lane >> 4;
    auto step = [&](int c, EcStage &s, int S) __attribute__((always_inline)) {
        store(s, S);
        __syncthreads();
        if (c + 2 < c_hi) load(c + 2, s);
        const _Float16 *b = lds + S * EC_BUF;
        ec_h8 ah[2], al[2];
#pragma unroll
        for (int i = 0; i < 2; ++i) {
            const int o = (wm * 32 + i * 16 + fr) * EC_LD + fq * 8;
            ah[i] = *reinterpret_cast<const ec_h8 *>(b + o);
            al[i] = *reinterpret_cast<const ec_h8 *>(b + EC_BM * EC_LD + o);
        }
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const int o = 2 * EC_BM * EC_LD + (wn * 64 + j * 16 + fr) * EC_LD + fq * 8;
            const ec_h8 bh = *reinterpret_cast<const ec_h8 *>(b + o);
            const ec_h8 bl = *reinterpret_cast<const ec_h8 *>(b + EC_BN * EC_LD + o);
#pragma unroll
            for (int i = 0; i < 2; ++i) {
                acc0[i][j] = __builtin_amdgcn_mfma_f32_16x16x32_f16(ah[i], bh, acc0[i][j], 0, 0, 0);
                acc1[i][j] = __builtin_amdgcn_mfma_f32_16x16x32_f16(ah[i], bl, acc1[i][j], 0, 0, 0);
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
                    if (a.res) v += a.res[(long long)gm * N + gn];
                    if (a.relu) v = isc_relu(v);
                }
                out[(long long)gm * N + gn] = v;
            }
    }
}

// out[m, n] = (relu)(slab_0 + ... + slab_{S-1} + bias[n] (+ res[m, n])): slabs ascending, the bias, the residual.
__global__ __launch_bounds__(256) void encoder_reduce_kernel(const float *slabs, int S, long long MN, int N,
                                                             const float *bias, const float *res, int relu, float *out) {
    const long long i4 = ((long long)blockIdx.x * 256 + threadIdx.x) * 4;     // (N % 16 == 0: a float4 stays in its row)
    if (i4 >= MN) return;
    float4 s = *reinterpret_cast<const float4 *>(slabs + i4);
    for (int k = 1; k < S; ++k) {
        const float4 v = *reinterpret_cast<const float4 *>(slabs + (long long)k * MN + i4);
        s.x += v.x; s.y += v.y; s.z += v.z; s.w += v.w;
    }
    const float4 b = *reinterpret_cast<const float4 *>(bias + (int)(i4 % N));
    s.x += b.x; s.y += b.y; s.z += b.z; s.w += b.w;
    if (res) {
        const float4 r = *reinterpret_cast<const float4 *>(res + i4);
        s.x += r.x; s.y += r.y; s.z += r.z; s.w += r.w;
    }
    if (relu) { s.x = isc_relu(s.x); s.y = isc_relu(s.y); s.z = isc_relu(s.z); s.w = isc_relu(s.w); }
    *reinterpret_cast<float4 *>(out + i4) = s;
}

// ------------------------------------------------------------------ tail
// Workgroup (q, b): q < a a: region (i, j) = (q / a, q % a) of image b, the mean over rows [floor(i h / a), ceil((i + 1)
// h / a)) and the same columns; q == a a: fc = the mean over x (x ascending) of every row, then the mean over y.  A
// thread owns channels tid, tid + 256, ...; sums run in one fixed order.
struct EcTailArgs {
    const float *x;             // [B, h, w, C]
    float *fc, *att;            // [B, C], [B, a, a, C]
    _Float16 *fc16, *att16;     // optional copies
    int h, w, C, a;
};
__global__ __launch_bounds__(256) void encoder_tail_kernel(const EcTailArgs t) {
    const int q = blockIdx.x, b = blockIdx.y, h = t.h, w = t.w, C = t.C, a = t.a;
    const float *xb = t.x + (long long)b * h * w * C;
    if (q < a * a) {
        const int i = q / a, j = q - i * a;
        const int y0 = (i * h) / a, y1 = ((i + 1) * h + a - 1) / a, x0 = (j * w) / a, x1 = ((j + 1) * w + a - 1) / a;
        const float cnt = (float)((y1 - y0) * (x1 - x0));
        for (int c = threadIdx.x; c < C; c += 256) {
            float s = 0.f;                      // (row sums first: a 1 x 1 grid over a large map keeps short sums)
            for (int y = y0; y < y1; ++y) {
                float r = 0.f;
                for (int x = x0; x < x1; ++x) r += xb[((long long)y * w + x) * C + c];
                s += r;
            }
            const float v = s / cnt;
            const long long o = ((long long)b * a * a + q) * C + c;
            t.att[o] = v;
            if (t.att16) t.att16[o] = (_Float16)v;
        }
    } else {
        for (int c = threadIdx.x; c < C; c += 256) {
            float s = 0.f;
            for (int y = 0; y < h; ++y) {
                float r = 0.f;
                for (int x = 0; x < w; ++x) r += xb[((long long)y * w + x) * C + c];
                s += r / (float)w;
            }
            const float v = s / (float)h;
            t.fc[(long long)b * C + c] = v;
            if (t.fc16) t.fc16[(long long)b * C + c] = (_Float16)v;
        }
    }
}

// ------------------------------------------------------------------ drivers
namespace {
long long ec_up64(long long n) { return (n + 63) / 64 * 64; }
int ec_stem_out(int n) { return (n - 1) / 2 + 1; }              // 7x7 / 2, pad 3
int ec_pool_out(int n) { return (n - 2) / 2 + 1; }              // = ceil((n - 3) / 2) + 1 for n >= 2 (n == 2: one clipped window)
int ec_s2_out(int n) { return (n - 1) / 2 + 1; }                // 1x1 / 2

bool ec_conv_shape_ok(long long B, long long h, long long w, long long Cin, long long N, int R, int stride) {
    if (B < 1 || h < 1 || w < 1 || h > 8192 || w > 8192 || Cin < 32 || Cin > 65536 || Cin % 32 || N < 16 || N > 65536 ||
        N % 16)
        return false;
    if (!((R == 1 && (stride == 1 || stride == 2)) || (R == 3 && stride == 1))) return false;
    return B * h * w <= (1LL << 22);             // (the row tiles ride on gridDim.y)
}
// Route of one convolution: 1 = one workgroup per tile, the epilogue in the kernel; n > 1 = the contraction split over n
// workgroups per tile, raw partial tiles to slabs, the reduce kernel behind them.  Auto (want <= 0): chosen from ONE
// image's rows M1 = ho wo, never from the batch - the route fixes the order in which a row's contraction is summed, so a
// rule that looked at B would give an image other bits in a batch than alone.  An image of fewer than 128 tiles (half
// the chip's 256 CUs) splits until about 256 workgroups per image run, 32 at the most, every share >= 2 chunks.
int ec_ksplit(long long M1, int N, int Cin, int R, int want) {
    const int nchunks = R * R * (Cin / 32);
    int s = want;
    if (s <= 0) {
        const long long tiles = ((M1 + EC_BM - 1) / EC_BM) * ((N + EC_BN - 1) / EC_BN);
        if (tiles >= 128) return 1;
        s = (int)((256 + tiles - 1) / tiles);
        if (s > 32) s = 32;
        if (s > nchunks / 2) s = nchunks / 2;
    }
    if (s > nchunks) s = nchunks;
    return s < 1 ? 1 : s;
}
// x [B, hi, wi, Cin] -> dst [B, ho, wo, N] on the route of ec_ksplit; n_kind counts per ISC_ENCODER_KIND_*.
int ec_launch_conv(const float *A, const float *zero, const _Float16 *Wp, const float *bias, const float *res, float *dst,
                   float *slabs, int B, int hi, int wi, int Cin, int N, int R, int stride, int relu, int ksplit_want,
                   hipStream_t st, long long *n_kind) {
    const int ho = stride == 2 ? ec_s2_out(hi) : hi, wo = stride == 2 ? ec_s2_out(wi) : wi;
    const int M = B * ho * wo;
    const int s = ec_ksplit((long long)ho * wo, N, Cin, R, ksplit_want);
    EcConvArgs a = {};
    a.A = A; a.zero = zero; a.W = Wp; a.bias = bias; a.res = res;
    a.out = s > 1 ? slabs : dst;
    a.hi = hi; a.wi = wi; a.ho = ho; a.wo = wo; a.Cin = Cin; a.N = N; a.M = M; a.stride = stride; a.relu = relu;
    a.ksplit = s;
    const dim3 grid((N + EC_BN - 1) / EC_BN, (M + EC_BM - 1) / EC_BM, s);
    if (R == 3) hipLaunchKernelGGL(encoder_conv_kernel<true>, grid, dim3(256), 0, st, a);
    else hipLaunchKernelGGL(encoder_conv_kernel<false>, grid, dim3(256), 0, st, a);
    ISC_LAUNCH_CHECK();
    ++n_kind[s > 1 ? ISC_ENCODER_KIND_SPLIT : ISC_ENCODER_KIND_DIRECT];
    ++n_kind[R == 3 ? ISC_ENCODER_KIND_R3 : ISC_ENCODER_KIND_R1];
    if (s > 1) {
        const long long MN = (long long)M * N;
        hipLaunchKernelGGL(encoder_reduce_kernel, dim3((unsigned)((MN / 4 + 255) / 256)), dim3(256), 0, st, slabs, s, MN,
                           N, bias, res, relu, dst);
        ISC_LAUNCH_CHECK();
        ++n_kind[ISC_ENCODER_KIND_REDUCE];
    }
    return ISC_OK;
}
void ec_count(const long long *n_kind) {
    for (int i = 0; i < ISC_ENCODER_KINDS; ++i) g_enc_launches[i] += n_kind[i];
}

bool ec_stem_shape_ok(long long B, long long H, long long W, int C0) {
    return B >= 1 && H >= 1 && W >= 1 && H <= 8192 && W <= 8192 && (C0 == 32 || C0 == 64) &&
           B * ec_stem_out((int)H) * ec_stem_out((int)W) <= (1LL << 22);
}
int ec_launch_stem(const void *img, int u8, int B, int H, int W, int C0, const float *wk, const float *bias, float *out,
                   hipStream_t st) {
    EcStemArgs a = {};
    a.img = img; a.wk = wk; a.bias = bias; a.out = out;
    a.H = H; a.W = W; a.Ho = ec_stem_out(H); a.Wo = ec_stem_out(W); a.C0 = C0; a.M = B * a.Ho * a.Wo;
    const size_t lds = (size_t)(147 * C0 + EC_ST_PIX * 147) * sizeof(float);
    const dim3 grid((a.M + EC_ST_PIX - 1) / EC_ST_PIX);
    if (u8) hipLaunchKernelGGL(encoder_stem_kernel<true>, grid, dim3(256), lds, st, a);
    else hipLaunchKernelGGL(encoder_stem_kernel<false>, grid, dim3(256), lds, st, a);
    ISC_LAUNCH_CHECK();
    return ISC_OK;
}
int ec_launch_pool(const float *x, int B, int h, int w, int C, float *out, hipStream_t st) {
    const int ho = ec_pool_out(h), wo = ec_pool_out(w);
    const long long n4 = (long long)B * ho * wo * (C / 4);
    hipLaunchKernelGGL(encoder_maxpool_kernel, dim3((unsigned)((n4 + 255) / 256)), dim3(256), 0, st, x, h, w, ho, wo, C, n4,
                       out);
    ISC_LAUNCH_CHECK();
    return ISC_OK;
}
int ec_launch_tail(const float *x, int B, int h, int w, int C, int a, float *fc, float *att, void *fc16, void *att16,
                   hipStream_t st) {
    EcTailArgs t = {};
    t.x = x; t.fc = fc; t.att = att; t.fc16 = static_cast<_Float16 *>(fc16); t.att16 = static_cast<_Float16 *>(att16);
    t.h = h; t.w = w; t.C = C; t.a = a;
    hipLaunchKernelGGL(encoder_tail_kernel, dim3(a * a + 1, B), dim3(256), 0, st, t);
    ISC_LAUNCH_CHECK();
    return ISC_OK;
}

// ---- the network: the stem and, per bottleneck, conv1 (1x1, the layer's stride in its first block), conv2 (3x3), conv3
// (1x1, + identity, ReLU) and in a layer's first block the downsample (1x1 at the same stride, no ReLU) - in this order,
// which is the order of isc_encoder_pack's `convs` and of the segments of the packed buffer.
struct EcConvDesc {
    int R, stride, Cin, N;
    long long w_off, b_off;     // bytes into the packed buffer
};
#define EC_MAX_BLOCKS 64
#define EC_MAX_CONVS (1 + 3 * EC_MAX_BLOCKS + 4)
struct EcNet {
    int n;
    EcConvDesc c[EC_MAX_CONVS];
    long long bytes;
};
bool ec_net_ok(const int *layers, int width) {
    if (!layers || (width != 32 && width != 64)) return false;
    int sum = 0;
    for (int l = 0; l < 4; ++l) {
        if (layers[l] < 1 || layers[l] > EC_MAX_BLOCKS) return false;
        sum += layers[l];
    }
    return sum <= EC_MAX_BLOCKS;
}
long long ec_up256(long long n) { return (n + 255) / 256 * 256; }
void ec_net(const int *layers, int width, EcNet *net) {
    long long at = 0;
    int n = 0;
    auto add = [&](int R, int stride, int Cin, int N) {
        EcConvDesc &d = net->c[n++];
        d.R = R; d.stride = stride; d.Cin = Cin; d.N = N;
        d.w_off = at;
        at += ec_up256(R == 7 ? (long long)147 * N * 4 : (long long)N * 2 * R * R * Cin * 2);
        d.b_off = at;
        at += ec_up256((long long)N * 4);
    };
    add(7, 2, 3, width);
    int inpl = width;
    for (int l = 0; l < 4; ++l) {
        const int p = width << l;
        for (int i = 0; i < layers[l]; ++i) {
            const int stride = (l > 0 && i == 0) ? 2 : 1;
            add(1, stride, inpl, p);
            add(3, 1, p, p);
            add(1, 1, p, 4 * p);
            if (i == 0) add(1, stride, inpl, 4 * p);
            inpl = 4 * p;
        }
    }
    net->n = n;
    net->bytes = at;
}
struct EcLayout {
    long long zero, act[5], slabs, total;       // in floats
    int Ho, Wo, hp, wp, hf, wf;                 // stem output, pool output, final grid
};
bool ec_image_ok(long long B, long long H, long long W) {
    // under 3 px the stem's grid is 1 x 1, which the ceil-mode pool refuses
    return B >= 1 && H >= 3 && W >= 3 && H <= 8192 && W <= 8192 &&
           B * ec_stem_out((int)H) * ec_stem_out((int)W) <= (1LL << 22);
}
EcLayout ec_layout(int B, int H, int W, const int *layers, int width, int ksplit) {
    EcLayout o;
    o.Ho = ec_stem_out(H); o.Wo = ec_stem_out(W);
    o.hp = ec_pool_out(o.Ho); o.wp = ec_pool_out(o.Wo);
    long long act = (long long)B * o.Ho * o.Wo * width, slab = 0;
    int h = o.hp, w = o.wp, inpl = width;
    auto conv = [&](int hi, int wi, int Cin, int N, int R, int stride) {
        const int ho = stride == 2 ? ec_s2_out(hi) : hi, wo = stride == 2 ? ec_s2_out(wi) : wi;
        const long long M = (long long)B * ho * wo;
        if (M * N > act) act = M * N;
        const int s = ec_ksplit((long long)ho * wo, N, Cin, R, ksplit);
        if (s > 1 && s * M * N > slab) slab = s * M * N;
    };
    for (int l = 0; l < 4; ++l) {
        const int p = width << l;
        for (int i = 0; i < layers[l]; ++i) {
            const int stride = (l > 0 && i == 0) ? 2 : 1;
            conv(h, w, inpl, p, 1, stride);
            if (i == 0) conv(h, w, inpl, 4 * p, 1, stride);
            if (stride == 2) { h = ec_s2_out(h); w = ec_s2_out(w); }
            conv(h, w, p, p, 3, 1);
            conv(h, w, p, 4 * p, 1, 1);
            inpl = 4 * p;
        }
    }
    o.hf = h; o.wf = w;
    long long at = 0;
    o.zero = at; at += 64;
    for (int i = 0; i < 5; ++i) { o.act[i] = at; at += ec_up64(act); }
    o.slabs = at; at += ec_up64(slab);
    o.total = at;
    return o;
}
}  // namespace

// ---- the parts on their own
extern "C" int isc_conv_pack(const float *w, const float *gamma, const float *beta, const float *mean, const float *var,
                             int N, int Cin, int R, void *planes, float *bias, void *stream) {
    if (!w || !planes) return ISC_E_NULL;
    if (gamma && (!beta || !mean || !var || !bias)) return ISC_E_NULL;
    if (!ec_conv_shape_ok(1, 1, 1, Cin, N, R, 1)) return ISC_E_SHAPE;
    if (!isc_aligned16(planes)) return ISC_E_ALIGN;
    const long long n = (long long)N * R * R * Cin;
    hipLaunchKernelGGL(encoder_pack_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, (hipStream_t)stream, w, gamma,
                       beta, mean, var, N, Cin, R * R, static_cast<_Float16 *>(planes), bias);
    ISC_LAUNCH_CHECK();
    ++g_enc_launches[ISC_ENCODER_KIND_PACK];
    return ISC_OK;
}

extern "C" int isc_encoder_stem_pack(const float *w, const float *gamma, const float *beta, const float *mean,
                                     const float *var, int C0, float *wk, float *bias, void *stream) {
    if (!w || !wk) return ISC_E_NULL;
    if (gamma && (!beta || !mean || !var || !bias)) return ISC_E_NULL;
    if (C0 != 32 && C0 != 64) return ISC_E_SHAPE;
    hipLaunchKernelGGL(encoder_stem_pack_kernel, dim3((147 * C0 + 255) / 256), dim3(256), 0, (hipStream_t)stream, w, gamma,
                       beta, mean, var, C0, wk, bias);
    ISC_LAUNCH_CHECK();
    ++g_enc_launches[ISC_ENCODER_KIND_PACK];
    return ISC_OK;
}

extern "C" int64_t isc_conv_workspace_bytes(int B, int h, int w, int Cin, int N, int R, int stride, int ksplit) {
    if (!ec_conv_shape_ok(B, h, w, Cin, N, R, stride) || ksplit < 0) return 0;
    const int ho = stride == 2 ? ec_s2_out(h) : h, wo = stride == 2 ? ec_s2_out(w) : w;
    const long long M = (long long)B * ho * wo;
    const int s = ec_ksplit((long long)ho * wo, N, Cin, R, ksplit);
    return (64 + (s > 1 ? ec_up64(s * M * N) : 0)) * (int64_t)sizeof(float);
}

extern "C" int isc_conv_fwd(const isc_conv_problem *q, void *stream) {
    if (!q) return ISC_E_NULL;
    if (!q->x || !q->planes || !q->bias || !q->workspace || !q->out) return ISC_E_NULL;
    if (!ec_conv_shape_ok(q->B, q->h, q->w, q->Cin, q->N, q->R, q->stride) || q->ksplit < 0) return ISC_E_SHAPE;
    if (q->workspace_bytes < isc_conv_workspace_bytes(q->B, q->h, q->w, q->Cin, q->N, q->R, q->stride, q->ksplit))
        return ISC_E_WORKSPACE;
    if (!isc_aligned16(q->x) || !isc_aligned16(q->planes) || !isc_aligned16(q->bias) || !isc_aligned16(q->workspace) ||
        !isc_aligned16(q->out) || (q->residual && !isc_aligned16(q->residual)))
        return ISC_E_ALIGN;
    hipStream_t st = (hipStream_t)stream;
    float *ws = static_cast<float *>(q->workspace);
    if (hipMemsetAsync(ws, 0, 64 * sizeof(float), st) != hipSuccess) return (int)hipGetLastError();
    long long n_kind[ISC_ENCODER_KINDS] = {};
    const int rc = ec_launch_conv(q->x, ws, static_cast<const _Float16 *>(q->planes), q->bias, q->residual, q->out, ws + 64,
                                  q->B, q->h, q->w, q->Cin, q->N, q->R, q->stride, q->relu, q->ksplit, st, n_kind);
    if (rc != ISC_OK) return rc;
    ec_count(n_kind);
    return ISC_OK;
}

extern "C" int isc_encoder_stem(const void *img, int img_u8, int B, int H, int W, int C0, const float *wk,
                                const float *bias, float *out, void *stream) {
    if (!img || !wk || !bias || !out) return ISC_E_NULL;
    if (!ec_stem_shape_ok(B, H, W, C0)) return ISC_E_SHAPE;
    if (!isc_aligned16(out) || (!img_u8 && ((uintptr_t)img & 3u)) || ((uintptr_t)wk & 3u) || ((uintptr_t)bias & 3u))
        return ISC_E_ALIGN;
    const int rc = ec_launch_stem(img, img_u8, B, H, W, C0, wk, bias, out, (hipStream_t)stream);
    if (rc != ISC_OK) return rc;
    ++g_enc_launches[ISC_ENCODER_KIND_STEM];
    return ISC_OK;
}

extern "C" int isc_encoder_maxpool(const float *x, int B, int h, int w, int C, float *out, void *stream) {
    if (!x || !out) return ISC_E_NULL;
    // (a 1-pixel side gives the stock op an empty output: it refuses)
    if (B < 1 || h < 2 || w < 2 || h > 8192 || w > 8192 || C < 4 || C % 4 || C > 65536 ||
        (long long)B * h * w > (1LL << 22))
        return ISC_E_SHAPE;
    if (!isc_aligned16(x) || !isc_aligned16(out)) return ISC_E_ALIGN;
    const int rc = ec_launch_pool(x, B, h, w, C, out, (hipStream_t)stream);
    if (rc != ISC_OK) return rc;
    ++g_enc_launches[ISC_ENCODER_KIND_POOL];
    return ISC_OK;
}

extern "C" int isc_encoder_tail(const float *x, int B, int h, int w, int C, int att_size, float *fc, float *att,
                                void *fc_f16, void *att_f16, void *stream) {
    if (!x || !fc || !att) return ISC_E_NULL;
    if (B < 1 || B > 65535 || h < 1 || w < 1 || h > 8192 || w > 8192 || C < 1 || C > 65536 || att_size < 1 ||
        att_size > 64)
        return ISC_E_SHAPE;
    // (scalar accesses: the element's own alignment is all the kernel needs)
    if (((uintptr_t)x & 3u) || ((uintptr_t)fc & 3u) || ((uintptr_t)att & 3u) || ((uintptr_t)fc_f16 & 1u) ||
        ((uintptr_t)att_f16 & 1u))
        return ISC_E_ALIGN;
    const int rc = ec_launch_tail(x, B, h, w, C, att_size, fc, att, fc_f16, att_f16, (hipStream_t)stream);
    if (rc != ISC_OK) return rc;
    ++g_enc_launches[ISC_ENCODER_KIND_TAIL];
    return ISC_OK;
}

// ---- the whole encoder
extern "C" int isc_encoder_num_convs(const int *layers, int width) {
    if (!ec_net_ok(layers, width)) return 0;
    EcNet net;
    ec_net(layers, width, &net);
    return net.n;
}

extern "C" int64_t isc_encoder_pack_bytes(const int *layers, int width) {
    if (!ec_net_ok(layers, width)) return 0;
    EcNet net;
    ec_net(layers, width, &net);
    return net.bytes;
}

extern "C" int isc_encoder_pack(const isc_encoder_conv_params *convs_host, int n_convs, const int *layers, int width,
                                void *packed, void *stream) {
    if (!convs_host || !packed || !layers) return ISC_E_NULL;
    if (!ec_net_ok(layers, width)) return ISC_E_SHAPE;
    EcNet net;
    ec_net(layers, width, &net);
    if (n_convs != net.n) return ISC_E_SHAPE;
    for (int i = 0; i < n_convs; ++i) {
        const isc_encoder_conv_params &c = convs_host[i];
        if (!c.w || !c.gamma || !c.beta || !c.mean || !c.var) return ISC_E_NULL;
    }
    if (((uintptr_t)packed & 255u) != 0) return ISC_E_ALIGN;
    char *base = static_cast<char *>(packed);
    for (int i = 0; i < n_convs; ++i) {
        const isc_encoder_conv_params &c = convs_host[i];
        const EcConvDesc &d = net.c[i];
        float *bias = reinterpret_cast<float *>(base + d.b_off);
        const int rc = d.R == 7 ? isc_encoder_stem_pack(c.w, c.gamma, c.beta, c.mean, c.var, d.N,
                                                        reinterpret_cast<float *>(base + d.w_off), bias, stream)
                                : isc_conv_pack(c.w, c.gamma, c.beta, c.mean, c.var, d.N, d.Cin, d.R, base + d.w_off, bias,
                                                stream);
        if (rc != ISC_OK) return rc;
    }
    return ISC_OK;
}

extern "C" int64_t isc_encoder_workspace_bytes(int B, int H, int W, const int *layers, int width) {
    if (!ec_net_ok(layers, width) || !ec_image_ok(B, H, W)) return 0;
    return ec_layout(B, H, W, layers, width, 0).total * (int64_t)sizeof(float);
}
// (a forced ksplit may need larger slabs than the cost rule's choice)
extern "C" int64_t isc_encoder_workspace_bytes_ksplit(int B, int H, int W, const int *layers, int width, int ksplit) {
    if (!ec_net_ok(layers, width) || !ec_image_ok(B, H, W) || ksplit < 0) return 0;
    return ec_layout(B, H, W, layers, width, ksplit).total * (int64_t)sizeof(float);
}

extern "C" int isc_encoder_final_grid(int H, int W, int *hf, int *wf) {
    if (!hf || !wf) return ISC_E_NULL;
    if (!ec_image_ok(1, H, W)) return ISC_E_SHAPE;
    int h = ec_pool_out(ec_stem_out(H)), w = ec_pool_out(ec_stem_out(W));
    for (int l = 1; l < 4; ++l) { h = ec_s2_out(h); w = ec_s2_out(w); }
    *hf = h; *wf = w;
    return ISC_OK;
}

extern "C" int isc_encoder_fwd(const isc_encoder_problem *q, void *stream) {
    if (!q) return ISC_E_NULL;
    if (!q->image || !q->packed || !q->workspace || !q->fc || !q->att) return ISC_E_NULL;
    const int B = q->B, H = q->H, W = q->W, width = q->width;
    if (!ec_net_ok(q->layers, width) || !ec_image_ok(B, H, W) || B > 65535 || q->att_size < 1 || q->att_size > 64 ||
        q->ksplit < 0)
        return ISC_E_SHAPE;
    EcNet net;
    ec_net(q->layers, width, &net);
    if (q->packed_bytes < net.bytes) return ISC_E_WORKSPACE;
    const EcLayout lay = ec_layout(B, H, W, q->layers, width, q->ksplit);
    if (q->workspace_bytes < lay.total * (int64_t)sizeof(float)) return ISC_E_WORKSPACE;
    if (!isc_aligned16(q->workspace) || !isc_aligned16(q->packed) || (!q->image_u8 && ((uintptr_t)q->image & 3u)) ||
        ((uintptr_t)q->fc & 3u) || ((uintptr_t)q->att & 3u) || ((uintptr_t)q->fc_f16 & 1u) || ((uintptr_t)q->att_f16 & 1u))
        return ISC_E_ALIGN;
    hipStream_t st = (hipStream_t)stream;
    float *ws = static_cast<float *>(q->workspace);
    const char *pk = static_cast<const char *>(q->packed);
    long long n_kind[ISC_ENCODER_KINDS] = {};
    auto Wf = [&](int i) { return reinterpret_cast<const float *>(pk + net.c[i].w_off); };
    auto Wh = [&](int i) { return reinterpret_cast<const _Float16 *>(pk + net.c[i].w_off); };
    auto Bf = [&](int i) { return reinterpret_cast<const float *>(pk + net.c[i].b_off); };

    if (hipMemsetAsync(ws + lay.zero, 0, 64 * sizeof(float), st) != hipSuccess) return (int)hipGetLastError();
    const float *zero = ws + lay.zero;
    float *cur = ws + lay.act[0], *nxt = ws + lay.act[1], *t1 = ws + lay.act[2], *t2 = ws + lay.act[3],
          *idn = ws + lay.act[4], *slabs = ws + lay.slabs;
    int rc = ec_launch_stem(q->image, q->image_u8, B, H, W, width, Wf(0), Bf(0), t1, st);
    if (rc != ISC_OK) return rc;
    ++n_kind[ISC_ENCODER_KIND_STEM];
    rc = ec_launch_pool(t1, B, lay.Ho, lay.Wo, width, cur, st);
    if (rc != ISC_OK) return rc;
    ++n_kind[ISC_ENCODER_KIND_POOL];
    int h = lay.hp, w = lay.wp, ci = 1, inpl = width;
    for (int l = 0; l < 4; ++l) {
        const int p = width << l;
        for (int i = 0; i < q->layers[l]; ++i) {
            const int stride = (l > 0 && i == 0) ? 2 : 1;
            const int c1 = ci, c2 = ci + 1, c3 = ci + 2, cd = ci + 3;
            const int ho = stride == 2 ? ec_s2_out(h) : h, wo = stride == 2 ? ec_s2_out(w) : w;
            rc = ec_launch_conv(cur, zero, Wh(c1), Bf(c1), nullptr, t1, slabs, B, h, w, inpl, p, 1, stride, 1, q->ksplit, st,
                                n_kind);
            if (rc != ISC_OK) return rc;
            rc = ec_launch_conv(t1, zero, Wh(c2), Bf(c2), nullptr, t2, slabs, B, ho, wo, p, p, 3, 1, 1, q->ksplit, st,
                                n_kind);
            if (rc != ISC_OK) return rc;
            const float *identity = cur;
            if (i == 0) {
                rc = ec_launch_conv(cur, zero, Wh(cd), Bf(cd), nullptr, idn, slabs, B, h, w, inpl, 4 * p, 1, stride, 0,
                                    q->ksplit, st, n_kind);
                if (rc != ISC_OK) return rc;
                identity = idn;
            }
            rc = ec_launch_conv(t2, zero, Wh(c3), Bf(c3), identity, nxt, slabs, B, ho, wo, p, 4 * p, 1, 1, 1, q->ksplit, st,
                                n_kind);
            if (rc != ISC_OK) return rc;
            float *sw = cur; cur = nxt; nxt = sw;
            ci += i == 0 ? 4 : 3;
            inpl = 4 * p;
            h = ho; w = wo;
        }
    }
    rc = ec_launch_tail(cur, B, h, w, inpl, q->att_size, q->fc, q->att, q->fc_f16, q->att_f16, st);
    if (rc != ISC_OK) return rc;
    ++n_kind[ISC_ENCODER_KIND_TAIL];
    ec_count(n_kind);
    return ISC_OK;
}
