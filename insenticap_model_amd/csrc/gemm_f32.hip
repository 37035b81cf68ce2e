// Grouped, K-segmented GEMM (NT forward, NN / TN backward) with fused epilogues, on two engines:
//   * fp32 MFMA (v_mfma_f32_32x32x2_f32): every layout, every size (tile kernels below);
//   * split-f16 (v_mfma_f32_32x32x16_f16 on hi/lo f16 planes of the fp32 operands, fp32 accumulators): forward and
//     backward launches alike - the large tiles gemm_h3_kernel (128 x 128) / gemm_h3x_kernel (256 x 128) /
//     gemm_h3m_kernel (64 x 128), the skinny tiles gemm_h3s_kernel (32 x 32, 64 x 64, 32 x 128 vocabulary; K split over
//     the waves of a workgroup and, for long contractions, over workgroups), h3_split_kernel for the weight planes
//     (and both operands of the TN layout); dispatch in h3s_plan / h3_plan / try_h3_tn further down.
//
//   acc[M,N] = sum_s A_s[M,K_s] * W_s[N,K_s]^T          (s = up to 4 K-segments)
//
// K-segments replace the reference's torch.cat([...],1) in front of nn.LSTMCell / nn.Linear
// (captioner.py:174,180 and the three summed projections of :107-110): no concatenated
// activation buffer and no packed weight copy is ever materialised - every segment reads the
// caller's tensors where they live.  Up to 3 independent problems share one launch.
//
// The fp32 engine, 256-thread workgroups = 4 wavefronts of 64; each wave owns 32 x 32 accumulator fragments built from
// 32x32x2 fp32 MFMAs (exact fp32 FMA chains, so the result matches an fp32 CPU GEMM to rounding-order noise -
// bf16/TF32-like paths would break the 1e-4 log-prob parity bound).  K is consumed in 32-wide chunks, one barrier per
// chunk, by two families of tile kernels:
//   * gemm_kernel, register-staged, every layout (NT / NN / TN): global -> registers -> LDS (double buffered, rows
//     padded to 36 floats so that the ds_read_b128 fragment reads are bank-conflict free); the finished tile is staged
//     through LDS once so that every epilogue sees (row, col) coordinates and writes full, coalesced rows.
//       L: 128 x 128 (4 waves stacked in M, TN=4)  - batch-sized problems
//       M:  64 x 128 (2 x 2 waves, TN=2)
//       S:  32 x 128 (4 waves side by side in N)   - small-M problems (beam rows, B<=128)
//   * the LDS-DMA tiles, NT layout only: global -> LDS by global_load_lds_dwordx4 into XOR-swizzled buffers, epilogues
//     straight from the accumulator registers.  One body (f32_dma_tile_body) under three geometries (F32Geom):
//       XL: 256 x 128 (gemm_xl_kernel, 3-deep ring),  LD: 128 x 128 (gemm_ld_kernel),  MD: 64 x 128 (gemm_md_kernel,
//       linear epilogue only).
// Small-M problems also have deterministic split-K (splitk_*_kernel) and a GEMV form (gemv_rows_kernel) further down.
//
// Epilogues, one definition each: epi_linear_finish (a float4 group or one element of a reduced tile), epi_linear_frag /
// epi_vocab_frag (straight from accumulator registers, over the fragment layouts Frag32 / Frag16), wave_vocab_tile128
// (one row's 128-column tile on one wave), lstm_cells around isc_lstm_cell (epi_lstm_frag16 keeps a copy of its own).  The
// split-f16 number format, its plane layout and the cell's arithmetic are in common.h.
#include <atomic>
#include <mutex>
#include <type_traits>
#include <utility>

#include "common.h"

typedef float f32x16 __attribute__((ext_vector_type(16)));

// compile-time indices for the kernels' unrolled pipelines (LDS buffers, fragment sets, DMA pieces)
using I0 = std::integral_constant<int, 0>;
using I1 = std::integral_constant<int, 1>;
using I2 = std::integral_constant<int, 2>;
using I3 = std::integral_constant<int, 3>;
// f(integral_constant<int, 0>{}) ... f(integral_constant<int, N - 1>{}): a loop whose index stays a constant expression.
// Not a `#pragma unroll` loop: where the compiler declines to unroll one (it did around the six-case linear epilogue of
// gemm_xl_kernel<0>), a register array indexed by the loop variable - the accumulators - goes to scratch.
template <class F, int... Is>
__device__ __forceinline__ void static_for_seq(F &&f, std::integer_sequence<int, Is...>) {
    (f(std::integral_constant<int, Is>{}), ...);
}
template <int N, class F>
__device__ __forceinline__ void static_for(F &&f) {
    static_for_seq(f, std::make_integer_sequence<int, N>{});
}

#define BK 32
#define LDT 36  // padded LDS row (floats): 36*r mod 64 is a distinct multiple of 4 for 16 rows

enum { EPI_LINEAR = 0, EPI_LSTM = 1, EPI_VOCAB = 2 };

struct DevSeg {
    const float *A;
    const float *W;
    int lda, ldw, K, a_f16;           // a_f16: A points at _Float16 rows, lda in halfs (isc_seg.a_f16)
    const _Float16 *A_hi, *A_lo;      // caller-provided planes of A ([M,K] contiguous) or null
};

struct DevASeg {                      // one K-segment of the split-f16 A operand
    const _Float16 *hi, *lo;
    int ld, K;                        // ld = row stride in halfs = 2 * K of the tensor the planes belong to
};

struct DevProb {
    DevSeg seg[ISC_MAX_SEG];
    int nseg, M, N, relu;
    const float *bias0, *bias1, *bias2;
    const uint8_t *mask;
    float mask_scale;
    int ldc, accumulate;
    int pre_div;                      // lstm: > 1: `pre` holds one row per pre_div rows (isc_lstm_problem.pre_div)
    float *C, *C_pre;
    // lstm
    const float *c_prev;
    float *h_out, *c_out, *gates_out, *hdrop;
    const uint8_t *hmask;
    const float *pre, *tab;
    const int64_t *tab_ids;
    long long tab_ids_stride;
    int H, m_fastest;
    // vocab
    float *pmax, *psum;
    int *pidx;
    long long ld_logits;
    int tiles_m, tiles_n, tile_start, ntile_total, grp_n;
    // split-K (small-M problems): workgroup (tile, ks) contracts chunk range ks and writes its raw
    // partial tile to slab[ks]; a second kernel sums the slabs in order and applies the epilogue
    int ksplit;
    float *slab;
    long long slab_stride;
    // split-f16 path (gemm_h3_kernel): W planes of the K-concatenated weights [N, Kp]; A planes by segment (either one
    // packed segment built by the split kernel, or the caller's per-tensor planes)
    const _Float16 *Wh, *Wl;
    DevASeg ap[ISC_MAX_SEG];
    int nap, Kp;
    _Float16 *h_hi, *h_lo;            // LSTM epilogue: planes of h_out for the consumers
};

struct DevLaunch {
    DevProb p[3];
    int nprob, total_tiles;
    const int *gate;            // optional: *gate == 0 -> the launch returns at once (isc_set_stream_gate; forward entry points)
};

// Operand layouts. "k-minor": element (row, k) at ptr[row*ld + k] (contraction index contiguous;
// activations [M,K] and nn.Linear weights [N,K] in the forward pass).  "k-major": element (row, k)
// at ptr[k*ld + row] - the operand is read through its transpose, which is how the backward pass
// consumes them: dX = dY * W uses W [K=N_out, N=K_in] as a k-major B operand ("NN"), and
// dW = dY^T * X contracts over the batch rows with both operands k-major ("TN").
template <int ROWS, bool KM>
struct Tile {
    // LDS footprint (floats) of one [ROWS x 32] operand tile
    static constexpr int SIZE = KM ? BK * (ROWS + 4) : ROWS * LDT;
    static constexpr int NLD = ROWS / 32;  // float4 loads per thread per chunk
};

// Logical tile -> (problem, tm, tn, k-split slice).  XCD-aware order: blocks with equal blockIdx%8 share
// an XCD (and its L2); give each XCD one contiguous run of logical tiles so that neighbours re-use
// A / W panels from L2.
__device__ __forceinline__ void map_tile(const DevLaunch &L, int &pi, int &tm, int &tn, int &ks, int &ksplit) {
    int logical;
    {
        const int nt = L.total_tiles, bid = blockIdx.x;
        const int q = nt >> 3, r = nt & 7, xcd = bid & 7, j = bid >> 3;
        logical = (xcd < r ? xcd * (q + 1) : r * (q + 1) + (xcd - r) * q) + j;
    }
    pi = 0;
    if (L.nprob > 1 && logical >= L.p[1].tile_start) pi = 1;
    if (L.nprob > 2 && logical >= L.p[2].tile_start) pi = 2;
    const DevProb &P = L.p[pi];
    int t = logical - P.tile_start;
    ksplit = P.ksplit > 1 ? P.ksplit : 1;
    ks = t % ksplit;
    t /= ksplit;
    if (P.m_fastest) {
        // weights are the larger operand: split the N tiles into 8 groups (one per XCD run) so that a
        // group's weight slice stays resident in that XCD's 4 MB L2 while the activations stream
        // through once: inside a group tm is the outer index and tn the inner one.
        const int per_grp = P.grp_n * P.tiles_m;
        const int g = t / per_grp, r = t - g * per_grp;
        const int rest = P.tiles_n - g * P.grp_n;
        const int gn = rest < P.grp_n ? rest : P.grp_n;
        tm = r / gn;
        tn = g * P.grp_n + (r - tm * gn);
    } else {
        tm = t / P.tiles_n;
        tn = t % P.tiles_n;
    }
}

// ---- epilogues, shared by the tile shapes ---------------------------------------------------------
// Where the accumulators of a wave's 32-row fragment sit, for the two MFMA shapes in use.  A lane holds NR rows x NC
// column blocks of CW columns; element (e, j) is tile row frow0 + row(e, lane), tile column fcol0 + CW j + col(lane).
// The lanes that share a row (equal row(e, .)) reduce over it with row_sum / row_reduce.
typedef float f32x4 __attribute__((ext_vector_type(4)));
// v_mfma_f32_32x32x*: f32x16 acc[NC]; one register index is one output row per half-wave, and the row's 32 NC columns
// sit on the 32 lanes of that half - reductions are 4 DPP steps inside the 16-lane rows + one swizzle across them.
struct Frag32 {
    static constexpr int CW = 32, NR = 16;
    static __device__ __forceinline__ int col(int lane) { return lane & 31; }
    static __device__ __forceinline__ int row(int e, int lane) { return (e & 3) + 8 * (e >> 2) + 4 * (lane >> 5); }
    template <int NC>
    static __device__ __forceinline__ float get(const f32x16 (&acc)[NC], int e, int j) { return acc[j][e]; }
    template <int NC>
    static __device__ __forceinline__ void set(f32x16 (&acc)[NC], int e, int j, float v) { acc[j][e] = v; }
    static __device__ __forceinline__ float row_sum(float v) { return half_sum(v); }
    template <class T, class Op>
    static __device__ __forceinline__ T row_reduce(T v, Op op) { return half_reduce(v, op); }
};
// v_mfma_f32_16x16x32_f16 (the large split-f16 tiles): f32x4 acc[2][NC], 2 row blocks x NC column blocks of 16 x 16; a
// row's 16 NC columns sit on the 16 lanes of ONE DPP row - reductions are four DPP steps, no swizzle.
struct Frag16 {
    static constexpr int CW = 16, NR = 8;
    static __device__ __forceinline__ int col(int lane) { return lane & 15; }
    static __device__ __forceinline__ int row(int e, int lane) { return (e >> 2) * 16 + 4 * (lane >> 4) + (e & 3); }
    template <int NC>
    static __device__ __forceinline__ float get(const f32x4 (&acc)[2][NC], int e, int j) { return acc[e >> 2][j][e & 3]; }
    template <int NC>
    static __device__ __forceinline__ void set(f32x4 (&acc)[2][NC], int e, int j, float v) { acc[e >> 2][j][e & 3] = v; }
    static __device__ __forceinline__ float row_sum(float v) { return row16_sum(v); }
    template <class T, class Op>
    static __device__ __forceinline__ T row_reduce(T v, Op op) { return row16_reduce(v, op); }
};

// Vocabulary epilogue of one fragment (layout F, NC column blocks), straight from the registers (no LDS round trip).
// Per row: max / arg-max / sum exp(x - max) over the wave's CW * NC columns.  frow0 = tile-relative first row of the
// fragment, fcol0 = tile-relative first column.  WN == 1 (the wave spans the 128-column tile) writes the tile
// statistics directly, otherwise they go to smx/ssm/six[wn][BM] for the cross-wave combine.
// Straight-line code but for the guards of the stores.  EDGE = false: every column of the fragment is inside N, and the
// column-validity selects (cok) fold away - only the last column tile of a launch pays them.
// The arg-max is the one of `if (x > m) { m = x; i = column; }` over ascending columns: the smallest column among
// the `==`-equal maxima, never a NaN, and the bits of THAT element (a row whose maxima are +0 and -0 reports the sign
// of the first).  In a lane it is that chain, as selects; across the lanes of a row it is three integer reductions -
// the maximum of the lanes' maxima as ordered keys, the smallest index among the lanes that hold it, the bits of the
// lane that has this index (every other lane contributes 0; in a row of -inf / NaN alone every lane holds -inf and the
// index 2^31 - 1) - of one DPP-operand instruction per step, where a (value, index) butterfly compares and selects
// three times per step.  (Integer, because fmaxf on a lane exchange's result first quiets both operands.)
template <bool EDGE, class F, int NC, int WN, int BM, class Acc>
__device__ __forceinline__ void epi_vocab_frag_cols(const DevProb &P, Acc &acc, int frow0, int fcol0, int wn, int lane,
                                                    int row0, int col0, int tn, float *smem) {
    constexpr int NR = F::NR, NONE = 0x7fffffff;
    const int M = P.M, N = P.N, gn0 = col0 + fcol0 + F::col(lane);
    float bv[NC];
    bool cok[NC];
#pragma unroll
    for (int j = 0; j < NC; ++j) {
        cok[j] = !EDGE || gn0 + j * F::CW < N;
        bv[j] = P.bias0[cok[j] ? gn0 + j * F::CW : N - 1];                   // (a padded column's logit is -inf below)
    }
    // Phased over the fragment's rows: the dependent reduction chains of the rows interleave.
    float mx[NR], sm[NR];
    int ix[NR];
#pragma unroll
    for (int e = 0; e < NR; ++e) {
        float m = -INFINITY;
        int i = NONE;
#pragma unroll
        for (int j = 0; j < NC; ++j) {
            const float x = cok[j] ? F::get(acc, e, j) + bv[j] : -INFINITY;
            F::set(acc, e, j, x);                                            // acc now holds the logits
            const bool gt = x > m;                                           // j ascending => smaller column wins ties
            m = gt ? x : m;
            i = gt ? gn0 + j * F::CW : i;
        }
        mx[e] = m;
        ix[e] = i;
    }
    if (P.C) {
#pragma unroll
        for (int e = 0; e < NR; ++e) {
            const int gm = row0 + frow0 + F::row(e, lane);
            if (gm < M) {
                float *crow = P.C + (long long)gm * P.ld_logits + gn0;
#pragma unroll
                for (int j = 0; j < NC; ++j)
                    if (cok[j]) crow[j * F::CW] = F::get(acc, e, j);
            }
        }
    }
    {
        // a lane's maximum (never a NaN) as the int that orders as the float does; -0 counts as +0, as `==` has it
        const auto key = [](float v) {
            const int b = __float_as_int(v + 0.f);
            return b ^ ((b >> 31) & 0x7fffffff);
        };
        const auto imax_ = [](int a, int b) { return a > b ? a : b; };
        const auto imin_ = [](int a, int b) { return a < b ? a : b; };
        const auto or_ = [](int a, int b) { return a | b; };
#pragma unroll
        for (int e = 0; e < NR; ++e) {
            const int mine = ix[e], own = key(mx[e]), top = F::row_reduce(own, imax_);
            ix[e] = F::row_reduce(own == top ? mine : NONE, imin_);
            mx[e] = __int_as_float(F::row_reduce(mine == ix[e] ? __float_as_int(mx[e]) : 0, or_));
        }
    }
#pragma unroll
    for (int e = 0; e < NR; ++e) {
        sm[e] = 0.f;
#pragma unroll
        for (int j = 0; j < NC; ++j) sm[e] += cok[j] ? __expf(F::get(acc, e, j) - mx[e]) : 0.f;   // padded columns add 0
    }
#pragma unroll
    for (int e = 0; e < NR; ++e) sm[e] = F::row_sum(sm[e]);
    if (F::col(lane) == 0) {
#pragma unroll
        for (int e = 0; e < NR; ++e) {
            const int row = frow0 + F::row(e, lane);
            if constexpr (WN == 1) {
                if (row0 + row < M) {
                    const long long o = (long long)(row0 + row) * P.ntile_total + tn;
                    P.pmax[o] = mx[e];
                    P.psum[o] = sm[e];
                    P.pidx[o] = ix[e];
                }
            } else {
                float *smx = smem, *ssm = smem + WN * BM;                     // [WN][BM] each
                int *six = reinterpret_cast<int *>(smem + 2 * WN * BM);
                smx[wn * BM + row] = mx[e];
                ssm[wn * BM + row] = sm[e];
                six[wn * BM + row] = ix[e];
            }
        }
    }
}

template <class F, int NC, int WN, int BM, class Acc>
__device__ __forceinline__ void epi_vocab_frag(const DevProb &P, Acc &acc, int frow0, int fcol0, int wn, int lane,
                                               int row0, int col0, int tn, float *smem) {
    if (col0 + fcol0 + F::CW * NC <= P.N)                                     // (uniform over the wave)
        epi_vocab_frag_cols<false, F, NC, WN, BM>(P, acc, frow0, fcol0, wn, lane, row0, col0, tn, smem);
    else
        epi_vocab_frag_cols<true, F, NC, WN, BM>(P, acc, frow0, fcol0, wn, lane, row0, col0, tn, smem);
}

// accumulator fragment -> Cs[BM][LDC] (row-major tile image in LDS)
template <int TN>
__device__ __forceinline__ void epi_stage_frag(float *Cs, int LDC, f32x16 (&acc)[TN], int frow0, int fcol0, int lane) {
#pragma unroll
    for (int j = 0; j < TN; ++j)
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            const int row = frow0 + Frag32::row(r, lane);
            const int col = fcol0 + j * 32 + Frag32::col(lane);
            Cs[row * LDC + col] = acc[j][r];
        }
}

// The linear epilogue of NE (4 or 1) consecutive outputs (gm, gn .. gn + NE - 1) whose contraction sums are o[]: three
// biases, accumulate, ReLU, pre-mask copy, keep-mask, store - one float4 per group where the row stride and the matrix
// border allow.  The one definition behind the staged tiles, the skinny tiles, the split-K reduction and the GEMV tail.
template <int NE>
__device__ __forceinline__ void epi_linear_finish(const DevProb &P, int gm, int gn, float (&o)[NE]) {
    static_assert(NE == 4 || NE == 1, "a float4 group or one element");
    const int N = P.N;
    float pre[NE];
#pragma unroll
    for (int e = 0; e < NE; ++e) {
        const int n = gn + e;
        pre[e] = 0.f;
        if (n < N) {
            if (P.bias0) o[e] += P.bias0[n];
            if (P.bias1) o[e] += P.bias1[n];
            if (P.bias2) o[e] += P.bias2[n];
            if (P.accumulate) o[e] += P.C[(long long)gm * P.ldc + n];
            if (P.relu) o[e] = isc_relu(o[e]);
            pre[e] = o[e];
            if (P.mask) o[e] = o[e] * (float)P.mask[(long long)gm * N + n] * P.mask_scale;
        }
    }
    float *dst = P.C + (long long)gm * P.ldc + gn;
    if constexpr (NE == 4) {
        if ((P.ldc & 3) == 0 && gn + 3 < N) {
            *reinterpret_cast<float4 *>(dst) = make_float4(o[0], o[1], o[2], o[3]);
            if (P.C_pre)
                *reinterpret_cast<float4 *>(P.C_pre + (long long)gm * P.ldc + gn) =
                    make_float4(pre[0], pre[1], pre[2], pre[3]);
            return;
        }
    }
    for (int e = 0; e < NE && gn + e < N; ++e) {
        dst[e] = o[e];
        if (P.C_pre) P.C_pre[(long long)gm * P.ldc + gn + e] = pre[e];
    }
}

template <int BM, int BN>
__device__ __forceinline__ void epi_linear_tile(const DevProb &P, const float *Cs, int row0, int col0, int tid,
                                                int ks, int ksplit) {
    constexpr int LDC = BN + 4;
    const int M = P.M, N = P.N;
    if (ksplit > 1) {      // raw partial tile -> slab[ks] ([M,N], ld = N, N % 4 == 0)
        float *slab = P.slab + (long long)ks * P.slab_stride;
        for (int idx = tid; idx < BM * (BN / 4); idx += 256) {
            const int row = idx / (BN / 4), c4 = (idx % (BN / 4)) * 4;
            const int gm = row0 + row, gn = col0 + c4;
            if (gm < M && gn < N)
                *reinterpret_cast<float4 *>(slab + (long long)gm * N + gn) =
                    *reinterpret_cast<const float4 *>(Cs + row * LDC + c4);
        }
        return;
    }
    for (int idx = tid; idx < BM * (BN / 4); idx += 256) {
        const int row = idx / (BN / 4), c4 = (idx % (BN / 4)) * 4;
        const int gm = row0 + row, gn = col0 + c4;
        if (gm >= M || gn >= N) continue;
        const float4 v = *reinterpret_cast<const float4 *>(Cs + row * LDC + c4);
        float o[4] = {v.x, v.y, v.z, v.w};
        epi_linear_finish<4>(P, gm, gn, o);
    }
}

// LSTM cell update (isc_lstm_cell, common.h) from the four gate pre-activations of NE (row, unit) elements.
// The epilogue's global operands - hoisted `pre` term, embedding-table row (behind its token id),
// c_prev - are fetched for all NE elements BEFORE any arithmetic: issued element by element inside the
// compute loop they formed NE serial dependent round trips (att-LSTM at B=4096: +24 us per launch).
template <int NE>
__device__ __forceinline__ void lstm_cells(const DevProb &P, const int (&gm)[NE], int unit, const bool (&ok)[NE],
                                           float (&g)[NE][4]) {
    const int H = P.H;
    const bool has_b = P.bias0 != nullptr, has_pre = P.pre != nullptr, has_tab = P.tab != nullptr;
    float q[NE][4], t[NE][4], b[4], cp[NE];
    long long tok[NE];
    if (has_tab) {
#pragma unroll
        for (int e = 0; e < NE; ++e) tok[e] = ok[e] ? P.tab_ids[(long long)gm[e] * P.tab_ids_stride] : 0;
    }
#pragma unroll
    for (int e = 0; e < NE; ++e) cp[e] = ok[e] ? P.c_prev[(long long)gm[e] * H + unit] : 0.f;
    if (has_pre && P.pre_div > 1) {      // one row of `pre` per image (uniform branch; one division per row)
#pragma unroll
        for (int e = 0; e < NE; ++e) {
            const long long pm = ok[e] ? (unsigned)gm[e] / (unsigned)P.pre_div : 0;
#pragma unroll
            for (int k = 0; k < 4; ++k) q[e][k] = ok[e] ? P.pre[pm * 4 * H + k * H + unit] : 0.f;
        }
    } else if (has_pre) {
#pragma unroll
        for (int e = 0; e < NE; ++e)
#pragma unroll
            for (int k = 0; k < 4; ++k) q[e][k] = ok[e] ? P.pre[(long long)gm[e] * 4 * H + k * H + unit] : 0.f;
    }
    if (has_tab) {
#pragma unroll
        for (int e = 0; e < NE; ++e)
#pragma unroll
            for (int k = 0; k < 4; ++k) t[e][k] = ok[e] ? P.tab[tok[e] * 4 * H + k * H + unit] : 0.f;
    }
    if (has_b) {
#pragma unroll
        for (int k = 0; k < 4; ++k) b[k] = P.bias0[k * H + unit] + P.bias1[k * H + unit];
    }
#pragma unroll
    for (int e = 0; e < NE; ++e) {
#pragma unroll
        for (int k = 0; k < 4; ++k) g[e][k] = isc_lstm_gate_sum(g[e][k], has_b, b[k], has_pre, q[e][k], has_tab, t[e][k]);
        float c2, h2;
        isc_lstm_cell(g[e], cp[e], c2, h2);
        if (ok[e]) {
            const long long o = (long long)gm[e] * H + unit;
            P.c_out[o] = c2;
            P.h_out[o] = h2;
            if (P.h_hi) {
                const long long po = plane_index(gm[e], unit, H);
                isc_split_f16(h2, P.h_hi[po], P.h_lo[po]);
            }
            if (P.hmask) P.hdrop[o] = h2 * (float)P.hmask[o] * P.mask_scale;
            if (P.gates_out) {
                float *go_ = P.gates_out + (long long)gm[e] * 4 * H + unit;
#pragma unroll
                for (int k = 0; k < 4; ++k) go_[k * H] = g[e][k];
            }
        }
    }
}

// gate-interleaved tile (columns = 4 gates x 32 units) in LDS -> cells of units tn*32 .. +32.  A thread's
// elements are rows tid/32 + 8*i of ONE unit (tid % 32).
template <int BM, int BN>
__device__ __forceinline__ void epi_lstm_tile(const DevProb &P, const float *Cs, int row0, int tn, int tid) {
    constexpr int LDC = BN + 4, NE = 4;
    static_assert(BM * 32 % (256 * NE) == 0, "tile rows per thread must be a multiple of the batch");
    const int u = tid & 31;
    for (int base = tid; base < BM * 32; base += 256 * NE) {
        int gm[NE];
        bool ok[NE];
        float g[NE][4];
#pragma unroll
        for (int e = 0; e < NE; ++e) {
            const int row = (base + 256 * e) >> 5;
            gm[e] = row0 + row;
            ok[e] = gm[e] < P.M;
            const float *cr = Cs + row * LDC + u;
            g[e][0] = cr[0]; g[e][1] = cr[32]; g[e][2] = cr[64]; g[e][3] = cr[96];
        }
        lstm_cells<NE>(P, gm, tn * 32 + u, ok, g);
    }
}

// The same from a 32 x 128 accumulator fragment (fragment j = gate j, lane&31 = unit; C/D row map): used by
// the XL tile, whose lone workgroup per CU has nobody to hide an LDS round trip behind.
__device__ __forceinline__ void epi_lstm_frag(const DevProb &P, f32x16 (&acc)[4], int frow0, int lane, int row0, int tn) {
#pragma unroll
    for (int half = 0; half < 2; ++half) {
        int gm[8];
        bool ok[8];
        float g[8][4];
#pragma unroll
        for (int e = 0; e < 8; ++e) {
            const int r = half * 8 + e;
            gm[e] = row0 + frow0 + Frag32::row(r, lane);
            ok[e] = gm[e] < P.M;
#pragma unroll
            for (int k = 0; k < 4; ++k) g[e][k] = acc[k][r];
        }
        lstm_cells<8>(P, gm, tn * 32 + (lane & 31), ok, g);
    }
}

// Numerics status (isc_status): word 1 = a split-f16 linear launch that staged CALLER data as fp32 rows (the raw region
// features of the prologue, training-mode activations) produced a non-finite pre-activation - an operand at or beyond the
// f16 range (|x| >= 65520: its hi plane is inf), or a NaN / inf fed in.
ISC_STATUS_DECL(gemm)

// Linear epilogue of one fragment (layout F, NC column blocks starting at tile column fcol0), straight from the
// registers.  EDGE: the fragment touches the matrix border (per-element predicates); FEAT: accumulate / pre-activation
// copy / keep-mask in play; CHECK: flag non-finite pre-activations.  Interior fragments run without per-element
// branches whatever the features.
template <class F, int NC, bool EDGE, bool FEAT, bool RELU, bool CHECK, class Acc>
__device__ __forceinline__ void epi_linear_frag_impl(const DevProb &P, const Acc &acc, int frow0, int fcol0, int lane,
                                                     int row0, int col0) {
    const int M = P.M, N = P.N, gn0 = col0 + fcol0 + F::col(lane);
    float b0[NC], b1[NC], b2[NC];
    bool cok[NC];
    const bool h0 = P.bias0 != nullptr, h1 = P.bias1 != nullptr, h2 = P.bias2 != nullptr;
    const bool f_acc = FEAT && P.accumulate, f_pre = FEAT && P.C_pre != nullptr, f_mask = FEAT && P.mask != nullptr;
    [[maybe_unused]] bool bad = false;
#pragma unroll
    for (int j = 0; j < NC; ++j) {
        const int gn = gn0 + j * F::CW;
        cok[j] = !EDGE || gn < N;
        b0[j] = (h0 && cok[j]) ? P.bias0[gn] : 0.f;
        b1[j] = (h1 && cok[j]) ? P.bias1[gn] : 0.f;
        b2[j] = (h2 && cok[j]) ? P.bias2[gn] : 0.f;
    }
#pragma unroll
    for (int e = 0; e < F::NR; ++e) {
        const int gm = row0 + frow0 + F::row(e, lane);
        if (EDGE && gm >= M) continue;
        float *crow = P.C + (long long)gm * P.ldc + gn0;
        float prev[NC];
        if (f_acc) {                                   // all NC loads of the row before any arithmetic
#pragma unroll
            for (int j = 0; j < NC; ++j) prev[j] = (!EDGE || cok[j]) ? crow[j * F::CW] : 0.f;
        }
#pragma unroll
        for (int j = 0; j < NC; ++j) {
            if (EDGE && !cok[j]) continue;
            float o = F::get(acc, e, j);
            if (h0) o += b0[j];
            if (h1) o += b1[j];
            if (h2) o += b2[j];
            if (f_acc) o += prev[j];
            if constexpr (CHECK) bad |= !(fabsf(o) <= 3.0e38f);
            if (RELU) o = isc_relu(o);
            if constexpr (FEAT) {
                const int gn = gn0 + j * F::CW;
                if (f_pre) P.C_pre[(long long)gm * P.ldc + gn] = o;
                if (f_mask) o = o * (float)P.mask[(long long)gm * N + gn] * P.mask_scale;
            }
            crow[j * F::CW] = o;
        }
    }
    if constexpr (CHECK) {
        if (__any(bad) && lane == 0) isc_flag_gemm(ISC_STATUS_WORD_LINEAR);
    }
}

template <class F, int NC, bool CHECK, class Acc>
__device__ __forceinline__ void epi_linear_frag(const DevProb &P, const Acc &acc, int frow0, int fcol0, int lane,
                                                int row0, int col0) {
    const bool feat = P.accumulate || P.C_pre || P.mask;
    const bool edge = !(row0 + frow0 + 32 <= P.M && col0 + fcol0 + F::CW * NC <= P.N);
    const bool relu = P.relu != 0;
#define ISC_EPI_CASE(E, FT, R) epi_linear_frag_impl<F, NC, E, FT, R, CHECK>(P, acc, frow0, fcol0, lane, row0, col0)
    if (edge) {
        if (relu) ISC_EPI_CASE(true, true, true); else ISC_EPI_CASE(true, true, false);
    } else if (feat) {
        if (relu) ISC_EPI_CASE(false, true, true); else ISC_EPI_CASE(false, true, false);
    } else {
        if (relu) ISC_EPI_CASE(false, false, true); else ISC_EPI_CASE(false, false, false);
    }
#undef ISC_EPI_CASE
}

template <int WM, int WN, int TN, int EPI, bool AKM, bool BKM>
__global__ __launch_bounds__(256) void gemm_kernel(const DevLaunch L) {
    ISC_GATE_RETURN(L);
    rows_kernarg_warm<ROWS_KERNARG_LINES(DevLaunch)>();      // (one batch of scalar loads for the launch descriptor: common.h)
    constexpr int BM = 32 * WM;
    constexpr int BN = 32 * TN * WN;
    constexpr int LDC = BN + 4;
    using TA = Tile<BM, AKM>;
    using TB = Tile<BN, BKM>;
    constexpr int A_LD = TA::NLD, B_LD = TB::NLD;
    extern __shared__ __attribute__((aligned(16))) float smem[];
    float *As = smem;                     // [2][TA::SIZE]
    float *Bs = smem + 2 * TA::SIZE;      // [2][TB::SIZE]
    float *Cs = smem;                     // [BM][LDC] (after the K loop)

    const int tid = threadIdx.x;
    const int lane = tid & 63;
    const int wave = tid >> 6;
    const int wm = wave / WN, wn = wave % WN;

    int pi, tm, tn, ks, ksplit;
    map_tile(L, pi, tm, tn, ks, ksplit);
    const DevProb &P = L.p[pi];
    const int M = P.M, N = P.N;
    const int row0 = tm * BM, col0 = tn * BN;

    // ---- global-load coordinates
    // k-minor tile: thread -> (row = tid/8 + 32*i, k = 4*(tid%8)); k-major tile of ROWS columns:
    // thread -> (k-row = tid/(ROWS/4) + (1024/ROWS)*i, column = 4*(tid % (ROWS/4)))
    const int lr = tid >> 3, lc = (tid & 7) * 4;
    constexpr int A_TPR = BM / 4, B_TPR = BN / 4;           // threads per k-row (k-major)
    const int akr = tid / A_TPR, akc = (tid % A_TPR) * 4;
    const int bkr = tid / B_TPR, bkc = (tid % B_TPR) * 4;
    long long wrow[B_LD];   // k-minor B: weight row of tile row n (LSTM tiles interleave the 4 gates)
    bool wok[B_LD];
#pragma unroll
    for (int i = 0; i < B_LD; ++i) {
        const int n = lr + 32 * i;
        if (EPI == EPI_LSTM) {
            wrow[i] = (long long)(n >> 5) * P.H + tn * 32 + (n & 31);
            wok[i] = true;
        } else {
            wrow[i] = col0 + n;
            wok[i] = (col0 + n) < N;
        }
    }
    bool aok[A_LD];
#pragma unroll
    for (int i = 0; i < A_LD; ++i) aok[i] = (row0 + lr + 32 * i) < M;
    const bool a_col_ok = (row0 + akc) < M;   // k-major A: this thread's 4 output rows exist
    const bool b_col_ok = (col0 + bkc) < N;

    f32x16 acc[TN];
#pragma unroll
    for (int j = 0; j < TN; ++j)
#pragma unroll
        for (int r = 0; r < 16; ++r) acc[j][r] = 0.f;
    int nchunks = 0;
    for (int s = 0; s < P.nseg; ++s) nchunks += (P.seg[s].K + BK - 1) / BK;

    // Per-thread source pointers of the current K-segment, advanced by one chunk per load (keeps the
    // 64-bit address arithmetic out of the loop); `fast` tiles (interior, K % 32 == 0) load unpredicated.
    // One register stage: chunk c+1 waits in it while chunk c is being contracted, is written to the
    // other LDS buffer in the middle of that contraction, and the stage is re-armed with chunk c+2 at
    // once - so a global load has a whole chunk of MFMAs (~4k cycles) to land.
    float4 ra[A_LD], rb[B_LD];
    const float *pa[A_LD], *pb[B_LD];
    long long stepA = BK, stepB = BK;
    int cs = 0, ck = 0, segK = 0;  // segment / k-offset of the chunk being loaded
    auto set_seg = [&](int si) __attribute__((always_inline)) {
        const DevSeg sg = P.seg[si];
        segK = sg.K;
        if constexpr (AKM) {
            stepA = (long long)BK * sg.lda;
#pragma unroll
            for (int i = 0; i < A_LD; ++i)
                pa[i] = sg.A + (long long)(akr + (1024 / BM) * i) * sg.lda + row0 + akc;
        } else {
#pragma unroll
            for (int i = 0; i < A_LD; ++i)
                pa[i] = sg.A + (long long)(row0 + lr + 32 * i) * sg.lda + lc;
        }
        if constexpr (BKM) {
            stepB = (long long)BK * sg.ldw;
#pragma unroll
            for (int i = 0; i < B_LD; ++i)
                pb[i] = sg.W + (long long)(bkr + (1024 / BN) * i) * sg.ldw + col0 + bkc;
        } else {
#pragma unroll
            for (int i = 0; i < B_LD; ++i) pb[i] = sg.W + wrow[i] * sg.ldw + lc;
        }
    };
    auto gload = [&](auto fastc) __attribute__((always_inline)) {
        constexpr bool FAST = decltype(fastc)::value;
#pragma unroll
        for (int i = 0; i < A_LD; ++i) {
            bool ok = true;
            if constexpr (!FAST) {
                if constexpr (AKM) ok = a_col_ok && (ck + akr + (1024 / BM) * i) < segK;
                else ok = aok[i] && (ck + lc) < segK;
            }
            ra[i] = ok ? *reinterpret_cast<const float4 *>(pa[i]) : make_float4(0.f, 0.f, 0.f, 0.f);
            pa[i] += stepA;
        }
#pragma unroll
        for (int i = 0; i < B_LD; ++i) {
            bool ok = true;
            if constexpr (!FAST) {
                if constexpr (BKM) ok = b_col_ok && (ck + bkr + (1024 / BN) * i) < segK;
                else ok = wok[i] && (ck + lc) < segK;
            }
            rb[i] = ok ? *reinterpret_cast<const float4 *>(pb[i]) : make_float4(0.f, 0.f, 0.f, 0.f);
            pb[i] += stepB;
        }
        ck += BK;
        if (ck >= segK) {
            ck = 0;
            if (++cs < P.nseg) set_seg(cs);
        }
    };
    auto sstore = [&](auto bufc) __attribute__((always_inline)) {
        constexpr int BUF = decltype(bufc)::value;
        float *a = As + BUF * TA::SIZE;
        if constexpr (AKM) {
#pragma unroll
            for (int i = 0; i < A_LD; ++i)
                *reinterpret_cast<float4 *>(a + (akr + (1024 / BM) * i) * (BM + 4) + akc) = ra[i];
        } else {
#pragma unroll
            for (int i = 0; i < A_LD; ++i)
                *reinterpret_cast<float4 *>(a + (lr + 32 * i) * LDT + lc) = ra[i];
        }
        float *b = Bs + BUF * TB::SIZE;
        if constexpr (BKM) {
#pragma unroll
            for (int i = 0; i < B_LD; ++i)
                *reinterpret_cast<float4 *>(b + (bkr + (1024 / BN) * i) * (BN + 4) + bkc) = rb[i];
        } else {
#pragma unroll
            for (int i = 0; i < B_LD; ++i)
                *reinterpret_cast<float4 *>(b + (lr + 32 * i) * LDT + lc) = rb[i];
        }
    };

    // MFMA 32x32x2 operand maps: lane l supplies A[i = l&31][k = l>>5] and B[k = l>>5][j = l&31].
    // Per 8-deep k-block a lane holds 4 consecutive k (k0 + 4*(l>>5) + t) of its row for both
    // operands; MFMA t consumes element t, so every k is covered exactly once.
    // Two fragment register sets: while the MFMAs of k-block kb run from one set, the fragments of
    // kb+1 (or of the next chunk's first k-block, after the barrier) are read into the other, so the
    // matrix pipe never waits for an LDS round trip - not even across a chunk boundary.
    static_assert(BK == 32, "the chunk body below is written for 4 k-blocks of 8");
    const int frow = lane & 31, fk = (lane >> 5) * 4;
    float fa[2][4], fb[2][TN][4];
    auto lfrag = [&](auto bufc, auto kbc, auto setc) __attribute__((always_inline)) {
        constexpr int BUF = decltype(bufc)::value, kb = decltype(kbc)::value, ST = decltype(setc)::value;
        const float *at = As + BUF * TA::SIZE;
        const float *bt = Bs + BUF * TB::SIZE;
        if constexpr (AKM) {
#pragma unroll
            for (int e = 0; e < 4; ++e) fa[ST][e] = at[(kb * 8 + fk + e) * (BM + 4) + wm * 32 + frow];
        } else {
            const float4 v = *reinterpret_cast<const float4 *>(at + (wm * 32 + frow) * LDT + kb * 8 + fk);
            fa[ST][0] = v.x; fa[ST][1] = v.y; fa[ST][2] = v.z; fa[ST][3] = v.w;
        }
#pragma unroll
        for (int j = 0; j < TN; ++j) {
            if constexpr (BKM) {
#pragma unroll
                for (int e = 0; e < 4; ++e)
                    fb[ST][j][e] = bt[(kb * 8 + fk + e) * (BN + 4) + (wn * TN + j) * 32 + frow];
            } else {
                const float4 v = *reinterpret_cast<const float4 *>(
                    bt + ((wn * TN + j) * 32 + frow) * LDT + kb * 8 + fk);
                fb[ST][j][0] = v.x; fb[ST][j][1] = v.y; fb[ST][j][2] = v.z; fb[ST][j][3] = v.w;
            }
        }
    };
    auto mma = [&](auto setc) __attribute__((always_inline)) {
        constexpr int ST = decltype(setc)::value;
#pragma unroll
        for (int e = 0; e < 4; ++e)
#pragma unroll
            for (int j = 0; j < TN; ++j)
                acc[j] = __builtin_amdgcn_mfma_f32_32x32x2f32(fa[ST][e], fb[ST][j][e], acc[j], 0, 0, 0);
    };
    // split-K: this workgroup's chunk range [c_lo, c_lo + nchunks) of the problem's chunk sequence
    int c_lo = 0;
    if (ksplit > 1) {
        const int cps = (nchunks + ksplit - 1) / ksplit;
        c_lo = ks * cps;
        int mine = nchunks - c_lo;
        nchunks = mine < 0 ? 0 : (mine < cps ? mine : cps);
    }
    // One chunk: LDS[CUR] holds it and fragment set 0 its first k-block; the register stage holds
    // chunk c+1 (if any).  Exactly one barrier per chunk, placed in front of the last k-block's MFMAs.
    auto chunk_body = [&](auto curc, auto nxtc, auto fastc, bool has1, bool has2) __attribute__((always_inline)) {
        lfrag(curc, I1{}, I1{});
        mma(I0{});
        if (has1) {
            sstore(nxtc);                 // LDS[NXT] was last read before the previous chunk's barrier
            if (has2) gload(fastc);
        }
        lfrag(curc, I2{}, I0{});
        mma(I1{});
        lfrag(curc, I3{}, I1{});
        mma(I0{});
        if (has1) {
            __syncthreads();              // every wave's stores of chunk c+1 have landed
            lfrag(nxtc, I0{}, I0{});
        }
        mma(I1{});
    };
    auto k_loop = [&](auto fastc) __attribute__((always_inline)) {
        if (nchunks == 0) return;
        {   // position the loader on chunk c_lo
            int skip = c_lo, si = 0;
            for (; si < P.nseg; ++si) {
                const int sc = (P.seg[si].K + BK - 1) / BK;
                if (skip < sc) break;
                skip -= sc;
            }
            set_seg(si);
            cs = si;
            ck = skip * BK;
#pragma unroll
            for (int i = 0; i < A_LD; ++i) pa[i] += stepA * skip;
#pragma unroll
            for (int i = 0; i < B_LD; ++i) pb[i] += stepB * skip;
        }
        gload(fastc);                             // chunk 0
        sstore(I0{});
        if (nchunks > 1) gload(fastc);            // chunk 1 -> register stage
        __syncthreads();
        lfrag(I0{}, I0{}, I0{});
        for (int c = 0; c < nchunks; c += 2) {
            chunk_body(I0{}, I1{}, fastc, c + 1 < nchunks, c + 2 < nchunks);
            if (c + 1 < nchunks) chunk_body(I1{}, I0{}, fastc, c + 2 < nchunks, c + 3 < nchunks);
        }
        __syncthreads();                          // the epilogue re-uses the operand buffers
    };
    bool fast = (row0 + BM <= M) && (EPI == EPI_LSTM || col0 + BN <= N);
    for (int si = 0; si < P.nseg; ++si) fast = fast && (P.seg[si].K % BK) == 0;
    if (fast) k_loop(std::true_type{});
    else k_loop(std::false_type{});

    if constexpr (EPI == EPI_VOCAB) {
        epi_vocab_frag<Frag32, TN, WN, BM>(P, acc, wm * 32, wn * TN * 32, wn, lane, row0, col0, tn, smem);
        if constexpr (WN > 1) {
            float *smx = smem;
            float *ssm = smem + WN * BM;
            int *six = reinterpret_cast<int *>(smem + 2 * WN * BM);
            __syncthreads();
            for (int row = tid; row < BM; row += 256) {
                const int gm = row0 + row;
                if (gm >= M) continue;
                float mx = smx[row];
                int ix = six[row];
#pragma unroll
                for (int w = 1; w < WN; ++w) {
                    const float ov = smx[w * BM + row];
                    const int oi = six[w * BM + row];
                    if (ov > mx || (ov == mx && oi < ix)) { mx = ov; ix = oi; }
                }
                float sm = 0.f;
#pragma unroll
                for (int w = 0; w < WN; ++w) {
                    const float wm_ = smx[w * BM + row];          // -inf: that wave had no valid column
                    if (wm_ > -INFINITY) sm += ssm[w * BM + row] * __expf(wm_ - mx);
                }
                const long long o = (long long)gm * P.ntile_total + tn;
                P.pmax[o] = mx;
                P.psum[o] = sm;
                P.pidx[o] = ix;
            }
        }
        return;
    }

    epi_stage_frag<TN>(Cs, LDC, acc, wm * 32, wn * TN * 32, lane);
    __syncthreads();
    if (EPI == EPI_LINEAR) epi_linear_tile<BM, BN>(P, Cs, row0, col0, tid, ks, ksplit);
    else if (EPI == EPI_LSTM) epi_lstm_tile<BM, BN>(P, Cs, row0, tn, tid);
}

// ---------------------------------------------------------------- LDS-DMA tiles (NT layout): XL 256 x 128, LD 128 x 128, MD 64 x 128
// Geometry of an fp32 LDS-DMA tile kernel: WM x WN waves, each owning FM x TN accumulator fragments of 32 x 32; NBUF LDS
// buffers in a ring with NBUF - 1 chunks of DMA in flight; PER staging pieces of the chunk NBUF - 1 ahead are issued
// after each MFMA group (one MFMA per accumulator fragment) of k-blocks 0 - 2.  Everything else follows from these.
template <int WM_, int WN_, int FM_, int TN_, int NBUF_, int PER_>
struct F32Geom {
    static constexpr int WM = WM_, WN = WN_, FM = FM_, TN = TN_, NBUF = NBUF_, PER = PER_, AHEAD = NBUF_ - 1;
    static constexpr int BM = 32 * FM * WM, BN = 32 * TN * WN;
    static constexpr int TSA = BM * BK, TSB = BN * BK;           // floats per A / W buffer
    static constexpr int LDS_BYTES = NBUF * (TSA + TSB) * (int)sizeof(float);
    static constexpr int NW = WM * WN, THREADS = 64 * NW;
    static constexpr int APW = BM / 8 / NW, BPW = BN / 8 / NW;   // 8-row staging pieces of A / of W a wave issues
    static constexpr int DMAS = APW + BPW;                       // LDS-DMA instructions per wave and chunk
    static constexpr int WAIT = (NBUF - 2) * DMAS;               // the steady-state vmcnt in front of the barrier: the
                                                                 // largest immediate dma_wait_stages<AHEAD - 1, DMAS> emits
    static_assert(THREADS == 256 && NBUF >= 2, "four waves, at least a double buffer");
    static_assert(APW * 8 * NW == BM && BPW * 8 * NW == BN, "the staging pieces divide evenly over the waves");
    static_assert(APW % 2 == 0 && BPW % 2 == 0, "piece parity = bit 2 of the swizzle's (row >> 1) & 7");
    static_assert(DMAS % PER == 0 && DMAS <= PER * 12, "a chunk's pieces fit behind the MFMA groups of k-blocks 0 - 2");
    static_assert(WAIT < 64, "vmcnt range");
};
// XL, for batch-sized problems: each wave owns a 64 x 128 accumulator (2 x 4 fragments, 128 AGPRs) - twice the MFMAs
// per staged byte of the 128 x 128 tile.  144 KB of LDS = one workgroup per CU, which has to cover its own DMA round
// trips: a 3-deep ring keeps chunk c+2 in flight while chunk c is contracted, so only a counted vmcnt (never 0 in
// steady state) precedes the barrier, and the 12 pieces of a chunk go out one by one in the shadow of 8-MFMA groups.
using F32TileXL = F32Geom<4, 1, 2, 4, 3, 1>;
// LD: the L tile's geometry (4 waves stacked in M, 32 x 128 accumulator each) without its register stage and ds_write
// pass (~9 % of the register-staged loop).  64 KB of LDS keep two workgroups on a CU, so an epilogue-heavy kernel -
// the vocabulary projection: 16 chunks of MFMAs, then per-row softmax statistics - still has a neighbour to hide its
// epilogue behind, which the XL tile does not.  Chunk c+1's eight pieces per wave are issued inside k-block 0 of
// chunk c and retired with vmcnt(0).
using F32TileLD = F32Geom<4, 1, 1, 4, 2, 2>;
// MD: the LD scheme on the M geometry (2 x 2 waves, 32 x 64 accumulator each; linear epilogue) for the per-step
// projections with N = 512: their 64-row tiles are what balances 4096 x 512 outputs over 256 CUs, and at one to three
// workgroups per CU the register-staged form of that tile leaves the matrix pipe idle over its chunk-boundary round
// trips.
using F32TileMD = F32Geom<2, 2, 1, 2, 2, 2>;

// s_waitcnt vmcnt that leaves the youngest `in_flight` (at most MAXF) stages of DMAS instructions outstanding; the
// immediates are compile-time
template <int MAXF, int DMAS>
__device__ __forceinline__ void dma_wait_stages(int in_flight) {
    if constexpr (MAXF == 0) asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    else if (in_flight >= MAXF) asm volatile("s_waitcnt vmcnt(%0)" :: "n"(MAXF * DMAS) : "memory");
    else dma_wait_stages<MAXF - 1, DMAS>(in_flight);
}

// The body of gemm_xl_kernel / gemm_ld_kernel / gemm_md_kernel (geometry G).
// Operand chunks go global -> LDS by LDS-DMA (global_load_lds_dwordx4: no staging VGPRs, no ds_write pass).  M0 carries
// the LDS destination of an LDS-DMA; it is written in the same asm statement that uses it, with the one wait state the
// ISA asks for between an SALU write of M0 and a memory instruction with the LDS modifier: hipcc's hazard recogniser
// does not look inside inline asm.  An LDS-DMA writes lane-linear (wave-uniform base + 16 B * lane), which rules out
// padded rows: the tile image is [rows][8 slots of 16 B] with slot = k-quad ^ ((row >> 1) & 7), applied to the
// per-lane SOURCE address when staging and to the ds_read_b128 address when reading fragments (conflict-free for the
// instruction's four 16-lane groups).  The DMA is issued from inline asm: the compiler would otherwise drain every
// DMA (vmcnt(0)) in front of the next ds_read.  Ring positions are compile-time (the chunk loop is unrolled NBUF
// times), so every LDS offset is an immediate.
template <class G, int EPI>
__device__ __forceinline__ void f32_dma_tile_body(const DevLaunch &L) {
    constexpr int FM = G::FM, TN = G::TN, TSA = G::TSA, TSB = G::TSB, APW = G::APW, BPW = G::BPW, DMAS = G::DMAS;
    constexpr int NBUF = G::NBUF, AHEAD = G::AHEAD;
    static_assert(EPI == EPI_LINEAR || G::WN == 1, "the LSTM and vocabulary epilogues take the tile's whole rows");
    static_assert(EPI != EPI_LSTM || BPW == 4, "LSTM weight rows: wave w stages the 32 units of gate w");
    static_assert(BK == 32, "chunk body written for 4 k-blocks of 8");
    extern __shared__ __attribute__((aligned(16))) float smem[];
    float *As = smem;                     // [NBUF][TSA]
    float *Bs = smem + NBUF * TSA;        // [NBUF][TSB]

    const int tid = threadIdx.x;
    const int lane = tid & 63;
    const int w = tid >> 6, wm = w / G::WN, wn = w % G::WN;
    int pi, tm, tn, ks, ksplit;
    map_tile(L, pi, tm, tn, ks, ksplit);
    const DevProb &P = L.p[pi];
    const int M = P.M, N = P.N;
    const int row0 = tm * G::BM, col0 = tn * G::BN;

    // staging pieces (8 rows x 128 B each): A piece i of wave w = tile rows 8 (APW w + i) .. +8, W piece i = tile
    // columns 8 (BPW w + i) .. +8; lane -> (row = lane>>3, slot = lane&7).  Rows past the edge re-read the last valid
    // row (their results are never stored).
    int arow[APW];
    long long wrow[BPW];
#pragma unroll
    for (int i = 0; i < APW; ++i) {
        const int r = row0 + 8 * APW * w + 8 * i + (lane >> 3);
        arow[i] = r < M ? r : M - 1;
    }
#pragma unroll
    for (int i = 0; i < BPW; ++i) {
        if (EPI == EPI_LSTM) {
            wrow[i] = (long long)w * P.H + tn * 32 + 8 * i + (lane >> 3);     // gate w, unit tn*32 + ..
        } else {
            const int c = col0 + 8 * BPW * w + 8 * i + (lane >> 3);
            wrow[i] = c < N ? c : N - 1;
        }
    }
    const int lq = lane & 7, lh = lane >> 4;   // (tile row >> 1) & 7 == (4*(i&1) + lh) for both operands
    const float *pa[APW], *pb[BPW];
    int cs = 0, ck = 0, segK = 0;
    auto set_seg = [&](int si) __attribute__((always_inline)) {
        const DevSeg sg = P.seg[si];
        segK = sg.K;
#pragma unroll
        for (int i = 0; i < APW; ++i) pa[i] = sg.A + (long long)arow[i] * sg.lda + (lq ^ (4 * (i & 1) + lh)) * 4;
#pragma unroll
        for (int i = 0; i < BPW; ++i) pb[i] = sg.W + wrow[i] * sg.ldw + (lq ^ (4 * (i & 1) + lh)) * 4;
    };
    const unsigned a_lds0 = __builtin_amdgcn_readfirstlane((unsigned)(size_t)As + w * APW * 8 * BK * 4);
    const unsigned b_lds0 = __builtin_amdgcn_readfirstlane((unsigned)(size_t)Bs + w * BPW * 8 * BK * 4);
    auto dma = [&](auto bufc, auto idxc) __attribute__((always_inline)) {
        constexpr int BUF = decltype(bufc)::value, IDX = decltype(idxc)::value;
        if constexpr (IDX < APW) {
            asm volatile("s_mov_b32 m0, %0\n\ts_nop 0\n\tglobal_load_lds_dwordx4 %1, off"
                         :: "s"(a_lds0 + (BUF * TSA + 8 * IDX * BK) * 4), "v"(pa[IDX]) : "memory");
            pa[IDX] += BK;
        } else {
            asm volatile("s_mov_b32 m0, %0\n\ts_nop 0\n\tglobal_load_lds_dwordx4 %1, off"
                         :: "s"(b_lds0 + (BUF * TSB + 8 * (IDX - APW) * BK) * 4), "v"(pb[IDX - APW]) : "memory");
            pb[IDX - APW] += BK;
        }
        if constexpr (IDX == DMAS - 1) {   // the chunk is fully issued: move the loader on
            ck += BK;
            if (ck >= segK) {
                ck = 0;
                if (++cs < P.nseg) set_seg(cs);
            }
        }
    };

    f32x16 acc[FM][TN];
#pragma unroll
    for (int i = 0; i < FM; ++i)
#pragma unroll
        for (int j = 0; j < TN; ++j)
#pragma unroll
            for (int r = 0; r < 16; ++r) acc[i][j][r] = 0.f;

    const int frow = lane & 31, khalf = lane >> 5;
    const int fsw = (frow >> 1) & 7;       // identical for rows frow + 32*j
    float4 fa[2][FM], fb[2][TN];
    auto lfrag = [&](auto bufc, auto kbc, auto setc) __attribute__((always_inline)) {
        constexpr int BUF = decltype(bufc)::value, kb = decltype(kbc)::value, ST = decltype(setc)::value;
        const int slot = ((2 * kb + khalf) ^ fsw) * 4;
#pragma unroll
        for (int i = 0; i < FM; ++i)
            fa[ST][i] = *reinterpret_cast<const float4 *>(As + BUF * TSA + (wm * 32 * FM + i * 32 + frow) * BK + slot);
#pragma unroll
        for (int j = 0; j < TN; ++j)
            fb[ST][j] = *reinterpret_cast<const float4 *>(Bs + BUF * TSB + ((wn * TN + j) * 32 + frow) * BK + slot);
    };
    auto mma_e = [&](auto setc, auto ec) __attribute__((always_inline)) {
        constexpr int ST = decltype(setc)::value, e = decltype(ec)::value;
#pragma unroll
        for (int i = 0; i < FM; ++i) {
            const float a[4] = {fa[ST][i].x, fa[ST][i].y, fa[ST][i].z, fa[ST][i].w};
#pragma unroll
            for (int j = 0; j < TN; ++j) {
                const float b[4] = {fb[ST][j].x, fb[ST][j].y, fb[ST][j].z, fb[ST][j].w};
                acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x2f32(a[e], b[e], acc[i][j], 0, 0, 0);
            }
        }
    };
    // k-block kb of a chunk from fragment set kb & 1: four MFMA groups, group g = 4 kb + e followed by pieces
    // PER g .. + PER of the chunk AHEAD further on (when there is one) until that chunk is fully issued
    auto mma_dma = [&](auto kbc, auto farc, bool on) __attribute__((always_inline)) {
        constexpr int kb = decltype(kbc)::value;
        static_for<4>([&](auto ec) __attribute__((always_inline)) {
            mma_e(std::integral_constant<int, (kb & 1)>{}, ec);
            constexpr int P0 = G::PER * (4 * kb + decltype(ec)::value);
            if constexpr (P0 < DMAS) {
                if (on) static_for<G::PER>([&](auto pc) __attribute__((always_inline)) {
                    dma(farc, std::integral_constant<int, P0 + decltype(pc)::value>{});
                });
            }
        });
    };
    int nchunks = 0;
    for (int s = 0; s < P.nseg; ++s) nchunks += P.seg[s].K / BK;
    // Chunk c lives in buffer c % NBUF.  Buffer (c + AHEAD) % NBUF was last read in chunk c-1, whose reads all retired
    // (lgkmcnt(0)) in front of that chunk's barrier - so its DMA may start right away.
    auto chunk_body = [&](auto curc, int c) __attribute__((always_inline)) {
        constexpr int CUR = decltype(curc)::value;
        using Nxt = std::integral_constant<int, (CUR + 1) % NBUF>;
        using Far = std::integral_constant<int, (CUR + AHEAD) % NBUF>;
        const bool has1 = c + 1 < nchunks, far = c + AHEAD < nchunks;
        lfrag(curc, I1{}, I1{});
        mma_dma(I0{}, Far{}, far);
        lfrag(curc, I2{}, I0{});
        mma_dma(I1{}, Far{}, far);
        lfrag(curc, I3{}, I1{});
        mma_dma(I2{}, Far{}, far);
        if (has1) {
            // chunk c+1 must have landed; the chunks issued after it (what is left of them near the end) stay in flight
            dma_wait_stages<AHEAD - 1, DMAS>(nchunks - c - 2);
            __syncthreads();
            lfrag(Nxt{}, I0{}, I0{});
        }
        mma_dma(I3{}, Far{}, false);
    };
    set_seg(0);
    static_for<AHEAD>([&](auto qc) __attribute__((always_inline)) {
        if (decltype(qc)::value == 0 || decltype(qc)::value < nchunks)
            static_for<DMAS>([&](auto ic) __attribute__((always_inline)) { dma(qc, ic); });
    });
    dma_wait_stages<AHEAD - 1, DMAS>(nchunks - 1);
    __syncthreads();
    lfrag(I0{}, I0{}, I0{});
    for (int c = 0; c < nchunks; c += NBUF)
        static_for<NBUF>([&](auto bc) __attribute__((always_inline)) {
            constexpr int B = decltype(bc)::value;
            if (B == 0 || c + B < nchunks) chunk_body(bc, c + B);
        });

    static_for<FM>([&](auto ic) __attribute__((always_inline)) {
        constexpr int i = decltype(ic)::value;
        const int frow0 = wm * 32 * FM + 32 * i;
        if constexpr (EPI == EPI_VOCAB) epi_vocab_frag<Frag32, TN, 1, G::BM>(P, acc[i], frow0, 0, 0, lane, row0, col0, tn, smem);
        else if constexpr (EPI == EPI_LSTM) epi_lstm_frag(P, acc[i], frow0, lane, row0, tn);
        else epi_linear_frag<Frag32, TN, false>(P, acc[i], frow0, wn * 32 * TN, lane, row0, col0);
    });
}

template <int EPI>
__global__ __launch_bounds__(256) void gemm_xl_kernel(const DevLaunch L) {
    ISC_GATE_RETURN(L);
    f32_dma_tile_body<F32TileXL, EPI>(L);
}

template <int EPI>
__global__ __launch_bounds__(256) void gemm_ld_kernel(const DevLaunch L) {
    ISC_GATE_RETURN(L);
    f32_dma_tile_body<F32TileLD, EPI>(L);
}

__global__ __launch_bounds__(256) void gemm_md_kernel(const DevLaunch L) {
    ISC_GATE_RETURN(L);
    f32_dma_tile_body<F32TileMD, EPI_LINEAR>(L);
}

// ---- epilogues of the split-f16 tile kernels (accumulator layout Frag16) ------------------------------------------
// LSTM cells from a 32 x 128 gate-interleaved tile.  The kernels stage W so that tile column t = 32 gate + 16 hf + l
// holds (gate, unit 2 l + hf) of the tile's 32 units (h3_lstm_wrow): column block j = gate j >> 1, hf = j & 1, and lane l
// owns all four gates of the ADJACENT units 2 (l & 15), 2 (l & 15) + 1 for its 8 rows.  Every global operand of the
// epilogue (c_prev, the hoisted `pre` term, the embedding-table row, h / c out, the f16 planes of h) is then one
// float2 per lane and 16 lanes x 8 B = a full 128-byte segment per row - with one unit per lane (64-byte segments,
// twice the instructions) the att-LSTM's epilogue, which streams 16 KB per caption of `pre` and table rows, cost the
// kernel 14 us at B = 4096.  All loads of a row batch are issued before any arithmetic (see lstm_cells).
// This epilogue spells the cell's arithmetic out instead of calling isc_lstm_gate_sum / isc_lstm_cell: behind the
// calls the compiler moves a row's arithmetic under the row's store predicate, every row then waits for the stores of
// the row before it (gemm_h3x_kernel<lstm>: 136 -> 143 waits), and the 16384-row LSTM launches ran 0.6-0.8 % slower.
// The bit-identity tests across tile kernels hold the two spellings together.
__device__ __forceinline__ int h3_lstm_wrow_in_gate(int t) { return 2 * (t & 15) + ((t >> 4) & 1); }

__device__ __forceinline__ void epi_lstm_frag16(const DevProb &P, f32x4 (&acc)[2][8], int frow0, int lane, int row0,
                                                int tn) {
    const int H = P.H, u0 = tn * 32 + 2 * (lane & 15);
    const bool has_b = P.bias0 != nullptr, has_pre = P.pre != nullptr, has_tab = P.tab != nullptr;
    float2 b[4];
    if (has_b) {
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            const float2 x = *reinterpret_cast<const float2 *>(P.bias0 + k * H + u0);
            const float2 y = *reinterpret_cast<const float2 *>(P.bias1 + k * H + u0);
            b[k] = make_float2(x.x + y.x, x.y + y.y);
        }
    }
#pragma unroll
    for (int i = 0; i < 2; ++i) {            // one row block = 4 rows per lane at a time (register budget)
        int gm[4];
        bool ok[4];
        long long tok[4];
        float2 cp[4], q[4][4], t[4][4];
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            gm[r] = row0 + frow0 + i * 16 + 4 * (lane >> 4) + r;
            ok[r] = gm[r] < P.M;
        }
        if (has_tab) {
#pragma unroll
            for (int r = 0; r < 4; ++r) tok[r] = ok[r] ? P.tab_ids[(long long)gm[r] * P.tab_ids_stride] : 0;
        }
#pragma unroll
        for (int r = 0; r < 4; ++r)
            cp[r] = ok[r] ? *reinterpret_cast<const float2 *>(P.c_prev + (long long)gm[r] * H + u0) : make_float2(0.f, 0.f);
        if (has_pre && P.pre_div > 1) {  // one row of `pre` per image (uniform branch; one division per row)
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const long long pm = ok[r] ? (unsigned)gm[r] / (unsigned)P.pre_div : 0;
#pragma unroll
                for (int k = 0; k < 4; ++k)
                    q[r][k] = ok[r] ? *reinterpret_cast<const float2 *>(P.pre + pm * 4 * H + k * H + u0)
                                    : make_float2(0.f, 0.f);
            }
        } else if (has_pre) {
#pragma unroll
            for (int r = 0; r < 4; ++r)
#pragma unroll
                for (int k = 0; k < 4; ++k)
                    q[r][k] = ok[r] ? *reinterpret_cast<const float2 *>(P.pre + (long long)gm[r] * 4 * H + k * H + u0)
                                    : make_float2(0.f, 0.f);
        }
        if (has_tab) {
#pragma unroll
            for (int r = 0; r < 4; ++r)
#pragma unroll
                for (int k = 0; k < 4; ++k)
                    t[r][k] = ok[r] ? *reinterpret_cast<const float2 *>(P.tab + tok[r] * 4 * H + k * H + u0)
                                    : make_float2(0.f, 0.f);
        }
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            float h2[2], c2[2], ga[2][4];
#pragma unroll
            for (int hf = 0; hf < 2; ++hf) {
                float g[4];
#pragma unroll
                for (int k = 0; k < 4; ++k) {
                    g[k] = acc[i][2 * k + hf][r];
                    // the order of isc_lstm_gate_sum (common.h); written out, as is the cell below: see above
                    if (has_b) g[k] += hf ? b[k].y : b[k].x;
                    if (has_pre) g[k] += hf ? q[r][k].y : q[r][k].x;
                    if (has_tab) g[k] += hf ? t[r][k].y : t[r][k].x;
                }
                const float gi = isc_sigmoid(g[0]), gf = isc_sigmoid(g[1]), gg = isc_tanh(g[2]), go = isc_sigmoid(g[3]);
                c2[hf] = gf * (hf ? cp[r].y : cp[r].x) + gi * gg;
                h2[hf] = go * isc_tanh(c2[hf]);
                ga[hf][0] = gi; ga[hf][1] = gf; ga[hf][2] = gg; ga[hf][3] = go;
            }
            if (ok[r]) {
                const long long o = (long long)gm[r] * H + u0;
                *reinterpret_cast<float2 *>(P.c_out + o) = make_float2(c2[0], c2[1]);
                *reinterpret_cast<float2 *>(P.h_out + o) = make_float2(h2[0], h2[1]);
                if (P.h_hi) {
                    typedef _Float16 h2v __attribute__((ext_vector_type(2)));
                    _Float16 a0, a1, l0, l1;
                    isc_split_f16(h2[0], a0, l0);
                    isc_split_f16(h2[1], a1, l1);
                    const long long po = plane_index(gm[r], u0, H);          // u0 even: the pair stays in its 32-block
                    h2v hi = {a0, a1};
                    h2v lo = {l0, l1};
                    *reinterpret_cast<h2v *>(P.h_hi + po) = hi;
                    *reinterpret_cast<h2v *>(P.h_lo + po) = lo;
                }
                if (P.hmask) {
                    const uint8_t m0 = P.hmask[o], m1 = P.hmask[o + 1];
                    *reinterpret_cast<float2 *>(P.hdrop + o) =
                        make_float2(h2[0] * (float)m0 * P.mask_scale, h2[1] * (float)m1 * P.mask_scale);
                }
                if (P.gates_out) {
                    float *go_ = P.gates_out + (long long)gm[r] * 4 * H + u0;
#pragma unroll
                    for (int k = 0; k < 4; ++k)
                        *reinterpret_cast<float2 *>(go_ + k * H) = make_float2(ga[0][k], ga[1][k]);
                }
            }
        }
    }
}

// K-split form of the large split-f16 linear tile: workgroup (tile, ks) contracts its share of the k-blocks and stores the
// RAW partial tile to slab[ks] ([M, N] row-major); splitk_linear_kernel sums the slabs in fixed order and applies the
// epilogue.  For long contractions on few tiles - the classifier's dX over T x (B1 + B2) = 4160 rows is 132 tiles of
// K = 9984: a quarter of the chip's workgroup slots for 376 us; three slices of K fill it.
template <int NB, bool CHECK>
__device__ __forceinline__ void epi_slab_frag16(const DevProb &P, f32x4 (&acc)[2][NB], int frow0, int lane, int row0, int col0,
                                                int ks) {
    float *base = P.slab + (long long)ks * P.slab_stride;
    bool bad = false;
#pragma unroll
    for (int e = 0; e < Frag16::NR; ++e) {
        const int gm = row0 + frow0 + Frag16::row(e, lane);
        if (gm >= P.M) continue;
#pragma unroll
        for (int j = 0; j < NB; ++j) {
            const int gn = col0 + j * Frag16::CW + Frag16::col(lane);
            if (gn >= P.N) continue;
            const float o = Frag16::get(acc, e, j);
            if constexpr (CHECK) bad |= !(fabsf(o) <= 3.0e38f);
            base[(long long)gm * P.N + gn] = o;
        }
    }
    if constexpr (CHECK) {
        if (__any(bad) && lane == 0) isc_flag_gemm(ISC_STATUS_WORD_LINEAR);
    }
}

// ---------------------------------------------------------------- H3 tile: 128 x 128 on the f16 matrix cores
// fp32 operands, fp32 results, f16 MFMA rate.  Every operand value is split once into two f16 planes (isc_split_f16,
// common.h),
//     x = hi + lo * 2^-11,   hi = f16(x),   lo = f16((x - hi) * 2^11)
// which keeps >= 22 significant bits of x for |x| >= 2^-14 and an absolute error <= 2^-35 below (the subtraction is
// exact in fp32; tests/test_h3_math.py),
// and the contraction is taken as
//     C = sum hi_a hi_b  +  2^-11 * sum (hi_a lo_b + lo_a hi_b)
// on v_mfma_f32_32x32x16_f16: three MFMAs per 16-deep k-step instead of eight 32x32x2 fp32 ones at 1/16 the rate.
// f16 x f16 products are exact in the fp32 accumulator, the dropped lo_a lo_b term is <= 2^-22 relative, and the
// two sums live in separate accumulators so that the 2^-11 weight is applied once, in fp32, at the end.  Measured
// against an fp64 contraction the result is CLOSER than an fp32 fmaf chain (rms 1.0e-7 vs 2.6e-7 at K = 512,
// tools/h3_gemm_lab.hip) - the 1e-4 log-prob parity bound is not touched.  Domain: |x| < 65504 (f16 range of hi);
// beyond it hi is inf and the output NaN - loud, and far outside what the decoder's bounded activations reach.
// Geometry = the LD tile's (4 waves stacked in M, 32 x 128 accumulators, so the register epilogues are shared),
// operands by LDS-DMA from the pre-split planes: per 32-deep chunk four [128 x 32] f16 plane tiles of 8 KB
// (A hi, A lo, W hi, W lo), two buffers = 64 KB, two workgroups per CU.  64-byte LDS rows: slot s of row r holds
// k-octet q = s ^ ((r >> 2) & 3), which makes the ds_read_b128 fragment reads conflict-free.
typedef _Float16 h8 __attribute__((ext_vector_type(8)));

// A-operand fragment from an fp32 image row (32 floats = 8 chunks of 16 B, chunk c at position c ^ sw): the 8 values of
// k-octet `oct` (chunks 2*oct, 2*oct+1) split into their hi / lo halfs in registers - what h3_split_kernel would have
// written, bit for bit.
__device__ __forceinline__ void h3_frag_from_f32(const char *row, int oct, int sw, h8 &hi, h8 &lo) {
    const float4 v0 = *reinterpret_cast<const float4 *>(row + (((2 * oct) ^ sw) * 16));
    const float4 v1 = *reinterpret_cast<const float4 *>(row + (((2 * oct + 1) ^ sw) * 16));
    const float x[8] = {v0.x, v0.y, v0.z, v0.w, v1.x, v1.y, v1.z, v1.w};
#pragma unroll
    for (int e = 0; e < 8; ++e) {
        _Float16 h, l;
        isc_split_f16(x[e], h, l);
        hi[e] = h;
        lo[e] = l;
    }
}

// Diagnostic build only (-DH3_STAMP=1, tools/h3_stamp.sh; the shipped library compiles none of it): s_memtime stamps
// around the main loop and epilogue of gemm_h3_kernel<vocab> (slot 0) and of gemm_h3x_kernel's LSTM form with K = 1024
// (slot 1: att-LSTM), K = 1536 (slot 2: lang-LSTM) and its linear form (slot 3), summed over waves into g_h3_stamp[slot] =
// {waves, setup, main loop, epilogue} (shader cycles), read back by isc_debug_h3_stamps (16 words).  The stamps go to
// memory nothing else reads.
#ifndef H3_STAMP
#define H3_STAMP 0
#endif
#if H3_STAMP
#define H3_STAMP_AT(v) const unsigned long long v = __builtin_amdgcn_s_memtime()
__device__ unsigned long long g_h3_stamp[16];
extern "C" int isc_debug_h3_stamps(unsigned long long *out16_host, int reset) {
    if (out16_host && hipMemcpyFromSymbol(out16_host, HIP_SYMBOL(g_h3_stamp), sizeof(g_h3_stamp)) != hipSuccess) return 1;
    if (reset) {
        const unsigned long long z[16] = {};
        if (hipMemcpyToSymbol(HIP_SYMBOL(g_h3_stamp), z, sizeof(z)) != hipSuccess) return 1;
    }
    return ISC_OK;
}
#else
#define H3_STAMP_AT(v)
#endif

// Geometry of a large split-f16 tile kernel: WM x WN waves of 32 x (32 TN) accumulators each, NBUF LDS buffers in a
// ring with NBUF - 1 chunks of DMA in flight; KSLICE: the launch may split K over workgroups (raw partial tiles to
// slabs).  Everything else follows from these.
template <int WM_, int WN_, int TN_, int NBUF_, bool KSLICE_>
struct H3Geom {
    static constexpr int WM = WM_, WN = WN_, TN = TN_, NBUF = NBUF_, AHEAD = NBUF_ - 1;
    static constexpr bool KSLICE = KSLICE_;
    static constexpr int NB = 2 * TN;                            // 16-column blocks of a wave
    static constexpr int BM = 32 * WM, BN = 16 * NB * WN;
    static constexpr int PA = BM * 128, PB = BN * 128;           // bytes per A / W image (row = 128 B: 32 hi | 32 lo halfs)
    static constexpr int ST = PA + PB;                           // bytes per buffer
    static constexpr int LDS_BYTES = NBUF * ST;
    static constexpr int NW = WM * WN, THREADS = 64 * NW;
    static constexpr int APW = BM / 8 / NW, BPW = BN / 8 / NW;   // 8-row staging pieces of A / of W a wave issues
    static constexpr int DMAS = APW + BPW;                       // LDS-DMA instructions per wave and stage
    static_assert(TN == 2 || TN == 4, "two or four groups of column blocks per chunk");
    static_assert(APW * 8 * NW == BM && BPW * 8 * NW == BN && NBUF >= 2 && AHEAD * DMAS < 64, "pieces, ring, vmcnt range");
};
// 128 x 128, 4 x 1 waves, two buffers = 64 KB, two workgroups per CU (see above)
using H3Tile128 = H3Geom<4, 1, 4, 2, true>;
// 256 x 128 with EIGHT waves and three 48 KB buffers: one workgroup per CU keeps two chunks of DMA in flight (96 KB
// against the 64 KB of two 128-row workgroups with one chunk each) - these launches are bound by the DMA round trip,
// not by the matrix pipe: [4096 x 9984 x 512] 178 -> 137 us, [4096 x 2048 x 1536] 97 -> 76 us (tools/h3_gemm_lab.hip).
// Used when the launch has >= 224 such tiles.
using H3Tile256 = H3Geom<8, 1, 4, 3, false>;
// 64 x 128 (2 x 2 waves, 32 x 64 accumulators each; linear epilogue): launches whose 128-row tiling would leave CUs
// idle - the per-step projections with N = 512 at 4096 rows are 256 tiles of 64 x 128.  Per chunk: A planes 2 x 4 KB,
// W planes 2 x 8 KB; four buffers = 96 KB, one workgroup per CU, so the DMA round trip has to be covered by the
// workgroup's own prefetch depth, not by a neighbour.  (Round 3: six buffers = five chunks in flight measured the same as
// four / three - gate sum [4096 x 512 x 1024] 31.9 us either way - so the round trip is covered; what these N = 512
// launches pay is the ISSUE of their LDS-DMA pieces: six per wave and chunk against 24 MFMAs, where the 256-row kernel
// has 48.)
using H3Tile64 = H3Geom<2, 2, 2, 4, false>;

// The body of gemm_h3_kernel / gemm_h3x_kernel / gemm_h3m_kernel (geometry G).
// AF32: some activation segment comes as fp32 rows (split after the fragment read); false = every segment has planes,
// and the per-buffer test is compiled out of the fragment loads (it cost the all-planes decode loop ~5-10 %).
// AF16 (with AF32; linear epilogue): some activation segment comes as _Float16 rows (DevSeg.a_f16).  Such a value is its
// own hi and its lo is zero, so the row is staged as it is - one 128-byte line holds 64 k = TWO chunks - into every
// chunk's buffer (the second touch of a line hits L2; with two buffers the image of chunk c is gone before chunk c + 1
// runs), the fragment's hi is read from the half of the image row the chunk's parity names, and the al * bh MFMA, which
// would add exact zeros, is not issued: the result is the fp32-row form's on the up-cast values, bit for bit.
template <class G, int EPI, bool AF32, bool AF16 = false>
__device__ __forceinline__ void h3_tile_body(const DevLaunch &L) {
    static_assert(!AF16 || (AF32 && EPI == EPI_LINEAR), "f16 rows come next to fp32 rows, in isc_linear_fwd only");
    H3_STAMP_AT(stamp0);
    constexpr int NB = G::NB, NQ = NB / 2;              // NQ groups of two column blocks per chunk
    constexpr int PA = G::PA, ST = G::ST, APW = G::APW, BPW = G::BPW, NBUF = G::NBUF, AHEAD = G::AHEAD;
    static_assert(EPI == EPI_LINEAR || G::WN == 1, "the LSTM and vocabulary epilogues take the tile's whole rows");
    extern __shared__ __attribute__((aligned(16))) float smem[];
    char *lds = reinterpret_cast<char *>(smem);

    const int tid = threadIdx.x;
    const int lane = tid & 63;
    const int w = tid >> 6, wm = w / G::WN, wn = w % G::WN;
    int pi, tm, tn, ks, ksplit;
    map_tile(L, pi, tm, tn, ks, ksplit);
    const DevProb &P = L.p[pi];
    const int M = P.M, N = P.N, Kp = P.Kp;
    const int row0 = tm * G::BM, col0 = tn * G::BN;

    // staging in pieces of 8 rows x 128 B = whole lines of the interleaved plane layout (a row's 32 hi + 32 lo halfs
    // of a k-block): wave w issues A pieces APW w .. + APW and W pieces BPW w .. + BPW; piece ii = image rows
    // 8*ii .. +8, 8 lanes per row.  (Pieces of 16 rows x 64 B - hi and lo fetched by different instructions - touched
    // every line twice and ran 9-14 % slower: tools/h3_gemm_lab.hip, r02.)  Image position p of row r holds chunk
    // p ^ ((r>>1)&7).  W planes are K-packed [N, Kp]; A planes come by K-segment (P.ap: the split kernel's packed planes
    // as one segment, or the producers' per-tensor planes), switched at chunk boundaries.
    const _Float16 *src[APW + BPW];
    int arow[APW], aq[APW];
#pragma unroll
    for (int i = 0; i < APW; ++i) {
        const int t = 8 * APW * w + 8 * i + (lane >> 3);
        int ar = row0 + t;
        arow[i] = ar < M ? ar : M - 1;
        aq[i] = ((lane & 7) ^ ((t >> 1) & 7)) * 8;
    }
#pragma unroll
    for (int i = 0; i < BPW; ++i) {
        const int t = 8 * BPW * w + 8 * i + (lane >> 3);
        const int q = (lane & 7) ^ ((t >> 1) & 7);
        long long wr;
        if (EPI == EPI_LSTM) {
            wr = (long long)(t >> 5) * P.H + tn * 32 + h3_lstm_wrow_in_gate(t);     // (gate, unit): see epi_lstm_frag16
        } else {
            const int c = col0 + t;
            wr = c < N ? c : N - 1;
        }
        src[APW + i] = P.Wh + wr * 2 * Kp + q * 8;
    }
    int cs = 0, ck = 0, segK = 0;
    bool seg_f32 = false;                // the segment has no planes: its fp32 rows are staged (128 B per row and chunk,
    unsigned f32_bufs = 0;               // like a plane row) and split after the fragment read; bit b: buffer b holds fp32
    bool seg_f16 = false;                // AF16: the segment's rows are f16; bit b of f16_bufs: buffer b holds such a line,
    unsigned f16_bufs = 0, odd_bufs = 0; // bit b of odd_bufs: its chunk is the line's second half
    auto set_aseg = [&](int si) __attribute__((always_inline)) {
        const DevASeg a = P.ap[si];
        segK = a.K;
        seg_f32 = AF32 && a.hi == nullptr;
        if constexpr (AF16) {
            seg_f16 = seg_f32 && P.seg[si].a_f16 != 0;
            seg_f32 = seg_f32 && !seg_f16;
            if (seg_f16) {
#pragma unroll
                for (int i = 0; i < APW; ++i)
                    src[i] = reinterpret_cast<const _Float16 *>(P.seg[si].A) + (long long)arow[i] * P.seg[si].lda + aq[i];
                return;
            }
        }
#pragma unroll
        for (int i = 0; i < APW; ++i)
            src[i] = seg_f32 ? reinterpret_cast<const _Float16 *>(P.seg[si].A + (long long)arow[i] * P.seg[si].lda) + aq[i]
                             : a.hi + (long long)arow[i] * a.ld + aq[i];
    };
    int nchunks = Kp / 32;
    if constexpr (G::KSLICE) {
        // this workgroup's share of the k-blocks (ksplit > 1, linear epilogue only: raw partial tiles go to slabs)
        const int c_lo = ksplit > 1 ? (int)((long long)nchunks * ks / ksplit) : 0;
        const int c_hi = ksplit > 1 ? (int)((long long)nchunks * (ks + 1) / ksplit) : nchunks;
        int k0 = c_lo * 32;
        while (cs + 1 < P.nap && k0 >= P.ap[cs].K) { k0 -= P.ap[cs].K; ++cs; }
        set_aseg(cs);
        if (c_lo > 0) {
#pragma unroll
            for (int i = 0; i < APW; ++i) src[i] += (long long)(k0 >> 5) * 64;
#pragma unroll
            for (int i = 0; i < BPW; ++i) src[APW + i] += (long long)c_lo * 64;
            ck = k0;
        }
        nchunks = c_hi - c_lo;
    } else {
        set_aseg(0);
    }
    const unsigned lds0 = __builtin_amdgcn_readfirstlane((unsigned)(size_t)lds);
    const unsigned wv = __builtin_amdgcn_readfirstlane((unsigned)w);
    auto dma1 = [&](unsigned dst, const _Float16 *&p) __attribute__((always_inline)) {
        asm volatile("s_mov_b32 m0, %0\n\ts_nop 0\n\tglobal_load_lds_dwordx4 %1, off" :: "s"(dst), "v"(p) : "memory");
        p += 64;                                          // next 32-k block: 32 hi + 32 lo halfs further
    };
    auto stage = [&](int buf) __attribute__((always_inline)) {
        const unsigned b = lds0 + buf * ST;
        f32_bufs = (f32_bufs & ~(1u << buf)) | ((seg_f32 ? 1u : 0u) << buf);
        bool a_staged = false;
        if constexpr (AF16) {
            const bool odd = (ck & 32) != 0;                  // (chunk parity restarts with the segment: ck does)
            f16_bufs = (f16_bufs & ~(1u << buf)) | ((seg_f16 ? 1u : 0u) << buf);
            odd_bufs = (odd_bufs & ~(1u << buf)) | ((seg_f16 && odd ? 1u : 0u) << buf);
            if (seg_f16) {
                // a segment of an odd number of chunks ends on half a line: the lanes of its second half re-read the
                // first (nobody reads that part of the image) instead of running past the row's K halfs
                const bool tail = !odd && ck + 32 >= segK;
#pragma unroll
                for (int i = 0; i < APW; ++i) {
                    const _Float16 *p = src[i] - (tail && aq[i] >= 32 ? 32 : 0);
                    dma1(b + (APW * wv + i) * 1024, p);
                    if (odd) src[i] += 64;                    // the next line after the pair
                }
                a_staged = true;
            }
        }
        if (!a_staged) {
#pragma unroll
            for (int i = 0; i < APW; ++i) dma1(b + (APW * wv + i) * 1024, src[i]);
        }
#pragma unroll
        for (int i = 0; i < BPW; ++i) dma1(b + PA + (BPW * wv + i) * 1024, src[APW + i]);
        ck += 32;
        if (ck >= segK) {
            ck = 0;
            if (++cs < P.nap) set_aseg(cs);
        }
    };

    // v_mfma_f32_16x16x32_f16 (round 3; the 32x32x16 form of rounds 1-2 ran 7-16 % slower on the same tile, staging and
    // LDS image - tools/h3_mfma16_lab.hip): the wave's 32 x 16 NB tile = 2 row blocks x NB column blocks, ONE MFMA per
    // block, product term and 32-k chunk.  Fragment of lane l: row (l & 15) of the block, k-octet (l >> 4) = 16-byte
    // chunk (l >> 4) of the row image's hi half, chunk 4 + (l >> 4) of its lo half (positions XOR-swizzled as staged).
    f32x4 acc0[2][NB], acc1[2][NB];
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int j = 0; j < NB; ++j)
#pragma unroll
            for (int r = 0; r < 4; ++r) { acc0[i][j][r] = 0.f; acc1[i][j][r] = 0.f; }

    const int fr = lane & 15, fq = lane >> 4, fsw = (fr >> 1) & 7;
    const int ph = (fq ^ fsw) * 16, pl = ((4 + fq) ^ fsw) * 16;
    h8 ah[2][2], al[2][2], bh[2][2], bl[2][2];          // A: [set][row block]; W: [slot][column block of the group]
    bool a16[2] = {false, false};                       // AF16: A set s holds an f16 chunk (hi only)
    auto lfragA = [&](int buf, auto setc) __attribute__((always_inline)) {
        constexpr int S = decltype(setc)::value;
        const char *base = lds + buf * ST;
        if constexpr (AF16) {
            a16[S] = ((f16_bufs >> buf) & 1u) != 0;
            if (a16[S]) {
                const int po = (((int)((odd_bufs >> buf) & 1u) * 4 + fq) ^ fsw) * 16;
#pragma unroll
                for (int i = 0; i < 2; ++i) {
                    ah[S][i] = *reinterpret_cast<const h8 *>(base + (wm * 32 + i * 16 + fr) * 128 + po);
                    al[S][i] = h8{0, 0, 0, 0, 0, 0, 0, 0};
                }
                return;
            }
        }
#pragma unroll
        for (int i = 0; i < 2; ++i) {
            const int ra = (wm * 32 + i * 16 + fr) * 128;
            if (AF32 && ((f32_bufs >> buf) & 1u)) {
                h3_frag_from_f32(base + ra, fq, fsw, ah[S][i], al[S][i]);
            } else {
                ah[S][i] = *reinterpret_cast<const h8 *>(base + ra + ph);
                al[S][i] = *reinterpret_cast<const h8 *>(base + ra + pl);
            }
        }
    };
    auto lfragB = [&](int buf, auto grpc, auto slotc) __attribute__((always_inline)) {
        constexpr int Q = decltype(grpc)::value, SL = decltype(slotc)::value;
        const char *base = lds + buf * ST + PA;
#pragma unroll
        for (int j = 0; j < 2; ++j) {
            const int rb = (wn * 16 * NB + (Q * 2 + j) * 16 + fr) * 128;
            bh[SL][j] = *reinterpret_cast<const h8 *>(base + rb + ph);
            bl[SL][j] = *reinterpret_cast<const h8 *>(base + rb + pl);
        }
    };
    auto mma = [&](auto setc, auto grpc, auto slotc) __attribute__((always_inline)) {
        constexpr int S = decltype(setc)::value, Q = decltype(grpc)::value, SL = decltype(slotc)::value;
#pragma unroll
        for (int j = 0; j < 2; ++j)
#pragma unroll
            for (int i = 0; i < 2; ++i) {
                acc0[i][Q * 2 + j] = __builtin_amdgcn_mfma_f32_16x16x32_f16(ah[S][i], bh[SL][j], acc0[i][Q * 2 + j], 0, 0, 0);
                acc1[i][Q * 2 + j] = __builtin_amdgcn_mfma_f32_16x16x32_f16(ah[S][i], bl[SL][j], acc1[i][Q * 2 + j], 0, 0, 0);
                // (an f16 chunk has lo == 0: the third term would add exact zeros.  Guarding the one MFMA keeps the
                // accumulators in registers; two copies of the loop nest, or of the chunk, spilled 190-580 B per lane)
                if (!(AF16 && a16[S]))
                    acc1[i][Q * 2 + j] = __builtin_amdgcn_mfma_f32_16x16x32_f16(al[S][i], bh[SL][j], acc1[i][Q * 2 + j], 0, 0, 0);
            }
    };
    // one chunk's MFMAs with the W fragments of group q + 1 read under the MFMAs of group q; `between` runs in front of
    // the last group (the barrier, then the next chunk's A fragments into the other A set and its group-0 W fragments)
    auto chunk_mma = [&](int cur, auto setc, auto between) __attribute__((always_inline)) {
        if constexpr (NQ == 4) {
            lfragB(cur, I1{}, I1{}); mma(setc, I0{}, I0{});
            lfragB(cur, I2{}, I0{}); mma(setc, I1{}, I1{});
            lfragB(cur, I3{}, I1{}); mma(setc, I2{}, I0{});
            between();
            mma(setc, I3{}, I1{});
        } else {
            lfragB(cur, I1{}, I1{}); mma(setc, I0{}, I0{});
            between();
            mma(setc, I1{}, I1{});
        }
    };
    // NBUF buffers, AHEAD chunks in flight: the wait in front of a barrier leaves the younger stages outstanding
    auto wait_for = [&](int in_flight) __attribute__((always_inline)) { dma_wait_stages<AHEAD - 1, G::DMAS>(in_flight); };
    H3_STAMP_AT(stamp1);
#pragma unroll
    for (int q = 0; q < AHEAD; ++q)
        if (q == 0 || q < nchunks) stage(q);
    wait_for((nchunks < AHEAD ? nchunks : AHEAD) - 1);
    __syncthreads();
    lfragA(0, I0{});
    lfragB(0, I0{}, I0{});
    // per chunk: the second half's W fragments are read under the first half's MFMAs, the next chunk's A fragments
    // (into the other A set) and first-half W fragments under the second half's
    int ring = 0;                                      // ring position of chunk c; with two buffers it is the chunk's
    auto chunk = [&](int c, auto setc, auto nsetc) __attribute__((always_inline)) {    // parity = its A set: compile-time
        const int cur = NBUF == 2 ? decltype(setc)::value : ring;
        const int nxt = cur + 1 == NBUF ? 0 : cur + 1;
        int far = cur + AHEAD;                         // where chunk c + AHEAD goes: the buffer chunk c - 1 left,
        if (far >= NBUF) far -= NBUF;                  // last read in front of the previous barrier
        if (c + AHEAD < nchunks) stage(far);
        chunk_mma(cur, setc, [&]() __attribute__((always_inline)) {
            if (c + 1 < nchunks) {
                const int last = nchunks - 1 < c + AHEAD ? nchunks - 1 : c + AHEAD;
                wait_for(last - (c + 1));
                __syncthreads();
                lfragA(nxt, nsetc);
                lfragB(nxt, I0{}, I0{});
            }
        });
        ring = nxt;
    };
    for (int c = 0; c < nchunks; c += 2) {
        chunk(c, I0{}, I1{});
        if (c + 1 < nchunks) chunk(c + 1, I1{}, I0{});
    }
    H3_STAMP_AT(stamp2);
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int j = 0; j < NB; ++j)
#pragma unroll
            for (int r = 0; r < 4; ++r) acc0[i][j][r] = fmaf(acc1[i][j][r], ISC_SPLIT_LO_WEIGHT, acc0[i][j][r]);

    if constexpr (EPI == EPI_VOCAB) {
        epi_vocab_frag<Frag16, NB, 1, G::BM>(P, acc0, wm * 32, 0, 0, lane, row0, col0, tn, nullptr);
    } else if constexpr (EPI == EPI_LSTM) {
        epi_lstm_frag16(P, acc0, wm * 32, lane, row0, tn);
    } else {
        if (G::KSLICE && ksplit > 1) epi_slab_frag16<NB, AF32>(P, acc0, wm * 32, lane, row0, col0, ks);
        else epi_linear_frag<Frag16, NB, AF32>(P, acc0, wm * 32, wn * 16 * NB, lane, row0, col0);
    }
#if H3_STAMP
    // slot 0: the 128-row vocabulary form; slots 1 - 3: the 256-row LSTM (K = 1024, K = 1536) and linear forms
    const int slot = G::BM == 128 && EPI == EPI_VOCAB ? 0
                   : G::BM == 256 && EPI == EPI_LSTM ? (Kp == 1024 ? 1 : Kp == 1536 ? 2 : -1)
                   : G::BM == 256 && EPI == EPI_LINEAR ? 3 : -1;
    if (slot >= 0) {
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");           // the epilogue's stores have left
        H3_STAMP_AT(stamp3);
        if (lane == 0) {
            atomicAdd(&g_h3_stamp[4 * slot + 0], 1ull);
            atomicAdd(&g_h3_stamp[4 * slot + 1], stamp1 - stamp0);
            atomicAdd(&g_h3_stamp[4 * slot + 2], stamp2 - stamp1);
            atomicAdd(&g_h3_stamp[4 * slot + 3], stamp3 - stamp2);
        }
    }
#endif
}

template <int EPI, bool AF32>
__global__ __launch_bounds__(256, 2) void gemm_h3_kernel(const DevLaunch L) {
    ISC_GATE_RETURN(L);
    h3_tile_body<H3Tile128, EPI, AF32>(L);
}

template <int EPI, bool AF32>
__global__ __launch_bounds__(512) void gemm_h3x_kernel(const DevLaunch L) {
    ISC_GATE_RETURN(L);
    h3_tile_body<H3Tile256, EPI, AF32>(L);
}

template <bool AF32>
__global__ __launch_bounds__(256) void gemm_h3m_kernel(const DevLaunch L) {
    ISC_GATE_RETURN(L);
    rows_kernarg_warm<ROWS_KERNARG_LINES(DevLaunch)>();      // (one batch of scalar loads for the launch descriptor: common.h)
    h3_tile_body<H3Tile64, EPI_LINEAR, AF32>(L);
}

// The three geometries with f16 activation rows read natively (linear epilogue: isc_linear_fwd with isc_seg.a_f16).
template <class G>
__global__ __launch_bounds__(G::THREADS, G::LDS_BYTES <= 65536 ? 2 : 1) void gemm_h3_f16a_kernel(const DevLaunch L) {
    ISC_GATE_RETURN(L);
    h3_tile_body<G, EPI_LINEAR, true, true>(L);
}

// Operand split in front of gemm_h3_kernel: gathers the K-segments of one operand into the two packed f16 planes
// [rows, Kp].  One thread per 8 consecutive k (two float4 loads, one 16-byte store per plane).
struct SplitJob {
    const float *src[ISC_MAX_SEG];
    int ld[ISC_MAX_SEG];
    int kstart[ISC_MAX_SEG];
    int nseg, rows, Kp, first_block;
    _Float16 *hi, *lo;
    int transposed, _pad;             // source segments are [K_s, rows] (k-major): planes of the TRANSPOSE are built
};
#define H3_MAX_JOBS 12
struct SplitLaunch {
    SplitJob j[H3_MAX_JOBS];
    int njobs;
};

__global__ __launch_bounds__(256) void h3_split_kernel(const SplitLaunch S) {
    int ji = 0;
#pragma unroll
    for (int i = 1; i < H3_MAX_JOBS; ++i)
        if (i < S.njobs && (int)blockIdx.x >= S.j[i].first_block) ji = i;
    const SplitJob &J = S.j[ji];
    const int k8n = J.Kp >> 3;
    const long long idx = (long long)(blockIdx.x - J.first_block) * 256 + threadIdx.x;
    if (J.transposed) {
        // source segments are [K_s, rows] (k-major: the backward pass's W for dX = dY W, and both operands of dW = dY^T X);
        // plane row n = column n of the source.  One workgroup transposes a tile of 32 k x 64 n through LDS: the reads are
        // 256-byte row pieces, and each output row receives its whole 128-byte line (32 hi + 32 lo halfs of the k-block).
        __shared__ float t[32][65];
        const int ntile = (J.rows + 63) >> 6;
        const int bid = blockIdx.x - J.first_block;
        const int kb = bid / ntile, n0 = (bid - kb * ntile) * 64, kq = kb * 32;
        const float *sp = J.src[0];
        int ld = J.ld[0], k0 = 0;
#pragma unroll
        for (int sg = 1; sg < ISC_MAX_SEG; ++sg)
            if (sg < J.nseg && kq >= J.kstart[sg]) { sp = J.src[sg]; ld = J.ld[sg]; k0 = J.kstart[sg]; }
        const int tx = threadIdx.x & 63, ty = threadIdx.x >> 6;
#pragma unroll
        for (int r = 0; r < 8; ++r) {
            const int k = ty * 8 + r;
            t[k][tx] = n0 + tx < J.rows ? sp[(long long)(kq - k0 + k) * ld + n0 + tx] : 0.f;
        }
        __syncthreads();
        // thread -> (n = tid / 4, 8 consecutive k = 8 * (tid % 4)): four threads write one row's 64 B of hi and 64 B of lo
        const int n = threadIdx.x >> 2, q = (threadIdx.x & 3) * 8;
        if (n0 + n < J.rows) {
            float x[8];
#pragma unroll
            for (int e = 0; e < 8; ++e) x[e] = t[q + e][n];
            store_planes<8>(J.hi, J.lo, n0 + n, kq + q, J.Kp, x);
        }
        return;
    }
    if (idx >= (long long)J.rows * k8n) return;
    const int row = (int)(idx / k8n);
    int k = (int)(idx - (long long)row * k8n) * 8;
    const float *sp = J.src[0];
    int ld = J.ld[0], k0 = 0;
#pragma unroll
    for (int s = 1; s < ISC_MAX_SEG; ++s)
        if (s < J.nseg && k >= J.kstart[s]) { sp = J.src[s]; ld = J.ld[s]; k0 = J.kstart[s]; }
    const float *p = sp + (long long)row * ld + (k - k0);
    const float4 v0 = *reinterpret_cast<const float4 *>(p), v1 = *reinterpret_cast<const float4 *>(p + 4);
    const float x[8] = {v0.x, v0.y, v0.z, v0.w, v1.x, v1.y, v1.z, v1.w};
    store_planes<8>(J.hi, J.lo, row, k, J.Kp, x);        // 8 consecutive k never leave their 32-block
}

// ---------------------------------------------------------------- H3S: skinny split-f16 tiles for few-row launches
// (H3S_LAB_MODE = 1 / 2 / 3 builds time-only variants of the kernel below - DMA only / + fragment reads / MFMAs without
// reads - for tools/h3s_lab_modes.sh; 0, the default, compiles none of it.)
#ifndef H3S_LAB_MODE
#define H3S_LAB_MODE 0
#endif
// Launches with few rows (B <= a few hundred captions, beam rows, the 80-row seq2seq unroll) are not contraction-
// bound: each of their GEMMs streams a weight matrix far larger than its activations, and the step is a chain of
// such launches.  The fp32 route gave them a 32 x 128 tile per workgroup, split K over up to 16 workgroups, wrote
// [S, M, N] slabs and ran a second kernel to sum them and apply the epilogue (13 + 6 us per GEMM at M = 128).
// Here ONE launch does it.  Linear / LSTM: a workgroup owns a 32 x 32 output tile (LSTM: 8 hidden units x 4
// gates), so a [128 x 2048] launch spreads its weight stream over 256 workgroups, and its four waves take
// contiguous quarters of K; the four partial tiles meet in LDS, are summed in fixed order (deterministic) and
// the epilogue runs from the reduced tile.  Vocabulary projection: a 32 x 128 tile (its statistics are per 128
// columns), wave w owns columns 32w .. 32w+31 over the whole K.  Either way a wave is self-contained: it stages the
// 32-deep k-blocks of ITS operands - one [32 rows x 128 B] image each for A and W - into a private 4-slot LDS ring
// by LDS-DMA in pieces of 8 rows x 128 B (whole lines: a row's 32 hi + 32 lo halfs of a block are one line of the
// interleaved plane layout), three blocks in flight, ordered by its own vmcnt only: no barrier in the loop.
// LDS image: row r holds global 16-byte chunk c at position c ^ ((r >> 1) & 7) (conflict-free ds_read_b128 fragments).
// Weights come as f16 planes from the stream's weights scope; an activation segment comes as planes when its
// producer wrote them, else as fp32 rows (same 128 bytes per row and block) and is split after the fragment read.
__device__ __forceinline__ void h3s_dma(unsigned lds_addr, const char *src) {
    asm volatile("s_mov_b32 m0, %0\n\ts_nop 0\n\tglobal_load_lds_dwordx4 %1, off" :: "s"(lds_addr), "v"(src) : "memory");
}

// The MFMA operand fragments of one 32-deep k-block (two 16-deep steps) from 4 KB images: ia / iw = this lane's row
// (lane & 31) of the A / W image, fh = lane >> 5, fsw = the row's chunk swizzle.  A W image always holds planes; an A
// image holds planes or, with af32, fp32 rows that are split here.
__device__ __forceinline__ void h3s_read_frags(const char *ia, const char *iw, bool af32, int fh, int fsw, h8 (&a1)[2],
                                               h8 (&a2)[2], h8 (&b1)[2], h8 (&b2)[2]) {
#pragma unroll
    for (int kk = 0; kk < 2; ++kk) {
        if (af32) {
            h3_frag_from_f32(ia, 2 * kk + fh, fsw, a1[kk], a2[kk]);
        } else {
            a1[kk] = *reinterpret_cast<const h8 *>(ia + (((2 * kk + fh) ^ fsw) * 16));
            a2[kk] = *reinterpret_cast<const h8 *>(ia + (((4 + 2 * kk + fh) ^ fsw) * 16));
        }
        b1[kk] = *reinterpret_cast<const h8 *>(iw + (((2 * kk + fh) ^ fsw) * 16));
        b2[kk] = *reinterpret_cast<const h8 *>(iw + (((4 + 2 * kk + fh) ^ fsw) * 16));
    }
}

// The 128-column statistics of a BM-row vocabulary tile from its four 32-column waves' (epi_vocab_frag<Frag32, 1, 4, BM>).
template <int BM>
__device__ __forceinline__ void h3s_vocab_combine(const DevProb &P, const float *smem, int tid, int row0, int tn) {
    const float *smx = smem;
    const float *ssm = smem + 4 * BM;
    const int *six = reinterpret_cast<const int *>(smem + 2 * 4 * BM);
    if (tid < BM && row0 + tid < P.M) {
        const int row = tid;
        float mx = smx[row];
        int ix = six[row];
#pragma unroll
        for (int w = 1; w < 4; ++w) {
            const float ov = smx[w * BM + row];
            const int oi = six[w * BM + row];
            if (ov > mx || (ov == mx && oi < ix)) { mx = ov; ix = oi; }
        }
        float sm = 0.f;
#pragma unroll
        for (int w = 0; w < 4; ++w) {
            const float wm_ = smx[w * BM + row];          // -inf: that wave had no valid column
            if (wm_ > -INFINITY) sm += ssm[w * BM + row] * __expf(wm_ - mx);
        }
        const long long o = (long long)(row0 + row) * P.ntile_total + tn;
        P.pmax[o] = mx;
        P.psum[o] = sm;
        P.pidx[o] = ix;
    }
}

// T = 2 (K-split epilogues only) doubles the tile to 64 x 64: a loaded row then feeds two MFMA tiles instead of one, so
// a launch needs half the bytes per output - the shape for launches of several rounds of 32 x 32 tiles (LSTM cell at
// M = 512 ... 1024) that are still too few 128-row tiles to fill the chip.  Its slots are 16 KB (64-row images), its
// ring two slots, and a slot is re-issued as soon as its fragments sit in registers (before the MFMAs), so two
// blocks - 32 KB per wave - stay in flight as in the 4-slot ring of the small tile.
template <int EPI, int T, int NW = 4>
__global__ __launch_bounds__(64 * NW) void gemm_h3s_kernel(const DevLaunch L) {
    ISC_GATE_RETURN(L);
    rows_kernarg_warm<ROWS_KERNARG_LINES(DevLaunch)>();      // (one batch of scalar loads for the launch descriptor: common.h)
    constexpr bool KSPLIT = EPI != EPI_VOCAB;
    static_assert(T == 1 || (T == 2 && KSPLIT), "wide skinny tile: K-split epilogues only");
    static_assert(NW == 4 || (NW == 8 && T == 1), "eight waves: the small tiles only");
    constexpr int BM = 32 * T, BN = KSPLIT ? 32 * T : 128;
    // ring depth: 4 slots (three blocks in flight, 128 KB: one workgroup per CU) for the K-split tiles, whose launches
    // have at most ~256 workgroups; 2 slots (64 KB: two workgroups per CU) for the vocabulary projection, whose 79
    // column tiles x row tiles do not fit one round of single-workgroup CUs (316 workgroups at M = 128: 32 -> 17 us)
    // NW = 8: the K range over eight waves with two-slot rings (same 128 KB) - twice the waves issuing DMA
    constexpr int R = KSPLIT && T == 1 && NW == 4 ? 4 : 2, IMG = 4096 * T, SLOT = 2 * IMG, NP = 4 * T, LDR = BN + 1;
    constexpr bool EARLY = T == 2 || NW == 8;           // slot released after the fragment read, not after the MFMAs
    constexpr int LOGW = NW == 8 ? 3 : 2;
    extern __shared__ __attribute__((aligned(16))) float smem[];     // 4 waves x R slots x (A image + W image)
    char *lds = reinterpret_cast<char *>(smem);

    const int tid = threadIdx.x, lane = tid & 63;
    // wave index as a scalar: everything derived from it (k-range, segment cursor) then lives in SGPRs and the
    // descriptor fields it selects are fetched by scalar loads, not by vector loads that would sit in vmcnt
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    int pi, tm, tn, ks, ksplit;
    map_tile(L, pi, tm, tn, ks, ksplit);
    const DevProb &P = L.p[pi];
    const int M = P.M, N = P.N, Kp = P.Kp;
    const int row0 = tm * BM, col0 = tn * BN;
    const int fr = lane & 31, fh = lane >> 5;
    // this wave's 32-column block inside the tile (vocabulary tile on eight waves: waves w and w + 4 share block w
    // and take one half of K each)
    const int cw = KSPLIT ? 0 : (wave & 3);

    // DMA lanes: piece p covers image rows 8p + (lane >> 3); lane position lane & 7 fetches chunk pos ^ swizzle(row)
    const int prow = lane >> 3;
    int a_row[NP];
    const char *w_src[NP];
    int chunk_off[NP];
#pragma unroll
    for (int p = 0; p < NP; ++p) {
        const int r = 8 * p + prow;
        chunk_off[p] = ((lane & 7) ^ ((r >> 1) & 7)) * 16;
        const int ar = row0 + r;
        a_row[p] = ar < M ? ar : M - 1;                 // rows past the edge fetch a valid row, never stored
        long long wr;
        if (EPI == EPI_LSTM) {                          // image row r = gate r / (8T), unit tn*8T + r % (8T)
            wr = (long long)(p / T) * P.H + tn * (8 * T) + (p % T) * 8 + prow;
        } else {
            const int c = col0 + cw * 32 + r;
            wr = c < N ? c : N - 1;
        }
        w_src[p] = reinterpret_cast<const char *>(P.Wh) + wr * 4 * Kp + chunk_off[p];
    }
    // this wave's k-blocks, and a cursor over the A segments positioned on its first block
    // ... of this workgroup's share of K (P.ksplit > 1: long contractions on few tiles are also split over workgroups;
    // the partial tiles then go to slabs and splitk_linear_kernel sums them and applies the epilogue)
    const int nblk = Kp >> 5;
    const int g_lo = (int)((long long)nblk * ks / ksplit), g_hi = (int)((long long)nblk * (ks + 1) / ksplit);
    const int nb = g_hi - g_lo;
    const int khalf = wave >> 2;                         // (vocabulary tile, NW = 8)
    const int b_lo = KSPLIT ? g_lo + ((nb * wave) >> LOGW) : (NW == 8 ? (nblk * khalf) >> 1 : 0);
    const int b_hi = KSPLIT ? g_lo + ((nb * (wave + 1)) >> LOGW) : (NW == 8 ? (nblk * (khalf + 1)) >> 1 : nblk);
    const int n = b_hi - b_lo;
    int cs = 0, cb = b_lo;
    while (cs < P.nap - 1 && cb >= (P.ap[cs].K >> 5)) { cb -= P.ap[cs].K >> 5; ++cs; }
    int seg_blocks = 0;
    bool seg_f32 = false;
    const char *a_src[NP];
    auto set_aseg = [&](int si) __attribute__((always_inline)) {
        const DevASeg a = P.ap[si];
        seg_blocks = a.K >> 5;
        seg_f32 = a.hi == nullptr;
#pragma unroll
        for (int p = 0; p < NP; ++p) {
            if (seg_f32)
                a_src[p] = reinterpret_cast<const char *>(P.seg[si].A + (long long)a_row[p] * P.seg[si].lda) + chunk_off[p];
            else
                a_src[p] = reinterpret_cast<const char *>(a.hi + (long long)a_row[p] * a.ld) + chunk_off[p];
        }
    };
    set_aseg(cs);
    const unsigned ring = __builtin_amdgcn_readfirstlane((unsigned)(size_t)lds + wave * (R * SLOT));
    unsigned f32_bits = 0;                               // bit (block % R): that slot's A image holds fp32 rows
    int lb = b_lo;
    auto issue = [&](int i) __attribute__((always_inline)) {          // block i of this wave -> slot i % R
        const unsigned slot = ring + (i & (R - 1)) * SLOT;
        f32_bits = (f32_bits & ~(1u << (i & (R - 1)))) | ((seg_f32 ? 1u : 0u) << (i & (R - 1)));
#pragma unroll
        for (int p = 0; p < NP; ++p) h3s_dma(slot + p * 1024, a_src[p] + (long long)cb * 128);
#pragma unroll
        for (int p = 0; p < NP; ++p) h3s_dma(slot + IMG + p * 1024, w_src[p] + (long long)lb * 128);
        ++lb;
        if (++cb >= seg_blocks && cs + 1 < P.nap) { cb = 0; set_aseg(++cs); }
    };

    f32x16 acc0[T][T], acc1[T][T];
#pragma unroll
    for (int i = 0; i < T; ++i)
#pragma unroll
        for (int j = 0; j < T; ++j)
#pragma unroll
            for (int r = 0; r < 16; ++r) { acc0[i][j][r] = 0.f; acc1[i][j][r] = 0.f; }
    const int fsw = (fr >> 1) & 7;
    constexpr int AHEAD = EARLY ? R : R - 1;             // blocks issued before the loop / kept ahead of the consumer
    for (int i = 0; i < AHEAD && i < n; ++i) issue(i);
    for (int i = 0; i < n; ++i) {
        if (!EARLY && i + R - 1 < n) issue(i + R - 1);   // its slot was consumed in iteration i - 1
        const int younger = n - 1 - i < R - 1 ? n - 1 - i : R - 1;    // blocks issued after block i, still in flight
        if (T == 1) {                                    // 8 DMA instructions per block
            if (R > 3 && younger == 3) asm volatile("s_waitcnt vmcnt(24)" ::: "memory");
            else if (R > 2 && younger == 2) asm volatile("s_waitcnt vmcnt(16)" ::: "memory");
            else if (younger == 1) asm volatile("s_waitcnt vmcnt(8)" ::: "memory");
            else asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        } else {                                         // 16
            if (younger == 1) asm volatile("s_waitcnt vmcnt(16)" ::: "memory");
            else asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        }
#if H3S_LAB_MODE == 1                                      // lab: DMA only (tools/h3s_lab_modes.sh; wrong results)
        if (EARLY) { if (i + R < n) issue(i + R); }
        continue;
#endif
        const char *img = lds + wave * (R * SLOT) + (i & (R - 1)) * SLOT + fr * 128;
        const bool af32 = (f32_bits >> (i & (R - 1))) & 1u;
        h8 a1[T][2], a2[T][2], b1[T][2], b2[T][2];
#if H3S_LAB_MODE == 3                                      // lab: MFMAs on constant fragments, no LDS reads
        for (int kk = 0; kk < 2; ++kk) for (int t = 0; t < T; ++t) for (int e = 0; e < 8; ++e) {
            a1[t][kk][e] = (_Float16)1.f; a2[t][kk][e] = (_Float16)1.f; b1[t][kk][e] = (_Float16)2.f; b2[t][kk][e] = (_Float16)3.f; }
        if (false)
#endif
#pragma unroll
        for (int t = 0; t < T; ++t)
            h3s_read_frags(img + t * 4096, img + IMG + t * 4096, af32, fh, fsw, a1[t], a2[t], b1[t], b2[t]);
        if (EARLY) {
            asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");        // the fragments are in registers: the slot is free
            if (i + R < n) issue(i + R);
        }
#if H3S_LAB_MODE == 2                                      // lab: DMA + fragment reads, no MFMAs
        for (int kk = 0; kk < 2; ++kk) for (int t = 0; t < T; ++t)
            asm volatile("" :: "v"(a1[t][kk]), "v"(a2[t][kk]), "v"(b1[t][kk]), "v"(b2[t][kk]));
        continue;
#endif
#pragma unroll
        for (int kk = 0; kk < 2; ++kk)
#pragma unroll
            for (int ti = 0; ti < T; ++ti)
#pragma unroll
                for (int tj = 0; tj < T; ++tj) {
                    acc0[ti][tj] = __builtin_amdgcn_mfma_f32_32x32x16_f16(a1[ti][kk], b1[tj][kk], acc0[ti][tj], 0, 0, 0);
                    acc1[ti][tj] = __builtin_amdgcn_mfma_f32_32x32x16_f16(a1[ti][kk], b2[tj][kk], acc1[ti][tj], 0, 0, 0);
                    acc1[ti][tj] = __builtin_amdgcn_mfma_f32_32x32x16_f16(a2[ti][kk], b1[tj][kk], acc1[ti][tj], 0, 0, 0);
                }
    }
#pragma unroll
    for (int i = 0; i < T; ++i)
#pragma unroll
        for (int j = 0; j < T; ++j)
#pragma unroll
            for (int r = 0; r < 16; ++r) acc0[i][j][r] = fmaf(acc1[i][j][r], ISC_SPLIT_LO_WEIGHT, acc0[i][j][r]);
    __syncthreads();                                     // every wave is done with its ring: LDS is free

    if constexpr (EPI == EPI_VOCAB) {
        if (NW == 8) {                                   // upper-half-of-K partials -> the wave that owns the block
            float *xch = smem + (wave & 3) * (16 * 64);
            if (wave >= 4) {
#pragma unroll
                for (int r = 0; r < 16; ++r) xch[r * 64 + lane] = acc0[0][0][r];
            }
            __syncthreads();
            if (wave < 4) {
#pragma unroll
                for (int r = 0; r < 16; ++r) acc0[0][0][r] += xch[r * 64 + lane];
            }
            __syncthreads();                             // the exchange area is the statistics' combine area next
        }
        f32x16 accv[1] = {acc0[0][0]};
        if (NW == 4 || wave < 4) epi_vocab_frag<Frag32, 1, 4, BM>(P, accv, 0, wave * 32, wave, lane, row0, col0, tn, smem);
        __syncthreads();
        h3s_vocab_combine<BM>(P, smem, tid, row0, tn);
        return;
    } else {
        // partial tile of this wave -> LDS
        float *mine = smem + wave * (BM * LDR);
#pragma unroll
        for (int i = 0; i < T; ++i)
#pragma unroll
            for (int j = 0; j < T; ++j)
#pragma unroll
                for (int r = 0; r < 16; ++r)
                    mine[(i * 32 + Frag32::row(r, lane)) * LDR + j * 32 + fr] = acc0[i][j][r];
        __syncthreads();
        if (NW > 4 && tid >= 256) return;                // the epilogue maps 256 threads onto the tile
        auto red = [&](int row, int col) __attribute__((always_inline)) {
            const float *q = smem + row * LDR + col;
            float v = ((q[0] + q[BM * LDR]) + q[2 * BM * LDR]) + q[3 * BM * LDR];   // fixed order: bit-repeatable
            if (NW == 8) v += ((q[4 * BM * LDR] + q[5 * BM * LDR]) + q[6 * BM * LDR]) + q[7 * BM * LDR];
            return v;
        };
        if constexpr (EPI == EPI_LINEAR) {
#pragma unroll
            for (int q = 0; q < T * T; ++q) {
                const int grp = tid + 256 * q;                       // float4 group of the tile
                const int row = grp / (BN / 4), c4 = (grp % (BN / 4)) * 4;
                const int gm = row0 + row, gn = col0 + c4;
                if (gm >= M || gn >= N) continue;
                float o[4];
#pragma unroll
                for (int e = 0; e < 4; ++e) o[e] = red(row, c4 + e);
                if (ksplit > 1) {                                    // raw partial sums (N % 4 == 0 on this route)
                    *reinterpret_cast<float4 *>(P.slab + (long long)ks * P.slab_stride + (long long)gm * N + gn) =
                        make_float4(o[0], o[1], o[2], o[3]);
                    continue;
                }
                epi_linear_finish<4>(P, gm, gn, o);
            }
        } else {
            constexpr int UN = 8 * T, NR = T * T;                    // units of the tile; rows per thread
            const int rbase = tid / UN, u = tid % UN;
            int gm[NR];
            bool ok[NR];
            float g[NR][4];
#pragma unroll
            for (int e = 0; e < NR; ++e) {
                const int row = rbase + e * (256 / UN);
                gm[e] = row0 + row;
                ok[e] = gm[e] < M;
#pragma unroll
                for (int k = 0; k < 4; ++k) g[e][k] = red(row, k * UN + u);
            }
            lstm_cells<NR>(P, gm, tn * UN + u, ok, g);
        }
    }
}

// ---------------------------------------------------------------- H3V: the vocabulary tile of few-hundred-row launches
// Same 32 x 128 tile, statistics and epilogue as gemm_h3s_kernel<EPI_VOCAB> (wave w owns columns 32 w .. 32 w + 31 over
// the whole K), different operand movement.  There every wave stages its own copy of the A block next to its W block in
// a private two-slot ring - A is fetched four times and ONE 8 KB block per wave is in flight: 64 KB per CU against a
// ~1.7 us round trip is ~9.5 TB/s over the chip, and 316 workgroups x 512 KB take the 20 us they are measured at
// (B = 128).  Here a k-block stage is shared by the workgroup: the A block once (each wave brings a quarter) + the four
// waves' W blocks = 20 KB, three stages (60 KB: two workgroups per CU), two blocks in flight behind the one being
// multiplied, one barrier per block: 320 KB per workgroup.  B = 128: 20.2 -> 18.2 us (kernel trace), roll-out 1.385 -> 1.32 ms.  (Tried first: W fragments straight from global memory into the
// MFMA operand registers, no LDS for W - a lane then touches 16 bytes of a 128-byte row line per instruction, the L1
// does not merge the four touches of a line, and the launch pulled ~4x its bytes from L2: 26 us.)
#ifndef H3V_STAGES
#define H3V_STAGES 3        // (four stages, 80 KB, measured the same: B = 128 roll-out 1.324 vs 1.323 ms)
#endif
#define H3V_STAGE_BYTES (5 * 4096)
template <bool AF32>
__global__ __launch_bounds__(256) void gemm_h3v_kernel(const DevLaunch L) {
    ISC_GATE_RETURN(L);
    rows_kernarg_warm<ROWS_KERNARG_LINES(DevLaunch)>();
    constexpr int BM = 32, BN = 128;
    extern __shared__ __attribute__((aligned(16))) float smem[];     // stages of [A image 4 KB | 4 W images 4 KB each]
    char *lds = reinterpret_cast<char *>(smem);
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    int pi, tm, tn, ks, ksplit;
    map_tile(L, pi, tm, tn, ks, ksplit);
    const DevProb &P = L.p[pi];
    const int M = P.M, N = P.N, Kp = P.Kp, nblk = Kp >> 5;
    const int row0 = tm * BM, col0 = tn * BN;
    const int fr = lane & 31, fh = lane >> 5, fsw = (fr >> 1) & 7;

    // DMA lanes (pieces of 8 rows x 128 B; lane position lane & 7 fetches chunk pos ^ swizzle(row): the image layout of
    // gemm_h3s_kernel).  A: wave w brings rows 8 w .. 8 w + 7 of the block; W: the wave's own 32 columns, four pieces.
    const DevASeg a = P.ap[0];
    const bool af32 = AF32 && a.hi == nullptr;
    const char *asrc;
    const char *wsrc[4];
    {
        const int prow = 8 * wave + (lane >> 3);
        const int ar = row0 + prow < M ? row0 + prow : M - 1;
        const int choff = ((lane & 7) ^ ((prow >> 1) & 7)) * 16;
        asrc = af32 ? reinterpret_cast<const char *>(P.seg[0].A + (long long)ar * P.seg[0].lda) + choff
                    : reinterpret_cast<const char *>(a.hi + (long long)ar * a.ld) + choff;
#pragma unroll
        for (int p = 0; p < 4; ++p) {
            const int r = 8 * p + (lane >> 3);
            const int c = col0 + wave * 32 + r;
            wsrc[p] = reinterpret_cast<const char *>(P.Wh) + (long long)(c < N ? c : N - 1) * 4 * Kp +
                      ((lane & 7) ^ ((r >> 1) & 7)) * 16;
        }
    }
    const unsigned lds0 = __builtin_amdgcn_readfirstlane((unsigned)(size_t)lds);
    auto issue = [&](int b, int stage) __attribute__((always_inline)) {       // 5 DMA instructions per wave
        const unsigned base = lds0 + stage * H3V_STAGE_BYTES;
        h3s_dma(base + wave * 1024, asrc + (long long)b * 128);
#pragma unroll
        for (int p = 0; p < 4; ++p) h3s_dma(base + 4096 + wave * 4096 + p * 1024, wsrc[p] + (long long)b * 128);
    };
    f32x16 acc0, acc1;
#pragma unroll
    for (int r = 0; r < 16; ++r) { acc0[r] = 0.f; acc1[r] = 0.f; }
    constexpr int AHEAD = H3V_STAGES - 1;                  // blocks in flight behind the one being multiplied
    static_assert(AHEAD >= 1 && AHEAD <= 4, "stages");
#pragma unroll
    for (int i = 0; i < AHEAD; ++i)
        if (i < nblk) issue(i, i);
    int st = 0;                                            // stage of block b
    for (int b = 0; b < nblk; ++b) {
        const int younger = nblk - 1 - b < AHEAD - 1 ? nblk - 1 - b : AHEAD - 1;    // blocks issued after block b
        if (younger >= 3) asm volatile("s_waitcnt vmcnt(15)" ::: "memory");
        else if (younger == 2) asm volatile("s_waitcnt vmcnt(10)" ::: "memory");
        else if (younger == 1) asm volatile("s_waitcnt vmcnt(5)" ::: "memory");
        else asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        __syncthreads();                                   // block b is in LDS for every wave; stage of block b - 1 is free
        if (b + AHEAD < nblk) issue(b + AHEAD, st == 0 ? H3V_STAGES - 1 : st - 1);
        const char *ia = lds + st * H3V_STAGE_BYTES + fr * 128;
        const char *iw = ia + 4096 + wave * 4096;
        h8 a1[2], a2[2], b1[2], b2[2];
        h3s_read_frags(ia, iw, af32, fh, fsw, a1, a2, b1, b2);
#pragma unroll
        for (int kk = 0; kk < 2; ++kk) {
            acc0 = __builtin_amdgcn_mfma_f32_32x32x16_f16(a1[kk], b1[kk], acc0, 0, 0, 0);
            acc1 = __builtin_amdgcn_mfma_f32_32x32x16_f16(a1[kk], b2[kk], acc1, 0, 0, 0);
            acc1 = __builtin_amdgcn_mfma_f32_32x32x16_f16(a2[kk], b1[kk], acc1, 0, 0, 0);
        }
        st = st == H3V_STAGES - 1 ? 0 : st + 1;
    }
#pragma unroll
    for (int r = 0; r < 16; ++r) acc0[r] = fmaf(acc1[r], ISC_SPLIT_LO_WEIGHT, acc0[r]);
    __syncthreads();                                     // every wave is done with the stages: LDS is free
    f32x16 accv[1] = {acc0};
    epi_vocab_frag<Frag32, 1, 4, BM>(P, accv, 0, wave * 32, wave, lane, row0, col0, tn, smem);
    __syncthreads();
    h3s_vocab_combine<BM>(P, smem, tid, row0, tn);
}

// ---------------------------------------------------------------- split-K reduction + epilogue
// Sums the ksplit partial slabs in a fixed order (deterministic) and applies the epilogue the
// single-pass kernel would have applied.  blockIdx.y = problem.
__global__ __launch_bounds__(256) void splitk_linear_kernel(const DevLaunch L) {
    ISC_GATE_RETURN(L);
    rows_kernarg_warm<ROWS_KERNARG_LINES(DevLaunch)>();      // (one batch of scalar loads for the launch descriptor: common.h)
    const DevProb &P = L.p[blockIdx.y];
    const long long n4 = (long long)P.M * (P.N >> 2);
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    if (i >= n4) return;
    const int N = P.N, gm = (int)(i / (N >> 2)), gn = (int)(i % (N >> 2)) * 4;
    const float *sl = P.slab + (long long)gm * N + gn;
    float4 part[16];                            // every slab's float4 in flight before the first add
    const int S = P.ksplit;
#pragma unroll
    for (int s = 0; s < 16; ++s)
        part[s] = s < S ? *reinterpret_cast<const float4 *>(sl + (long long)s * P.slab_stride)
                        : make_float4(0.f, 0.f, 0.f, 0.f);
    float4 v = part[0];
#pragma unroll
    for (int s = 1; s < 16; ++s) { v.x += part[s].x; v.y += part[s].y; v.z += part[s].z; v.w += part[s].w; }
    float o[4] = {v.x, v.y, v.z, v.w};
    epi_linear_finish<4>(P, gm, gn, o);                 // (N % 4 == 0 on this route: no column past the border)
}

// (64 slab values in flight leave 16 registers of the 6-waves-per-SIMD budget, which the allocator meets or misses by
// two registers from build to build: the budget is stated)
__global__ __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(6))) void splitk_lstm_kernel(const DevLaunch L) {
    ISC_GATE_RETURN(L);
    const DevProb &P = L.p[0];
    const int H = P.H;
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    if (i >= (long long)P.M * H) return;
    const int gm = (int)(i / H), unit = (int)(i % H);
    // all 4 x ksplit slab values are requested before the first add: summed one by one behind a runtime
    // trip count they were 16 dependent L2 round trips (15 us for a [4 x 2048] cell update)
    float part[4][16];
    const int S = P.ksplit;                   // <= 16 (plan_splitk)
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        const float *sl = P.slab + (long long)gm * 4 * H + k * H + unit;
#pragma unroll
        for (int s = 0; s < 16; ++s) part[k][s] = s < S ? sl[(long long)s * P.slab_stride] : 0.f;
    }
    const int gma[1] = {gm};
    const bool ok[1] = {true};
    float g[1][4];
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        float a = part[k][0];
#pragma unroll
        for (int s = 1; s < 16; ++s) a += part[k][s];      // fixed order; the unused slots add 0
        g[0][k] = a;
    }
    // the sums are formed here: left to sink below the cell's loads, the 64 slab values would stay live across them
    asm volatile("" : "+v"(g[0][0]), "+v"(g[0][1]), "+v"(g[0][2]), "+v"(g[0][3]));
    lstm_cells<1>(P, gma, unit, ok, g);
}

// The statistics of one row's 128-column tile tn on one wave: lane l holds the contraction sums v[h] of columns
// 128 tn + l + 64 h.  Adds the bias, optionally writes the logits, and emits the tile's (max, arg-max, sum exp) the
// tile kernels' epilogue would have produced.
__device__ __forceinline__ void wave_vocab_tile128(const DevProb &P, int gm, int tn, const float (&v)[2], int lane) {
    float x[2];
    int col[2];
#pragma unroll
    for (int h = 0; h < 2; ++h) {
        col[h] = tn * 128 + lane + 64 * h;
        const bool ok = col[h] < P.N;
        x[h] = ok ? v[h] + P.bias0[col[h]] : -INFINITY;
        if (ok && P.C) P.C[(long long)gm * P.ld_logits + col[h]] = x[h];
    }
    float mx = x[0];
    int ix = col[0];
    if (x[1] > mx) { mx = x[1]; ix = col[1]; }             // equal: the lower column (h = 0) stays
    wave_argmax(mx, ix);
    float sm = (x[0] > -INFINITY ? __expf(x[0] - mx) : 0.f) + (x[1] > -INFINITY ? __expf(x[1] - mx) : 0.f);
    sm = wave_sum(sm);
    if (lane == 0) {
        const long long o = (long long)gm * P.ntile_total + tn;
        P.pmax[o] = mx;
        P.psum[o] = sm;
        P.pidx[o] = ix;
    }
}

// Vocabulary projection by split-K (few rows): sums the slabs in fixed order, adds the bias, optionally
// writes the logits, and emits the per-128-column (max, arg-max, sum exp) the single-pass kernel's epilogue
// would have produced.  One wavefront per (row, column tile): lane l holds columns l and l + 64 of the tile.
__global__ __launch_bounds__(256) void splitk_vocab_kernel(const DevLaunch L) {
    ISC_GATE_RETURN(L);
    const DevProb &P = L.p[0];
    const int lane = threadIdx.x & 63;
    const long long w = (long long)blockIdx.x * 4 + (threadIdx.x >> 6);
    const int n_tile = P.ntile_total;
    if (w >= (long long)P.M * n_tile) return;
    const int gm = (int)(w / n_tile), tn = (int)(w % n_tile);
    const int N = P.N, S = P.ksplit;
    float v[2];
#pragma unroll
    for (int h = 0; h < 2; ++h) {
        const int col = tn * 128 + lane + 64 * h;
        const bool ok = col < N;
        const float *sl = P.slab + (long long)gm * N + (ok ? col : 0);
        float part[16];
#pragma unroll
        for (int s = 0; s < 16; ++s) part[s] = (ok && s < S) ? sl[(long long)s * P.slab_stride] : 0.f;
        float a = part[0];
#pragma unroll
        for (int s = 1; s < 16; ++s) a += part[s];
        v[h] = a;
    }
    wave_vocab_tile128(P, gm, tn, v, lane);
}

// ---------------------------------------------------------------- few rows: fused GEMV kernels (exact fp32)
// Beam rows of one image (5), roll-outs of a handful of captions: with M <= 8 rows a "GEMM" is M matrix-vector
// products that stream the weights once - no tile shape reuses anything, the 32-row MFMA tiles of the skinny kernel
// are 84-97 % padding, and its launches sit at the latency of their 8-block DMA chains (LSTM cell at 5 rows: 9.4 us
// for 16.8 MB of weight planes = 1.8 TB/s).  Here the weights are read as they are (fp32, no planes, no split - the
// arithmetic is exact fp32 FMA) by wide per-lane loads with the whole launch's traffic in flight at once:
//   * a workgroup (4 waves) stages the M activation rows [M, K] of the launch in LDS (fp32, all segments, <= 128 KB);
//   * a wave owns 4 weight rows at a time (linear / vocabulary: 4 consecutive output columns; LSTM: the i, f, g, o
//     rows of one hidden unit); lane l takes the float4 at k = 256 c + 4 l of each row for up to 8 chunks c - 32
//     loads of 16 B per lane in flight (the vocabulary tile: 8 rows x 2 chunks) - and accumulates 4 x M dot products;
//   * the 4 M (<= 32) per-lane sums are reduced across the 64 lanes by a reduce-scatter butterfly (each step halves
//     the values a lane carries: 31 shuffles instead of 32 x 6), fixed order, deterministic;
//   * epilogues from LDS: linear (biases, accumulate, ReLU, keep-mask, pre-mask copy), LSTM cell (lstm_cells<1>: the
//     same code as the tile kernels - hoisted term, token-table row, planes of h for consumers, saved gates),
//     vocabulary (logits + the per-128-column max / arg-max / sum-exp statistics of the tile kernels' epilogue).
// north_star's "fused LSTM gate GEMV + sigmoid/tanh" is this kernel's <EPI_LSTM> form.
#define GEMV_MAX_ROWS 8
#define GEMV_MAX_K 4096
// v[0 .. NV) per lane -> after the call v[0] of lane l holds the 64-lane sum of value index l / (64 / NV).
template <int HALF, int MASK, int NV>
__device__ __forceinline__ void wave_reduce_scatter_step(float (&v)[NV], int lane) {
    const bool up = (lane & MASK) != 0;
#pragma unroll
    for (int i = 0; i < HALF; ++i) {
        const float send = up ? v[i] : v[i + HALF];
        const float keep = up ? v[i + HALF] : v[i];
        v[i] = keep + __shfl_xor(send, MASK, 64);
    }
    if constexpr (HALF > 1) wave_reduce_scatter_step<HALF / 2, MASK / 2, NV>(v, lane);
}
template <int NV>
__device__ __forceinline__ void wave_reduce_scatter(float (&v)[NV], int lane) {
    static_assert(NV == 32 || NV == 64, "4 or 8 weight rows x 8 activation rows");
    wave_reduce_scatter_step<NV / 2, 32, NV>(v, lane);
    if (NV == 32) v[0] += __shfl_xor(v[0], 1, 64);
}

// One batch of CB 256-wide k-chunks: NR x CB unconditional 16-byte loads per lane (a lane past the segment's end reads
// the row's last float4 again and meets a zero activation: no branch sits between a load and its use, so the loads
// stay in flight together - a predicated load gets its own s_waitcnt), then the FMAs.
template <int NR, int CB>
__device__ __forceinline__ void gemv_batch(const float *Wb, const long long (&wrow)[NR], long long ldw, int Ks, int c0,
                                           const float *Ak, int Ktot, int lane, float (&acc)[NR * GEMV_MAX_ROWS]) {
    constexpr int MR = GEMV_MAX_ROWS;
    float4 w[NR][CB];
    int kc[CB];
    bool in[CB];
#pragma unroll
    for (int c = 0; c < CB; ++c) {
        const int kk = c0 + c * 256 + lane * 4;
        in[c] = kk < Ks;
        kc[c] = in[c] ? kk : Ks - 4;
    }
#pragma unroll
    for (int r = 0; r < NR; ++r)
#pragma unroll
        for (int c = 0; c < CB; ++c) w[r][c] = *reinterpret_cast<const float4 *>(Wb + wrow[r] * ldw + kc[c]);
#pragma unroll
    for (int c = 0; c < CB; ++c) {
#pragma unroll
        for (int m = 0; m < MR; ++m) {
            float4 a = *reinterpret_cast<const float4 *>(Ak + (long long)m * Ktot + kc[c]);
            a.x = in[c] ? a.x : 0.f; a.y = in[c] ? a.y : 0.f; a.z = in[c] ? a.z : 0.f; a.w = in[c] ? a.w : 0.f;
#pragma unroll
            for (int r = 0; r < NR; ++r) {
                float t = acc[r * MR + m];
                t = fmaf(w[r][c].x, a.x, t);
                t = fmaf(w[r][c].y, a.y, t);
                t = fmaf(w[r][c].z, a.z, t);
                t = fmaf(w[r][c].w, a.w, t);
                acc[r * MR + m] = t;
            }
        }
    }
}

// NQ x 4 weight rows against the MR staged activation rows over this wave's share of K: chunks [g_lo, g_hi) of the
// launch's chunk list (the segments' 256-wide chunks, concatenated); at most CBMAX chunks per batch.
template <int NQ, int CBMAX>
__device__ __forceinline__ void gemv_accumulate(const DevProb &P, const long long (&wrow)[NQ * 4], const float *As,
                                                int Ktot, int lane, int g_lo, int g_hi,
                                                float (&acc)[NQ * 4 * GEMV_MAX_ROWS]) {
    constexpr int NR = NQ * 4, MR = GEMV_MAX_ROWS;
#pragma unroll
    for (int i = 0; i < NR * MR; ++i) acc[i] = 0.f;
    int koff = 0, g0 = 0;
    for (int s = 0; s < P.nseg; ++s) {
        const int Ks = P.seg[s].K, nch = (Ks + 255) >> 8;
        const float *Wb = P.seg[s].W;
        const long long ldw = P.seg[s].ldw;
        const float *Ak = As + koff;
        const int lo = g_lo > g0 ? g_lo - g0 : 0, hi = g_hi - g0 < nch ? g_hi - g0 : nch;   // this segment's chunks (uniform)
        int c0 = lo * 256, rem = hi - lo;
        if constexpr (CBMAX >= 8) {
            while (rem >= 8) { gemv_batch<NR, 8>(Wb, wrow, ldw, Ks, c0, Ak, Ktot, lane, acc); c0 += 2048; rem -= 8; }
        }
        if constexpr (CBMAX >= 4) {
            while (rem >= 4) { gemv_batch<NR, 4>(Wb, wrow, ldw, Ks, c0, Ak, Ktot, lane, acc); c0 += 1024; rem -= 4; }
        }
        while (rem >= 2) { gemv_batch<NR, 2>(Wb, wrow, ldw, Ks, c0, Ak, Ktot, lane, acc); c0 += 512; rem -= 2; }
        if (rem >= 1) gemv_batch<NR, 1>(Wb, wrow, ldw, Ks, c0, Ak, Ktot, lane, acc);
        koff += Ks;
        g0 += nch;
    }
}

// NW waves per workgroup.  Linear / LSTM (NW = 4): a tile is 4 / KS quads (4 output columns, or the 4 gate rows of a
// hidden unit), each contracted by KS waves over 1 / KS of the chunk list (P.ksplit = KS in {1, 2, 4}: long contractions
// spread over more waves so that every wave's loads fit one batch and the launch fills the chip - the LSTM cell over
// K = 2048 at KS = 2 is 256 workgroups of 4 waves with 16 loads each); the KS partial sums meet in LDS in fixed order.
// Vocabulary (NW = 8): a tile is 128 columns (its statistics are per 128), wave w takes columns 16 w .. 16 w + 15 in
// two rounds of 8 rows.
template <int EPI, int NW>
__global__ __launch_bounds__(64 * NW) void gemv_rows_kernel(const DevLaunch L) {
    ISC_GATE_RETURN(L);
    rows_kernarg_warm<ROWS_KERNARG_LINES(DevLaunch)>();      // (one batch of scalar loads for the launch descriptor: common.h)
    constexpr int MR = GEMV_MAX_ROWS, NT = 64 * NW;
    extern __shared__ __attribute__((aligned(16))) float smem[];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    int pi = 0;
    if (L.nprob > 1 && (int)blockIdx.x >= L.p[1].tile_start) pi = 1;
    if (L.nprob > 2 && (int)blockIdx.x >= L.p[2].tile_start) pi = 2;
    const DevProb &P = L.p[pi];
    const int tile = blockIdx.x - P.tile_start;
    const int M = P.M, N = P.N;
    int Ktot = 0, nchunk = 0;
    for (int s = 0; s < P.nseg; ++s) { Ktot += P.seg[s].K; nchunk += (P.seg[s].K + 255) >> 8; }
    float *As = smem;                                   // [MR][Ktot]
    float *red = smem + (long long)MR * Ktot;           // linear / LSTM: [4 waves][32]; vocabulary: [MR][128]
    {                                                   // stage the activations (rows >= M: zeros)
        int koff = 0;
        for (int s = 0; s < P.nseg; ++s) {
            const int Ks = P.seg[s].K, q4 = Ks >> 2;
            const float *Ab = P.seg[s].A;
            const long long lda = P.seg[s].lda;
            for (int k4 = tid; k4 < q4; k4 += NT) {     // all MR row loads of a column in flight (rows >= M: row M - 1)
                float4 v[MR];
#pragma unroll
                for (int m = 0; m < MR; ++m)
                    v[m] = *reinterpret_cast<const float4 *>(Ab + (long long)(m < M ? m : M - 1) * lda + k4 * 4);
#pragma unroll
                for (int m = 0; m < MR; ++m) {
                    if (m >= M) v[m] = make_float4(0.f, 0.f, 0.f, 0.f);
                    *reinterpret_cast<float4 *>(As + (long long)m * Ktot + koff + k4 * 4) = v[m];
                }
            }
            koff += Ks;
        }
    }
    __syncthreads();

    if constexpr (EPI == EPI_VOCAB) {
        const int col0 = tile * 128;
        for (int rnd = 0; rnd < 2; ++rnd) {
            long long wrow[8];
#pragma unroll
            for (int r = 0; r < 8; ++r) {
                const int c = col0 + wave * 16 + rnd * 8 + r;
                wrow[r] = c < N ? c : N - 1;
            }
            float acc[8 * MR];
            gemv_accumulate<2, 2>(P, wrow, As, Ktot, lane, 0, nchunk, acc);
            wave_reduce_scatter<64>(acc, lane);          // lane l: value (row r = l / 8 of the round, m = l % 8)
            red[(lane & 7) * 128 + wave * 16 + rnd * 8 + (lane >> 3)] = acc[0];
        }
        __syncthreads();
        for (int m = wave; m < M; m += NW) {
            const float v[2] = {red[m * 128 + lane], red[m * 128 + lane + 64]};
            wave_vocab_tile128(P, m, tile, v, lane);
        }
    } else {
        const int KS = P.ksplit;                         // 1, 2 or 4 (gemv_run)
        const int qpw = NW / KS;                         // quads per workgroup
        const int qw = wave / KS, ks = wave - qw * KS;   // this wave: quad qw of the tile, k-slice ks
        const int quad = tile * qpw + qw;
        long long wrow[4];
        bool live;
        if constexpr (EPI == EPI_LSTM) {
            live = quad < P.H;
#pragma unroll
            for (int r = 0; r < 4; ++r) wrow[r] = (long long)r * P.H + (live ? quad : 0);
        } else {
            live = quad * 4 < N;
#pragma unroll
            for (int r = 0; r < 4; ++r) { const int c = quad * 4 + r; wrow[r] = c < N ? c : N - 1; }
        }
        float acc[4 * MR];
        gemv_accumulate<1, 8>(P, wrow, As, Ktot, lane, nchunk * ks / KS, nchunk * (ks + 1) / KS, acc);
        wave_reduce_scatter<32>(acc, lane);              // lanes 2 i, 2 i + 1: value i = (row r = i / 8, m = i % 8)
        if ((lane & 1) == 0) red[wave * 32 + (lane >> 1)] = acc[0];
        __syncthreads();
        if (ks == 0 && live) {                           // the quad's first wave sums the KS partials in order
            const float *rq = red + wave * 32;
            if constexpr (EPI == EPI_LSTM) {
                if (lane < M) {
                    const int gm[1] = {lane};
                    const bool ok[1] = {true};
                    float g[1][4];
#pragma unroll
                    for (int k = 0; k < 4; ++k) {
                        float v = rq[k * MR + lane];
                        for (int j = 1; j < KS; ++j) v += rq[j * 32 + k * MR + lane];
                        g[0][k] = v;
                    }
                    lstm_cells<1>(P, gm, quad, ok, g);
                }
            } else {
                const int m = lane >> 2, e = lane & 3, n = quad * 4 + e;
                if (lane < 4 * MR && m < M && n < N) {
                    float o[1] = {rq[e * MR + m]};
                    for (int j = 1; j < KS; ++j) o[0] += rq[j * 32 + e * MR + m];
                    epi_linear_finish<1>(P, m, n, o);
                }
            }
        }
    }
}

// ---------------------------------------------------------------- host side
static int check_segs(const isc_seg *seg, int nseg) {
    if (nseg < 1 || nseg > ISC_MAX_SEG) return ISC_E_SHAPE;
    for (int s = 0; s < nseg; ++s) {
        if (!seg[s].A || !seg[s].W) return ISC_E_NULL;
        if (seg[s].K <= 0 || (seg[s].K % BK) != 0) return ISC_E_SHAPE;
        if ((seg[s].lda & 3) || (seg[s].ldw & 3)) return ISC_E_ALIGN;
        if (!isc_aligned16(seg[s].A) || !isc_aligned16(seg[s].W)) return ISC_E_ALIGN;
    }
    return ISC_OK;
}

static void copy_segs(DevProb &d, const isc_seg *seg, int nseg) {
    d.nseg = nseg;
    for (int s = 0; s < nseg; ++s) {
        d.seg[s].A = seg[s].A; d.seg[s].W = seg[s].W;
        d.seg[s].lda = seg[s].lda; d.seg[s].ldw = seg[s].ldw; d.seg[s].K = seg[s].K; d.seg[s].a_f16 = seg[s].a_f16;
        d.seg[s].A_hi = static_cast<const _Float16 *>(seg[s].A_hi);
        d.seg[s].A_lo = static_cast<const _Float16 *>(seg[s].A_lo);
    }
}

// isc_seg.a_f16: A holds _Float16 rows.  Only isc_linear_fwd on the large split-f16 kernels reads them; every other entry
// point answers ISC_E_SHAPE in front of any launch (a kernel must never read halfs as floats).
static bool segs_any_f16(const isc_seg *seg, int nseg) {
    for (int s = 0; s < nseg && s < ISC_MAX_SEG; ++s)
        if (seg[s].a_f16) return true;
    return false;
}

// A kernel launched with more than 64 KB of dynamic LDS has its limit raised once (k1: a second kernel under the same
// flag).  `done` is the call site's own flag; idempotent: a race only repeats the same call.
template <class K>
static int lds_attr_once(std::atomic<bool> &done, size_t bytes, K k0, K k1 = nullptr) {
    if (bytes <= 65536 || done.load()) return ISC_OK;
    for (K k : {k0, k1}) {
        if (!k) continue;
        hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void *>(k), hipFuncAttributeMaxDynamicSharedMemorySize,
                                           (int)bytes);
        if (e != hipSuccess) return (int)e;
    }
    done.store(true);
    return ISC_OK;
}

// isc_f32_launches(kind): launches of the exact-fp32 kernels so far, by kind (a failed launch counts too).  0 / 1 / 2 =
// gemm_kernel on the 128 / 64 / 32-row tile (every layout and epilogue), 3 = XL, 4 = LD, 5 = MD, 6 = a split-K reduce.
enum { F32_KIND_XL = 3, F32_KIND_LD = 4, F32_KIND_MD = 5, F32_KIND_REDUCE = 6, F32_KINDS = 7 };
static std::atomic<long long> g_f32_launches[F32_KINDS];
extern "C" long long isc_f32_launches(int kind) {
    return kind >= 0 && kind < F32_KINDS ? g_f32_launches[kind].load() : -1;
}

template <int WM, int WN, int TN, int EPI, bool AKM, bool BKM>
static int launch_cfg(const DevLaunch &L, hipStream_t st) {
    constexpr int BM = 32 * WM, BN = 32 * TN * WN;
    constexpr size_t k_bytes = (size_t)2 * (Tile<BM, AKM>::SIZE + Tile<BN, BKM>::SIZE) * sizeof(float);
    constexpr size_t c_bytes = (size_t)BM * (BN + 4) * sizeof(float);
    constexpr size_t lds = k_bytes > c_bytes ? k_bytes : c_bytes;
    static std::atomic<bool> attr_set{false};
    if (int rc = lds_attr_once(attr_set, lds, &gemm_kernel<WM, WN, TN, EPI, AKM, BKM>)) return rc;
    hipLaunchKernelGGL((gemm_kernel<WM, WN, TN, EPI, AKM, BKM>), dim3(L.total_tiles), dim3(256), lds, st, L);
    ++g_f32_launches[WM == 4 ? 0 : (WM == 2 ? 1 : 2)];
    ISC_LAUNCH_CHECK();
    return ISC_OK;
}

template <class G, int EPI>
static constexpr auto f32_dma_kernel() {
    if constexpr (std::is_same_v<G, F32TileXL>) return &gemm_xl_kernel<EPI>;
    else if constexpr (std::is_same_v<G, F32TileLD>) return &gemm_ld_kernel<EPI>;
    else return &gemm_md_kernel;
}

// One launch of an fp32 LDS-DMA tile kernel of geometry G (the tiling of L is the caller's).
template <class G, int EPI>
static int launch_f32_dma(const DevLaunch &L, hipStream_t st) {
    static_assert(EPI == EPI_LINEAR || !std::is_same_v<G, F32TileMD>, "the 64-row kernel has the linear epilogue only");
    constexpr size_t lds = G::LDS_BYTES;       // XL 147456: one workgroup per CU; LD 65536: two; MD 49152: three
    constexpr auto kernel = f32_dma_kernel<G, EPI>();
    static std::atomic<bool> attr_set{false};
    if (int rc = lds_attr_once(attr_set, lds, kernel)) return rc;
    hipLaunchKernelGGL(kernel, dim3(L.total_tiles), dim3(G::THREADS), lds, st, L);
    ++g_f32_launches[std::is_same_v<G, F32TileXL> ? F32_KIND_XL : (std::is_same_v<G, F32TileLD> ? F32_KIND_LD : F32_KIND_MD)];
    ISC_LAUNCH_CHECK();
    return ISC_OK;
}

// Tile shapes: 0 = L 128x128 (4 waves stacked in M), 1 = M 64x128 (2x2 waves; MD by LDS-DMA for plain linear NT launches),
// 2 = S 32x128 (4 waves in N), 3 = XL 256x128 (LDS-DMA ring, NT layout only), 4 = LD 128x128 by LDS-DMA (NT layout only)
static const int kTileBM[5] = {128, F32TileMD::BM, 32, F32TileXL::BM, F32TileLD::BM};

static std::atomic<int> g_md_enabled{1};   // isc_set_tile_override(102 / 103): MD path off / on (A/B measurements)

template <int EPI, bool AKM, bool BKM>
static int launch_any(const DevLaunch &L, int tile, hipStream_t st) {
    if constexpr (EPI == EPI_LINEAR && !AKM && !BKM) {
        if (tile == 1 && g_md_enabled.load()) {
            bool plain = true;
            for (int i = 0; i < L.nprob; ++i) plain = plain && L.p[i].ksplit <= 1;
            if (plain) return launch_f32_dma<F32TileMD, EPI_LINEAR>(L, st);
        }
    }
    if constexpr (!AKM && !BKM) {
        if (tile == 3) return launch_f32_dma<F32TileXL, EPI>(L, st);
        if (tile == 4) return launch_f32_dma<F32TileLD, EPI>(L, st);
    }
    if (tile == 0) return launch_cfg<4, 1, 4, EPI, AKM, BKM>(L, st);
    if (tile == 1) return launch_cfg<2, 2, 2, EPI, AKM, BKM>(L, st);
    return launch_cfg<1, 4, 1, EPI, AKM, BKM>(L, st);
}

// bm x bn output tiles, summed over the problems of a launch
static long long count_tiles(const DevLaunch &L, int bm, int bn) {
    long long t = 0;
    for (int i = 0; i < L.nprob; ++i) t += (long long)((L.p[i].M + bm - 1) / bm) * ((L.p[i].N + bn - 1) / bn);
    return t;
}

// Tile shape choice by a small cost model.  The most loaded CU works through n = ceil(blocks / 256)
// workgroups; its time is n * BM / efficiency, where the efficiency depends on the tile (MFMAs per
// staged byte and per barrier) and on how many workgroups share the CU (the 128/64/32-row tiles rely
// on a co-resident workgroup to cover their chunk-boundary stalls, the XL tile is pipelined to run
// alone).  Calibrated on tools/gemm_big.py / gemm_bench.py.
// Process-wide tuning knobs (tile override, split-f16 mode): plain configuration words, read once per launch
// (atomics: flipping them from another thread is a data-race-free, if pointless, thing to do).  They select a
// kernel; they carry no data between calls.
static std::atomic<int> g_tile_override{-1};
extern "C" int isc_set_tile_override(int tile) {
    if (tile == 102 || tile == 103) {          // measurement switch for the MD path, leaves the tile choice alone
        g_md_enabled.store(tile == 103);
        return g_tile_override.load();
    }
    return g_tile_override.exchange((tile >= 0 && tile <= 4) ? tile : -1);
}

// nt: the launch is in the NT layout (the LDS-DMA tiles XL / LD exist for it; MD replaces M for the linear epilogue
// inside launch_any); use_ld: let the cost model consider the LD tile
static int pick_tile(const DevLaunch &L, bool allow_xl, bool nt = true, bool use_ld = true) {
    const int ovr = g_tile_override.load();
    if (ovr == 4) return nt ? 4 : 0;
    if (ovr >= 0) return (ovr == 3 && !allow_xl) ? 0 : ovr;
    static const double eff[5][3] = {{0.80, 1.00, 1.00},    // L : 1, 2, >=3 workgroups on the busiest CU
                                     {0.55, 0.80, 0.90},    // M
                                     {0.35, 0.50, 0.62},    // S
                                     {1.10, 1.10, 1.10},    // XL
                                     {0.85, 1.06, 1.12}};   // LD
    int best = 0;
    double best_cost = 1e30;
    static const int order[5] = {3, 4, 0, 1, 2};            // larger / DMA tiles first: they win near-ties
    for (int k = 0; k < 5; ++k) {
        const int t = order[k];
        if (t == 3 && !allow_xl) continue;
        if (t == 4 && !(nt && use_ld)) continue;
        const long long n = (count_tiles(L, kTileBM[t], 128) + 255) / 256;
        const double cost = (double)n * kTileBM[t] / eff[t][n >= 3 ? 2 : (int)n - 1];
        if (cost < best_cost * 0.97) { best_cost = cost; best = t; }
    }
    return best;
}

static void finish_tiling(DevLaunch &L, int tile) {
    const int BM = kTileBM[tile], BN = 128;
    int start = 0;
    for (int i = 0; i < L.nprob; ++i) {
        DevProb &p = L.p[i];
        p.tiles_m = (p.M + BM - 1) / BM;
        p.tiles_n = (p.N + BN - 1) / BN;
        p.tile_start = start;
        long long wbytes = 0, abytes = 0;
        for (int s = 0; s < p.nseg; ++s) { wbytes += (long long)p.N * p.seg[s].K; abytes += (long long)p.M * p.seg[s].K; }
        p.m_fastest = wbytes > abytes;  // partition the larger operand across XCDs
        p.grp_n = (p.tiles_n + 7) / 8;
        // ... or the smaller one when the fabric-traffic estimate of the grouped order is under half of row-major's: the C workgroups an XCD runs at a
        // time form an a x b block of tiles and fetch a row panels + b column panels per round; a weight slice that
        // fits the XCD's L2 is fetched once.  (The classifier at B = 16384 has the larger A, and row-major order put
        // 64 different weight panels per round through each L2: 2.7 GB per launch, r03_e PMC; grouped: 8 A + W = 0.3 GB.)
        {
            const double Ap = 4.0 * BM * (double)(abytes / (p.M > 0 ? p.M : 1)), Wp = 4.0 * BN * (double)(wbytes / (p.N > 0 ? p.N : 1));
            const double A = 4.0 * abytes, W = 4.0 * wbytes, L2 = 3.0 * 1048576.0;
            const int C = BM >= 256 ? 32 : 64;
            const double rounds = (double)p.tiles_m * p.tiles_n / (8.0 * C);
            const int b = p.tiles_n < C ? p.tiles_n : C, a = C / p.tiles_n > 1 ? C / p.tiles_n : 1;
            const double row = W <= L2 ? A + 8.0 * W : 8.0 * rounds * (a * Ap + b * Wp);
            const int gb = p.grp_n < C ? p.grp_n : C, ga = C / p.grp_n > 1 ? C / p.grp_n : 1;
            const double grp = p.grp_n * Wp <= L2 ? 8.0 * A + W : 8.0 * rounds * (ga * Ap + gb * Wp);
            if (!p.m_fastest && grp < 0.5 * row) p.m_fastest = 1;   // (the opposite switch measured worse at B = 128)
        }
        start += p.tiles_m * p.tiles_n * (p.ksplit > 1 ? p.ksplit : 1);
    }
    L.total_tiles = start;
}

// ---- split-f16 path (gemm_h3_kernel) ----
// isc_set_h3_mode: 0 = off, 1 = auto, 2 = large kernels whenever the shapes allow, 3 / 4 = skinny kernel (32 / 64 tiles)
static std::atomic<int> g_h3_mode{1};
static std::atomic<long long> g_h3_launches{0}, g_h3x_launches{0}, g_h3_f16a_launches{0};
// isc_h3_kernel_launches(kind): launches of the split-f16 kernels so far, by instantiation (a failed launch counts too;
// the epilogue is the entry point's, so it has no kind).  3 g + f = a large tile of geometry g (0 / 1 / 2 = 128 / 256 /
// 64 rows) reading its activations as planes (f = 0), fp32 rows (1) or f16 rows (2); 9 / 10 / 11 = gemm_h3s_kernel 32 x
// 32 on four waves, on eight, 64 x 64; 12 / 13 = its vocabulary form 32 x 128 on four / eight waves; 14 / 15 =
// gemm_h3v_kernel on planes / on fp32 rows; 16 = an h3_split_kernel launch (plain or transposing, any number of jobs).
enum { H3_KIND_TILE = 0, H3_KIND_S32 = 9, H3_KIND_S32_W8 = 10, H3_KIND_S64 = 11, H3_KIND_SV = 12, H3_KIND_SV_W8 = 13,
       H3_KIND_V = 14, H3_KIND_V_F32 = 15, H3_KIND_SPLIT = 16, H3_KINDS = 17 };
static std::atomic<long long> g_h3_kernel_launches[H3_KINDS];
extern "C" long long isc_h3_kernel_launches(int kind) {
    return kind >= 0 && kind < H3_KINDS ? g_h3_kernel_launches[kind].load() : -1;
}
extern "C" long long isc_h3_launches(void) { return g_h3_launches.load(); }
extern "C" long long isc_h3_f16a_launches(void) { return g_h3_f16a_launches.load(); }
extern "C" long long isc_h3x_launches(void) { return g_h3x_launches.load(); }
extern "C" int isc_set_h3_mode(int mode) {
    if (mode >= 0 && mode <= 4) return g_h3_mode.exchange(mode);
    return g_h3_mode.load();
}
static std::atomic<int> g_gemv_rows{GEMV_MAX_ROWS};
static std::atomic<long long> g_gemv_launches{0};
extern "C" int isc_set_gemv_rows(int rows) {           // 0 = off; returns the previous value
    if (rows >= 0 && rows <= GEMV_MAX_ROWS) return g_gemv_rows.exchange(rows);
    return g_gemv_rows.load();
}
extern "C" long long isc_gemv_launches(void) { return g_gemv_launches.load(); }

// Every forward path is written as a pair: `*_plan` holds the path's conditions and nothing else - it launches nothing,
// writes nothing into the launch and leaves the weights scope as it is - and returns what the launch needs; `*_run`
// takes that answer and launches.  route_nt() strings the pairs together, isc_linear_f16_native asks the plans alone.

// The matrix-vector kernels take the launch when every problem has <= g_gemv_rows rows and fits the LDS image.
// Returns the longest contraction of the launch (it sizes the LDS image), 0 when the path does not apply.
template <int EPI>
static int gemv_plan(const DevLaunch &L) {
    const int rows = g_gemv_rows.load(), mode = g_h3_mode.load();
    if (rows <= 0 || mode > 1 || g_tile_override.load() >= 0) return 0;
    int kmax = 0;
    for (int i = 0; i < L.nprob; ++i) {
        const DevProb &p = L.p[i];
        if (p.M > rows || p.ksplit > 1) return 0;
        int K = 0;
        for (int s = 0; s < p.nseg; ++s) {
            if ((p.seg[s].K & 3) || (p.seg[s].lda & 3) || (p.seg[s].ldw & 3)) return 0;
            K += p.seg[s].K;
        }
        if (K > GEMV_MAX_K) return 0;
        if (EPI == EPI_LSTM && (p.H <= 0 || p.N != 4 * p.H)) return 0;
        kmax = K > kmax ? K : kmax;
    }
    return kmax;          // > 0 where the path applies: check_segs has turned K <= 0 away
}

template <int EPI>
static int gemv_run(DevLaunch &L, int kmax, hipStream_t st) {
    constexpr int NW = EPI == EPI_VOCAB ? 8 : 4;
    int start = 0;
    for (int i = 0; i < L.nprob; ++i) {
        DevProb &p = L.p[i];
        int nchunk = 0;
        for (int s = 0; s < p.nseg; ++s) nchunk += (p.seg[s].K + 255) >> 8;
        // K slices inside the workgroup: at most 4 chunks (16 loads) per wave, and enough workgroups for the chip
        const int quads = EPI == EPI_LSTM ? p.H : (p.N + 3) / 4;
        int KS = 1;
        if (EPI != EPI_VOCAB) {       // the smallest of 1, 2, 4 with <= 4 chunks per wave and >= 200 workgroups
            while (KS < 4 && KS * 2 <= nchunk && ((nchunk + KS - 1) / KS > 4 || (long long)quads * KS / NW < 200)) KS *= 2;
        }
        p.ksplit = KS;
        p.tile_start = start;
        start += EPI == EPI_VOCAB ? (p.N + 127) / 128 : (quads + NW / KS - 1) / (NW / KS);
    }
    L.total_tiles = start;
    const size_t lds = ((size_t)GEMV_MAX_ROWS * kmax + (EPI == EPI_VOCAB ? GEMV_MAX_ROWS * 128 : NW * 32)) * sizeof(float);
    static std::atomic<bool> attr_set{false};                     // (the limit of the largest image, once)
    if (int rc = lds_attr_once(attr_set, ((size_t)GEMV_MAX_ROWS * GEMV_MAX_K + GEMV_MAX_ROWS * 128) * sizeof(float),
                               &gemv_rows_kernel<EPI, NW>))
        return rc;
    hipLaunchKernelGGL((gemv_rows_kernel<EPI, NW>), dim3(L.total_tiles), dim3(64 * NW), lds, st, L);
    for (int i = 0; i < L.nprob; ++i) L.p[i].ksplit = 0;          // (the kernel has its copy; a failed launch counts too)
    ++g_gemv_launches;
    ISC_LAUNCH_CHECK();
    return ISC_OK;
}

#define H3_MIN_TILES 160
#define H3_MIN_TILES_SCOPE 16
// (tests / A-B runs: 0 keeps long contractions on few large tiles in one slice of K)
static std::atomic<int> g_h3_ksplit{1};
extern "C" int isc_set_h3_ksplit(int on) { return g_h3_ksplit.exchange(on < 0 ? 0 : (on > 2 ? 2 : on)); }
// Tile geometry of a vocabulary launch on the large split-f16 kernels: 0 = auto (launch_h3_big: 128 rows, which measures
// faster), 128 / 256 = that many rows whatever the tile count (tests / A-B runs; a row's statistics are the same bits
// either way).  Any other value changes nothing.  Returns the previous value.
static std::atomic<int> g_h3_vocab_tile{0};
extern "C" int isc_set_h3_vocab_tile(int rows) {
    if (rows == 0 || rows == 128 || rows == 256) return g_h3_vocab_tile.exchange(rows);
    return g_h3_vocab_tile.load();
}

// The reduce launch behind a K-split launch, by epilogue: sums the slabs in fixed order and finishes the outputs.
// (every split - the fp32 32-row tile's, the skinny and the large split-f16 kernels' - writes linear-epilogue slabs)
static int launch_splitk_linear_reduce(const DevLaunch &L, hipStream_t st) {
    long long mx = 0;
    for (int i = 0; i < L.nprob; ++i) {
        const long long n4 = (long long)L.p[i].M * (L.p[i].N >> 2);
        if (n4 > mx) mx = n4;
    }
    hipLaunchKernelGGL(splitk_linear_kernel, dim3((unsigned)((mx + 255) / 256), L.nprob), dim3(256), 0, st, L);
    ++g_f32_launches[F32_KIND_REDUCE];
    ISC_LAUNCH_CHECK();
    return ISC_OK;
}

template <int EPI>
static int launch_splitk_reduce(const DevLaunch &L, hipStream_t st) {
    const DevProb &p = L.p[0];
    if constexpr (EPI == EPI_LSTM) {          // plain [M, 4H] pre-activation slabs, then the cell update
        const long long n = (long long)p.M * p.H;
        hipLaunchKernelGGL(splitk_lstm_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, L);
        ++g_f32_launches[F32_KIND_REDUCE];
        ISC_LAUNCH_CHECK();
        return ISC_OK;
    } else if constexpr (EPI == EPI_VOCAB) {  // raw [S, M, V] slabs, then the per-128-column statistics: a wave per (row, tile)
        const long long waves = (long long)p.M * p.ntile_total;
        hipLaunchKernelGGL(splitk_vocab_kernel, dim3((unsigned)((waves + 3) / 4)), dim3(256), 0, st, L);
        ++g_f32_launches[F32_KIND_REDUCE];
        ISC_LAUNCH_CHECK();
        return ISC_OK;
    } else {
        return launch_splitk_linear_reduce(L, st);
    }
}

static bool h3_any_f32(const DevLaunch &L) {
    for (int i = 0; i < L.nprob; ++i)
        for (int s = 0; s < L.p[i].nap; ++s)
            if (!L.p[i].ap[s].hi) return true;
    return false;
}

static bool h3_any_f16(const DevLaunch &L) {              // an f16 segment read natively (caller's planes go first)
    for (int i = 0; i < L.nprob; ++i)
        for (int s = 0; s < L.p[i].nseg; ++s)
            if (L.p[i].seg[s].a_f16 && !(L.p[i].seg[s].A_hi && L.p[i].seg[s].A_lo)) return true;
    return false;
}

template <class G, int EPI, bool AF32>
static constexpr auto h3_tile_kernel() {
    if constexpr (std::is_same_v<G, H3Tile128>) return &gemm_h3_kernel<EPI, AF32>;
    else if constexpr (std::is_same_v<G, H3Tile256>) return &gemm_h3x_kernel<EPI, AF32>;
    else return &gemm_h3m_kernel<AF32>;
}

// One launch of a large split-f16 tile kernel of geometry G (the tiling of L is the caller's).
template <class G, int EPI>
static int launch_h3_tile(const DevLaunch &L, hipStream_t st) {
    static_assert(EPI == EPI_LINEAR || !std::is_same_v<G, H3Tile64>, "the 64-row kernel has the linear epilogue only");
    constexpr size_t lds = G::LDS_BYTES;
    constexpr auto planes = h3_tile_kernel<G, EPI, false>(), f32_rows = h3_tile_kernel<G, EPI, true>();
    constexpr int kind = H3_KIND_TILE + 3 * (std::is_same_v<G, H3Tile128> ? 0 : (std::is_same_v<G, H3Tile256> ? 1 : 2));
    static std::atomic<bool> attr_set{false}, attr16_set{false};           // (above 64 KB: one workgroup per CU)
    if (int rc = lds_attr_once(attr_set, lds, planes, f32_rows)) return rc;
    if (h3_any_f16(L)) {
        if constexpr (EPI == EPI_LINEAR) {
            constexpr auto f16_rows = &gemm_h3_f16a_kernel<G>;
            if (int rc = lds_attr_once(attr16_set, lds, f16_rows)) return rc;
            hipLaunchKernelGGL(f16_rows, dim3(L.total_tiles), dim3(G::THREADS), lds, st, L);
            ++g_h3_kernel_launches[kind + 2];
            ISC_LAUNCH_CHECK();
            ++g_h3_f16a_launches;
            return ISC_OK;
        } else {
            return ISC_E_SHAPE;
        }
    }
    const bool rows32 = h3_any_f32(L);
    const auto kernel = rows32 ? f32_rows : planes;
    hipLaunchKernelGGL(kernel, dim3(L.total_tiles), dim3(G::THREADS), lds, st, L);
    ++g_h3_kernel_launches[kind + (rows32 ? 1 : 0)];
    ISC_LAUNCH_CHECK();
    return ISC_OK;
}

static int h3_kp(const DevProb &p) {
    int Kp = 0;
    for (int s = 0; s < p.nseg; ++s) Kp += p.seg[s].K;
    return Kp;
}

// Weight planes kept across launches while the caller guarantees the weights do not change
// (isc_h3_weights_begin / _end, include/insenticap_hip.h): a roll-out splits each weight matrix once, not once
// per step.  Host-side table, valid on the stream order of the launches that filled it.
struct H3WEntry {
    const float *W[ISC_MAX_SEG];
    int ldw[ISC_MAX_SEG], K[ISC_MAX_SEG], nseg, rows, transposed;
    const _Float16 *hi, *lo;
};
// One scope per stream (isc_h3_weights_begin(buf, bytes, stream)): the slot table is guarded by a mutex, a slot's
// entries are only touched by launches on its own stream (which the caller issues in one order, like the launches
// themselves), so two host threads driving two captioners on two streams never see each other's planes.
#define H3W_MAX_ENTRIES 72
struct H3WScope {
    hipStream_t stream = nullptr;
    char *buf = nullptr;
    size_t bytes = 0, used = 0;
    H3WEntry e[H3W_MAX_ENTRIES];
    int n = 0;
    bool active = false;
};
// 64 slots: more than the streams a process can hold per device (torch hands out 32 pool streams per device and priority,
// plus the default stream); begin never takes over a SUSPENDED slot of another stream.  With 16 slots a test session
// that kept many captioners / training graphs alive ran out of them, and after such a take-over a captured training
// graph (seq2seq branch) computed its loss from planes one update old (graph vs eager 6.0207 / 6.0188; order-dependent).
#define H3W_MAX_SCOPES 64
static H3WScope g_h3w[H3W_MAX_SCOPES];
static std::mutex g_h3w_mu;

static H3WScope *h3w_scope_of(hipStream_t st) {
    std::lock_guard<std::mutex> lk(g_h3w_mu);
    for (int i = 0; i < H3W_MAX_SCOPES; ++i)
        if (g_h3w[i].active && g_h3w[i].stream == st) return &g_h3w[i];
    return nullptr;
}

extern "C" int64_t isc_splitk_workspace_bytes(int64_t M, int64_t N) {
    if (M <= 0 || N <= 0) return 0;
    const int64_t b = 16 * M * N * (int64_t)sizeof(float);            // plan_splitk: S <= 16 slabs of [M, N]
    return (b + 255) / 256 * 256;
}
extern "C" int64_t isc_h3_weights_workspace_bytes(int64_t weight_elements, int with_transposes) {
    if (weight_elements <= 0) return 0;
    const int64_t one = weight_elements * 2 * (int64_t)sizeof(uint16_t);     // hi + lo f16 plane per value
    const int64_t b = one * (with_transposes ? 2 : 1);
    return (b + 1048575) / 1048576 * 1048576;
}

extern "C" int isc_h3_weights_begin(void *buf, long long bytes, void *stream) {
    if (!buf || bytes <= 0) return ISC_E_NULL;
    if ((uintptr_t)buf & 255) return ISC_E_ALIGN;
    std::lock_guard<std::mutex> lk(g_h3w_mu);
    H3WScope *slot = nullptr;
    for (int i = 0; i < H3W_MAX_SCOPES; ++i)                     // the stream's own slot (active or suspended)
        if (g_h3w[i].buf && g_h3w[i].stream == (hipStream_t)stream) slot = &g_h3w[i];
    for (int i = 0; !slot && i < H3W_MAX_SCOPES; ++i)            // a free one
        if (!g_h3w[i].buf) slot = &g_h3w[i];
    // No take-over of another stream's SUSPENDED slot: its owner may be a captured graph that still reads those planes
    // (round 4: a training graph computed a loss from planes one update old after such a take-over).  More live scopes
    // than slots: this caller runs without one (every launch splits its weights into the workspace).
    if (!slot) return ISC_E_WORKSPACE;
    slot->stream = (hipStream_t)stream;
    slot->buf = static_cast<char *>(buf); slot->bytes = (size_t)bytes; slot->used = 0; slot->n = 0;
    slot->active = true;
    return ISC_OK;
}
extern "C" int isc_h3_weights_end(void *stream) {
    std::lock_guard<std::mutex> lk(g_h3w_mu);
    for (int i = 0; i < H3W_MAX_SCOPES; ++i)
        if (g_h3w[i].buf && g_h3w[i].stream == (hipStream_t)stream) {
            g_h3w[i].active = false; g_h3w[i].n = 0; g_h3w[i].used = 0; g_h3w[i].buf = nullptr;
        }
    return ISC_OK;
}
extern "C" int isc_h3_weights_suspend(void *stream) {
    std::lock_guard<std::mutex> lk(g_h3w_mu);
    for (int i = 0; i < H3W_MAX_SCOPES; ++i)
        if (g_h3w[i].active && g_h3w[i].stream == (hipStream_t)stream) g_h3w[i].active = false;
    return ISC_OK;
}
extern "C" int isc_h3_weights_resume(void *buf, void *stream) {
    if (!buf) return ISC_E_NULL;
    std::lock_guard<std::mutex> lk(g_h3w_mu);
    for (int i = 0; i < H3W_MAX_SCOPES; ++i)
        if (!g_h3w[i].active && g_h3w[i].buf == static_cast<char *>(buf) && g_h3w[i].stream == (hipStream_t)stream) {
            g_h3w[i].active = true;
            return ISC_OK;
        }
    return ISC_E_STATE;
}

// Re-split every weight the stream's scope (active or suspended) holds planes of, from the weights' CURRENT values, into
// the same planes: what an optimiser step calls after it has written the weights in place, so that the next forward /
// backward sweeps resume the scope instead of rebuilding it plane by plane (39 one-job split launches per XE iteration at
// B = 128 became ceil(entries / H3_MAX_JOBS) launches).  Enqueued on `stream`, i.e. ordered after whatever wrote the
// weights there; the caller orders other streams.
extern "C" int isc_h3_weights_refresh(void *stream) {
    H3WScope *sc = nullptr;
    {
        std::lock_guard<std::mutex> lk(g_h3w_mu);
        for (int i = 0; i < H3W_MAX_SCOPES; ++i)
            if (g_h3w[i].buf && g_h3w[i].stream == (hipStream_t)stream) sc = &g_h3w[i];
    }
    if (!sc) return ISC_E_STATE;
    int i = 0;
    while (i < sc->n) {
        SplitLaunch S = {};
        int blocks = 0;
        for (; i < sc->n && S.njobs < H3_MAX_JOBS; ++i) {
            const H3WEntry &e = sc->e[i];
            SplitJob &J = S.j[S.njobs++];
            int k0 = 0;
            for (int sg = 0; sg < e.nseg; ++sg) {
                J.src[sg] = e.W[sg]; J.ld[sg] = e.ldw[sg]; J.kstart[sg] = k0;
                k0 += e.K[sg];
            }
            J.nseg = e.nseg; J.rows = e.rows; J.Kp = k0; J.first_block = blocks;
            J.hi = const_cast<_Float16 *>(e.hi); J.lo = const_cast<_Float16 *>(e.lo);
            J.transposed = e.transposed;
            blocks += e.transposed ? ((e.rows + 63) / 64) * (k0 >> 5) : (int)(((long long)e.rows * (k0 >> 3) + 255) / 256);
        }
        hipLaunchKernelGGL(h3_split_kernel, dim3(blocks), dim3(256), 0, (hipStream_t)stream, S);
        ++g_h3_kernel_launches[H3_KIND_SPLIT];
        ISC_LAUNCH_CHECK();
    }
    return ISC_OK;
}

static const H3WEntry *h3w_find(const H3WScope *sc, const DevProb &p, int transposed = 0) {
    if (!sc) return nullptr;
    for (int i = 0; i < sc->n; ++i) {
        const H3WEntry &e = sc->e[i];
        bool eq = e.nseg == p.nseg && e.rows == p.N && e.transposed == transposed;
        for (int s = 0; eq && s < p.nseg; ++s)
            eq = e.W[s] == p.seg[s].W && e.ldw[s] == p.seg[s].ldw && e.K[s] == p.seg[s].K;
        if (eq) return &e;
    }
    return nullptr;
}

// 256-row tiles when they fill the chip, else the 128-row kernel.  The vocabulary projection stays on the 128-row
// kernel unless isc_set_h3_vocab_tile(256) sends it to the other: a one-workgroup-per-CU kernel runs the statistics
// epilogue of its eight waves with the matrix pipe idle, where a second, out-of-phase workgroup on the CU overlaps it
// with the main loop.  Measured at the headline shape [16384 x 10000 x 512], five alternating runs of the benchmark:
// 128 rows 456-459 us per launch, 256 rows 472-489 us (with the branchy epilogue of before, ~1300 VALU + 340 SALU
// instructions per wave against ~860 + 40 now: 128 rows 477-483 us; [4096 x 9984 x 512] in the lab then 162 us
// against 174 us, and 173 us for a persistent 256-row form with the next tile's first two chunks in flight before the
// epilogue - what is exposed is the epilogue's own VALU time, not the workgroup turnover).
template <int EPI>
static int launch_h3_big(DevLaunch &L, hipStream_t st) {
    bool rows256 = count_tiles(L, 256, 128) >= 224;                   // (round 3: 160 - the three h-projections on this kernel - measured the same)
    if (EPI == EPI_VOCAB) rows256 = g_h3_vocab_tile.load() == 256;    // 0 (auto) = 128 rows: see above
    if (rows256) {
        ++g_h3x_launches;
        finish_tiling(L, 3);
        return launch_h3_tile<H3Tile256, EPI>(L, st);
    }
    finish_tiling(L, 4);
    return launch_h3_tile<H3Tile128, EPI>(L, st);
}

// The activation operand of a split-f16 launch: the caller's per-tensor planes where given; a segment without planes is
// read as fp32 rows and split in registers after the fragment read (ap.hi == nullptr) - no split launch, no plane copy
// in memory.  Also sets the packed contraction length.
static void h3_set_a(DevProb &p) {
    p.Kp = h3_kp(p);
    p.nap = p.nseg;
    for (int s = 0; s < p.nseg; ++s) {
        const int K = p.seg[s].K;
        const bool planes = p.seg[s].A_hi && p.seg[s].A_lo;
        p.ap[s] = DevASeg{planes ? p.seg[s].A_hi : nullptr, planes ? p.seg[s].A_lo : nullptr, 2 * K, K};
    }
}

// Operand-split jobs of one launch: add() lays the planes of an operand out in the workspace and queues its job.
struct H3Planner {
    SplitLaunch S = {};
    char *at;
    int blocks = 0;
    H3WScope *scope;                                   // the launch stream's weights scope, or null
    explicit H3Planner(float *ws, H3WScope *sc = nullptr) : at(reinterpret_cast<char *>(ws)), scope(sc) {}
    // planes of segments [s0, s1) of an operand, K-packed
    void add(const DevProb &p, bool is_w, int rows, const _Float16 *&hi, const _Float16 *&lo, int s0 = 0, int s1 = -1,
             int transposed = 0) {
        if (s1 < 0) s1 = p.nseg;
        SplitJob &J = S.j[S.njobs++];
        J.transposed = transposed;
        int k0 = 0;
        for (int s = s0; s < s1; ++s) {
            J.src[s - s0] = is_w ? p.seg[s].W : p.seg[s].A;
            J.ld[s - s0] = is_w ? p.seg[s].ldw : p.seg[s].lda;
            J.kstart[s - s0] = k0;
            k0 += p.seg[s].K;
        }
        J.nseg = s1 - s0; J.rows = rows; J.Kp = k0; J.first_block = blocks;
        const size_t bytes = (((size_t)rows * k0 * 4) + 255) & ~(size_t)255;      // hi and lo interleaved
        J.hi = reinterpret_cast<_Float16 *>(at); at += bytes;
        J.lo = J.hi + 32;
        hi = J.hi; lo = J.lo;
        blocks += transposed ? ((rows + 63) / 64) * (k0 >> 5) : (int)(((long long)rows * (k0 >> 3) + 255) / 256);
    }
    // weight operand: cached planes if the caller opened a weights scope, else planes in the workspace
    void add_w(const DevProb &p, const _Float16 *&hi, const _Float16 *&lo, int transposed = 0) {
        if (const H3WEntry *e = h3w_find(scope, p, transposed)) { hi = e->hi; lo = e->lo; return; }
        const size_t bytes = (((size_t)p.N * h3_kp(p) * 4) + 255) & ~(size_t)255;
        if (scope && scope->n < H3W_MAX_ENTRIES && scope->used + bytes <= scope->bytes) {
            char *keep = at;
            at = scope->buf + scope->used;
            add(p, true, p.N, hi, lo, 0, -1, transposed);
            at = keep;
            scope->used += bytes;
            H3WEntry &e = scope->e[scope->n++];
            e.nseg = p.nseg; e.rows = p.N; e.hi = hi; e.lo = lo; e.transposed = transposed;
            for (int s = 0; s < p.nseg; ++s) { e.W[s] = p.seg[s].W; e.ldw[s] = p.seg[s].ldw; e.K[s] = p.seg[s].K; }
            return;
        }
        add(p, true, p.N, hi, lo, 0, -1, transposed);
    }
    int launch(hipStream_t st) {
        if (!S.njobs) return ISC_OK;
        hipLaunchKernelGGL(h3_split_kernel, dim3(blocks), dim3(256), 0, st, S);
        ++g_h3_kernel_launches[H3_KIND_SPLIT];
        ISC_LAUNCH_CHECK();
        return ISC_OK;
    }
};

// What the large split-f16 kernels need to take a launch (take == false: the path does not apply).
struct H3Plan {
    bool take = false, half_tile = false;     // half_tile: the 64-row tile
    int ksplit = 1;                           // slices of K (> 1: slabs behind the planes in the workspace, then the reduce)
    long long need = 0;                       // floats of the workspace the weight planes take without a weights scope
    H3WScope *scope = nullptr;                // the launch stream's weights scope, or null
};

template <int EPI>
static H3Plan h3_plan(const DevLaunch &L, float *ws, long long ws_floats, hipStream_t st, int transposed) {
    H3Plan h;
    const int h3_mode = g_h3_mode.load();
    if (h3_mode == 0 || g_tile_override.load() >= 0 || !ws || ((uintptr_t)ws & 255)) return h;
    const long long tiles = count_tiles(L, 128, 128), tiles64 = count_tiles(L, 64, 128);
    long long need = 0;
    for (int i = 0; i < L.nprob; ++i) {
        const DevProb &p = L.p[i];
        if (p.ksplit > 1) return h;
        const long long Kp = h3_kp(p);
        if (Kp > (1 << 20)) return h;
        need += (long long)p.N * Kp + 1024;               // floats: the weight planes (2 x 2 bytes per element) when the
                                                          // stream has no weights scope; activations are never copied
    }
    // linear launches that cannot give every CU a 128-row tile: the 64-row tile, unless it then needs more rounds of
    // the chip than it saves in bytes per workgroup (rounds x (rows + 128 columns) of operand lines per workgroup:
    // [4608 x 512] K=2048 is 288 64-row tiles = two rounds, 97 us, against one round of 144 128-row tiles)
    h.half_tile = EPI == EPI_LINEAR && tiles < 256 && ((tiles64 + 255) / 256) * 192 < ((tiles + 255) / 256) * 256;
    h.scope = h3w_scope_of(st);
    // inside a weights scope the planes are already there and the skinny kernel has taken what it does better
    // (h3s_plan came first): whatever is left with a few tiles is still faster here than on the fp32 tiles
    const long long min_tiles = h.scope && h3_mode == 1 ? H3_MIN_TILES_SCOPE
                                                        : (EPI == EPI_LINEAR && tiles < 256 ? H3_MIN_TILES / 2 : H3_MIN_TILES);
    if (h3_mode != 2 && tiles < min_tiles) return h;
    if (need > ws_floats) return h;
    if (L.nprob > H3_MAX_JOBS) return h;
    h.need = need;
    h.take = true;
    // a long contraction on few 128 x 128 tiles (one problem, linear epilogue): S slices of K so that the launch fills
    // the chip's 512 workgroup slots, raw partial tiles to slabs behind the planes in the workspace, then the reduce
    // (backward dX contractions only - `transposed` - unless forced: a forward launch keeps ONE summation order at every
    // batch size, so that a ReLU's sign at a pre-activation of ~0 does not depend on how many rows share the launch)
    // (f16 rows are read in one slice of K: the line pairs of a slice would have to start on an even chunk)
    if (!h.half_tile && EPI == EPI_LINEAR && L.nprob == 1 && (L.p[0].N & 3) == 0 && !h3_any_f16(L) &&
        (g_h3_ksplit.load() == 2 || (transposed && g_h3_ksplit.load()))) {
        const DevProb &p = L.p[0];
        const int nblk = h3_kp(p) / 32;
        if (count_tiles(L, 256, 128) < 224 && tiles <= 200 && nblk >= 64) {
            int S = (int)(512 / tiles);
            if (S > 8) S = 8;
            while (S > 1 && nblk / S < 24) --S;
            const long long used = (need + 255) & ~255LL, slab = (long long)p.M * p.N;
            while (S > 1 && used + S * slab > ws_floats) --S;
            h.ksplit = S;
        }
    }
    return h;
}

// Lays the weight planes of every problem out (the scope's, or in the caller's workspace), launches the operand split
// and the GEMM.  Returns the launches' status.
template <int EPI>
static int h3_run(DevLaunch &L, const H3Plan &h, float *ws, hipStream_t st, int transposed) {
    H3Planner pl(ws, h.scope);
    for (int i = 0; i < L.nprob; ++i) {
        DevProb &p = L.p[i];
        h3_set_a(p);
        pl.add_w(p, p.Wh, p.Wl, transposed);
    }
    int rc = pl.launch(st);
    if (rc) return rc;
    if (h.half_tile) {
        finish_tiling(L, 1);
        rc = launch_h3_tile<H3Tile64, EPI_LINEAR>(L, st);
    } else {
        const int S = h.ksplit;
        if (S > 1) {
            DevProb &p = L.p[0];
            p.ksplit = S;
            p.slab = ws + ((h.need + 255) & ~255LL);
            p.slab_stride = (long long)p.M * p.N;
        }
        rc = launch_h3_big<EPI>(L, st);
        if (!rc && S > 1) rc = launch_splitk_linear_reduce(L, st);
        if (S > 1) L.p[0].ksplit = 0;
    }
    ++g_h3_launches;
    return rc;
}

// ---- skinny split-f16 path (gemm_h3s_kernel): few-row launches inside a weights scope ----
static std::atomic<long long> g_h3s_launches{0};
extern "C" long long isc_h3s_launches(void) { return g_h3s_launches.load(); }
#define H3S_MAX_ROWS 2048
#define H3S_MAX_ROWS_NN 4096
#define H3S_EIGHT_WAVES_MIN_K 1024
#define H3S_MAX_WGS_VOCAB 384

// (tests / A-B runs: 0 sends vocabulary launches of the skinny path back to gemm_h3s_kernel<EPI_VOCAB>)
static std::atomic<int> g_h3v_on{1};
extern "C" int isc_set_h3v(int on) { return g_h3v_on.exchange(on < 0 ? 0 : on); }
// workgroups up to which a vocabulary launch stays skinny: isc_set_h3v(0) off, (1) on, (n > 1) on with the limit n
static long long h3s_max_wgs_vocab() {
    const int v = g_h3v_on.load();
    return v > 1 ? v : (v == 1 ? 512 : H3S_MAX_WGS_VOCAB);
}

template <int EPI, int T, int NW = 4>
static int launch_h3s(const DevLaunch &L, hipStream_t st) {
    // waves x ring slots x (A image + W image): 128 KB for the K-split tiles, 64 KB for the vocabulary projection
    constexpr size_t lds = (size_t)NW * (EPI != EPI_VOCAB && T == 1 && NW == 4 ? 4 : 2) * 8192 * T;
    static std::atomic<bool> attr_set{false};
    if (int rc = lds_attr_once(attr_set, lds, &gemm_h3s_kernel<EPI, T, NW>)) return rc;
    hipLaunchKernelGGL((gemm_h3s_kernel<EPI, T, NW>), dim3(L.total_tiles), dim3(64 * NW), lds, st, L);
    ++g_h3_kernel_launches[EPI == EPI_VOCAB ? (NW == 8 ? H3_KIND_SV_W8 : H3_KIND_SV)
                                            : (T == 2 ? H3_KIND_S64 : (NW == 8 ? H3_KIND_S32_W8 : H3_KIND_S32))];
    ISC_LAUNCH_CHECK();
    return ISC_OK;
}

// Tile choice of a skinny launch.  One workgroup per CU and every workgroup ingest-bound (~35-40 GB/s per CU), so a
// launch costs ~4 us + its rounds of the chip x the bytes a workgroup takes in: per k ~6.5 ns for the 32 x 32 tile,
// twice that for the 64 x 64 tile (four times the outputs), against ~30 ns for a 128 x 128 tile of the large kernels
// (kernel-trace medians of tools/skinny_bench.py in modes 3 / 4 / 2, M = 128 ... 2048; LSTM cell K = 1536: M = 512
// 43 / 24 / 41 us, M = 1024 79 / 45 / 53 us, M = 2048 149 / 88 / 61 us).  So: the tile with fewer weighted rounds, and
// the large kernels past ~4.6 of them.  The vocabulary tile (32 x 128, two workgroups per CU) crosses earlier:
// M = 128 24 vs 28 us, M = 256 38 vs 22 us.
// Returns the tile factor T (1 or 2), or 0 when the large kernels should take the launch (auto mode only).
#define H3S_WIDE_COST 2.0
#define H3S_MAX_COST 4.6
template <int EPI>
static int h3s_pick_tile(const DevLaunch &L, int mode) {
    const long long w1 = count_tiles(L, 32, EPI == EPI_VOCAB ? 128 : 32), w2 = count_tiles(L, 64, 64);
    bool wide_ok = EPI != EPI_VOCAB;
    for (int i = 0; i < L.nprob; ++i)
        if (EPI == EPI_LSTM && (L.p[i].H & 15)) wide_ok = false;
    if (mode == 4) return wide_ok ? 2 : 1;
    if (mode == 3) return 1;
    // (with gemm_h3v_kernel up to 512 workgroups = one round at two per CU: M = 160 / 192 roll-outs 1.67 / 1.79 -> 1.63 / 1.78 ms)
    if (EPI == EPI_VOCAB) return w1 < h3s_max_wgs_vocab() ? 1 : 0;
    const double c1 = (double)((w1 + 255) / 256), c2 = wide_ok ? H3S_WIDE_COST * (double)((w2 + 255) / 256) : 1e30;
    if ((c1 < c2 ? c1 : c2) >= H3S_MAX_COST) return 0;
    return c2 < c1 ? 2 : 1;
}

static void h3s_tile_problem(DevProb &p, int bm, int bn, int &start, int ksplit = 1) {
    p.ksplit = ksplit;
    p.tiles_m = (p.M + bm - 1) / bm;
    p.tiles_n = (p.N + bn - 1) / bn;
    p.tile_start = start;
    // One slice of the column tiles per XCD (map_tile's grouped order) once there are several row tiles: the XCD's
    // workgroups then share a weight slice of 1/8 that its L2 keeps, instead of every XCD streaming most of W.
    p.m_fastest = p.tiles_m > 1 ? 1 : 0;
    p.grp_n = (p.tiles_n + 7) / 8;
    start += p.tiles_m * p.tiles_n * ksplit;
}

// Cross-workgroup K split of a skinny linear launch: a long contraction on few tiles (the classifier's dX at B = 128:
// [2560 x 512] over K = 9984 is 320 wide tiles = 1.25 rounds of ~130 us each) packs the chip better in S slices -
// cost in k per workgroup-round, as h3s_pick_tile, plus ~1000 for the reduce launch.  S <= 8, >= 16 k-blocks per slice.
static int h3s_pick_ksplit(const DevLaunch &L, int T, long long slab_floats) {
    const long long w = count_tiles(L, 32 * T, 32 * T);
    long long mn = 0;
    int kp_min = 1 << 30, kp_max = 0;
    for (int i = 0; i < L.nprob; ++i) {
        const DevProb &p = L.p[i];
        if (p.N & 3) return 1;
        mn += (long long)p.M * p.N;
        const int kp = h3_kp(p);
        if (kp < kp_min) kp_min = kp;
        if (kp > kp_max) kp_max = kp;
    }
    if (kp_min < 4096) return 1;
    int best = 1;
    long long best_cost = ((w + 255) / 256) * kp_max;
    for (int S = 2; S <= 8; ++S) {
        if (kp_min / S < 512 || S * mn > slab_floats) break;
        const long long cost = ((w * S + 255) / 256) * (kp_max / S) + 1000;
        if (cost < best_cost) { best_cost = cost; best = S; }
    }
    return best;
}

template <int EPI>
static int launch_h3s_t(const DevLaunch &L, int T, hipStream_t st) {
    if constexpr (EPI != EPI_VOCAB) {
        if (T == 2) return launch_h3s<EPI, 2>(L, st);
        int kp_min = 1 << 30;
        for (int i = 0; i < L.nprob; ++i) {
            const int kq = L.p[i].Kp / (L.p[i].ksplit > 1 ? L.p[i].ksplit : 1);
            if (kq < kp_min) kp_min = kq;
        }
        // from 32 k-blocks on, eight waves (four blocks or more each) beat four when activation segments arrive as
        // fp32 rows (training: the in-register split is shared by twice the waves; kernel-trace sums of an XE
        // iteration at B = 128: LSTM cells -9 %, linears -3 %); with every operand on planes (the decode loop) four
        // waves with four-slot rings are the faster form (LSTM cell 9.5 vs 10.3 us)
        if (kp_min >= H3S_EIGHT_WAVES_MIN_K && h3_any_f32(L)) return launch_h3s<EPI, 1, 8>(L, st);
    }
    if constexpr (EPI == EPI_VOCAB) {
        // one activation segment (the classifier over h_lang): workgroup-shared k-block stages (gemm_h3v_kernel)
        bool v_ok = g_h3v_on.load() != 0;
        for (int i = 0; i < L.nprob; ++i)
            if (L.p[i].nap != 1 || L.p[i].ksplit > 1) v_ok = false;
        if (v_ok) {
            const size_t lds = H3V_STAGES * H3V_STAGE_BYTES;
            static std::atomic<bool> attr_set{false};
            if (int rc = lds_attr_once(attr_set, lds, &gemm_h3v_kernel<true>,
                                       &gemm_h3v_kernel<false>))
                return rc;
            const bool rows32 = h3_any_f32(L);
            if (rows32) hipLaunchKernelGGL((gemm_h3v_kernel<true>), dim3(L.total_tiles), dim3(256), lds, st, L);
            else hipLaunchKernelGGL((gemm_h3v_kernel<false>), dim3(L.total_tiles), dim3(256), lds, st, L);
            ++g_h3_kernel_launches[rows32 ? H3_KIND_V_F32 : H3_KIND_V];
            ISC_LAUNCH_CHECK();
            return ISC_OK;
        }
        // one workgroup per CU at most (M <= 96 at V = 10 000; beam rows): eight waves, two per column block
        if (L.total_tiles <= 256) return launch_h3s<EPI, 1, 8>(L, st);
    }
    return launch_h3s<EPI, 1>(L, st);
}

// What the skinny kernels need to take a launch.  T == 0: the path does not apply - mode off / tile override, no weights
// scope on this stream in auto mode (the weight planes would have to be rebuilt per launch), more rows than
// H3S_MAX_ROWS, or a launch the large split-f16 kernels do better (h3s_pick_tile).
// Modes 3 / 4 force the 32 x 32 / 64 x 64 tile (tests): without a scope the weight planes then go to the workspace.
struct H3sPlan {
    int T = 0;                                // tile factor: 32 T x 32 T outputs
    int ksplit = 1;                           // slices of K across workgroups (> 1: slabs, then the reduce)
    H3WScope *scope = nullptr;                // the launch stream's weights scope, or null
};

template <int EPI>
static H3sPlan h3s_plan(const DevLaunch &L, float *ws, long long ws_floats, hipStream_t st, int transposed) {
    H3sPlan h;
    const int mode = g_h3_mode.load();
    if ((mode != 1 && mode != 3 && mode != 4) || g_tile_override.load() >= 0) return h;
    h.scope = h3w_scope_of(st);
    if (!h.scope && mode == 1) return h;
    long long need = 0;
    for (int i = 0; i < L.nprob; ++i) {
        const DevProb &p = L.p[i];
        // (dX contractions over a vocabulary-sized K - long K, few tiles - also run here above H3S_MAX_ROWS, K-split)
        if (p.M > (transposed && h3_kp(p) >= 4096 ? H3S_MAX_ROWS_NN : H3S_MAX_ROWS)) return h;
        if (EPI == EPI_LSTM && (p.H & 7)) return h;
        for (int sg = 0; sg < p.nseg; ++sg)
            if (p.seg[sg].K & 31) return h;                 // (the backward entry point accepts other K)
        const long long Kp = h3_kp(p);
        if (Kp > (1 << 20)) return h;
        need += (long long)p.N * Kp + 256;
    }
    const int T = h3s_pick_tile<EPI>(L, mode);
    if (!T) return h;                                     // the large kernels' launch
    if (!ws || ((uintptr_t)ws & 255) || need > ws_floats) return h;   // planes that do not fit the scope go here
    if (L.nprob > H3_MAX_JOBS) return h;
    h.T = T;
    if constexpr (EPI == EPI_LINEAR) h.ksplit = h3s_pick_ksplit(L, T, ws_floats - need - 64);
    return h;
}

template <int EPI>
static int h3s_run(DevLaunch &L, const H3sPlan &h, float *ws, long long ws_floats, hipStream_t st, int transposed) {
    const int T = h.T, S = h.ksplit;
    float *slab = ws + ((ws_floats - 64) & ~63LL);        // slabs from the end of the workspace, planes from its start
    H3Planner pl(ws, h.scope);
    int start = 0;
    for (int i = 0; i < L.nprob; ++i) {
        DevProb &p = L.p[i];
        h3_set_a(p);
        pl.add_w(p, p.Wh, p.Wl, transposed);
        h3s_tile_problem(p, 32 * T, EPI == EPI_VOCAB ? 128 : 32 * T, start, S);
        if (S > 1) {
            p.slab_stride = (long long)p.M * p.N;
            slab -= S * p.slab_stride;
            p.slab = slab;
        }
    }
    L.total_tiles = start;
    int rc = pl.launch(st);                               // weight planes not yet in the scope (first use only)
    if (rc) return rc;
    rc = launch_h3s_t<EPI>(L, T, st);
    ++g_h3s_launches;
    if (!rc && S > 1) rc = launch_splitk_linear_reduce(L, st);
    return rc;
}

// 2 M N K summed over the K-segments of a problem (isc_linear_problem or DevProb)
template <class P>
static double contraction_flops(const P &p) {
    double f = 0;
    for (int s = 0; s < p.nseg; ++s) f += 2.0 * p.M * p.N * (double)p.seg[s].K;
    return f;
}
// dW contractions below this: the fp32 tiles' launch is as quick as the transposing split plus the split-f16 launch
#define H3_TN_MIN_FLOPS 2.5e8

// Rows [k0, k0 + kc) of a single-segment TN problem: A and W advanced by k0 rows.  `later` (a slice after the first, or
// a later pass over the problem): accumulate onto what is in C, the biases went in with the first.
// (a multi-segment problem is only ever taken whole: k0 = 0, kc = its packed K)
static DevProb tn_k_slice(const DevProb &p, long long k0, long long kc, bool later) {
    DevProb q = p;
    if (p.nseg == 1) {
        q.seg[0].A = p.seg[0].A + k0 * p.seg[0].lda;
        q.seg[0].W = p.seg[0].W + k0 * p.seg[0].ldw;
        q.seg[0].K = (int)kc;
    }
    if (later) { q.accumulate = 1; q.bias0 = q.bias1 = q.bias2 = nullptr; }
    return q;
}

// One launch of TN problems that share their A (= dY; one problem, or several): plans the transposed planes of A once
// and of each W in the workspace, launches the split, tiles and launches the GEMM - the large tiles, the 64-row tile or
// the skinny tile by the tile count (`skinny_only`: a group is always skinny: each of its problems alone is) - and counts
// the launch in g_h3_launches whichever kernel ran.
static int tn_launch(DevLaunch &Lc, float *ws, int mode, bool skinny_only, hipStream_t st) {
    H3Planner pl(ws, nullptr);
    const _Float16 *ah = nullptr, *al = nullptr;
    const int kc = h3_kp(Lc.p[0]);
    pl.add(Lc.p[0], false, Lc.p[0].M, ah, al, 0, -1, 1);
    for (int i = 0; i < Lc.nprob; ++i) {
        DevProb &q = Lc.p[i];
        pl.add(q, true, q.N, q.Wh, q.Wl, 0, -1, 1);
        q.nap = 1;
        q.ap[0] = DevASeg{ah, al, 2 * kc, kc};
        q.nseg = 1;                                           // the kernels see one packed K-segment
        q.seg[0].K = kc;
        q.Kp = kc;
        q.ksplit = 1;
    }
    int rc = pl.launch(st);
    if (rc) return rc;
    const long long tiles = count_tiles(Lc, 128, 128);
    if (!skinny_only && tiles >= H3_MIN_TILES) {
        rc = launch_h3_big<EPI_LINEAR>(Lc, st);
    } else if (!skinny_only && tiles >= H3_MIN_TILES / 2) {
        finish_tiling(Lc, 1);
        rc = launch_h3_tile<H3Tile64, EPI_LINEAR>(Lc, st);
    } else {
        int T = h3s_pick_tile<EPI_LINEAR>(Lc, mode == 2 ? 1 : mode), start = 0;
        if (!T) T = 2;
        for (int i = 0; i < Lc.nprob; ++i) h3s_tile_problem(Lc.p[i], 32 * T, 32 * T, start);
        Lc.total_tiles = start;
        rc = launch_h3s_t<EPI_LINEAR>(Lc, T, st);
    }
    if (rc) return rc;
    ++g_h3_launches;
    return ISC_OK;
}

// The problems of Lp (packed K each) in slices of `step` rows of K, one tn_launch per slice.
// (every slice is a fresh launch descriptor with its problems copied by value - one host copy of a DevProb per problem and
// slice more than slicing in place would make, next to a split launch and a GEMM launch per slice)
static int tn_run_chunks(const DevLaunch &Lp, long long K, long long step, bool later, float *ws, int mode,
                         bool skinny_only, hipStream_t st) {
    for (long long k0 = 0; k0 < K; k0 += step) {
        const long long kc = K - k0 < step ? K - k0 : step;
        DevLaunch Lc = {};
        Lc.nprob = Lp.nprob;
        for (int i = 0; i < Lp.nprob; ++i) Lc.p[i] = tn_k_slice(Lp.p[i], k0, kc, later || k0 > 0);
        if (int rc = tn_launch(Lc, ws, mode, skinny_only, st)) return rc;
    }
    return ISC_OK;
}

// dW = dY^T X (ISC_LAYOUT_TN: both operands are [K_s, .] with the contraction over their ROWS) on the split-f16
// kernels: planes of dY^T [M, Kp] and X^T [N, Kp] are built by the transposing split into the workspace (both operands
// are activations: new every call, never cached), then the NT kernels run as for any linear problem - the large tiles,
// the 64-row tile or the skinny tile by size.  A single-segment problem whose planes exceed the workspace goes through it
// in K chunks that accumulate into C.  Problems of a launch are handled one by one; returns the bit mask of the problems
// that went out on this path (the caller runs the others - a segment with K % 32 != 0, a small contraction - on the
// fp32 tiles); rc != 0 reports a launch error.
static unsigned try_h3_tn(DevLaunch &L, float *ws, long long ws_floats, hipStream_t st, int &rc) {
    const int mode = g_h3_mode.load();
    if (mode == 0 || g_tile_override.load() >= 0 || !ws || ((uintptr_t)ws & 255)) return 0;
    long long chunk[3];
    unsigned take = 0;
    for (int i = 0; i < L.nprob; ++i) {
        const DevProb &p = L.p[i];
        const long long Kp = h3_kp(p);
        bool ok = true;
        for (int s = 0; s < p.nseg; ++s) ok = ok && (p.seg[s].K & 31) == 0;
        if (contraction_flops(p) < H3_TN_MIN_FLOPS && mode != 2) ok = false;
        const long long per_k = (long long)p.M + p.N;
        chunk[i] = Kp;
        if (ok && per_k * Kp + 1024 > ws_floats) {
            // planes larger than the workspace: K chunks that accumulate into C - a multi-segment problem segment by
            // segment (the [fc | label] block of the att-LSTM's dW at B >= 512 is two segments of T B rows: 22-45 GFLOP
            // that used to stay on the fp32 tiles, 0.2-0.4 ms per sweep)
            chunk[i] = ((ws_floats - 1024) / per_k) & ~31LL;
            if (chunk[i] < 512) ok = false;
        }
        if (ok) take |= 1u << i;
    }
    // Several dW contractions from ONE dY (the weight gradients of the layers that consumed the same pre-activation
    // gradient: lang-LSTM's three input blocks from dG2, att-LSTM's from dG1): the transposing split of dY happens once,
    // the problems share one launch of the skinny tiles - 3 x (split + GEMM) -> 1 + 1 launches, and dY^T's planes
    // (the larger operand: [2048, T B] against [512, T B]) are built once instead of three times.
    if (L.nprob >= 2 && take == (1u << L.nprob) - 1u) {
        bool same = true;
        long long n_sum = 0;
        const DevProb &p0 = L.p[0];
        for (int i = 0; i < L.nprob; ++i) {
            const DevProb &p = L.p[i];
            same = same && p.nseg == 1 && p.seg[0].A == p0.seg[0].A && p.seg[0].lda == p0.seg[0].lda &&
                   p.seg[0].K == p0.seg[0].K && p.M == p0.M &&
                   (long long)((p.M + 127) / 128) * ((p.N + 127) / 128) < H3_MIN_TILES / 2;
            n_sum += p.N;
        }
        const long long K = p0.nseg == 1 ? p0.seg[0].K : 0;
        // planes of dY^T and of every X^T for kc rows at a time: the whole K when it fits the workspace, else equal chunks
        // (multiples of 32) that accumulate into C - the B = 512 / 1024 iterations contract over 10 240 / 22 080 rows
        const long long per_k = (long long)p0.M + n_sum;
        const long long kc_max = ((ws_floats - 1024LL * (L.nprob + 1)) / (per_k > 0 ? per_k : 1)) & ~31LL;
        if (same && K > 0 && kc_max >= 2048) {
            const long long nchunk = (K + kc_max - 1) / kc_max;
            const long long kc0 = ((K + nchunk - 1) / nchunk + 31) & ~31LL;
            rc = tn_run_chunks(L, K, kc0, false, ws, mode, true, st);
            return take;
        }
    }
    for (int i = 0; i < L.nprob; ++i) {
        if (!(take & (1u << i))) continue;
        const DevProb &pfull = L.p[i];
        const bool by_seg = pfull.nseg > 1 && chunk[i] < h3_kp(pfull);   // does not fit: one single-segment pass per segment
        const int npass = by_seg ? pfull.nseg : 1;
        for (int pass = 0; pass < npass; ++pass) {
            DevLaunch L1 = {};
            L1.nprob = 1;
            L1.p[0] = pfull;
            if (by_seg) {
                L1.p[0].nseg = 1;
                L1.p[0].seg[0] = pfull.seg[pass];
            }
            rc = tn_run_chunks(L1, h3_kp(L1.p[0]), chunk[i], pass > 0, ws, mode, false, st);
            if (rc) return take;
        }
    }
    return take;
}

// Split-K plan for launches with too few tiles to occupy the chip (small M): every workgroup would
// otherwise walk the whole contraction serially (~0.8 us per 32-deep chunk).  Returns the split count
// (1 = no split) and carves one [S, M, N] slab region per problem out of the caller's workspace.
static int plan_splitk(DevLaunch &L, float *ws, long long ws_floats) {
    if (!ws || ws_floats <= 0) return 1;
    const long long blocks = count_tiles(L, 32, 128);
    long long need1 = 0;
    int min_chunks = 1 << 30;
    for (int i = 0; i < L.nprob; ++i) {
        const DevProb &p = L.p[i];
        if (p.N & 3) return 1;
        need1 += (long long)p.M * p.N;
        int ch = 0;
        for (int s = 0; s < p.nseg; ++s) ch += (p.seg[s].K + BK - 1) / BK;
        if (ch < min_chunks) min_chunks = ch;
    }
    if (blocks >= 384) return 1;
    long long S = 768 / blocks;
    if (S > 16) S = 16;
    if (S > min_chunks / 4) S = min_chunks / 4;      // keep >= 4 chunks per split
    if (S > ws_floats / need1) S = ws_floats / need1;
    if (S < 2) return 1;
    float *at = ws;
    for (int i = 0; i < L.nprob; ++i) {
        DevProb &p = L.p[i];
        p.ksplit = (int)S;
        p.slab = at;
        p.slab_stride = (long long)p.M * p.N;
        at += S * p.slab_stride;
    }
    return (int)S;
}

// The one routing chain of the forward (NT) entry points, in this order:
//   1. the matrix-vector kernels (few rows)                      gemv_plan
//   2. the skinny split-f16 kernels (inside a weights scope)     h3s_plan
//   3. fp32 split-K: the 32-row tile with the linear epilogue writes slabs, the reduce kernel of EPI finishes them
//   4. the large split-f16 kernels                               h3_plan
//   5. the fp32 tiles by the cost model (allow_xl: the 256-row tile may be chosen)
// decide_only: launches nothing and leaves the weights scope alone; returns 1 when step 4 - the one path that reads
// isc_seg.a_f16 rows - would take the launch, 0 when another step would.  Otherwise returns the launches' status.
template <int EPI>
static int route_nt(DevLaunch &L, float *ws, long long ws_floats, hipStream_t st, bool allow_xl, bool decide_only) {
    if (const int kmax = gemv_plan<EPI>(L)) return decide_only ? 0 : gemv_run<EPI>(L, kmax, st);
    const H3sPlan hs = h3s_plan<EPI>(L, ws, ws_floats, st, 0);
    if (hs.T) return decide_only ? 0 : h3s_run<EPI>(L, hs, ws, ws_floats, st, 0);
    if (plan_splitk(L, ws, ws_floats) > 1) {
        if (decide_only) return 0;
        finish_tiling(L, 2);
        const int rc = launch_any<EPI_LINEAR, false, false>(L, 2, st);
        return rc ? rc : launch_splitk_reduce<EPI>(L, st);
    }
    const H3Plan h = h3_plan<EPI>(L, ws, ws_floats, st, 0);
    if (h.take) return decide_only ? 1 : h3_run<EPI>(L, h, ws, st, 0);
    if (decide_only) return 0;
    const int tile = pick_tile(L, allow_xl, true, true);
    finish_tiling(L, tile);
    return launch_any<EPI, false, false>(L, tile, st);
}

// isc_linear_fwd.  decide_only: route_nt's answer (< 0 for a bad argument).
static int linear_fwd_run(const isc_linear_problem *pr, int n_prob, void *stream, bool decide_only) {
    if (!pr) return ISC_E_NULL;
    if (n_prob < 1 || n_prob > 3) return ISC_E_SHAPE;
    DevLaunch L = {};
    L.nprob = n_prob;
    L.gate = isc_stream_gate_(stream);
    for (int i = 0; i < n_prob; ++i) {
        const isc_linear_problem &q = pr[i];
        int rc = check_segs(q.seg, q.nseg);
        if (rc) return rc;
        if (!q.C) return ISC_E_NULL;
        if (q.M <= 0 || q.N <= 0) return ISC_E_SHAPE;
        if (q.keep_mask && q.ldc != q.N) return ISC_E_SHAPE;
        DevProb &d = L.p[i];
        copy_segs(d, q.seg, q.nseg);
        d.M = q.M; d.N = q.N; d.relu = q.relu;
        d.bias0 = q.bias0; d.bias1 = q.bias1; d.bias2 = q.bias2;
        d.mask = q.keep_mask; d.mask_scale = q.mask_scale;
        d.ldc = q.ldc; d.C = q.C; d.C_pre = q.C_pre; d.accumulate = q.accumulate;
    }
    return route_nt<EPI_LINEAR>(L, pr[0].splitk_ws, pr[0].splitk_ws_floats, (hipStream_t)stream, true, decide_only);
}

// What the native form asks of an f16 segment (K % 32 == 0 is check_segs')
static bool f16_segs_aligned(const isc_linear_problem *pr, int n_prob) {
    for (int i = 0; i < n_prob; ++i)
        for (int s = 0; s < pr[i].nseg && s < ISC_MAX_SEG; ++s)
            if (pr[i].seg[s].a_f16 && ((pr[i].seg[s].lda & 7) || !isc_aligned16(pr[i].seg[s].A))) return false;
    return true;
}

extern "C" int isc_linear_f16_native(const isc_linear_problem *pr, int n_prob, void *stream) {
    if (!pr || n_prob < 1 || n_prob > 3 || !f16_segs_aligned(pr, n_prob)) return 0;
    return linear_fwd_run(pr, n_prob, stream, true) == 1 ? 1 : 0;
}

extern "C" int isc_linear_fwd(const isc_linear_problem *pr, int n_prob, void *stream) {
    bool any16 = false;
    for (int i = 0; pr && i < n_prob && i < 3; ++i) any16 = any16 || segs_any_f16(pr[i].seg, pr[i].nseg);
    if (any16) {                       // f16 rows: the large split-f16 kernels or nothing
        if (!f16_segs_aligned(pr, n_prob)) return ISC_E_ALIGN;
        const int native = linear_fwd_run(pr, n_prob, stream, true);
        if (native != 1) return native < 0 ? native : ISC_E_SHAPE;
    }
    return linear_fwd_run(pr, n_prob, stream, false);
}

// dX contractions outside a weights scope still go to the split-f16 kernels from this size on (the classifier's dX over
// a zero-padded copy of W_c that autograd.py keeps out of the scope on purpose - B = 512: 105 GFLOP, 606 us on the fp32
// tiles -, the prologue's d att_e = d att_p W at B >= 256: 19 GFLOP, 283 us at B = 1024): planes of this call's W^T go to
// the workspace, one split launch of at most 20 MB against 0.2-0.3 ms saved
#define H3_NN_MIN_FLOPS 5.0e9

// One backward launch: validates, fills the launch, routes it (isc_gemm_bwd below).
static int gemm_bwd_run(const isc_linear_problem *pr, int n_prob, int layout, hipStream_t st) {
    DevLaunch L = {};
    L.nprob = n_prob;
    bool k32 = true;
    for (int i = 0; i < n_prob; ++i) {
        const isc_linear_problem &q = pr[i];
        if (q.nseg < 1 || q.nseg > ISC_MAX_SEG || !q.C) return q.C ? ISC_E_SHAPE : ISC_E_NULL;
        if (q.M <= 0 || q.N <= 0 || (q.N & 3) || (q.ldc & 3)) return ISC_E_SHAPE;
        if (layout == ISC_LAYOUT_TN && (q.M & 3)) return ISC_E_SHAPE;
        for (int s = 0; s < q.nseg; ++s) {
            const isc_seg &g = q.seg[s];
            if (!g.A || !g.W) return ISC_E_NULL;
            // NN with K % 4 != 0 (vocabulary-sized K): the caller pads A's rows to lda with zeros
            if (g.K <= 0) return ISC_E_SHAPE;
            if ((g.lda & 3) || (g.ldw & 3) || !isc_aligned16(g.A) || !isc_aligned16(g.W)) return ISC_E_ALIGN;
            k32 = k32 && (g.K & 31) == 0;
        }
        DevProb &d = L.p[i];
        copy_segs(d, q.seg, q.nseg);
        d.M = q.M; d.N = q.N; d.relu = 0;
        d.bias0 = q.bias0; d.bias1 = q.bias1; d.bias2 = q.bias2;
        d.ldc = q.ldc; d.C = q.C; d.accumulate = q.accumulate;
    }
    float *ws = pr[0].splitk_ws;
    const long long ws_floats = pr[0].splitk_ws_floats;
    const int mode = g_h3_mode.load();
    const bool nn_big = mode == 1 && n_prob == 1 && contraction_flops(pr[0]) >= H3_NN_MIN_FLOPS;
    if (layout == ISC_LAYOUT_NN && k32 && (h3w_scope_of(st) || mode >= 2 || nn_big)) {
        // inside a weights scope (the BPTT sweep): dX = dY W on planes of W^T built once per scope - the skinny tiles for
        // few rows, the large split-f16 kernels otherwise; dY is read as fp32 rows and split in registers
        const H3sPlan hs = h3s_plan<EPI_LINEAR>(L, ws, ws_floats, st, 1);
        if (hs.T) return h3s_run<EPI_LINEAR>(L, hs, ws, ws_floats, st, 1);
        const H3Plan h = h3_plan<EPI_LINEAR>(L, ws, ws_floats, st, 1);
        if (h.take) return h3_run<EPI_LINEAR>(L, h, ws, st, 1);
    }
    if (layout == ISC_LAYOUT_TN) {
        int rc_h3 = ISC_OK;
        const unsigned took = try_h3_tn(L, ws, ws_floats, st, rc_h3);
        if (rc_h3) return rc_h3;
        if (took) {                                     // the rest of the launch stays on the fp32 tiles
            int n = 0;
            for (int i = 0; i < L.nprob; ++i)
                if (!(took & (1u << i))) { if (n != i) L.p[n] = L.p[i]; ++n; }
            if (n == 0) return ISC_OK;
            L.nprob = n;
        }
    }
    const int S = plan_splitk(L, ws, ws_floats);
    const int tile = S > 1 ? 2 : pick_tile(L, false, false);
    finish_tiling(L, tile);
    int rc = layout == ISC_LAYOUT_NN ? launch_any<EPI_LINEAR, false, true>(L, tile, st)
                                     : launch_any<EPI_LINEAR, true, true>(L, tile, st);
    if (rc || S == 1) return rc;
    return launch_splitk_linear_reduce(L, st);
}

// Backward-pass contractions on the same kernel (include/insenticap_hip.h: isc_gemm_bwd).
extern "C" int isc_gemm_bwd(const isc_linear_problem *pr, int n_prob, int layout, void *stream) {
    if (!pr) return ISC_E_NULL;
    if (n_prob < 1 || n_prob > 3 || (layout != ISC_LAYOUT_NN && layout != ISC_LAYOUT_TN)) return ISC_E_SHAPE;
    for (int i = 0; i < n_prob; ++i)
        if (segs_any_f16(pr[i].seg, pr[i].nseg)) return ISC_E_SHAPE;          // fp32 operands only
    // dW = sum over segments of A_s^T W_s where some segments have a row count the split-f16 kernels cannot take (K % 32
    // != 0: the once-per-caption block of the att-LSTM's dW has B rows, 80 in the seq2seq unroll) and others are large:
    // two launches - the K % 32 == 0 segments first (split-f16), the rest accumulating on the fp32 tiles - instead of
    // the whole sum on the fp32 tiles (3.5 GFLOP, 82 us per iteration)
    if (layout == ISC_LAYOUT_TN && n_prob == 1 && pr[0].nseg > 1 && pr[0].nseg <= ISC_MAX_SEG && g_h3_mode.load() != 0) {
        isc_linear_problem a = pr[0], b = pr[0];
        a.nseg = b.nseg = 0;
        for (int s = 0; s < pr[0].nseg; ++s) {
            isc_linear_problem &to = pr[0].seg[s].K > 0 && (pr[0].seg[s].K & 31) == 0 ? a : b;
            to.seg[to.nseg++] = pr[0].seg[s];
        }
        if (a.nseg > 0 && b.nseg > 0 && contraction_flops(a) >= H3_TN_MIN_FLOPS) {
            const int rc = gemm_bwd_run(&a, 1, layout, (hipStream_t)stream);
            if (rc) return rc;
            b.accumulate = 1; b.bias0 = b.bias1 = b.bias2 = nullptr;
            return gemm_bwd_run(&b, 1, layout, (hipStream_t)stream);
        }
    }
    return gemm_bwd_run(pr, n_prob, layout, (hipStream_t)stream);
}

extern "C" int isc_lstm_fwd(const isc_lstm_problem *q, void *stream) {
    if (!q) return ISC_E_NULL;
    int rc = check_segs(q->seg, q->nseg);
    if (rc) return rc;
    if (segs_any_f16(q->seg, q->nseg)) return ISC_E_SHAPE;                    // fp32 activations only
    if (!q->c_prev || !q->h_out || !q->c_out) return ISC_E_NULL;
    if ((!q->b_ih || !q->b_hh) && !q->pre) return ISC_E_NULL;       // biases may only be folded into `pre`
    if ((q->b_ih == nullptr) != (q->b_hh == nullptr)) return ISC_E_NULL;
    if (q->tab && !q->tab_ids) return ISC_E_NULL;
    if (q->M <= 0 || q->H <= 0 || (q->H % 32) != 0) return ISC_E_SHAPE;
    if (q->h_keep_mask && !q->hdrop_out) return ISC_E_NULL;
    if (q->pre_div > 1 && (!q->pre || q->M % q->pre_div)) return ISC_E_SHAPE;
    DevLaunch L = {};
    L.nprob = 1;
    L.gate = isc_stream_gate_(stream);
    DevProb &d = L.p[0];
    copy_segs(d, q->seg, q->nseg);
    d.M = q->M; d.N = 4 * q->H; d.H = q->H;
    d.bias0 = q->b_ih; d.bias1 = q->b_hh;
    d.c_prev = q->c_prev; d.h_out = q->h_out; d.c_out = q->c_out; d.gates_out = q->gates_out;
    d.hmask = q->h_keep_mask; d.mask_scale = q->mask_scale; d.hdrop = q->hdrop_out;
    if ((q->h_hi == nullptr) != (q->h_lo == nullptr)) return ISC_E_NULL;
    d.h_hi = static_cast<_Float16 *>(q->h_hi); d.h_lo = static_cast<_Float16 *>(q->h_lo);
    d.pre = q->pre; d.tab = q->tab; d.tab_ids = q->tab_ids; d.tab_ids_stride = q->tab_ids_stride;
    d.pre_div = q->pre_div > 1 ? q->pre_div : 1;
    // XL only for the bias-only cell: a hoisted `pre` term or an embedding-table gather adds 8-16 B of
    // epilogue reads per output, which the XL tile's lone workgroup per CU cannot overlap with MFMA work
    // (in the roll-out: att-LSTM 168 us on the 128x128 tile vs 178 us on XL; lang-LSTM 223 vs 206; with the
    // batched epilogue loads of lstm_cells the two are within 2 % of each other on either cell)
    return route_nt<EPI_LSTM>(L, q->splitk_ws, q->splitk_ws_floats, (hipStream_t)stream, !q->pre && !q->tab, false);
}

extern "C" int isc_vocab_fwd(const float *h, int ldh, const float *W, int ldw, const float *bias,
                             int M, int V, int K, float *logits, int64_t ld_logits,
                             float *part_max, float *part_sum, int32_t *part_idx,
                             const void *h_hi, const void *h_lo,
                             float *splitk_ws, int64_t splitk_ws_floats, void *stream) {
    if (!h || !W || !bias || !part_max || !part_sum || !part_idx) return ISC_E_NULL;
    isc_seg sg = {h, W, ldh, ldw, K, 0, h_hi, h_lo};
    int rc = check_segs(&sg, 1);
    if (rc) return rc;
    if (M <= 0 || V <= 0) return ISC_E_SHAPE;
    DevLaunch L = {};
    L.nprob = 1;
    L.gate = isc_stream_gate_(stream);
    DevProb &d = L.p[0];
    copy_segs(d, &sg, 1);
    d.M = M; d.N = V; d.bias0 = bias;
    d.C = logits; d.ld_logits = ld_logits;
    d.pmax = part_max; d.psum = part_sum; d.pidx = part_idx;
    d.ntile_total = (V + 127) / 128;
    // Few rows (beam search, small batches): the 16-chunk contraction of a 32-row tile is a serial walk of ~27 us, so
    // route_nt splits it over K.  Many rows end on the 128x128 LDS-DMA tile: at [4096 x 10000 x 512] 121 TFLOP/s there,
    // 115 on the register-staged 128x128 tile and 108 on XL, whose lone workgroup per CU has nothing to hide the per-row
    // softmax statistics of the epilogue behind (3k VALU instructions per wave at the end of a 16-chunk tile).
    return route_nt<EPI_VOCAB>(L, splitk_ws, splitk_ws_floats, (hipStream_t)stream, false, false);
}
