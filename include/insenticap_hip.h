/*
 * insenticap_hip.h - C ABI of libinsenticap_hip.so (gfx950 / MI355X).
 *
 * The upstream project (ezeli/InSentiCap_model) has no FFI or plugin layer: its
 * caption decoder is pure Python on stock torch ops. The drop-in boundary is the
 * Python class surface of `Captioner` / `Detector`; this header
 * is the native boundary underneath it: one entry point per
 * fused unit of the reference's decode step. Each declaration cites the reference
 * lines it replaces.
 *
 * Conventions (all entry points):
 *   - plain pointers and sizes only; every pointer is a DEVICE pointer unless the
 *     name ends in _host; tensors are row-major fp32, ids are int64 ("LongTensor");
 *   - no allocation, no ownership transfer, no device synchronisation: work is enqueued on
 *     `stream` (a hipStream_t passed as void*);
 *   - no data-carrying global state: entry points may be called from several host threads on
 *     distinct streams at once (tests/test_gpu_threads.py).  What the library keeps is (a) two
 *     process-wide tuning words, isc_set_tile_override / isc_set_h3_mode / isc_set_gemv_rows (atomic; they pick a
 *     kernel, never change a result beyond fp32 summation order), (b) launch counters (atomic),
 *     and (c) the split-f16 weights scopes, which are keyed by stream (isc_h3_weights_begin);
 *   - return value: 0 ok; <0 bad argument / unsupported shape (ISC_E_*);
 *     >0 a hipError_t from the launch. Never throws, never exits.
 *   - leading dimensions are in elements; every row start must be 16-byte aligned
 *     and every contraction length a multiple of 32.
 */
#ifndef INSENTICAP_HIP_H
#define INSENTICAP_HIP_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define ISC_OK 0
#define ISC_E_NULL (-1)      /* required pointer is null */
#define ISC_E_SHAPE (-2)     /* unsupported size (K %32, dims %32, too many segments ...) */
#define ISC_E_ALIGN (-3)     /* pointer or leading dimension not 16-byte aligned */
#define ISC_E_WORKSPACE (-4) /* caller-provided workspace too small */
#define ISC_E_STATE (-5)     /* nothing to resume (isc_h3_weights_resume) */

#define ISC_MAX_SEG 4

/* Library / build identification ("gfx950", ABI version). */
int isc_abi_version(void);
const char *isc_target_arch(void);
/* Tuning / test hook: force the GEMM tile shape of isc_linear_fwd / isc_lstm_fwd / isc_vocab_fwd /
 * isc_gemm_bwd (0 = 128x128, 1 = 64x128, 2 = 32x128, 3 = 256x128 LDS-DMA ring, 4 = 128x128 LDS-DMA [3 and 4: NT
 * layout only; other layouts fall back to 0]); -1 (default) = the cost model picks.  Results are identical up to fp32
 * summation order for every shape; process-wide, not meant to be flipped while launches are in flight
 * on other threads.  Returns the previous value. */
int isc_set_tile_override(int tile);
/* Split-f16 GEMM path of the forward entry points (isc_linear_fwd / isc_lstm_fwd / isc_vocab_fwd): fp32 operands
 * are split into two f16 planes each (x = hi + lo * 2^-11) inside the caller's workspace and contracted with three
 * f16 MFMAs per k-step into fp32 accumulators - fp32 in, fp32 out, error against an fp64 contraction no larger than
 * an fp32 FMA chain's (tests/test_gpu_h3.py), at 2-2.5x the fp32 MFMA rate.  Operand domain |x| < 65504.
 * mode 0 = off (fp32 MFMA tiles only); 1 = auto (default): on a stream that holds a weights scope a launch takes the
 * skinny split-f16 kernel (one launch per GEMM, no split-K slabs; 32 x 32 or 64 x 64 tiles, whichever needs fewer
 * rounds of the chip) while that is at most ~4 rounds of small tiles, else the large split-f16 kernels; without a
 * scope, launches of >= 160 128x128 tiles take the large kernels and the rest the fp32 tiles; 2 = the large kernels
 * whenever shapes and workspace allow; 3 / 4 = the skinny kernel with 32 x 32 / 64 x 64 tiles whenever shapes allow
 * (test hooks: without a scope the weight planes go to the workspace).  The planes of a launch must fit the
 * workspace.  A tile override (>= 0) also disables the path.  Returns the previous mode. */
int isc_set_h3_mode(int mode);
/* Number of launches that went out on the split-f16 path so far (process-wide; measurement / test hook);
 * isc_h3x_launches: those of them that took the 256x128 eight-wave tile (launches of >= 224 such tiles). */
long long isc_h3_launches(void);
/* Few rows (beam rows of one image, a handful of captions): isc_linear_fwd / isc_lstm_fwd / isc_vocab_fwd launches
 * whose problems all have M <= rows (default and maximum 8) and K <= 4096 go out as ONE fused matrix-vector kernel
 * each (gemv_rows_kernel: weights read as fp32 with the whole launch's traffic in flight, exact fp32 FMA, activations
 * staged in LDS, LSTM cell / vocabulary statistics in the epilogue - north_star's "fused LSTM gate GEMV +
 * sigmoid/tanh").  Modes 0 and 1 of isc_set_h3_mode only (2-4 force the split-f16 kernels).  rows = 0 switches the
 * path off; returns the previous value.  isc_gemv_launches: launches that went out this way (test hook). */
int isc_set_gemv_rows(int rows);
long long isc_gemv_launches(void);
long long isc_h3x_launches(void);
/* Launches that took the skinny split-f16 kernel (few rows: one launch per GEMM instead of split-K + reduce). */
long long isc_h3s_launches(void);
/* Launches of the exact-fp32 GEMM kernels since the library was loaded, by kind (process-wide, read-only; test hook:
 * the one way to tell which fp32 kernel a launch took).  kind 0 / 1 / 2 = the register-staged gemm_kernel on the
 * 128 / 64 / 32-row tile, every layout (NT, NN, TN) and epilogue summed; 3 = the 256-row LDS-DMA tile (XL); 4 = the
 * 128-row LDS-DMA tile (LD); 5 = the 64-row LDS-DMA tile (MD: what tile 1 runs for plain linear NT launches); 6 = a
 * split-K reduce launch of any epilogue (linear, LSTM, vocabulary; the reduce behind a K-split of the split-f16
 * kernels included).  Any other kind returns -1.  A call turned away on the host counts nowhere. */
long long isc_f32_launches(int kind);
/* Launches of the split-f16 GEMM kernels since the library was loaded, by kernel instantiation (process-wide,
 * read-only; host counters incremented at the launch sites; test hook: the one way to tell which split-f16 kernel a
 * launch took).  kind 3 g + f = a large tile of geometry g (0 / 1 / 2 = gemm_h3_kernel 128 rows / gemm_h3x_kernel 256
 * rows / gemm_h3m_kernel 64 rows) whose activations are all planes (f = 0), some fp32 rows (f = 1), or f16 rows
 * (f = 2: gemm_h3_f16a_kernel); 9 / 10 / 11 = gemm_h3s_kernel 32 x 32 on four waves / 32 x 32 on eight waves / 64 x 64
 * (linear and LSTM epilogue); 12 / 13 = its vocabulary form, 32 x 128 on four / eight waves; 14 / 15 = gemm_h3v_kernel
 * on planes / on fp32 rows; 16 = a launch of h3_split_kernel (plain or transposing, any number of jobs, a weights
 * refresh included).  The epilogue is fixed by the entry point and has no kind.  Any other kind returns -1.
 * isc_h3_launches / isc_h3x_launches / isc_h3s_launches / isc_h3_f16a_launches keep their meaning (per entry-point
 * launch, by path). */
long long isc_h3_kernel_launches(int kind);
/* Weights scope of the split-f16 path.  Between _begin and _end the caller guarantees that no weight matrix passed
 * to the forward entry points changes (a roll-out's decode loop): each weight operand is then split into its planes
 * once, into `buf` (device memory, 256-byte aligned; 64 MB holds the decoder's matrices), and later launches with
 * the same weight segments reuse them instead of re-splitting per step.  A scope belongs to ONE stream: only
 * launches on `stream` see it, and they must be issued in one order (as a stream's launches are anyway); up to 64
 * streams may hold a scope - active or suspended - at once (ISC_E_WORKSPACE beyond that: run without; a suspended scope
 * of another stream is never taken over).  Without a scope, or when `buf` is
 * full, every launch splits its weights into the workspace.  _begin discards the stream's earlier entries; _end
 * closes its scope (`buf` may then be reused). */
int isc_h3_weights_begin(void *buf, long long bytes, void *stream);
int isc_h3_weights_end(void *stream);
/* _suspend leaves the stream's scope (no launch sees it any more) but keeps its planes; _resume(buf, stream) re-opens
 * it as it was - the caller vouches that no weight has changed since (Captioner keys it on the parameters' version
 * counters, so consecutive eval-mode calls split the weights once, not once per call) - or returns ISC_E_STATE when
 * the slot has meanwhile been recycled (then: _begin).  Between the two, launches on the stream run without a scope. */
int isc_h3_weights_suspend(void *stream);
int isc_h3_weights_resume(void *buf, void *stream);
/* Re-split every weight the stream's scope (active or suspended) holds planes of from the weights' current values - for an
 * optimiser that has just updated them in place on the same stream: the scope can then be resumed instead of rebuilt entry
 * by entry (few batched split launches instead of one per weight operand).  ISC_E_STATE: the stream has no scope. */
int isc_h3_weights_refresh(void *stream);

/* One K-segment of a contraction: acc += A[M,K] * W[N,K]^T.  Replaces the
 * torch.cat([...],1) + nn.Linear / nn.LSTMCell pattern of captioner.py:174-175,180-181. */
typedef struct {
    const float *A; /* [M, K] activations, leading dim lda */
    const float *W; /* [N, K] weight slice (row-major, K contiguous), leading dim ldw */
    int32_t lda, ldw, K;
    /* 0: A is fp32 (above).  1: A points at _Float16 rows [M, K] with lda in HALFS - isc_linear_fwd only, and only
     * where the launch takes the large split-f16 kernels, which read such rows natively (an f16 value is its own hi
     * plane and has lo == 0, so the result equals the fp32 path's on the up-cast values bit for bit).  Needs
     * K % 32 == 0, lda % 8 == 0 and a 16-byte aligned A.  isc_linear_f16_native tells beforehand whether a launch will
     * be read natively; every entry point that cannot read halfs returns ISC_E_SHAPE for a_f16 = 1 and launches
     * nothing - convert with isc_f16_to_f32 first. */
    int32_t a_f16;
    /* Optional (forward entry points, split-f16 path): the f16 planes of A as a producer wrote them
     * (isc_lstm_problem.h_hi / h_lo ...): hi = f16(x), lo = f16((x - hi) * 2048), in ONE buffer of 2*M*K halfs with the
     * two planes interleaved per 32-wide k-block (so that a chunk consumes whole 128-byte lines):
     *     hi(m, k) = buf[m*2K + (k/32)*64 + k%32],   lo(m, k) = the same + 32;   A_hi = buf, A_lo = buf + 32 halfs.
     * Every plane pointer pair of this header uses that layout for its own [rows, width] tensor (K % 32 == 0).
     * When present and the launch takes the split-f16 path, A is read from the planes instead of being split again;
     * `A` must still be valid (the fp32 tiles read it).  Null = split on the fly. */
    const void *A_hi, *A_lo;
} isc_seg;

/* y = act(sum_seg A_s W_s^T + bias0 + bias1) [* keep_mask * mask_scale]
 * Replaces nn.Linear(+ReLU)(+Dropout) of captioner.py:137-154 (fc_embed, cpt2fc, att_embed,
 * att2att, senti2att) and the per-step projections h2att / h2word / label2word
 * (captioner.py:26,51-52) and cont2att+senti2att+h2att of the gate (captioner.py:107-110).
 * Up to 3 independent problems are grouped in one launch (n_prob). */
typedef struct {
    isc_seg seg[ISC_MAX_SEG];
    int32_t nseg, M, N, relu;
    const float *bias0, *bias1, *bias2; /* [N] or null (the gate sums three nn.Linear outputs) */
    const uint8_t *keep_mask;   /* [M,N] contiguous 0/1 dropout keep-mask or null */
    float mask_scale;           /* 1/(1-p) */
    int32_t ldc;
    float *C;                   /* [M,N] */
    float *C_pre;               /* optional: activation before the mask (captioner.fc_feats attr) */
    int32_t accumulate;         /* C += result (gradient accumulation) */
    int32_t _pad;
    /* Optional split-K workspace (of the FIRST problem of a launch): when a launch has too few tiles to
     * occupy the chip (small M), the contraction is split over ksplit workgroups per tile, partial tiles go
     * to [ksplit, M, N] slabs in this buffer and a second kernel reduces them in fixed order and applies
     * the epilogue (bitwise reproducible). NULL disables it. */
    float *splitk_ws;
    int64_t splitk_ws_floats;
} isc_linear_problem;

int isc_linear_fwd(const isc_linear_problem *probs_host, int n_prob, void *stream);
/* 1 when isc_linear_fwd, called now with these problems on `stream`, reads their isc_seg.a_f16 = 1 segments natively
 * (the large split-f16 kernels take the launch and every such segment meets the alignment rules), else 0: the caller
 * then converts those segments (isc_f16_to_f32) and clears the flag.  The answer comes from the dispatch of
 * isc_linear_fwd itself, run without launching.  isc_h3_f16a_launches: launches that read at least one f16 segment
 * natively (test hook). */
int isc_linear_f16_native(const isc_linear_problem *probs_host, int n_prob, void *stream);
long long isc_h3_f16a_launches(void);
/* dst[r, c] = (float)src[r, c] for _Float16 src [rows, cols] (leading dims ld_src in halfs, ld_dst in floats; exact).
 * isc_f16_convert_launches: how often it ran (test hook: the native f16 path must not move it). */
int isc_f16_to_f32(const void *src, int64_t ld_src, float *dst, int64_t ld_dst, int64_t rows, int64_t cols,
                   void *stream);
long long isc_f16_convert_launches(void);

/* Backward-pass contractions of the same layers (what autograd derives for nn.Linear /
 * nn.LSTMCell / the classifier in train_xe.py:190, decoder.py:165), on the same MFMA kernel:
 *   ISC_LAYOUT_NN  C[M,N] (+)= sum_s A_s[M,K_s] * W_s[K_s,N]      dX = dY * W
 *                  (W_s row-major [K_s,N]: an nn.Linear weight [out=K_s, in=N] as stored)
 *   ISC_LAYOUT_TN  C[M,N] (+)= sum_s A_s[K_s,M]^T * W_s[K_s,N]    dW = dY^T * X
 *                  (contraction over the K_s batch rows; A_s = dY [rows, M], W_s = X [rows, N])
 * bias/relu/mask fields are ignored except bias0..2 (added), M/N/ldc %4 == 0. */
#define ISC_LAYOUT_NN 1
#define ISC_LAYOUT_TN 2
int isc_gemm_bwd(const isc_linear_problem *probs_host, int n_prob, int layout, void *stream);

/* Fused LSTMCell: gates = sum_seg A_s W_s^T + b_ih + b_hh (row blocks i,f,g,o of 4H),
 * c' = sig(f) c + sig(i) tanh(g), h' = sig(o) tanh(c').  Replaces nn.LSTMCell at
 * captioner.py:175 (att_lstm) and :181 (lang_lstm).  h_out/c_out may not alias inputs.
 * gates_out (optional, [M,4H], activated i,f,g,o) is saved for the backward pass.
 * h_keep_mask (optional) additionally writes hdrop_out = h' * mask * scale
 * (the nn.Dropout on h_lang, captioner.py:182). */
typedef struct {
    isc_seg seg[ISC_MAX_SEG];
    int32_t nseg, M, H, _pad;
    const float *b_ih, *b_hh; /* [4H] */
    const float *c_prev;      /* [M,H] contiguous */
    float *h_out, *c_out;     /* [M,H] contiguous */
    float *gates_out;         /* [M,4H] or null */
    const uint8_t *h_keep_mask; /* [M,H] or null */
    float mask_scale;
    float *hdrop_out;         /* [M,H], required iff h_keep_mask */
    void *h_hi, *h_lo;        /* optional: f16 planes of h_out ([M,H] each) for consumers' isc_seg.A_hi / A_lo */
    /* Hoisted step-invariant inputs (optional): gates += pre[m,:] + tab[tab_ids[m*tab_ids_stride],:].
     * `pre` [M,4H] holds fc W_fc^T + label W_x^T + b_ih + b_hh computed once per call (b_ih/b_hh may
     * then be null); `tab` [V,4H] = relu(Emb) W_x^T replaces the word-embedding K-segment when the
     * weights are frozen (inference). */
    const float *pre;
    const float *tab;
    const int64_t *tab_ids;
    int64_t tab_ids_stride;
    float *splitk_ws;           /* optional split-K workspace, see isc_linear_problem */
    int64_t splitk_ws_floats;
    /* pre_div > 1: `pre` holds one row per IMAGE of M / pre_div images ([M / pre_div, 4H]) and row m adds
     * pre[m / pre_div] - the captions drawn for one image share its fc / label term (isc_step_plan.row_div).
     * M % pre_div == 0; 0 or 1 = one row of `pre` per row. */
    int32_t pre_div, _pad2;
} isc_lstm_problem;

int isc_lstm_fwd(const isc_lstm_problem *prob_host, void *stream);

/* Vocabulary projection with fused log-softmax statistics (captioner.py:183):
 * logits = h W^T + b.  Per 128-column tile the kernel emits (max, argmax, sum exp(x-max));
 * the [M,V] logits are only stored when `logits` is non-null (XE / beam / sampling).
 * n_tile = ceil(V/128); part_* are [M, n_tile].  With a split-K workspace (optional, see
 * isc_linear_problem) launches of few rows contract K in parallel slices and a reduce kernel forms the
 * same outputs (V % 4 == 0 required for that route; otherwise the single-pass kernel runs).
 * h_hi / h_lo (optional): f16 planes of h ([M,K] contiguous, see isc_seg.A_hi). */
int isc_vocab_fwd(const float *h, int ldh, const float *W, int ldw, const float *bias,
                  int M, int V, int K, float *logits, int64_t ld_logits,
                  float *part_max, float *part_sum, int32_t *part_idx,
                  const void *h_hi, const void *h_lo,
                  float *splitk_ws, int64_t splitk_ws_floats, void *stream);

/* logp[m, :] = logits[m, :] - logsumexp(row) in place, using the tile statistics.
 * (F.log_softmax of captioner.py:183 when the full [B,V] row is an API output.) */
int isc_logsoftmax_apply(float *logits, int64_t ld_logits, int M, int V,
                         const float *part_max, const float *part_sum, float *lse_out,
                         void *stream);
/* The same for all T steps of a teacher-forced unroll in ONE launch: logits [B,T,V] with row (b,t) at b*ld_b + t*ld_t,
 * tile statistics stacked per step [T,B,n_tile] (each step's isc_vocab_fwd / isc_step_fwd wrote its slice).
 * src (may be NULL = in place): raw logits stacked per step, contiguous [T*B, V] - what ONE isc_vocab_fwd over all
 * steps' h_lang [T*B, H] writes (torch.stack(outputs, dim=1) of captioner.py:232 happens in this kernel's store). */
int isc_logsoftmax_apply_steps(float *logits, int64_t ld_b, int64_t ld_t, int B, int T, int V,
                               const float *part_max, const float *part_sum, const float *src, int step_rows,
                               void *stream);
/* step_rows (0 = B): rows per step of the statistics / src stacks - row (t, b) sits at t*step_rows + b.  The stacks of a
 * merged unroll (isc_step_plan.pair_rows_c) hold both branches' rows per step; each branch's [B,T,V] log-probs come from
 * its own call with part_max / part_sum / src pointing at the branch's first row. */

/* Additive attention scan (ContentAttention captioner.py:23-35 / SentiAttention :50-62):
 *   e_r = w . tanh(P[b,r,:] + q[b,:] (+ q2[b,:])) + *w_bias ; alpha = softmax_r(e) ;
 *   out[b,:] = sum_r alpha_r V[b,r,:]
 * P: [B,R,A] projected features, V: [B,R,D] features, q: [B,A] (h projection incl. bias),
 * q2: optional [B,A] (label2word term), alpha_out: [B, alpha_ld] slice of the per-call
 * weights tensor.  Two independent scans (content + sentiment words) can be issued in
 * one launch. */
typedef struct {
    const float *P, *V, *q, *q2, *w;
    const float *w_bias; /* device pointer to the scalar bias of the alpha layer */
    int32_t R, A, D;
    int32_t rows;     /* rows of THIS problem; 0 = the launch's B.  The two problems of a launch may differ: the merged
                       * step of two sibling unrolls (isc_step_plan.pair_rows_c) scans the regions for its first rows and
                       * the sentiment words for the rest in ONE launch. */
    float *out;       /* [B,D] */
    float *alpha_out; /* [B,*] row stride alpha_ld, R values written per row */
    int64_t alpha_ld;
    void *out_hi, *out_lo; /* optional: f16 planes of `out` ([B,D] each, see isc_seg.A_hi) */
    /* Optional gather mode: region r of row b is row row_ids[b*row_ids_ld + r] of P / V, which are then tables
     * [n_rows, A] / [n_rows, D] shared by all rows.  The sentiment words of captioner.py:307-312 in eval mode:
     * word_embed(id) and senti2att(word_embed(id)) depend on the id alone, so two vocabulary-sized tables
     * (cache-resident) replace the per-caption [B,M,.] copies that were streamed from HBM every step. */
    const int64_t *row_ids;
    int64_t row_ids_ld;
    /* row_div > 1: the rows come in groups of row_div that attend to the SAME features - P, V, q2 and row_ids hold one
     * entry per group (`rows / row_div` of them: the n captions drawn for one image share its regions) and row b reads
     * entry b / row_div; q, out, alpha_out and the planes stay per row.  One workgroup then serves up to 8 rows of a
     * group from ONE pass over the group's P and V rows (attn_scan_group_kernel), with per row the arithmetic - and the
     * bits - of the plain launch on the expanded tensors.  rows % row_div == 0; 0 or 1 = the plain launch. */
    int32_t row_div, _pad;
} isc_scan_problem;

int isc_attn_scan_fwd(const isc_scan_problem *probs_host, int n_prob, int B, void *stream);

/* Both scans, the gate sum and the gate mix of one decode step (captioner.py:96-118) in ONE launch (few rows, inference):
 * G[i] holds the rows of scan i's V carried through the gate's projection - G[0][b,r,:] = cont2att.weight V_c[b,r,:],
 * G[1] = senti2att.weight V_s rows (a table indexed by scan[1].row_ids in gather mode), no bias - so that
 *   z = zh + (b_gc + sum_r alpha_r G[0][b,r,:]) + (b_gs + sum_m alpha'_m G[1][.,:]) = h2att(h) + cont2att(v) + senti2att(s),
 *   beta = sigmoid(w_gate . tanh(z) + *b_gate),  f = beta v + (1 - beta) s
 * come out of the scan's own attention weights: the step's gate GEMM and gate-mix launches disappear, for R x A more
 * floats streamed per row (why the host uses it for few rows only).  scan[0] = content, scan[1] = sentiment words; their
 * .out / planes are optional here (v and s are only needed through f); A == D <= 1024 for both; zh [B,A] is the h-term
 * incl. its bias.  alpha outputs as in isc_attn_scan_fwd.
 * scan[i].row_div is honoured per scan, independently: the rows of a group of scan[0].row_div rows share ONE entry of the
 * content scan's P / V / G[0]; the rows of a group of scan[1].row_div rows share one entry of the sentiment scan's q2,
 * row_ids and per-row P / V / G[1] (one image captioned under several sentiment labels: isc_step_plan.senti_div).
 * B % row_div == 0, else ISC_E_SHAPE with nothing launched.  q, zh, f, beta and the alphas stay per row. */
typedef struct {
    isc_scan_problem scan[2];
    const float *G[2];
    const float *zh;
    const float *b_gc, *b_gs;     /* [A] biases of cont2att / senti2att */
    const float *w_gate;          /* [A] attention.att_alpha.weight */
    const float *b_gate;          /* device scalar or NULL */
    float *f;                     /* [B,D] */
    void *f_hi, *f_lo;            /* optional planes of f */
    float *beta;                  /* optional, row stride beta_ld */
    int64_t beta_ld;
} isc_scan_gate_args;
int isc_attn_scan_gate_fwd(const isc_scan_gate_args *args_host, int B, void *stream);

/* Gate fusion (captioner.py:111-117): beta = sigmoid(w . tanh(z[b,:]) + *w_bias);
 * out = beta*v + (1-beta)*s.  z = cont2att(v)+senti2att(s)+h2att(h) from isc_linear_fwd. */
int isc_gate_mix_fwd(const float *z, const float *w, const float *w_bias, const float *v,
                     const float *s, int B, int A, int D, float *out, float *beta_out,
                     int64_t beta_ld, void *out_hi, void *out_lo, void *stream);   /* out_hi/lo: optional planes of out */

/* xt[b,:] = relu(Emb[ids[b]]) (+ add[b,:])   (captioner.py:170-172), ids int64.  W % 4 == 0; emb, out and (when given)
 * add are moved as 16-byte vectors: a pointer that is not 16-byte aligned -> ISC_E_ALIGN before any launch. */
int isc_embed_relu_fwd(const float *emb, int V, int W, const int64_t *ids, int64_t ids_stride,
                       const float *add, int B, float *out, void *stream);

/* out[b,:] = mean_c relu(Emb[ids[b,c]])   (captioner.py:201-202) */
int isc_embed_relu_mean_fwd(const float *emb, int V, int W, const int64_t *ids, int C, int B,
                            float *out, void *stream);

/* out[b,m,:] = relu(Emb[m==0 ? pad_id : ids[b,m-1]]) [* mask*scale]  (captioner.py:307-311) */
int isc_embed_senti_words_fwd(const float *emb, int V, int W, const int64_t *ids, int n_words,
                              int64_t pad_id, int B, const uint8_t *keep_mask, float mask_scale,
                              float *out, void *stream);

/* Device-side state of one roll-out (forward_rl, captioner.py:317-344): no host sync per
 * step; `alive` is a [T+1] int32 counter array (alive[t] = #unfinished rows before step t,
 * alive[0] preset to B) that reproduces the reference's early `break`. */
typedef struct {
    int32_t B, V, T, t;          /* t = current step */
    int32_t n_tile, W;           /* vocab tiles, word-emb dim */
    const float *part_max, *part_sum;
    const int32_t *part_idx;
    const float *logits;         /* [B,V] row stride ld_logits; needed iff forced != null or sample_u != null */
    int64_t ld_logits;
    const int64_t *forced;       /* optional [B,T] tokens to replay instead of argmax */
    const float *sample_u;       /* optional [B,T] uniforms for inverse-CDF sampling */
    int64_t eos_id;
    int64_t *seq;                /* [B,T] */
    float *seq_logprobs;         /* [B,T] */
    float *seq_masks;            /* [B,T] */
    int32_t *unfinished;         /* [B] */
    int32_t *alive;              /* [T+1] */
    int64_t *raw_tokens;         /* optional [B,T]: token before the `* unfinished` masking */
    const float *emb;            /* word embedding [V,W] */
    const float *xt_add;         /* optional [B,W] sentiment-label embedding */
    float *xt_next;              /* [B,W] input of step t+1 */
} isc_rollout_step;

/* W % 4 == 0.  With xt_next set, emb, xt_next and (when given) xt_add are moved as 16-byte vectors: one of them not
 * 16-byte aligned -> ISC_E_ALIGN before any launch (without xt_next none of the three is read). */
int isc_rollout_finalize(const isc_rollout_step *s_host, void *stream);
long long isc_rollout_finalize_launches(void);   /* launches so far (tests: isc_rows_ext.fin_prev saves them) */

/* Controlled sampling of the sampled roll-out: temperature, top-k, nucleus (top-p).  Per row, tokens are ranked by raw
 * logit (largest first, ties to the smaller id), mass w_i = exp((x_i - x_max) / temperature); top-k keeps the first k
 * ranks (0 or >= V: off); top-p, applied to the survivors with summed mass W_k, keeps rank j iff the mass of the ranks
 * in front of it is < top_p * W_k (rank 0 always; >= 1: off); the draw is the inverse CDF over the kept set in
 * vocabulary order against sample_u * (kept mass).  seq_logprobs stays the MODEL's log_softmax(x)[token];
 * sampling_logprobs (optional, [B,T]) receives log(w_token / kept mass).  Everything else - seq, seq_masks, <EOS>, the
 * `alive` counters, raw_tokens, xt_next - as isc_rollout_finalize with sample_u (required here, as are the logits;
 * `forced` must be null).  One launch, no host read; integer (fixed-point) mass sums: bit-repeatable.
 * temperature must be finite and > 0, top_k >= 0, top_p > 0: otherwise ISC_E_SHAPE before any launch.  With xt_next set,
 * emb / xt_next / xt_add not 16-byte aligned -> ISC_E_ALIGN before any launch, as isc_rollout_finalize. */
typedef struct {
    float temperature;
    int32_t top_k;
    float top_p;
    float *sampling_logprobs;
} isc_sample_filter;
int isc_rollout_finalize_filtered(const isc_rollout_step *s_host, const isc_sample_filter *f_host, void *stream);

/* Token constraints of the roll-out - the beam search's rules (captioner.py:394-399) carried to it.  At step t a live
 * row may not choose: one of ban_ids[0 .. n_ban) (the caller's <PAD>, <SOS>, <UNK>); under no_repeat the token fed into
 * the step - seq[b, t-1], first_id (<SOS>) at t = 0; eos_id while t < min_len.  Duplicated ids are legal (<SOS> may equal
 * <PAD>, the previous token may be a banned special).  f NULL: isc_rollout_finalize's choice over the allowed ids -
 * arg-max with ties to the smaller id, or the inverse CDF in vocabulary order against sample_u * (allowed mass); the
 * 128-column tiles that hold a banned id (at most n_ban + 2 per row) are re-read and their statistics recomputed over
 * the allowed columns, nothing is subtracted from the row sum.  f given: isc_rollout_finalize_filtered's choice with the
 * banned ids out of the ranking, the histograms, the kept mass and the draw (ban, then temperature, top-k, top-p; masses
 * relative to the largest ALLOWED logit; integer sums, bit-repeatable).  seq_logprobs stays the MODEL's
 * log_softmax(x)[token] over the full row, sampling_logprobs is taken under the restricted distribution; finished rows,
 * the `alive` counters, raw_tokens and xt_next as without constraints.  A step at which nothing is banned (an all-zero
 * struct; min_len alone once t >= min_len) is served by the two entry points above, bit for bit.
 * Before any launch: a null struct -> ISC_E_NULL; n_ban outside [0, 8], an id outside [0, V), min_len outside [0, T],
 * `forced` together with any constraint, V <= n_ban + 2 (no allowed id left), n_tile != ceil(V / 128) -> ISC_E_SHAPE;
 * logits missing (every constrained form reads them) -> ISC_E_NULL; with xt_next set, emb / xt_next / xt_add not 16-byte
 * aligned -> ISC_E_ALIGN, as isc_rollout_finalize. */
typedef struct {
    int64_t ban_ids[8];
    int32_t n_ban;
    int32_t no_repeat;
    int64_t first_id;
    int32_t min_len;
} isc_decode_constraints;
int isc_rollout_finalize_constrained(const isc_rollout_step *s_host, const isc_sample_filter *f_host /* may be NULL */,
                                     const isc_decode_constraints *c_host, void *stream);

/* isc_rollout_finalize_filtered (c NULL) or isc_rollout_finalize_constrained with f given - the same kernels, the same
 * choice, the same outputs bit for bit - that additionally keeps, per (b, t) of a step that runs, what the backward of
 * sampling_logprobs reads (isc_logsoftmax_bwd_raw_filtered): kstar = the boundary rank key K* (the kept set is
 * { key <= K* } minus the banned ids), gmax = the largest allowed logit, logz = log(kept mass) (the term of
 * sampling_logprobs), ban (optional, [B,T,10]) = the row's banned ids at a constrained step, -1 for unused slots.  A step
 * behind the early break (alive[t] == 0) and an unconstrained step's ban entries are not written: the caller zero-fills
 * kstar / gmax / logz (and sampling_logprobs) and fills ban with -1 up front.  s, f, sv or one of kstar / gmax / logz
 * NULL -> ISC_E_NULL; everything else as the entry it forwards to. */
typedef struct {
    int64_t *kstar;              /* [B,T] */
    float *gmax;                 /* [B,T] */
    float *logz;                 /* [B,T] */
    int32_t *ban;                /* optional [B,T,10] */
} isc_filter_saved;
int isc_rollout_finalize_saved(const isc_rollout_step *s_host, const isc_sample_filter *f_host,
                               const isc_decode_constraints *c_host /* may be NULL */, const isc_filter_saved *sv_host,
                               void *stream);

/* Scheduled sampling of the teacher-forced unrolls (captioner.py:219-228): out_ids[b] = u_select[b] < ss_prob
 * ? a draw from exp(logp[b,:]) (inverse CDF with uniform u_draw[b], vocabulary order) : base_ids[b*stride].
 * logp = the previous step's normalised output, part_* = that step's tile statistics from isc_vocab_fwd. */
int isc_sched_sample(const float *logp, int64_t ld, int M, int V, const float *part_max,
                     const float *part_sum, const int32_t *part_idx, const float *u_select,
                     const float *u_draw, float ss_prob, const int64_t *base_ids, int64_t base_stride,
                     int64_t *out_ids, void *stream);
/* The same draw from the row's RAW logits (the statistics describe them: exp(x - max) against the tile masses, as
 * isc_rollout_finalize draws): an unroll with scheduled sampling then normalises its logits once, after its last step
 * (isc_logsoftmax_apply_steps), instead of once per step. */
int isc_sched_sample_raw(const float *logits, int64_t ld, int M, int V, const float *part_max,
                     const float *part_sum, const int32_t *part_idx, const float *u_select,
                     const float *u_draw, float ss_prob, const int64_t *base_ids, int64_t base_stride,
                     int64_t *out_ids, void *stream);

/* Beam step (sample(), captioner.py:390-409), batched over images: for every live beam row
 * apply the -inf masks (PAD,SOS,UNK, last word), take its top-`beam` (value, id) pairs
 * from logp = logits - lse (descending, ties to the smaller word id).  The candidate merge with the reference's
 * stable ordering and fp64 score sums is isc_beam_merge below (or the host mirror's Python / numpy forms). */
int isc_beam_topk(const float *logits, int64_t ld_logits, const float *part_max,
                  const float *part_sum, int n_tile, int rows, int V, int beam,
                  const int64_t *last_word, int64_t pad_id, int64_t sos_id, int64_t unk_id,
                  int mask_special, int decoding_constraint, float *top_val, int64_t *top_idx,
                  void *stream);
/* isc_beam_topk with a per-row list of further banned ids (isc_beam_ngram_ban's output): row r also masks
 * ban_ids[r * ban_ld + 0 .. min(ban_cnt[r], 256)) to -inf - for the top-`beam` only, the log-softmax normaliser stays
 * that of the whole row.  Both kernels of isc_beam_topk take the list (the tile-selecting one admits ban_cnt[r] more
 * tiles).  Duplicates and ids outside [0, V) are harmless.  ban_ids / ban_cnt NULL -> ISC_E_NULL, ban_ld < 1 ->
 * ISC_E_SHAPE, V <= 4 + beam (the masks could leave fewer than `beam` words) is the caller's to exclude. */
int isc_beam_topk_banned(const float *logits, int64_t ld_logits, const float *part_max,
                         const float *part_sum, int n_tile, int rows, int V, int beam,
                         const int64_t *last_word, int64_t pad_id, int64_t sos_id, int64_t unk_id,
                         int mask_special, int decoding_constraint, const int64_t *ban_ids, const int32_t *ban_cnt,
                         int64_t ban_ld, float *top_val, int64_t *top_idx, void *stream);

/* Ban lists of a beam step (no reference counterpart: its only token rule is decoding_constraint, captioner.py:394-399):
 * no n-gram twice in a caption, no <EOS> before min_len words.  Row r holds a candidate with the generated words
 * w = words[r, 0 .. L), L = min(len[r], t) (a live candidate has L == t at step t; <SOS> is not among them).  With
 * n = no_repeat_ngram >= 1 and L >= n - 1, pre = w[L - n + 1 .. L) (empty for n = 1): for every position j in [n - 1, L)
 * with w[j - n + 1 .. j) == pre, ascending, w[j] is appended to the row's list (duplicates kept); then eos_id when
 * t < min_len.  ban_cnt[r] = entries written (at most T).  One wave64 per row: lanes test 64 positions at a time, a ballot
 * and a prefix population count place the matches in order - no atomics, no LDS, bit-repeatable, capturable.
 * The list of step t is built from the tables the merge / select of step t - 1 wrote (t = 0: the empty tables) and is
 * read by isc_rows_step_banned_fwd / isc_beam_topk_banned at step t.  live_in (optional): reads 0 -> nothing is written.
 * Before any launch: a null struct or table -> ISC_E_NULL; rows < 1, T outside [1, 256], no_repeat_ngram outside [0, 4],
 * min_len outside [0, T], t outside [0, T), ban_ld < T -> ISC_E_SHAPE. */
typedef struct {
    int32_t rows, T, t;
    int32_t no_repeat_ngram, min_len, _pad;
    int64_t eos_id;
    const int64_t *words;     /* [rows, T] */
    const int32_t *len;       /* [rows] */
    int64_t *ban_ids;         /* [rows, ban_ld] */
    int32_t *ban_cnt;         /* [rows] */
    int64_t ban_ld;
    const int32_t *live_in;
} isc_beam_ngram_ban_args;
int isc_beam_ngram_ban(const isc_beam_ngram_ban_args *args_host, void *stream);

/* Candidate merge of a batched beam search on the device (captioner.py:378-411), one step: from the step's top-`beam`
 * (value, id) pairs per live row, form every image's candidates in the reference's insertion order (an ended
 * candidate carries itself, a live one contributes its `beam` children), add scores in fp64 (the reference sums
 * Python floats) and keep the first `beam` of a STABLE descending sort.  State (scores, last words, word lists,
 * lengths) is double-buffered by the caller; `gather` receives, per new row, its source row inside
 * [next-state rows ; current-state rows]; `done[i]` latches when every candidate of image i has ended (the image is
 * then frozen); live[t+1] counts the images still searching.  beam <= 8.  No host read is needed between steps. */
typedef struct {
    int32_t n_img, beam, T, t;
    int64_t eos_id;
    const float *top_val;     /* [n_img*beam, beam] log-probs of isc_beam_topk */
    const int64_t *top_idx;   /* [n_img*beam, beam] */
    const double *score_in;   /* [n_img*beam] */
    double *score_out;
    const int64_t *last_in;   /* [n_img*beam] last word of every candidate = the token fed to the next step */
    int64_t *last_out;
    const int64_t *words_in;  /* [n_img*beam, T] */
    int64_t *words_out;
    const int32_t *len_in;    /* [n_img*beam] */
    int32_t *len_out;
    int32_t *done;            /* [n_img] */
    int64_t *gather;          /* [n_img*beam] */
    int32_t *live;            /* [T+1] */
} isc_beam_merge_args;

int isc_beam_merge(const isc_beam_merge_args *args_host, void *stream);
/* Diverse beam search (Vijayakumar et al. 2016; no reference counterpart): isc_beam_merge with the search's `beam` rows
 * split into `groups` groups of B' = beam / groups ranks (group g owns ranks g B' .. (g + 1) B' - 1), handled in this
 * order.  Group g's candidates, in insertion order: its parents by rank, an ended one carried as ONE candidate, a live
 * one contributing its `beam` children in the row's top-`beam` order (at t == 0: the group's first row alone).  A
 * child's key is (s_parent + (double)logp) - lambda * (double)c, c = candidates selected AT THIS STEP by the groups in
 * front of g that appended the same token (carried ones appended nothing); a carried candidate's key is its score; one
 * fp64 add, one multiply, one subtract, never contracted.  The group keeps the first B' of a stable descending sort by
 * key; score_out holds the un-augmented sum.  done / live / gather as isc_beam_merge; new rows are group-major.
 * One wave64 per search, a loop over the groups, no atomics beyond the live counter: bit-repeatable.
 * groups < 1, beam % groups != 0, lambda negative or not finite -> ISC_E_SHAPE. */
int isc_beam_merge_groups(const isc_beam_merge_args *args_host, int groups, double lambda, void *stream);
/* State re-ordering of a beam step: out[p, r, :] = (gather[r] < rows ? state_next : state_cur)[p, gather[r] % rows, :]
 * for the `planes` [rows, H] planes of the recurrent state (h|c x layer), gather as written by isc_beam_merge. */
int isc_beam_gather(const float *state_next, const float *state_cur, const int64_t *gather, float *out,
                    int planes, int rows, int H, void *stream);

/* Up to ISC_COPY_MULTI_MAX device-to-device copies in ONE launch (dst[i] <- src[i], bytes[i] each; non-overlapping): the
 * input copies in front of a graph replay (features, word ids, labels into the graph's static buffers). */
#define ISC_COPY_MULTI_MAX 8
int isc_copy_multi(void *const *dst, const void *const *src, const int64_t *bytes, int n, void *stream);

/* Masked NLL (XECriterion, captioner.py:427-440): returns sum and token count in out[0..1].
 * logp [B,T,V] contiguous, target [B,T] int64, lengths [B] int32. */
int isc_xe_loss_fwd(const float *logp, const int64_t *target, const int32_t *lengths, int B,
                    int T, int V, float *out2, void *stream);

/* ------------------------------------------------------------------ whole decode step */

/* One forward_step (captioner.py:168-186) as ONE host call: enqueues the att-LSTM, the attention
 * projections (+ the h-term of the gate), the attention scan(s), the gate contraction + mix, the
 * lang-LSTM, the vocabulary projection and (optionally) the in-place log-softmax on `stream`.
 * It exists to take ~10 descriptor-building FFI calls per step off the host: at B <= 128 the step
 * is launch-bound.  Every pointer is a device pointer; nn.Linear weights are contiguous [out,in].
 * Branch selection like captioner.py:96-118: att_e == NULL -> sentiment words only (seq2seq),
 * words_e == NULL -> regions only (xe), both -> both + gate. */
typedef struct {
    int32_t rows, H, E, A, W, V, R, Mw;
    /* weights */
    const float *Wih1, *Whh1;           /* att_lstm.weight_ih [4H, H+E+W] (ld = H+E+W), weight_hh [4H,H] */
    const float *Wih2, *Whh2;           /* lang_lstm.weight_ih [4H, E+H], weight_hh */
    const float *b_ih2, *b_hh2;
    const float *W_h2att, *b_h2att, *w_alpha_c, *b_alpha_c;      /* attention.cont_att.* */
    const float *W_h2word, *b_h2word, *w_alpha_s, *b_alpha_s;    /* attention.senti_att.* */
    const float *W_gh, *b_gh, *W_gc, *b_gc, *W_gs, *b_gs, *w_gate, *b_gate; /* attention.{h2att,cont2att,senti2att,att_alpha} */
    const float *W_cls, *b_cls;
    /* step-invariant activations */
    const float *pre1;                  /* [rows,4H] hoisted fc/label/bias term of the att-LSTM */
    const float *tab;                   /* [V,4H] relu(Emb) W_x^T or NULL */
    const float *att_p, *att_e;         /* [rows,R,A], [rows,R,E] or NULL */
    const float *words_p, *words_e;     /* [rows,Mw,A], [rows,Mw,W] or NULL */
    const float *label_w;               /* [rows,A] or NULL */
    /* per step */
    const float *xt;                    /* [rows,W] relu(Emb[token]) (ignored when tab) */
    const int64_t *tok;                 /* token ids (row stride tok_stride), required iff tab */
    int64_t tok_stride;
    const float *h1_prev, *c1_prev, *h2_prev, *c2_prev;   /* [rows,H] */
    float *h1, *c1, *h2, *c2;
    float *g1, *g2;                     /* optional activated gates [rows,4H] (training) */
    float *qa, *v, *qw, *s, *z, *f;     /* [rows,A] / [rows,E] workspaces (branch-dependent) */
    float *alpha_c, *alpha_s, *beta;    /* optional attention-weight outputs */
    int64_t alpha_c_ld, alpha_s_ld, beta_ld;
    const uint8_t *out_mask;            /* dropout keep-mask on h_lang or NULL */
    float out_scale;
    int32_t apply_logsoftmax;           /* normalise `logits` in place after the projection */
    float *hdrop;                       /* [rows,H], required iff out_mask */
    float *logits;                      /* [rows,V] (row stride ld_logits) or NULL */
    int64_t ld_logits;
    float *pmax, *psum;                 /* [rows, ceil(V/128)] */
    int32_t *pidx;
    float *splitk_ws;                   /* optional split-K workspace shared by the step's launches */
    int64_t splitk_ws_floats;
    /* Optional f16 planes of the recurrent state (split-f16 path, see isc_seg.A_hi): [rows,H] each.  The *_prev
     * planes must hold the split of h1_prev / h2_prev (zeros for a zero state); the step writes the planes of h1 / h2
     * from the LSTM epilogues, so a roll-out that swaps (prev, next) every step never splits its state again.  All
     * eight or none. */
    const void *h1_prev_hi, *h1_prev_lo, *h2_prev_hi, *h2_prev_lo;
    void *h1_hi, *h1_lo, *h2_hi, *h2_lo;
    /* Optional plane workspace of the step's own intermediates v, s, f ([rows,E] f16 each; used with the state
     * planes): the scans and the gate write them, the gate sum and the lang-LSTM read them. */
    void *v_hi, *v_lo, *s_hi, *s_lo, *f_hi, *f_lo;
    /* Optional gather mode of the sentiment-word scan (isc_scan_problem.row_ids): words_p / words_e are then the
     * [V,A] / [V,W] tables and words_ids [rows, Mw] (row stride words_ids_ld) the word ids incl. the leading <PAD>. */
    const int64_t *words_ids;
    int64_t words_ids_ld;
    /* Optional (few rows, inference; both attentions): the scans' features through the gate's projection -
     * gate_Gc [rows,R,A] = cont2att.weight att_e rows, gate_Gs = senti2att.weight words_e rows ([rows,Mw,A], or the
     * [V,A] table in gather mode).  Both non-NULL: scans + gate sum + gate mix run as isc_attn_scan_gate_fwd. */
    const float *gate_Gc, *gate_Gs;
    /* Merged step of two sibling unrolls (train_xe.py:160-181: the XE unroll over image regions and the seq2seq unroll
     * over sentiment words share every LSTM / classifier weight, captioner.py:168-186).  pair_rows_c > 0: the first
     * pair_rows_c of the `rows` rows attend to the regions only (att_p / att_e / qa / v / alpha_c index them from 0), the
     * remaining rows to the sentiment words only (words_p / words_e / label_w / qw / s / alpha_s index THEM from 0), no
     * gate; s must equal v + pair_rows_c * E (one [rows,E] attended-feature block feeds the lang-LSTM).  Both LSTM cells
     * and the classifier then run once over all rows, the two h-projections as two problems of one launch and the two
     * scans as the two problems of one isc_attn_scan_fwd launch.  fp32 rows only (no state planes).  0 = off. */
    /* senti_div (with row_div > 1): inside an image the rows come in LABEL GROUPS of senti_div consecutive rows - the
     * beams of one (image, sentiment) search, when one image is captioned under several sentiment labels.  The
     * content-side tensors (att_p, att_e, gate_Gc) keep one entry per IMAGE, row r reads entry r / row_div; the
     * sentiment-side tensors (pre1, label_w, words_ids, per-row words_p / words_e, per-row gate_Gs) hold one entry per
     * label group, row r reads entry r / senti_div.  row_div % senti_div == 0; 0 = as row_div (one label per image);
     * 1 = a label per row.  Every output is, per row, bit for bit that of the plain step on the expanded tensors. */
    int32_t pair_rows_c, senti_div;
    /* row_div > 1: `rows` = images x row_div decode rows, row r belongs to image r / row_div (the captions drawn per
     * image by a sampled roll-out), and the step-invariant tensors of an image - pre1, att_p, att_e, label_w, words_ids
     * (per-row words_p / words_e as well) - hold one entry per IMAGE, as documented for isc_rows_ext.row_div.
     * isc_step_fwd hands it to the att-LSTM (isc_lstm_problem.pre_div) and to both scans (isc_scan_problem.row_div);
     * everything else of the step is per row as always.  rows % row_div == 0; not with pair_rows_c.  With the fused gate
     * scan (gate_Gc / gate_Gs) gate_Gc is per image as well.  isc_rows_step_fwd ignores it: the few-row step
     * takes isc_rows_ext.row_div.  0 or 1 = off.  A violated divisibility, or row_div > 1 without pre1
     * (the rule of isc_lstm_problem.pre_div), is ISC_E_SHAPE with nothing launched.
     * pre_rows != 0 (with row_div > 1, isc_step_fwd only): pre1 holds one row per decode ROW all the same - grouped
     * teacher-forced training, whose sentiment labels (part of the hoisted term) differ between an image's captions. */
    int32_t row_div, pre_rows;
} isc_step_plan;

int isc_step_fwd(const isc_step_plan *plan_host, void *stream);

/* Stream gate: the general kernels' form of isc_rows_ext.live_in.  While a gate is set for `stream`, the forward
 * launches enqueued on it - isc_linear_fwd, isc_lstm_fwd, isc_vocab_fwd (hence every launch of isc_step_fwd),
 * isc_attn_scan_fwd, isc_attn_scan_gate_fwd, isc_beam_topk - carry `flag` (a device int32) and return at once when it
 * reads 0 at RUN time.  A batched beam search (captioner.py:351-420 for many images at a time) gates step t by live[t]
 * of isc_beam_merge, the images still searching before it: the host looks at that counter only every fourth step
 * (graphs of four steps), and the up to three steps enqueued past the end of the search then cost their launches
 * instead of a full step each.  The small launches of a step (embedding gather, state re-order, merge) are not gated:
 * after the end they copy the finished images' rows along, as they always did.
 * Host state read at enqueue / capture time, per stream; flag == NULL clears it - do that as soon as the gated run of
 * launches is enqueued.  The reference has no counterpart (its loop breaks on the host, captioner.py:379-381). */
int isc_set_stream_gate(const int32_t *flag, void *stream);

/* ------------------------------------------------------------------ decode rows (at most 8 rows, inference)
 * The same forward_step (captioner.py:168-186) for the few-row regimes of the reference: the `beam_size` rows of one
 * image inside sample() (captioner.py:380-411, one batch-1 forward_step per live candidate there), a greedy roll-out
 * of a handful of captions (captioner.py:317-344).  Every contraction is then a few matrix-vector products that
 * stream the weights once and every launch is a few microseconds of dependent memory round trips; csrc/rows.hip holds
 * kernels built for that (weights straight to registers ahead of everything else, 16-lane-per-weight-row layout,
 * index chains in a wave of their own).  Five launches: att-LSTM, the three projections of h_att, the gated scan,
 * lang-LSTM, classifier.  The plan is isc_step_fwd's; this entry point requires both attentions with the
 * pre-projected gate rows (gate_Gc / gate_Gs), A == E == W <= 512, no saved gates, no dropout mask, no in-place
 * log-softmax (isc_rows_step_supported tells) and ignores the f16 plane pointers (nothing on this path reads planes).
 *
 * isc_rows_ext adds what the few-row callers fold into the step:
 *  - src_row: row r of h*_prev / c*_prev is read from row src_row[r] (the beam search's re-ordering of the recurrent
 *    state after each merge, captioner.py:405-409, as an index on the loads instead of a gather launch); NULL = r;
 *  - stats_tile: the column-tile width of pmax / psum / pidx ([rows, ceil(V / stats_tile)]; isc_rows_stats_tile(V):
 *    about V / 256 so that one round of workgroups covers the chip - NOT isc_vocab_fwd's 128);
 *  - beam > 0: per (row, tile) the 8 largest MASKED logits and their word ids, descending, ties to the smaller id
 *    (cand_val / cand_idx [rows, n_tile, 8]; masks as captioner.py:394-399: <PAD>, <SOS>, <UNK> when mask_special,
 *    the row's last word when decoding_constraint) - the input of isc_beam_select.
 *  - row_div > 1: the step-invariant tensors of the plan that belong to an IMAGE (pre1, att_p, att_e, gate_Gc, label_w,
 *    words_ids; per-row words_p / words_e / gate_Gs as well) hold one entry per image and row r uses entry r / row_div -
 *    the `beam` rows of an image share its regions (captioner.py:366-377 expands nothing either: it decodes candidate by
 *    candidate), so a search keeps one copy per image instead of `beam`; rows % row_div == 0;
 *  - senti_div (with row_div > 1): label groups of senti_div consecutive rows inside an image, as isc_step_plan.senti_div -
 *    att_p / att_e / gate_Gc stay per image, pre1 / label_w / words_ids / per-row words_p / words_e / gate_Gs are per label
 *    group and row r uses entry r / senti_div (one image searched under two labels: row_div = 2 * beam, senti_div = beam);
 *    row_div % senti_div == 0, else ISC_E_SHAPE with nothing launched; 0 = as row_div;
 *  - live_in: optional device int; when it reads 0 every launch of the step returns at once (and isc_beam_select with it):
 *    a search captured as ONE graph of T steps ends itself on the device (live[t] of isc_beam_select: images still
 *    searching before step t) instead of the host reading that counter between graphs of a few steps.
 * `logits` of the plan is optional here as well (row stride ld_logits). */
typedef struct {
    const int64_t *src_row;
    int32_t stats_tile, beam;
    float *cand_val;
    int32_t *cand_idx;
    const int64_t *last_word;     /* [rows] required iff decoding_constraint */
    int64_t pad_id, sos_id, unk_id;
    int32_t mask_special, decoding_constraint;
    int32_t row_div, senti_div;   /* senti_div: label groups inside an image, as isc_step_plan.senti_div (0 = as row_div) */
    const int32_t *live_in;
    /* optional: the PREVIOUS step's greedy roll-out finalize folded into this step's first launch (a roll-out of T steps is
     * then T finalize launches shorter but one: only the last step's runs on its own).  fin_prev describes that step as
     * isc_rollout_finalize would get it (t = the previous step; forced, sample_u and xt_next NULL: arg-max decoding with the
     * token table), except that its `unfinished` is only READ - the updated flags go to fin_unfinished_out ([rows], another
     * array: every workgroup of the launch reads the old flags) - and the plan's `tok` is ignored: the launch derives the
     * fed tokens from the previous step's tile statistics (still in pmax / psum / pidx when it runs).  Needs plan->tab,
     * row_div <= 1, no src_row, no live_in, at most 4 rows (measured: B = 1 0.70 -> 0.65 ms per roll-out, B = 4 0.76 ->
     * 0.74; at 8 rows the fold outlasts the launch it saves: 0.86 -> 0.90). */
    const isc_rollout_step *fin_prev;
    int32_t *fin_unfinished_out;
} isc_rows_ext;
/* A per-row list of further banned ids for the step's tile candidates (ext->beam > 0), as isc_beam_ngram_ban writes it: row
 * r's candidate mask also bans ids[r * ld + 0 .. cnt[r]) (duplicates and ids outside [0, V) are harmless).  Only cand_val /
 * cand_idx change: pmax / psum / pidx and `logits` are those of the launch without a list.  The first 8 entries of every
 * row are fetched ahead of the weight stream like the row's last word, a longer list is walked in the epilogue.  The list
 * travels next to isc_rows_ext, not inside it (that struct's size is pinned): isc_rows_step_banned_fwd /
 * isc_rows_vocab_banned_fwd are isc_rows_step_fwd / isc_rows_vocab_fwd with it; the entry points without it launch the
 * kernels without it, which are the kernels as they were.  A null list, ids or cnt -> ISC_E_NULL; ld < 1 or ext->beam <= 0 ->
 * ISC_E_SHAPE; nothing is launched then. */
typedef struct {
    const int64_t *ids;       /* [rows, ld] */
    const int32_t *cnt;       /* [rows] */
    int64_t ld;
} isc_rows_ban;
int isc_rows_stats_tile(int V);
int isc_rows_step_supported(const isc_step_plan *plan_host);
/* The same answer from a plan's integers alone, and the launches' own shape conditions one by one (the launch functions
 * take their geometry from the code behind these: a step isc_rows_step_supported accepts is a step all five launches
 * take).  Host arithmetic only: nothing is issued, no pointer is read.  1 = accepted.
 *  - isc_rows_vocab_supported: the classifier on M rows of width K over V columns at isc_rows_stats_tile(V);
 *  - isc_rows_lstm_supported: an LSTM cell of H units over up to three K-segments (0 = absent), each cut at 256;
 *  - isc_rows_linear_supported: the grouped projections of K inputs onto Ntot outputs in all. */
int isc_rows_shape_supported(int rows, int H, int E, int A, int W, int V, int R, int Mw, int has_tab);
int isc_rows_vocab_supported(int M, int V, int K);
int isc_rows_lstm_supported(int M, int H, int K0, int K1, int K2);
int isc_rows_linear_supported(int M, int K, int Ntot);
int isc_rows_step_fwd(const isc_step_plan *plan_host, const isc_rows_ext *ext_host, void *stream);
int isc_rows_step_banned_fwd(const isc_step_plan *plan_host, const isc_rows_ext *ext_host, const isc_rows_ban *ban_host,
                             void *stream);
/* The classifier launch of that step alone (tests, tools): statistics per stats_tile columns (+ tile candidates). */
int isc_rows_vocab_fwd(const float *h, int ldh, const float *W, int ldw, const float *bias, int M, int V, int K,
                       float *part_max, float *part_sum, int32_t *part_idx, float *logits, int64_t ld_logits,
                       const isc_rows_ext *ext_host, void *stream);
int isc_rows_vocab_banned_fwd(const float *h, int ldh, const float *W, int ldw, const float *bias, int M, int V, int K,
                              float *part_max, float *part_sum, int32_t *part_idx, float *logits, int64_t ld_logits,
                              const isc_rows_ext *ext_host, const isc_rows_ban *ban_host, void *stream);
/* Cache policy of the rows kernels' weight streams: 0 = default policy everywhere, 1 (default) = the classifier's weights
 * non-temporal (read once per step: they pass through without evicting the LSTM / projection weights that the XCD L2s
 * keep from step to step), 2 = every stream non-temporal.  Returns the previous value. */
int isc_set_rows_nt(int mode);
long long isc_rows_launches(void);    /* launches of rows kernels so far (tests assert the path was taken) */
/* Which instantiation the last launches took (tests assert the route of every launch they make).  Writes the most recent
 * min(n, 16, launches so far) records, oldest first, 8 ints each: kernel (0 = rows_lstm_kernel, 1 = rows_linear_kernel,
 * 2 = rows_scan_gate_kernel, 3 = rows_vocab_kernel), MR (0 for the scan), UPW (LSTM) / NP (classifier) / 1 when every
 * region is in flight at once (scan), NT, BAN, S, J, K-slices.  Returns the launches recorded so far; `out` may be
 * NULL.  Host bookkeeping: reading touches no device. */
long long isc_rows_routes(int32_t *out, int n);
/* isc_attn_scan_gate_fwd (and with it isc_step_fwd's gated scan) runs launches of up to this many rows on the rows scan
 * kernel - one 1024-thread workgroup per row, the row's rows of P / V / G in flight at once - when the shape is its own
 * (v / s not wanted on their own, R <= isc_set_rows_scan_regions, Mw <= 12, A = D <= 512); default 256, 0 = never (attn_scan_gate_kernel walks
 * the regions).  rows < 0 only queries.  Returns the previous value. */
int isc_set_rows_scan_max(int rows);
/* ... and up to this many content regions (default 256; up to 36 all of a row's regions are in flight at once, larger
 * grids - the reference encoder's 14 x 14 = 196 - are walked 36 regions at a time by the same kernel).  regions < 0
 * only queries.  Returns the previous value. */
int isc_set_rows_scan_regions(int regions);
/* Vocabulary launches of the skinny split-f16 path (isc_vocab_fwd / isc_step_fwd at a few hundred rows, one activation
 * segment): 1 (default) = gemm_h3v_kernel (k-block stages shared by the workgroup: the activation block fetched once, two
 * blocks in flight; taken up to 512 workgroups), 0 = the per-wave-ring gemm_h3s_kernel form it replaced (tests, A/B runs),
 * n > 1 = on, taken up to n workgroups (tuning).  Returns the previous value. */
int isc_set_h3v(int on);
/* Long contractions on few large split-f16 tiles (one linear problem of < ~200 128 x 128 tiles and >= 64 k-blocks - the
 * classifier's dX over all T x B rows of a training iteration): the k-blocks are cut into up to 8 slices per tile so that
 * the launch fills the chip, partial tiles go to slabs in the caller's workspace and the split-K reduce kernel sums them
 * in fixed order and applies the epilogue (deterministic).  1 (default) = for isc_gemm_bwd's NN launches (dX = dY W),
 * 2 = for forward launches as well (tests: a forward launch otherwise keeps one summation order at every batch size),
 * 0 = never.  Returns the previous value. */
int isc_set_h3_ksplit(int on);
/* Tile geometry of a vocabulary launch (isc_vocab_fwd / isc_step_fwd) once the large split-f16 kernels have it: 0
 * (default) = auto, which is the 128-row tile at every size (the 256-row tile the other epilogues take from 224 tiles on
 * measures 3-7 % slower at [16384 x 10000 x 512]: its statistics epilogue is not overlapped by a second workgroup),
 * 128 / 256 = that geometry at any tile count (tests, A/B runs).  A row's pmax / psum / pidx and logits are the same bits
 * under either geometry.  Any other value changes nothing.  Returns the previous value. */
int isc_set_h3_vocab_tile(int rows);

/* Top-k + candidate merge of one beam step in ONE launch (captioner.py:390-411), from the tile statistics and tile
 * candidates isc_rows_step_fwd left: per row the log-softmax normaliser is folded from (pmax, psum), the row's top-`beam`
 * (raw logit descending, ties to the smaller word id; log-prob = (x - max) - log(sum)) is merged out of its tiles'
 * sorted candidate lists, then the image's candidates are formed, scored in fp64 and stably ranked exactly as
 * isc_beam_merge does.  src_row[r] receives the PARENT row of new row r (usable as the next step's isc_rows_ext.src_row; an
 * ended candidate's state is never read again, captioner.py:383-385, so carried rows point at their parent's state as well);
 * top_val / top_idx (optional, [n_img*beam, beam]) receive the rows' top-k for inspection. */
typedef struct {
    int32_t n_img, beam, T, t;
    int32_t n_tile, V;
    int64_t eos_id;
    const float *part_max, *part_sum;     /* [n_img*beam, n_tile] */
    const float *cand_val;                /* [n_img*beam, n_tile, 8] */
    const int32_t *cand_idx;
    const double *score_in;
    double *score_out;
    const int64_t *last_in;
    int64_t *last_out;
    const int64_t *words_in;
    int64_t *words_out;
    const int32_t *len_in;
    int32_t *len_out;
    int32_t *done;
    int64_t *src_row;
    int32_t *live;
    float *top_val;
    int64_t *top_idx;
    const int32_t *live_in;               /* optional: reads 0 -> the launch returns at once (see isc_rows_ext.live_in) */
    /* optional: the recurrent state re-ordered here as well (what isc_beam_gather does in a launch of its own):
     * state_out[p, r, :] = state_in[p, parent(r), :] for the state_planes [n_img*beam, H] planes (h | c x layer) the
     * step has just written; the next step then reads plain rows (no isc_rows_ext.src_row: its kernels stage their
     * activations without a dependent index load in front).  state_out must not alias state_in; H % 4 == 0. */
    const float *state_in;
    float *state_out;
    int32_t state_planes, H;
} isc_beam_select_args;
int isc_beam_select(const isc_beam_select_args *args_host, void *stream);
/* isc_beam_select under isc_beam_merge_groups' rule: the same launch (tile-list merges, side waves, state re-ordering),
 * its rank phase a chain of `groups` rounds - round g ranks group g's candidates by their keys, eight lanes per
 * candidate, and leaves its B' winners' tokens in LDS for the rounds behind it.  groups == 1 (the plain search for any
 * lambda) launches isc_beam_select's kernel.  Same refusals as isc_beam_select, and
 * ISC_E_SHAPE for groups < 1, beam % groups != 0, lambda negative or not finite. */
int isc_beam_select_groups(const isc_beam_select_args *args_host, int groups, double lambda, void *stream);

/* Reverse-sweep counterpart (one BPTT step, see autograd.py): lang-LSTM cell backward, input-gradient
 * contractions, gate / scan backward, att-LSTM cell backward, recurrent gradients for step t-1.
 * `first` = last time step (no incoming recurrent gradients), `last` = step 0 (no outgoing ones). */
typedef struct {
    int32_t rows, H, E, A, W, R, Mw, first, last;
    int32_t pair_rows_c;                /* > 0: the merged step of isc_step_plan.pair_rows_c - rows [0, pair_rows_c) carry the
                                           content scan, the rest the sentiment scan; d_feat is one [rows,E] block, dqa / de_c /
                                           dwc_rows index the content rows from 0, dqw / de_s / dws_rows the sentiment rows */
    const float *Wih1, *Whh1, *Wih2, *Whh2;
    const float *W_h2att, *w_alpha_c, *W_h2word, *w_alpha_s, *W_gh, *W_gc, *W_gs, *w_gate;
    const float *att_p, *att_e, *words_p, *words_e, *label_w;
    /* saved activations of this step */
    const float *g1, *c1_prev, *c1, *g2, *c2_prev, *c2;
    const float *qa, *qw, *v, *s, *z;
    const float *alpha_c, *alpha_s, *beta;
    int64_t alpha_c_ld, alpha_s_ld, beta_ld;
    /* gradients */
    const float *dhd;                   /* [rows,H] d loss / d h_lang of this step (classifier path) */
    float *dG1, *dG2;                   /* [rows,4H] this step's slices of the time-stacked buffers */
    float *dG1_sum;                     /* [rows,4H] running sum over time */
    float *d_feat, *dh1, *dv, *ds;      /* [rows,E] / [rows,H] scratch */
    float *dh2_rec, *dh1_rec;           /* recurrent gradients (in: from t+1, out: for t-1) */
    const float *dc1_in, *dc2_in;       /* cell-state gradients from t+1 (ignored when first) */
    float *dc1_out, *dc2_out;
    float *dqa, *dqw, *dz;              /* [rows,A] this step's slices */
    float *dP_att, *dV_att, *dP_w, *dV_w;       /* accumulated over time */
    float *dwc_rows, *dws_rows, *dwg_rows, *dbg_rows;
    float *splitk_ws;                   /* optional split-K workspace */
    int64_t splitk_ws_floats;
    float *de_c, *de_s;                 /* optional [rows,R] / [rows,Mw]: this step's d e of the two scans (isc_scan_bwd_problem.de_out);
                                           dP_att / dP_w and dV_att / dV_w may then be NULL (isc_attn_dp_from_de, _dv_from_alpha) */
    int32_t row_div, _pad;              /* > 1: rows = images x row_div (isc_step_plan.row_div): att_p / att_e, words_p /
                                           words_e and label_w hold one entry per IMAGE - handed to both scans
                                           (isc_scan_bwd_problem.row_div: dP_* / dV_* must be NULL); everything else is
                                           per row.  rows % row_div == 0, not with pair_rows_c.  0 or 1 = off */
} isc_step_bwd_plan;

int isc_step_bwd(const isc_step_bwd_plan *plan_host, void *stream);

/* ------------------------------------------------------------------ backward (BPTT) */

/* d logits = d logp - softmax * rowsum(d logp)  (autograd of F.log_softmax, captioner.py:183).
 * Output rows have stride ld_out >= V; the padding columns are zero-filled. remap_T > 0
 * writes input row (b,t) = b*T+t to output row t*B+b (time-major copy for the BPTT sweep). */
int isc_logsoftmax_bwd(const float *dlogp, const float *logp, int64_t ld_in, int M, int V,
                       float *dlogits, int64_t ld_out, int remap_T, void *stream);

/* Pointwise part of the LSTMCell backward (captioner.py:175,181): from d h (= dh + dh2),
 * d c_next and the saved activated gates produces d(pre-activation gates) [M,4H] and d c_prev.
 * dgates_sum (optional) += dgates: the step-invariant fc / label inputs of the att-LSTM only
 * need the sum over time. */
int isc_lstm_bwd(const float *dh, const float *dh2, const float *dc_next, const float *gates,
                 const float *c_prev, const float *c, int M, int H, float *dgates, float *dc_prev,
                 float *dgates_sum, void *stream);

/* Backward of isc_attn_scan_fwd for one step. dP / dV / dw_rows accumulate over time steps when
 * `accumulate` is set (first processed step writes). dq [B,A] is also the gradient of q2.
 * dw_rows [B,A]: per-row partial of d w (column-summed once after the loop; deterministic). */
typedef struct {
    const float *P, *V, *q, *q2, *w, *alpha, *dout;
    int64_t alpha_ld;
    int32_t R, A, D, accumulate;
    float *dP, *dV, *dq, *dw_rows;
    float *de_out;            /* optional [B,R]: this step's d e (softmax backward); required when dP is NULL */
    int32_t rows;             /* rows of THIS problem; 0 = the launch's B (see isc_scan_problem.rows) */
    /* row_div > 1: the rows come in groups of row_div that attended to the SAME features (isc_scan_problem.row_div):
     * P, V and q2 hold one entry per group and row b reads entry b / row_div; q, alpha, dout, dq, dw_rows and de_out
     * stay per row - the per-row arithmetic, and the bits, of the plain launch on the expanded tensors.  dP and dV must
     * then be NULL (row_div workgroups would read-modify-write one image's entry: ISC_E_SHAPE) - they are formed after
     * the sweep by isc_attn_dp_from_de_group / isc_attn_dv_from_alpha_group.  rows % row_div == 0; 0 or 1 = per row. */
    int32_t row_div;
} isc_scan_bwd_problem;

int isc_attn_scan_bwd(const isc_scan_bwd_problem *probs_host, int n_prob, int B, void *stream);
/* dV may be NULL in a problem above: the caller then forms dV once after its sweep from the per-step gradients,
 * dV[b,r,:] = sum_{t = T-1 .. 0} alpha[b*alpha_ld_b + t*alpha_ld_t + r] * dout[(t*B + b)*D + :] (the sweep's order of
 * additions: bit-identical to the per-step accumulation), instead of re-reading and re-writing [B,R,D] at every step. */
int isc_attn_dv_from_alpha(const float *alpha, int64_t alpha_ld_b, int64_t alpha_ld_t, const float *dout,
                           int B, int T, int R, int D, float *dV, int dout_step_rows, void *stream);
/* dout_step_rows (0 = B): rows per step of `dout` - dout row (t, b) at t*dout_step_rows + b (merged unroll, as above). */
/* dP may be NULL as well (with de_out given): dP[b,r,a] = sum_{t = T-1 .. 0} de[(t*B + b)*R + r] * w[a] *
 * (1 - tanh^2(P[b,r,a] + q[(t*B + b)*A + a] (+ q2[b*A + a]))) is then formed once after the sweep - P read once, the
 * tanh terms recomputed; same expression and order of additions as the per-step accumulation.  Any R (the grid walks
 * region chunks: the reference encoder's 14 x 14 = 196 regions are six chunks at A = 512), any A, D with A % 4 == D % 4 == 0. */
int isc_attn_dp_from_de(const float *P, const float *q, const float *q2, const float *w, const float *de,
                        int B, int T, int R, int A, float *dP, void *stream);
/* The two reductions over the rows of an IMAGE (isc_scan_bwd_problem.row_div = group): the B decode rows are B / group
 * images x group rows, row i*group + j = row j of image i; alpha, dout, q and de stay per row, P, q2, dV and dP hold one
 * entry per image:
 *   dV[i,r,:] = sum_j sum_t alpha[(i*group + j)*alpha_ld_b + t*alpha_ld_t + r] * dout[(t*dout_step_rows + i*group + j)*D + :]
 *   dP[i,r,a] = sum_j sum_t de[(t*B + i*group + j)*R + r] * w[a] * (1 - tanh^2(P[i,r,a] + q[(t*B + i*group + j)*A + a] (+ q2[i*A + a])))
 * added in ONE fixed order - j ascending outermost, t = T-1 down to 0 inside - by one thread per output element (no
 * atomics: two runs give the same bits).  group == 1 is isc_attn_dv_from_alpha / isc_attn_dp_from_de, which forward
 * here: same kernels, same bits.  The LDS image of alpha / de is [group*T][regions of a chunk]: group*T beyond the 15000
 * rows that 60000 bytes hold for one region, or B % group != 0: ISC_E_SHAPE. */
int isc_attn_dv_from_alpha_group(const float *alpha, int64_t alpha_ld_b, int64_t alpha_ld_t, const float *dout,
                                 int B, int group, int T, int R, int D, float *dV, int dout_step_rows, void *stream);
int isc_attn_dp_from_de_group(const float *P, const float *q, const float *q2, const float *w, const float *de,
                              int B, int group, int T, int R, int A, float *dP, void *stream);

/* Backward of isc_gate_mix_fwd: dv = beta*dfeat, ds = (1-beta)*dfeat, dz, per-row partials of
 * d w (dw_rows [B,A]) and d w_bias (db_rows [B]). */
int isc_gate_mix_bwd(const float *z, const float *w, const float *v, const float *s, const float *beta,
                     int64_t beta_ld, const float *dfeat, int B, int A, int D, float *dv, float *ds,
                     float *dz, float *dw_rows, float *db_rows, int accumulate, void *stream);

/* Embedding + ReLU backward: demb[id(r),:] += scale * dout[r / rows_per_grad,:] * (emb[id(r),:] > 0)
 * [* mask]. pad_first = n_words+1 selects the sentiment-word layout (row 0 of every image = <PAD>).
 * Deterministic (no floating-point atomics): the positions of one id are summed in ascending order by the
 * workgroup of its first occurrence.  Rows with id == skip_id are left untouched (nn.Embedding's
 * padding_idx row, whose gradient the caller discards; -1 = none).  W <= 1024. */
int isc_embed_relu_bwd(const float *emb, int V, int W, const int64_t *ids, int64_t ids_stride,
                       int n_rows, int rows_per_grad, int pad_first, int64_t pad_id, const float *dout,
                       float scale, const uint8_t *keep_mask, float mask_scale, float *demb,
                       int64_t skip_id, void *stream);
/* The same gradient, bit for bit, through a position index built in `workspace` (>= (4 V + 64 + n_rows) * 4 bytes,
 * 16-byte aligned): count per id, offsets, every position dropped into its id's segment, one workgroup per
 * occurring id that sorts its segment and sums in ascending position order.  Linear in n_rows where the entry
 * point above is quadratic (each workgroup scans the id array); falls back to it without a workspace or below
 * 1024 positions. */
int isc_embed_relu_bwd_ws(const float *emb, int V, int W, const int64_t *ids, int64_t ids_stride,
                          int n_rows, int rows_per_grad, int pad_first, int64_t pad_id,
                          const float *dout, float scale, const uint8_t *keep_mask, float mask_scale,
                          float *demb, int64_t skip_id, void *workspace, int64_t workspace_bytes, void *stream);

/* out[n] (+)= sum_m x[m,n]  (bias gradients). With a workspace of >= 64*N floats tall matrices are
 * summed in two deterministic stages (row chunks in parallel, then the chunks in order). */
int isc_colsum(const float *x, int64_t ld, int M, int N, float *out, int accumulate, float *workspace,
               int64_t workspace_floats, void *stream);

/* Several column sums in at most two launches (the bias gradients of one backward sweep): job i sums x_i [M_i, N_i]
 * over its rows into each of its n_out outputs (tied biases share one reduction), or adds to them (accumulate).
 * Fixed order, deterministic.  workspace: sum over jobs with M >= 256 of ceil-chunks * N floats (<= 64 N each). */
#define ISC_COLSUM_MAX_JOBS 24
#define ISC_COLSUM_MAX_OUT 3
typedef struct {
    const float *x;
    int64_t ld;
    int32_t M, N;
    float *out[ISC_COLSUM_MAX_OUT];
    int32_t n_out, accumulate;
} isc_colsum_job;
int isc_colsum_multi(const isc_colsum_job *jobs_host, int n_jobs, float *workspace, int64_t workspace_floats,
                     void *stream);

/* dz = dy * (y > 0) [* mask * scale]  (ReLU + Dropout backward of the prologue layers);
 * y == NULL skips the ReLU test (pure nn.Dropout backward, captioner.py:182). */
int isc_relu_mask_bwd(const float *dy, const float *y, const uint8_t *keep_mask, float scale, int64_t n,
                      float *dz, void *stream);

/* XECriterion backward: dlogp (pre-zeroed [B,T,V]) gets -gout/count at every unmasked target;
 * sum_count = the two floats written by isc_xe_loss_fwd. */
int isc_xe_loss_bwd(const int64_t *target, const int32_t *lengths, int B, int T, int V,
                    const float *gout, const float *sum_count, float *dlogp, void *stream);

/* XECriterion backward in the sparse form isc_logsoftmax_bwd_sparse takes: coef [B,T] = -gout/count at unmasked
 * tokens and 0 elsewhere (the column of row (b,t) is target[b,t] itself) - no [B,T,V] tensor. */
int isc_xe_loss_bwd_sparse(const int32_t *lengths, int B, int T, const float *gout, const float *sum_count,
                           float *coef, void *stream);

/* RewardCriterion (self_critical/utils.py:169-177; called at models/decoder.py:160): the masked REINFORCE loss
 * -sum(logp * mask * reward) / sum(mask) over [B,T] fp32 tensors, one launch each way.
 * fwd: out2 = { sum(-logp*mask*reward), sum(mask) } (the caller divides: keeps sum and count for the backward and for
 * data-parallel normalisation).  bwd: d_seq_logprobs[b,t] = -gout[0] * mask * reward / sum_count[1]. */
int isc_reward_loss_fwd(const float *seq_logprobs, const float *seq_masks, const float *reward, int B, int T,
                        float *out2, void *stream);
int isc_reward_loss_bwd(const float *seq_masks, const float *reward, int B, int T, const float *gout,
                        const float *sum_count, float *d_seq_logprobs, void *stream);

/* Group reward of self-critical RL on n sampled captions per image (rows image-major: row r = i*n + j is sample j of
 * image i): a sample's baseline is the mean score of the image's OTHER n - 1 samples, so no greedy roll-out is needed.
 *   baseline[i,j] = (sum over k != j, k ascending, of scores[i,k]) / (n - 1)            fp64
 *   adv[i,j]      = scores[i,j] - baseline[i,j]                                         fp64
 *   reward[r,t]   = (float)(adv[r] + cls_flag * (double)cls_reward[r,t]) for every t    (unmasked: the criterion masks;
 *                   the product is rounded before the addition - no fused multiply-add); (float)adv[r] when
 *                   cls_reward == NULL
 *   stats4        = { mean of scores, mean of adv, mean of cls_reward over all I*n*T entries (0 when NULL), mean of the
 *                   stored reward floats }, accumulated in fp64
 * scores [I*n] fp64 (the host's CIDEr-D scores, uploaded as they are), cls_reward / reward [I*n, T] fp32 contiguous,
 * stats4 four doubles - all device memory.  Two launches, no atomics: one thread per (row, step) for the reward, then one
 * workgroup of 256 threads for the statistics - thread x adds its elements x, x + 256, ... ascending, the 256 partial sums
 * are added pairwise (stride 128, 64, ..., 1) - so two runs give the same bits.  The statistics pass is one workgroup
 * over I*n*T values: meant for training batches (thousands of rows), not for millions.
 * n < 2, I < 1 or T < 1: ISC_E_SHAPE, nothing is launched or written. */
int isc_group_reward(const double *scores, int I, int n, const float *cls_reward, double cls_flag, int T,
                     float *reward, double *stats4, void *stream);

/* CIDEr-D of N hypotheses on the device: scores[r] = what isc_cider_score (include/insenticap_cider.h) gives for row r -
 * the mean over the references of the row's image, x 10 - fp64 throughout.  All pointers are device memory.
 *   hyp [N, T] int64, contiguous: the raw roll-out rows (a leading sos_id is dropped, the row is cut at its first eos_id,
 *     eos_id is appended: L <= T + 1 words); row r belongs to image r / row_div (1: one row per image; n: the grouped
 *     roll-out's n rows per image).  Ids in [0, 65534] (csrc/cider_key.h: 16-bit key fields) - an id is never an index,
 *     so a larger one reads nothing out of bounds, it only aliases another id.
 *   table [capacity] 16-byte slots {uint64 key, double log(max(1, df))}, key 0 = empty, capacity a power of two, home
 *     slot isc_cider_hash(key) & (capacity - 1), linear probing (isc_cider_table_fill).  A lookup makes at most
 *     `capacity` probes: a table without an empty slot answers "absent", it cannot spin.
 *   the batch's cooked references (isc_cider_cook_fill) as CSR arrays: image i owns captions img_cap_off[i] ..
 *     img_cap_off[i + 1] (n_img + 1 entries, every image at least one caption - the caller's check, as the host scorer's
 *     -2), caption c owns the entries ord_off[5 c] .. ord_off[5 c + 4] of ref_keys / ref_vals (its k-grams of order o + 1
 *     start at ord_off[5 c + o]), ref_norms [4 c + o], ref_length [c].
 *   n, sigma, ref_len: isc_cider_params.
 * One wave64 per hypothesis, one lane per position, four hypotheses per workgroup; no workspace, no LDS, no atomics;
 * every sum runs in the host scorer's order (first-occurrence order within an order, references ascending), so two
 * launches give the same bits and only exp, sqrt and the division can differ from the host's.  One launch, no host
 * read: capturable.
 * N < 1, T outside [1, 63], row_div < 1, n outside [1, 4], a capacity that is no power of two >= 2, or fewer than
 * ceil(N / row_div) images: ISC_E_SHAPE, nothing is launched or written. */
int isc_cider_dev_score(const int64_t *hyp, int64_t N, int T, int row_div, const void *table, int64_t capacity,
                        const int32_t *img_cap_off, int64_t n_img, const int32_t *ord_off, const double *ref_norms,
                        const double *ref_length, const uint64_t *ref_keys, const double *ref_vals, int n, double sigma,
                        double ref_len, int64_t sos_id, int64_t eos_id, double *scores, void *stream);

/* BLEU of N hypotheses on the device: what isc_bleu_score (include/insenticap_cider.h) gives for row r - the integer
 * statistics exactly, the four scores in the order of operations of bleu_scorer.py:233-242, fp64 without contraction.
 * All pointers are device memory.
 *   hyp [N, T] int64, contiguous, normalised as isc_cider_dev_score normalises (L <= T + 1 words); row r belongs to image
 *     r / row_div.  Ids in [0, 65534]; an id is never an index, so a larger one reads nothing out of bounds.
 *   the batch's cooked references (isc_bleu_cook_fill, one image after the other): image i owns the entries
 *     img_ent_off[5 i] .. img_ent_off[5 i + 4] of ref_keys (csrc/cider_key.h keys) / ref_counts (the largest count of the
 *     n-gram in one of the image's references), its (o + 1)-grams start at img_ent_off[5 i + o]; and the captions
 *     img_cap_off[i] .. img_cap_off[i + 1] of ref_lens (words of each reference; n_img + 1 offsets, every image at least
 *     one caption - the caller's check).
 *   order 1..4: scores [N] = BLEU-order (4: the reference's reward, scores[3]); order 0: scores [N, 4].
 *   stats [N, 10] int32 = testlen, reflen, guess[0..3], correct[0..3], or NULL.
 * One wave64 per hypothesis, one lane per word, four hypotheses per workgroup; no workspace, no LDS, no atomics; the
 * statistics are integer sums, the float tail is wave-uniform: two launches give the same bits, and order k gives the
 * bits of column k - 1 of order 0.  One launch, no host read: capturable.
 * N < 1, T outside [1, 63], row_div < 1, order outside [0, 4], or fewer than ceil(N / row_div) images: ISC_E_SHAPE,
 * nothing is launched or written. */
int isc_bleu_dev_score(const int64_t *hyp, int64_t N, int T, int row_div, const int32_t *img_ent_off,
                       const uint64_t *ref_keys, const int32_t *ref_counts, const int32_t *img_cap_off,
                       const int32_t *ref_lens, int64_t n_img, int order, int64_t sos_id, int64_t eos_id, double *scores,
                       int32_t *stats, void *stream);

/* Back-off n-gram language models on the device: what isc_lm_score (include/insenticap_cider.h, where the model, the slot
 * and the walk are defined) gives for row r, in bits - only float32 -> float64 conversions and float64 additions in a
 * fixed order are involved.  All pointers are device memory.
 *   hyp [N, T] int64, contiguous, normalised as isc_cider_dev_score normalises; T <= 62 (T + 2 scored positions).  An id
 *     outside [0, V) becomes the "no word" id: an id is never an index, so it reads nothing out of bounds.
 *   labels [N] int64 (the model of each row) or NULL (model 0); n_lm models in ONE array of 16-byte slots (csrc/lm_slot.h):
 *     model l owns slots[lm_off[l] .. lm_off[l] + lm_capacity[l]) (int64 [n_lm] each, the capacity a power of two with at
 *     least one empty slot) and has order lm_order[l] (int32 [n_lm], 1 .. 4).  The caller vouches for these three arrays:
 *     they are device memory, no host check can read them.
 *   eos_mode 0 ('word') / 1 ('end'), unk_as_word, V <= 65531: see isc_lm_score.
 *   score [N] float64 (log10); n_scored [N], n_oov [N] int32 or NULL; tok_logp [N, T + 2] float64 or NULL.
 * One wave64 per row, one lane per scored position, four rows per workgroup; a lane walks at most 2 order - 1 probe
 * chains; the row's sum runs over the lanes in ascending order.  No workspace, no LDS, no atomics.  One launch, no host
 * read: capturable.  A label outside [0, n_lm): score NaN, n_scored -1, n_oov 0, no table is read.
 * N < 1, T outside [1, 62], n_lm < 1, V outside [1, 65531], eos_mode outside {0, 1}: ISC_E_SHAPE, nothing is launched. */
int isc_lm_dev_score(const int64_t *hyp, int64_t N, int T, const int64_t *labels, int n_lm, const void *slots,
                     const int64_t *lm_off, const int64_t *lm_capacity, const int32_t *lm_order, int V, int eos_mode,
                     int unk_as_word, int64_t sos_id, int64_t eos_id, double *score, int32_t *n_scored, int32_t *n_oov,
                     double *tok_logp, void *stream);

/* Sentiment-word reward (self_critical/utils.py:154-166): every position of a caption row is paid the weight of its word
 * where the word belongs to the lexicon of the row's sentiment label; the words that were paid are marked, and
 * isc_sw_decay later multiplies the marked words' weights (models/decoder.py:174-176).  All pointers are device memory.
 *   tok [N, T] int64, contiguous; every position is looked at (also those behind <EOS>: the criterion masks).  An id is
 *     compared as a 64-bit integer before it becomes an index: an id outside [0, V) - negative, or >= 2^32 with low bits
 *     that are a valid index - reads nothing and is paid 0.
 *   labels [N] int64.  weights [n_labels, V] float64; state [n_labels, V] uint8: 0 = not in the lexicon, 1 = in it, 2 = in
 *     it and used since the last decay.  Membership is the state, never "weight != 0".
 *   w = weights[label, tok] where state[label, tok] != 0, else 0.  reward64 [N, T] float64 or NULL gets w.  reward_io
 *     [N, T] float32 or NULL: accumulate == 0 -> (float)w (`flag` is not applied); accumulate != 0 -> reward_io +
 *     (float)flag * (float)w, the product rounded to float32 before the addition, never contracted: the bits of torch's
 *     `rewards + flag * sw` on float32 tensors.  row_hits [N] int32 or NULL: the row's number of paid positions.
 *   mark != 0: a paid position stores 2 into state[label, tok] - a plain store of a constant; many lanes and rows may
 *     store it to the same byte.
 *   A label outside [0, n_labels): NaN in the row of reward_io and reward64, -1 in row_hits, no table is read, nothing is
 *     marked (the convention of isc_lm_dev_score).
 * One wave64 per row, four rows per workgroup, lanes stride over the positions (any T >= 1); row_hits from ballots.  No
 * LDS, no atomics, no workspace, no host read; one launch: capturable.
 * N < 1, T < 1, n_labels < 1, V < 1: ISC_E_SHAPE, nothing is launched or written. */
int isc_sw_reward(const int64_t *tok, int64_t N, int T, const int64_t *labels, int n_labels, int V, const double *weights,
                  uint8_t *state, double flag, float *reward_io, int accumulate, double *reward64, int32_t *row_hits,
                  int mark, void *stream);
/* Where state[i] == 2: weights[i] *= factor in float64 (the bits of Python's `w *= factor`) and state[i] = 1; i < n (=
 * n_labels * V).  n < 1: ISC_E_SHAPE, nothing is launched. */
int isc_sw_decay(double *weights, uint8_t *state, int64_t n, double factor, void *stream);

/* Log-softmax backward with the criteria's gradient handed over SPARSE: XECriterion (captioner.py:427-440) and the
 * REINFORCE gather (captioner.py:336) touch one column per (caption, step) row, so their d log-prob is `coef[m]` at
 * column `ids[m]` - up to ISC_SPARSE_MAX such (ids, coef) pairs (HOST arrays of device pointers to [M] vectors, rows
 * in [B,T] order) plus an optional dense part `dlogp_dense` [M, ld_in] (NULL when every consumer of the log-probs was
 * one of the two criteria: no [B,T,V] gradient tensor is then written or read at all).
 *   dlogits[m', v] = scale * (dense[m,v] + sum_j coef_j[m] [v == ids_j[m]] - exp(logp[m,v]) * (sum_v dense + sum_j coef_j))
 * `scale`: optional device scalar (isc_grad_scale's out2[0]); rows are written time-major when remap_T > 0 and
 * columns V..ld_out-1 are zero-filled, as isc_logsoftmax_bwd does. */
#define ISC_SPARSE_MAX 2
int isc_logsoftmax_bwd_sparse(const float *dlogp_dense, const float *logp, int64_t ld_in, int M, int V,
                              const int64_t *const *ids_host, const float *const *coef_host, int n_sparse,
                              const float *scale, float *dlogits, int64_t ld_out, int remap_T, int out_step_rows,
                              void *stream);
/* out_step_rows (0 = M / remap_T): rows per step of the time-major output - input row (b,t) goes to output row
 * t*out_step_rows + b (a merged unroll's d logits hold both branches' rows per step; dlogits then points at this
 * branch's first row). */

/* The criteria on RAW logits (training iterations that never materialise the [B,T,V] log-probs, captioner.py:183 + 232):
 * the criteria read one column per (caption, step) row, and log p(id) = (x[id] - max) - log(sum exp) follows from the raw
 * logits and the classifier's tile statistics - the same bits isc_logsoftmax_apply_steps would have stored.
 * Logits row (b,t) at raw + b*ld_b + t*ld_t; statistics row of (b,t) = t*step_rows + b (0 = B); ids / out / coef in
 * [B,T] order.
 *   isc_gather_logp_raw:     out[b,t] = log p(ids[b,t]) (* live[t] when given: captioner.py:336 after the early break)
 *   isc_xe_loss_tokens_fwd:  XECriterion on such per-token log-probs: out2 = { -sum_{t < len_b} tlp[b,t], count }
 *   isc_logsoftmax_bwd_raw:  d logits (time-major rows t*out_step_rows + b, zero-padded to ld_out) from up to
 *                            ISC_SPARSE_MAX (ids, coef) pairs, as isc_logsoftmax_bwd_sparse forms it from stored log-probs. */
int isc_gather_logp_raw(const float *raw, int64_t ld_b, int64_t ld_t, int B, int T, int V, const float *part_max,
                        const float *part_sum, int step_rows, const int64_t *ids, const float *live, float *out,
                        void *stream);
int isc_xe_loss_tokens_fwd(const float *tlp, const int32_t *lengths, int B, int T, float *out2, void *stream);
int isc_logsoftmax_bwd_raw(const float *raw, int64_t ld_b, int64_t ld_t, int B, int T, int V, const float *part_max,
                           const float *part_sum, int step_rows, const int64_t *const *ids_host,
                           const float *const *coef_host, int n_sparse, const float *scale, float *dlogits, int64_t ld_out,
                           int out_step_rows, void *stream);

/* isc_logsoftmax_bwd_raw plus the gradient of the SAMPLED distribution's log-probability (filtered sampling:
 * isc_rollout_finalize_saved), in one launch and one pass over the raw logits.  Per row (b,t), with c = flt_coef[b,t],
 * K = { v : rank key(x_v, v) <= kstar[b,t] } minus the row's ban[b,t,0..10) ids (-1: unused slot; ban NULL: none) and
 * q_v = exp((x_v - gmax[b,t]) * inv_tau - logz[b,t]) (clamped to 1):
 *     d logits[t*out_step_rows + b, v] = (the n_sparse model pairs' term of isc_logsoftmax_bwd_raw)
 *                                        + scale * c * inv_tau * ([v == flt_tok[b,t]] - [v in K] * q_v).
 * The two terms are rounded separately and then added: in bits, isc_logsoftmax_bwd_raw's result plus the result of this
 * call with n_sparse = 0.  n_sparse may be 0 (part_max / part_sum may then be NULL).  A row whose coefficients are all
 * zero is written as zeros without reading its logits; columns outside K other than flt_tok get exactly 0; pad columns
 * [V, ld_out) are zero.  flt_tok / kstar int64 [B,T], flt_coef / gmax / logz fp32 [B,T], ban int32 [B,T,10].
 * A missing pointer -> ISC_E_NULL, sizes (and inv_tau not finite and > 0, n_sparse outside [0, ISC_SPARSE_MAX]) ->
 * ISC_E_SHAPE, before any launch.  No atomics: bit-repeatable; no host read: capturable. */
int isc_logsoftmax_bwd_raw_filtered(const float *raw, int64_t ld_b, int64_t ld_t, int B, int T, int V,
                                    const float *part_max, const float *part_sum, int step_rows,
                                    const int64_t *const *ids_host, const float *const *coef_host, int n_sparse,
                                    const int64_t *flt_tok, const float *flt_coef, float inv_tau, const int64_t *kstar,
                                    const float *gmax, const float *logz, const int32_t *ban, const float *scale,
                                    float *dlogits, int64_t ld_out, int out_step_rows, void *stream);

/* The frozen sentence-sentiment classifier of the RL rewards, forward in eval mode (sent_senti_cls.py:38-56; called by
 * self_critical/utils.py:120-151 for the classifier reward and by decoder.py:133-136 for the XE sentiment labels):
 *   x = relu(Emb[tokens]);  out = LSTM(x);  w[b,t] = mean_h sigmoid(ex2(relu(ex0(out[t,b])))) for t < lens[b], else 0;
 *   feats[b] = sum_t w[b,t] out[t,b];  logits = cls3(relu(cls0(feats)));  pred = argmax (lowest index on ties);
 *   reward[b,:] = pred[b] == labels[b] ? w[b,:] : 0.
 * tokens [B,L] int64 (row stride tokens_ld); EVERY entry, also past a row's length, must be a valid id (they are read -
 * clamped into [0, V) - but never reach a sum: the recurrence is causal and the pooling stops at the length).
 * lens [B] int32 on the device, each in [1, L] (clamped there).  The thirteen parameter tensors as the module's state_dict
 * stores them (contiguous): emb [V,W]; w_ih [4H,W], w_hh [4H,H], b_ih, b_hh [4H] (gate rows i,f,g,o); ex0 / ex2 / cls0
 * [H,H] + [H]; cls3 [k,H] + [k].  labels [B] int64, optional (required iff reward).
 * Outputs: logits [B,k]; weights [B,T_out] and reward [B,T_out] (optional) contiguous, exactly 0 at and beyond a row's
 * length and in columns L..T_out-1; pred [B] int32; feats [B,H] (optional: the pooled features, for tests).
 * T + 7 launches on `stream`, no host read, no allocation: the time-major embedding gather (which also clears the zero
 * state), ONE input GEMM over all L*B rows (isc_linear_fwd), L fused cells (isc_lstm_fwd, one K-segment h W_hh^T, pre =
 * the step's rows of the input GEMM), two excitation GEMMs, the pooling kernel, the head GEMM and the k-way head.  The
 * GEMMs get no split-K workspace: one launch each, on the fp32 MFMA tiles (or, on a stream that holds a weights scope,
 * the scope's kernels).  Pooling and head sum in a fixed order without atomics: two calls give the same bits.
 * W % 32 == H % 32 == 0 (they may differ), V >= 1, 1 <= k <= 8, 1 <= L <= 4096, T_out >= L, B >= 1: anything else
 * ISC_E_SHAPE; a workspace smaller than isc_sent_cls_workspace_bytes(B, L, W, H) ISC_E_WORKSPACE, not 16-byte aligned
 * ISC_E_ALIGN - all before any launch, nothing is written then. */
typedef struct {
    int32_t B, L, W, H, V, k, T_out, _pad;
    const int64_t *tokens;
    int64_t tokens_ld;
    const int32_t *lens;
    const float *emb, *w_ih, *w_hh, *b_ih, *b_hh;
    const float *ex0_w, *ex0_b, *ex2_w, *ex2_b;
    const float *cls0_w, *cls0_b, *cls3_w, *cls3_b;
    const int64_t *labels;
    void *workspace;
    int64_t workspace_bytes;
    float *logits, *weights;
    int32_t *pred;
    float *reward, *feats;
} isc_sent_cls_problem;
int64_t isc_sent_cls_workspace_bytes(int B, int L, int W, int H);
int isc_sent_cls_fwd(const isc_sent_cls_problem *prob_host, void *stream);
long long isc_sent_cls_launches(void);    /* kernels enqueued by isc_sent_cls_fwd so far (measurement / test hook) */

/* ---- the classifier's own training (train_sent_senti_cls_rnn.py:110-126): saved-activation forward, CrossEntropyLoss,
 * and the whole reverse sweep, on the library's kernels.  Every floating-point sum runs in one fixed order without atomics
 * (two calls give the same bits; the only atomics are the integer counters of isc_embed_relu_bwd_ws's position index from
 * 1024 rows on, whose segments are sorted before they are summed), allocates nothing, never reads back, and validates before the first launch (nothing is written
 * when a call returns an error).
 *
 * isc_sent_cls_head_loss - the k-way head with its loss (two launches: one wave per caption, then one thread per output):
 *   logits[b,j] = hid[b,:] . cls3_w[j,:] + cls3_b[j]   (the bits of isc_sent_cls_fwd's head);  pred = arg-max, lowest index
 *   on ties;  loss_rows[b] = logsumexp(z) - z[label] in the max-subtracted form;  dz8[b,j] = g (softmax_j - [j == label]) / B
 *   in a [B,8] buffer whose columns k..7 are zero;  dhid[b,:] = sum_j dz8[b,j] cls3_w[j,:] (j ascending);
 *   loss[0] = mean of loss_rows, wrong[0] = rows with pred != label, dw3[j,:] = sum_b dz8[b,j] hid[b,:],
 *   db3[j] = sum_b dz8[b,j] (b ascending).  hid [B,H] is the head's hidden layer after ReLU and dropout; labels [B] int64,
 *   each in [0, k).  1 <= k <= 8, H % 4 == 0, B >= 1 (ISC_E_SHAPE); hid, cls3_w, dz8, dhid, dw3 16-byte aligned
 *   (ISC_E_ALIGN).  g: the gradient scale (below).
 *
 * isc_sent_cls_pool_bwd - backward of the squeeze-excite pooling (one workgroup per caption, a wave per step), from
 *   dfeats [B,H], the saved pre-sigmoid e2 and dropped LSTM outputs o ([L*B,H], time-major rows t*B+b), the saved token
 *   weights [B, ldw] and lens [B] (clamped into [0, L]).  For t < len:
 *     dw[b,t] = dfeats[b,:] . o[t,b,:];  de2[t,b,h] = (dw[b,t] / H) s (1 - s), s = sigmoid(e2[t,b,h]);
 *     d_o[t,b,:] = weights[b,t] dfeats[b,:];
 *   for t >= len both output rows (and dw[b,t]) are written as exact zeros whatever they held.  dw [B,L] is optional.
 *   H % 4 == 0, 1 <= L <= 4096, ldw >= L (ISC_E_SHAPE); the five [.,H] tensors 16-byte aligned (ISC_E_ALIGN). */
int isc_sent_cls_head_loss(const float *hid, const float *cls3_w, const float *cls3_b, const int64_t *labels, int B, int H,
                           int k, float g, float *logits, int32_t *pred, float *loss_rows, float *dz8, float *dhid,
                           float *dw3, float *db3, float *loss, int32_t *wrong, void *stream);
int isc_sent_cls_pool_bwd(const float *dfeats, const float *e2, const float *o, const float *weights, int64_t ldw,
                          const int32_t *lens, int B, int L, int H, float *de2, float *d_o, float *dw, void *stream);

/* One training iteration's problem: what isc_sent_cls_train_fwd and isc_sent_cls_bwd share (the backward is called with the
 * struct the forward was called with, gradients and workspace filled in).  Sizes, tokens, lens, the thirteen parameters and
 * labels (required) as in isc_sent_cls_problem; H % 32 == W % 32 == 0, W <= 1024 (the embedding gradient).
 * Dropout: three optional uint8 keep-masks - emb_keep [L*B, W] and out_keep [L*B, H] over the time-major rows t*B+b,
 * hid_keep [B, H] - sharing mask_scale = 1 / (1 - p).  Null = no dropout at that place; with all three null the forward is
 * the eval forward and its logits equal isc_sent_cls_fwd's bit for bit.
 * grad_scale = S: the sweep runs on S dz and every gradient leaves times S - the caller multiplies by 1 / S.  dz is of the
 * order 1 / B and de2 carries a further 1 / H: below the f16 normal range, where the split-f16 contractions keep bits
 * relative to 2^-14.  S a power of two makes both scalings exact.
 * saved (isc_sent_cls_train_saved_bytes): written by the forward, read by the backward -
 *   x (after ReLU and emb_keep) | Xg | activated gates [L,B,4H] | c [L,B,H] | h [L,B,H] (raw: the recurrence input) |
 *   o [L,B,H] (dropped; o = h without out_keep) | e1 | e2 | zero state | feats | hid | dz8 | dhid | loss_rows.
 * isc_sent_cls_train_fwd: the launch sequence of isc_sent_cls_fwd (L + 7, the cells with gates_out and, under out_keep,
 *   h_keep_mask / hdrop_out; the head GEMM with hid_keep in its epilogue; + 1 launch for emb_keep) with the head replaced
 *   by isc_sent_cls_head_loss (2 launches): L + 8 launches, + 1 with emb_keep.
 *   Outputs: logits [B,k], weights [B,T_out], pred [B], loss [1], wrong [1] int32, d_cls3_w [k,H], d_cls3_b [k].
 * isc_sent_cls_bwd: the reverse sweep, one call.  Library calls enqueued (isc_sent_cls_bwd_launches counts them):
 *     1            prepare: d_emb = 0, the token ids time-major (<PAD> behind each length), d_w_hh = 0 when L == 1
 *     3            head hidden layer: ReLU / hid_keep mask, TN (d_cls0_w), NN (dfeats)
 *     1            isc_sent_cls_pool_bwd
 *     5            excitation: TN (d_ex2_w), NN, ReLU mask, TN (d_ex0_w), NN accumulating onto d_o
 *     [out_keep]   the LSTM-output dropout mask
 *     2 L - 1      per step t = L-1 .. 0: isc_lstm_bwd, and for t > 0 one NN  dgates[t] W_hh  for the step before
 *     [L > 1]      d_w_hh: ONE TN over the (L-1) B rows  dgates[1:]^T h[:L-1]
 *     4            d_w_ih (ONE TN over L B rows), dx (one NN), the embedding gradient (isc_embed_relu_bwd_ws, skip_id =
 *                  pad_id: nn.Embedding's padding_idx), the five bias gradients (one isc_colsum_multi; d_b_ih and d_b_hh
 *                  share a reduction)
 *   = 2 L + 13 + [L > 1] + [out_keep].  (A call is one kernel, except: a TN / NN contraction on the split-f16 route is a
 *   plane split plus the GEMM (TN only), isc_colsum_multi is up to two, the embedding gradient one or five.)
 *   Rows at and behind a caption's length are exact zeros from isc_sent_cls_pool_bwd on, and isc_lstm_bwd maps zero dh /
 *   dc_next to zeros, so the contractions over all L B rows need no masking and the tokens there change no bit.
 *   workspace: isc_sent_cls_bwd_workspace_bytes(B, L, W, H, V).  splitk_ws (optional, 256-byte aligned): handed to the TN
 *   contractions - the split-f16 route of isc_gemm_bwd builds its planes there; the NN contractions get none and stay on
 *   the exact-fp32 tiles (one kernel each, also inside the step loop).
 * Errors as isc_sent_cls_fwd, all before any launch. */
typedef struct {
    int32_t B, L, W, H, V, k, T_out, _pad;
    const int64_t *tokens;
    int64_t tokens_ld;
    const int32_t *lens;
    const float *emb, *w_ih, *w_hh, *b_ih, *b_hh;
    const float *ex0_w, *ex0_b, *ex2_w, *ex2_b;
    const float *cls0_w, *cls0_b, *cls3_w, *cls3_b;
    const int64_t *labels;
    const uint8_t *emb_keep, *out_keep, *hid_keep;
    float mask_scale, grad_scale;
    int64_t pad_id;
    void *saved;
    int64_t saved_bytes;
    void *workspace;            /* isc_sent_cls_bwd only */
    int64_t workspace_bytes;
    float *splitk_ws;           /* isc_sent_cls_bwd only, optional */
    int64_t splitk_ws_floats;
    float *logits, *weights;
    int32_t *pred;
    float *loss;
    int32_t *wrong;
    /* gradients (times grad_scale): d_cls3_w / d_cls3_b are the forward's outputs, the other eleven the backward's */
    float *d_emb, *d_w_ih, *d_w_hh, *d_b_ih, *d_b_hh;
    float *d_ex0_w, *d_ex0_b, *d_ex2_w, *d_ex2_b;
    float *d_cls0_w, *d_cls0_b, *d_cls3_w, *d_cls3_b;
} isc_sent_cls_train_problem;
int64_t isc_sent_cls_train_saved_bytes(int B, int L, int W, int H);
int64_t isc_sent_cls_bwd_workspace_bytes(int B, int L, int W, int H, int V);
int isc_sent_cls_train_fwd(const isc_sent_cls_train_problem *prob_host, void *stream);
int isc_sent_cls_bwd(const isc_sent_cls_train_problem *prob_host, void *stream);
long long isc_sent_cls_bwd_launches(void);    /* library calls enqueued by isc_sent_cls_bwd so far (test hook) */

/* The frozen image-sentiment detector, forward in eval mode (sentiment_detector.py:30-60; called by decoder.py:83 for the
 * image labels of an RL iteration and by decoder.py:182-192 in front of a beam search):
 *   x = conv_{n-1}( ... conv_0(features) ... ), 3x3, padding 1, cross-correlation, channels C -> C/2 -> C/4 ..., NO
 *   non-linearity between the convolutions;  r = relu(x);  m[b,j,p] = bs[j] + r[b,p,:] . Ws[j,:]  (the 1x1 conv);
 *   z = FC_{f-1}( ... FC_0(mean_p m) ... )  (k x k layers, no activation between them);  prob = softmax(z);
 *   maps[b,p] = sum_j prob_j m[b,j,p];  scores[b] = max_j prob_j;  labels[b] = the first arg-max, or neu_idx when
 *   scores[b] < threshold (compared in fp32).
 * feats [B,h,w,C] channels-last as the region grid is stored, contiguous, fp32 or (feats_f16 = 1) _Float16 - read as
 * they are: no im2col buffer, no padded copy, no up-cast copy.  packed: the conv weights as isc_senti_det_pack wrote
 * them.  conv_b[i] [C >> (i+1)]; senti_w [k, C >> n_convs], senti_b [k]; fc_w[l] [k,k] row-major (out, in), fc_b[l] [k].
 * The convolutions are implicit GEMMs on the split-f16 engine (row (b h + y) w + x, contraction over 9 taps x Cin,
 * tap-major; three v_mfma_f32_16x16x32_f16 terms, the 2^-11 weight applied once): operand domain |x| < 65504.  A tap
 * outside the image's own grid reads a zeroed line of the workspace - exact zeros, whatever the neighbouring image holds;
 * every output row of image b depends on image b alone.  f16 features are their own hi plane: the result equals the call
 * on the up-cast values bit for bit.
 * Route per conv layer, chosen on the host from the tile count (64 x 128 tiles): one workgroup per tile with bias (and
 * ReLU behind the last layer) in the kernel, or - few tiles - the contraction split over `ksplit` workgroups per tile, raw
 * partial tiles to slabs of the workspace and a reduce kernel that sums them in ascending order and adds the bias.
 * ksplit: 0 = auto, n >= 1 forces n (clamped to the layer's 9 Cin / 32 chunks).  No atomics anywhere: two calls give the
 * same bits.  A non-finite logit raises the numerics status word non-finite vocabulary logits raise
 * (ISC_STATUS_NONFINITE_STATS) and its label is neu_idx.
 * One memset node + n_convs .. 2 n_convs + 1 launches on `stream`; no allocation, no host read: capturable.
 * Shapes: every conv's Cin = C >> i a multiple of 32, 1 <= n_convs <= 4, 0 <= n_fcs <= 4, 1 <= k <= 8, 0 <= neu_idx < k,
 * 1 <= h w <= ISC_SENTI_DET_MAX_HW (the k maps of an image stay in LDS: 8 x 1024 floats), B h w <= 2^22: anything else
 * ISC_E_SHAPE; a workspace under isc_senti_det_workspace_bytes(B, h, w, C, n_convs, ksplit) ISC_E_WORKSPACE; feats, packed,
 * workspace, conv_out or a conv bias not 16-byte aligned ISC_E_ALIGN - all before any launch, nothing is written then.
 * conv_out (optional, [B h w, C >> n_convs]): the post-ReLU activations, for tests. */
#define ISC_SENTI_DET_MAX_CONVS 4
#define ISC_SENTI_DET_MAX_FCS 4
#define ISC_SENTI_DET_MAX_HW 1024
/* isc_senti_det_launches(kind): launches so far, per kind (host-atomic, read-only; -1 for an unknown kind) */
#define ISC_SENTI_DET_KIND_DIRECT 0     /* conv, one workgroup per tile */
#define ISC_SENTI_DET_KIND_SPLIT 1      /* conv, contraction split over workgroups */
#define ISC_SENTI_DET_KIND_REDUCE 2     /* slab reduce behind a split conv */
#define ISC_SENTI_DET_KIND_TAIL 3       /* 1x1 conv, pooling, FCs, softmax, decision */
#define ISC_SENTI_DET_KIND_PACK 4       /* weight pack, one per conv layer */
#define ISC_SENTI_DET_KIND_F16 5        /* conv launches (of either route) that read _Float16 rows natively */
#define ISC_SENTI_DET_KINDS 6
typedef struct {
    const void *feats;
    int32_t feats_f16, B, h, w, C, n_convs, n_fcs, k, neu_idx, ksplit;
    float threshold;
    int32_t _pad;
    const void *packed;
    const float *conv_b[ISC_SENTI_DET_MAX_CONVS];
    const float *senti_w, *senti_b;
    const float *fc_w[ISC_SENTI_DET_MAX_FCS], *fc_b[ISC_SENTI_DET_MAX_FCS];
    void *workspace;
    int64_t workspace_bytes;
    float *logits, *maps;
    int64_t *labels;
    float *scores;
    float *conv_out;
} isc_senti_det_problem;
/* bytes of the packed weights: per conv layer i the hi/lo planes (layout: isc_seg.A_hi) of [C >> (i+1), 9 (C >> i)] with
 * k = (ky 3 + kx) Cin + ci, layer after layer; 0 for a shape the library refuses */
int64_t isc_senti_det_pack_bytes(int C, int n_convs);
/* conv_w_host: HOST array of n_convs device pointers [Cout, Cin, 3, 3] fp32 contiguous; one launch per layer.  The
 * weights are frozen: once per weight version. */
int isc_senti_det_pack(const float *const *conv_w_host, int C, int n_convs, void *packed, void *stream);
int64_t isc_senti_det_workspace_bytes(int B, int h, int w, int C, int n_convs, int ksplit);
int isc_senti_det_fwd(const isc_senti_det_problem *prob_host, void *stream);
long long isc_senti_det_launches(int kind);

/* Training the image-sentiment detector (train_senti.py:68-86): the saved-activation forward with the loss, and the whole
 * reverse sweep in one call.  Shape domain, weights and layouts as isc_senti_det_fwd; feats fp32 [B,h,w,C].
 * isc_senti_det_train_fwd:
 *   packs the conv weights (they move every step: one launch per layer), runs the frozen forward's conv launches - the same
 *   kernel, the same route choice (ksplit = 0) - without the ReLU, then  r = relu(keep x2 mask_scale)  (keep: optional
 *   uint8 [B,h,w,C >> n_convs], channels-last; null = no dropout), the tail kernel (which also keeps the
 *   pooled means and every FC activation) and the head loss:  loss = scale mean_b CE(logits_b, labels_b)  in the stable form
 *   and dz = d loss / d logits.  labels [B] int64 on the device.  With keep null, logits and maps equal isc_senti_det_fwd's
 *   bit for bit.  What the backward reads of the tail - pooled means, FC outputs, dz - and the loss come from a second
 *   evaluation of the same maps in double, in the tail kernel itself: pooled sums, FC layers, softmax and the image's
 *   cross-entropy term (the frozen tail's fp32 sum over up to 1024 pixels would otherwise stand, through dz and times
 *   |pooled|, in every gradient); those logits differ from the ones handed out by a few fp32 ulp.  A label outside
 *   [0, k) makes that image's loss term and dz NaN (torch raises there): the loss and every gradient come out NaN.
 *   Launches: 2 n_convs + 3, + 1 per conv layer on the split route (its slab reduce).
 * isc_senti_det_bwd (called with the struct the forward was called with, gradients and workspace filled in):
 *     1          per image: dz back through the FCs to dpool, sum_p r[b,p,:], dr[b,:] = sum_j dpool[b,j]/(h w) Ws[j,:] and
 *                the image's power-of-two scale (below)
 *     1          d senti_conv, d FC weights and biases: one ordered sum over the images each; the common scale
 *     1          dx2 = dr [x2 keep > 0] keep mask_scale, times the image's scale
 *     per conv layer i = n_convs-1 .. 0:
 *       1        d bias = sum_m dY[m,:], fixed order
 *       1        d weight [Cout,Cin,3,3]: the implicit TN contraction  sum_m dY[m,co] X[pixel(m) + (ky-1,kx-1), ci]  over
 *                the M = B h w rows on the split-f16 MFMA engine (64 x 128 output tiles, both operands staged through
 *                LDS transposed, X read where it lies; out-of-grid taps are exact zeros)
 *       2 [i>0]  dX = conv3x3(dY, W') with W'[ci,co,ky,kx] = W[co,ci,2-ky,2-kx]: the flipped-transposed pack and a launch of
 *                the forward's convolution kernel (no bias, no ReLU; + 1 slab reduce on the split route)
 *   = 4 n_convs + 1 launches (+ 1 per dX on the split route, + 1 with dx_out); n_fcs and the mask change neither count.
 *   Scaling: dz <= scale / B and dx2 carries a further 1 / (h w) and |Ws|: far below the f16 normal range.  Every image's
 *   dx2 is multiplied by e_b = 2^-floor(log2 max_c |dr[b,c]|) before it meets the split-f16 planes (so an image's dX rows
 *   depend on that image alone), the contractions over m bring the rows to the common scale E = min_b e_b as they load them
 *   and multiply by 1 / E in fp32 in their epilogue - all exact powers of two, all read from device memory.
 *   No allocation, no host read, no atomics; every cross-image and cross-pixel sum runs in a fixed order.
 * saved: isc_senti_det_train_saved_bytes (forward writes, backward reads); workspace (backward only):
 * isc_senti_det_bwd_workspace_bytes.  dx_out (optional, tests): [B h w, C/2] the gradient of conv_0's output, unscaled
 * (n_convs >= 2).  Errors as isc_senti_det_fwd (ISC_E_NULL / SHAPE / WORKSPACE / ALIGN), all before any launch. */
typedef struct {
    const float *feats;
    int32_t B, h, w, C, n_convs, n_fcs, k, _pad;
    float mask_scale, scale;
    const float *conv_w[ISC_SENTI_DET_MAX_CONVS], *conv_b[ISC_SENTI_DET_MAX_CONVS];
    const float *senti_w, *senti_b;
    const float *fc_w[ISC_SENTI_DET_MAX_FCS], *fc_b[ISC_SENTI_DET_MAX_FCS];
    const int64_t *labels;
    const uint8_t *keep;
    void *saved;
    int64_t saved_bytes;
    void *workspace;            /* isc_senti_det_bwd only */
    int64_t workspace_bytes;
    float *logits, *maps, *loss;
    float *d_conv_w[ISC_SENTI_DET_MAX_CONVS], *d_conv_b[ISC_SENTI_DET_MAX_CONVS];
    float *d_senti_w, *d_senti_b;
    float *d_fc_w[ISC_SENTI_DET_MAX_FCS], *d_fc_b[ISC_SENTI_DET_MAX_FCS];
    float *dx_out;
} isc_senti_det_train_problem;
int64_t isc_senti_det_train_saved_bytes(int B, int h, int w, int C, int n_convs, int n_fcs);
int64_t isc_senti_det_bwd_workspace_bytes(int B, int h, int w, int C, int n_convs);
int isc_senti_det_train_fwd(const isc_senti_det_train_problem *prob_host, void *stream);
int isc_senti_det_bwd(const isc_senti_det_train_problem *prob_host, void *stream);
/* launches so far (test hook; -1 for an unknown kind) */
#define ISC_SENTI_DET_TRAIN_KIND_FWD 0      /* all launches of isc_senti_det_train_fwd */
#define ISC_SENTI_DET_TRAIN_KIND_BWD 1      /* all launches of isc_senti_det_bwd */
#define ISC_SENTI_DET_TRAIN_KIND_REDUCE 2   /* of either: slab reduces behind split-route convolutions */
#define ISC_SENTI_DET_TRAIN_KINDS 3
long long isc_senti_det_bwd_launches(int kind);
/* The kernels of the sweep on their own (tests).
 * isc_senti_det_dw: dw [Cout,Cin,3,3] = unscale sum_m dy[m,co] ratio[b(m)] x[pixel(m) + tap, ci];  dy [M, ldy] (ldy >=
 *   Cout, ldy % 4 == 0), x [B,h,w,Cin]; ratio [B] and unscale [1] on the device, null = 1.  Cin % 32 == 0, Cout % 16 == 0.
 * isc_senti_det_pack_flipped: planes of W' [Cin, 9 Cp] (Cp = Cout rounded up to 32, the padding zero) from w [Cout,Cin,3,3];
 *   2 Cin 9 Cp halfs. */
int isc_senti_det_dw(const float *dy, int ldy, const float *x, int B, int h, int w, int Cin, int Cout, const float *ratio,
                     const float *unscale, float *dw, void *stream);
int isc_senti_det_pack_flipped(const float *w, int Cout, int Cin, void *planes, void *stream);
/* Float offsets into isc_senti_det_bwd's workspace of what its first two launches leave (tests): out6 = g [n_fcs][B][8]
 * (d loss / d output of FC l), dpool [B][8], rsum [B, C >> n_convs] (sum_p r), dr [B, C >> n_convs], e_b [B], E / e_b [B]. */
int isc_senti_det_bwd_tail_offsets(int B, int h, int w, int C, int n_convs, int64_t *out6);

/* The concept detector (concept_detector.py; train_cpt.py, detect_concepts.py, test_cpt.py) - csrc/concept.hip.  One
 * wave64 per row, no atomics, every sum in a fixed order (two calls give the same bits), no allocation and no host read:
 * capturable.
 *
 * isc_concept_head: logits [B, C] fp32 (leading dimension ld >= C; C any positive number) ->
 *   probs  [B, C]   sigmoid(logits)                                   (contiguous; optional)
 *   idx    [B, num] int64: the `num` best concepts of a row, best first   (optional)
 *   scores [B, num] their probabilities                               (optional)
 *   words  [B, num] int64 = concept_word[idx] through the [C] int64 table of vocabulary ids (optional; needs the table)
 *   hits [B], n_true [B] int32 with a 0/1 target matrix [B, C] (uint8, or int64 with targets_i64 != 0): n_true = the
 *     row's targets that are set, hits = how many of the picked concepts are set - numerator and denominators of the
 *     precision / recall loop of train_cpt.py:113-122 (the picks are distinct: a set intersection).  Optional.
 * ORDER: the larger LOGIT first; on equal logits the lower index first; -0.0 equals +0.0; +-inf are ordinary values; a
 * NaN ranks below every number (lower index first among NaNs) and raises ISC_STATUS_NONFINITE_STATS.  The reference
 * sorts the fp32 probabilities with an unstable sort (concept_detector.py:28); sigmoid is monotone, so this is the
 * reference's answer wherever that is defined, and a fixed one where probabilities saturate or tie.
 * num outside [1, ISC_CONCEPT_MAX_NUM] or > C, B < 1, C < 1, ld < C: ISC_E_SHAPE, nothing is launched.
 *
 * isc_concept_loss: MultiLabelClsLoss (concept_detector.py:44-58) from the LOGITS:
 *   out3 = { -mean(t log s(z)), -mean((1 - t) log(1 - s(z))), their sum }  over all B C elements, evaluated as
 *   t softplus(-z) and (1 - t) softplus(z), softplus(x) = max(x, 0) + log1p(exp(-|x|)): finite for every finite z (the
 *   reference's result.log() of a saturated fp32 sigmoid gives inf or NaN there).  Elements in fp32, sums in fp64: per-row
 *   wave sums (lane l: columns l, l + 64, ... ascending, then the butterfly) into the workspace, then one wave over the
 *   rows in the same fixed order.  dz (optional, [B, C] contiguous) = (s(z) - t) g / (B C), written in the same pass.
 *   targets [B, C] contiguous, uint8 or (targets_i64 != 0) int64 - any non-zero value is 1; both give the same bits.
 *   workspace: isc_concept_loss_workspace_bytes(B) bytes, 8-byte aligned.  Two launches.
 *
 * isc_senti_words_from_concepts: preprocess.py:288-301 on the device.  idx [B, num] int64 concept indices (leading
 * dimension idx_ld; an index outside [0, C) contributes nothing), a CSR table off [C + 1] int32, word [nnz] int64
 * (vocabulary ids), score [nnz] float64.  Per image the entries of its concepts are taken in concept order, then list
 * order; the scores are summed per word in float64 in that order (the host's bits); the words are ordered by sum,
 * descending, exactly equal sums in first-occurrence order (Python's stable sort over the dict's insertion order); the
 * first n_out <= ISC_SENTI_WORDS_MAX_OUT ids go to out [B, n_out] int64, the rest - all of it for an image without an
 * entry - is pad_id.  One wave per image, candidates in LDS.  CAP: an image may stage num * max_list <=
 * ISC_SENTI_WORDS_CAP candidates, max_list = the longest list of the table as isc_senti_words_pack_check (host
 * offsets) reports it: a larger product is ISC_E_SHAPE there and here, nothing is launched - never a silent cut. */
#define ISC_CONCEPT_MAX_NUM 16
#define ISC_SENTI_WORDS_CAP 1024
#define ISC_SENTI_WORDS_MAX_OUT 20
int isc_concept_head(const float *logits, int64_t ld, int B, int C, int num, float *probs, int64_t *idx, float *scores,
                     const int64_t *concept_word, int64_t *words, const void *targets, int targets_i64, int32_t *hits,
                     int32_t *n_true, void *stream);
int64_t isc_concept_loss_workspace_bytes(int B);
int isc_concept_loss(const float *logits, int64_t ld, int B, int C, const void *targets, int targets_i64, float g,
                     void *workspace, int64_t workspace_bytes, float *out3, float *dz, void *stream);
int isc_senti_words_cap(void);
int isc_senti_words_pack_check(const int32_t *off_host, int C, int num, int *max_list_out);
int isc_senti_words_from_concepts(const int64_t *idx, int64_t idx_ld, int B, int num, int C, const int32_t *off,
                                  const int64_t *word, const double *score, int max_list, int n_out, int64_t pad_id,
                                  int64_t *out, void *stream);

/* The concept detector's eval forward (concept_detector.py:10-18,24-30): h1 = relu(feats W0^T + b0); h2 = relu(h1 W2^T +
 * b2); logits = h2 W5^T + b5; then isc_concept_head - FOUR library launches (besides the optional conversion below): three isc_linear_fwd (whose dispatch they
 * inherit: the few-row route, the split-f16 routes, the exact engine under isc_set_h3_mode(0)) and the head.
 * feats [B, F] fp32 or (feats_f16 = 1) _Float16 with leading dimension feats_ld in elements: float16 rows are read
 * natively where isc_linear_f16_native says so, else converted once (isc_f16_to_f32) into the workspace.  W0 [H, F],
 * W2 [H, H], W5 [C, H] contiguous fp32 as the state_dict stores them.  Outputs as isc_concept_head's (all optional);
 * logits [B, C] optional (16-byte aligned).  splitk_ws: optional workspace handed to the linear launches.
 * F % 32 == 0, H % 32 == 0 (isc_linear_fwd contracts in 32-deep chunks), C >= 1, 1 <= num <= min(C,
 * ISC_CONCEPT_MAX_NUM), feats_ld >= F: anything else ISC_E_SHAPE; feats not 16-byte aligned or feats_ld % 4 != 0
 * ISC_E_ALIGN; a workspace under isc_concept_workspace_bytes(B, F, H, C) ISC_E_WORKSPACE - all before any launch. */
typedef struct {
    const void *feats;
    int64_t feats_ld;
    int32_t feats_f16, B, F, H, C, num;
    const float *w0, *b0, *w2, *b2, *w5, *b5;
    const int64_t *concept_word;
    void *workspace;
    int64_t workspace_bytes;
    float *splitk_ws;
    int64_t splitk_ws_floats;
    float *logits, *probs;
    int64_t *idx;
    float *scores;
    int64_t *words;
} isc_concept_problem;
int64_t isc_concept_workspace_bytes(int B, int F, int H, int C);
int isc_concept_fwd(const isc_concept_problem *prob_host, void *stream);
long long isc_concept_launches(void);     /* library launches enqueued by isc_concept_fwd so far: four per call besides the
                                           * optional isc_f16_to_f32 conversion, which has its own counter (test hook) */

/* Power-of-two gradient scale for a backward sweep whose contractions run on the split-f16 engine: out4[0..1] = { S, 1/S },
 * S = 2^k with max |x| over the given tensors (HOST arrays of device pointers / element counts, <= ISC_SCALE_SRC_MAX)
 * brought into [2^-4, 2^-3); S = 1 when they are all zero.  out4[2..3] are state words of the multi-workgroup reduction:
 * the caller hands them in ZEROED (once; every call leaves them zeroed).  The caller multiplies what enters the sweep by
 * S (exact) and the parameter gradients by 1/S (exact): gradients of a token-mean loss are <= 1/N_tokens, below the f16
 * normal range at training batch sizes, where the planes x = hi + lo 2^-11 would keep ~22 bits relative to 2^-14 instead
 * of to the element. */
#define ISC_SCALE_SRC_MAX 4
int isc_grad_scale(const float *const *src_host, const int64_t *numel_host, int n_src, float *out4, void *stream);

/* Workspace sizes (the library allocates nothing; these say what to hand it).
 * isc_splitk_workspace_bytes: bytes that let a launch with an [M, N] output use the deepest K split (16 slabs);
 *   isc_*_problem.splitk_ws may be smaller (fewer slabs) or NULL (no split, no out-of-scope split-f16 launches).
 * isc_h3_weights_workspace_bytes: bytes of an isc_h3_weights_begin buffer that holds the f16 planes (hi + lo) of
 *   `weight_elements` fp32 weight values, twice that when the backward's transposed planes are wanted too. */
int64_t isc_splitk_workspace_bytes(int64_t M, int64_t N);
int64_t isc_h3_weights_workspace_bytes(int64_t weight_elements, int with_transposes);

/* Sticky numerics status.  The caller registers two 32-bit words of HOST memory that the device can write (pinned /
 * mapped: hipHostMalloc, a pinned torch tensor) with isc_set_status_words - per device, after selecting it; NULL
 * unregisters.  A kernel that meets a non-finite value stores 1 into its word (error path only; nothing is written
 * otherwise), and isc_status reads the words on the host WITHOUT any device call: it reports what the work the host has
 * already waited for has flagged.  Bits of the return value:
 *   ISC_STATUS_NONFINITE_STATS (1)  a vocabulary-statistics row (max / sum exp) was non-finite when a decode step folded
 *                                   it (roll-out finalize, scheduled sampling, log-softmax passes, beam top-k)
 *   ISC_STATUS_NONFINITE_LINEAR (2) a split-f16 linear launch over caller data staged as fp32 rows (the prologue's raw
 *                                   region features, training-mode activations) produced a non-finite pre-activation
 * Either means an operand left the split-f16 domain |x| < 65504 (its hi plane is inf) or was NaN / inf on entry (the
 * linear epilogues' ReLU lets NaN through, as torch's does, so it reaches the statistics); results since the last clean
 * read are not to be trusted.  isc_set_h3_mode(0) runs the exact-fp32 tiles, whose domain is fp32's.
 * reset != 0 clears the words when any bit was set.  Both calls act on the CURRENT device (hipGetDevice). */
#define ISC_STATUS_NONFINITE_STATS 1
#define ISC_STATUS_NONFINITE_LINEAR 2
int isc_set_status_words(unsigned int *host_words2);
int isc_status(int reset);

/* clip_gradient (train_xe.py:19-23, decoder.py:14-18: elementwise clamp_ to +-clip, in place)
 * followed by torch.optim.Adam's update (captioner.py:422-423), all tensors in one launch.
 * Pointer tables are HOST arrays of device pointers. clip <= 0 disables the clamp. */
#define ISC_ADAM_MAX_TENSORS 48
int isc_clamp_adam(float *const *params_host, float *const *grads_host, float *const *exp_avg_host,
                   float *const *exp_avg_sq_host, const int64_t *numel_host, int n_tensors, double lr,
                   double beta1, double beta2, double eps, double weight_decay, double clip, int step,
                   void *stream);
/* The same launch with its step-dependent scalars in DEVICE memory: hyper3_dev = {lr, 1 - beta1^step,
 * sqrt(1 - beta2^step)} as floats (what isc_clamp_adam derives from lr / step on the host, in double).  For a training
 * iteration captured into a HIP graph: kernel arguments are frozen at capture, the caller rewrites these three
 * floats before every replay (train_graph.py). */
int isc_clamp_adam_hyper(float *const *params_host, float *const *grads_host, float *const *exp_avg_host,
                         float *const *exp_avg_sq_host, const int64_t *numel_host, int n_tensors,
                         const float *hyper3_dev, double beta1, double beta2, double eps, double weight_decay,
                         double clip, void *stream);

/* ---- The image encoder (csrc/encoder.hip): the reference's models/encoder.py in eval mode, from pixels to fc [B, C] and
 * att [B, a, a, C] (C = 32 width), every batch norm folded into the convolution in front of it.  A bottleneck ResNet of
 * layers[4] blocks at base width `width` (32 or 64: the stem keeps its weights in LDS); the reference is {3, 4, 23, 3}
 * at 64.  Every activation is channels-last fp32 [B, h, w, C].  Status codes, never throws; every shape, alignment and
 * workspace check in front of the first launch, nothing written on refusal; no allocation and no host read inside a call
 * (a forward at a fixed image size is capturable); no atomics: two runs give the same bits.
 *
 * Convolution order (isc_encoder_pack's `convs`, isc_encoder_num_convs of them): the stem, then per block conv1, conv2,
 * conv3 and - in the first block of a layer - the downsample.  Each entry: the weight [N, Cin, R, R] and the batch norm
 * behind it (weight, bias, running_mean, running_var; eps = 1e-5), all fp32 on the device.  The pack computes
 * w' = w g / sqrt(v + eps), b' = beta - mu g / sqrt(v + eps) in double, rounds once to fp32 and splits w' into the f16
 * planes [N, 2 R R Cin], k = tap Cin + ci (the stem: fp32 [147, C0], k = (ky 7 + kx) 3 + c).  packed: 256-byte aligned.
 *
 * isc_encoder_fwd: image [B, H, W, 3], uint8 (image_u8 != 0: x / 255, then (x - mean) / std of the reference's
 * preprocess, as the stem's taps load) or fp32 already normalised; H, W >= 3 (below, the ceil-mode pool has no output),
 * B Ho Wo <= 2^22, B <= 65535, 1 <= att_size <= 64: else ISC_E_SHAPE.  ksplit: 0 = every convolution's route by the cost
 * rule (per image: independent of B), n >= 1 = n workgroups per tile forced (capped at the chunk count); workspace at least
 * isc_encoder_workspace_bytes_ksplit(..., ksplit) (== isc_encoder_workspace_bytes for ksplit 0), packed_bytes at least
 * isc_encoder_pack_bytes: else ISC_E_WORKSPACE.  fc_f16 / att_f16: optional float16 copies (round to nearest even). */
#define ISC_ENCODER_KIND_STEM 0
#define ISC_ENCODER_KIND_POOL 1
#define ISC_ENCODER_KIND_DIRECT 2   /* convolution, one workgroup per tile */
#define ISC_ENCODER_KIND_SPLIT 3    /* convolution, contraction split over workgroups */
#define ISC_ENCODER_KIND_REDUCE 4   /* slab reduce behind a split convolution */
#define ISC_ENCODER_KIND_TAIL 5
#define ISC_ENCODER_KIND_PACK 6     /* weight pack, one per convolution */
#define ISC_ENCODER_KIND_R1 7       /* convolution launches (of either route) of the 1x1 form */
#define ISC_ENCODER_KIND_R3 8       /* ... of the 3x3 form */
#define ISC_ENCODER_KINDS 9
long long isc_encoder_launches(int kind);

typedef struct {
    const float *w, *gamma, *beta, *mean, *var;
} isc_encoder_conv_params;

typedef struct {
    const void *image;
    int image_u8, B, H, W;
    int layers[4];
    int width, att_size, ksplit, _pad;
    const void *packed;
    int64_t packed_bytes;
    void *workspace;
    int64_t workspace_bytes;
    float *fc, *att;
    void *fc_f16, *att_f16;
} isc_encoder_problem;

int isc_encoder_num_convs(const int *layers4, int width);                  /* 0: refused */
int64_t isc_encoder_pack_bytes(const int *layers4, int width);             /* 0: refused */
int isc_encoder_pack(const isc_encoder_conv_params *convs_host, int n_convs, const int *layers4, int width, void *packed,
                     void *stream);
int64_t isc_encoder_workspace_bytes(int B, int H, int W, const int *layers4, int width);
int64_t isc_encoder_workspace_bytes_ksplit(int B, int H, int W, const int *layers4, int width, int ksplit);
int isc_encoder_final_grid(int H, int W, int *hf, int *wf);                 /* the layer-4 grid of an H x W image */
int isc_encoder_fwd(const isc_encoder_problem *prob_host, void *stream);

/* The parts on their own (tests).
 * isc_conv_pack: planes of one convolution, R in {1, 3}; gamma null: no fold, `bias` not written.
 * isc_conv_fwd: out [B ho wo, N] = (relu)(conv(x) + bias[n] (+ residual[m, n])); x [B, h, w, Cin]; R = 1: stride 1 or
 *   2, ho = (h - 1) / stride + 1; R = 3: stride 1, pad 1.  Cin % 32 == 0, N % 16 == 0, B h w <= 2^22.
 * isc_encoder_stem_pack / isc_encoder_stem: wk [147, C0], C0 in {32, 64}; out [B, (H - 1) / 2 + 1, (W - 1) / 2 + 1, C0].
 * isc_encoder_maxpool: 3x3 / 2, pad 0, ceil mode: out [B, (h - 2) / 2 + 1, (w - 2) / 2 + 1, C]; h, w >= 2, C % 4 == 0.
 * isc_encoder_tail: fc [B, C] = mean over w, then over h; att [B, a, a, C] = adaptive average pool.
 * Alignment: x, planes, bias, residual, workspace and out of isc_conv_fwd, `out` of the stem and both tensors of the
 * max-pool 16 bytes (vector accesses); wk, bias and fp32 pixels of the stem, x / fc / att of the tail 4 bytes, the float16
 * copies 2 bytes (scalar accesses): else ISC_E_ALIGN.  Order of the checks in every call: null pointers, shape,
 * workspace size, alignment - a call wrong in two ways gets the first of these codes.
 * The route of a convolution (ksplit 0) is chosen from ONE image's rows h_out w_out, never from B: an image gets the
 * same bits in a batch as alone. */
typedef struct {
    const float *x;
    int B, h, w, Cin, N, R, stride, relu, ksplit, _pad;
    const void *planes;
    const float *bias, *residual;
    void *workspace;
    int64_t workspace_bytes;
    float *out;
} isc_conv_problem;
int isc_conv_pack(const float *w, const float *gamma, const float *beta, const float *mean, const float *var, int N,
                  int Cin, int R, void *planes, float *bias, void *stream);
int64_t isc_conv_workspace_bytes(int B, int h, int w, int Cin, int N, int R, int stride, int ksplit);
int isc_conv_fwd(const isc_conv_problem *prob_host, void *stream);
int isc_encoder_stem_pack(const float *w, const float *gamma, const float *beta, const float *mean, const float *var,
                          int C0, float *wk, float *bias, void *stream);
int isc_encoder_stem(const void *img, int img_u8, int B, int H, int W, int C0, const float *wk, const float *bias,
                     float *out, void *stream);
int isc_encoder_maxpool(const float *x, int B, int h, int w, int C, float *out, void *stream);
int isc_encoder_tail(const float *x, int B, int h, int w, int C, int att_size, float *fc, float *att, void *fc_f16,
                     void *att_f16, void *stream);

#ifdef __cplusplus
}
#endif
#endif
