// Back-off n-gram language models on the device (isc_lm_dev_score): what csrc/cider.cpp lm_score_row does for one row,
// done by one wave64 in the form of cider_dev_kernel.  Lane i owns scored position i of the sentence (at most T + 2 <= 64
// positions) and reads the <= 3 words in front of it from the lower lanes by cross-lane reads; every lane then walks its
// own back-off chain - at most 2 * order - 1 probe chains of random 16-byte slot reads - and the row's sum is taken over
// the lanes in ascending order in float64.  No LDS, no workspace, no atomics, no barrier: the four waves of a workgroup
// are independent.  Only float32 -> float64 conversions and float64 additions in a fixed order are involved, so the host
// scorer, the device and two launches give the same bits.
#include "common.h"
#include "lm_slot.h"

#define LM_WAVES 4      // rows per workgroup

__device__ __forceinline__ double lm_lane_f64(double v, int j) {
    return __longlong_as_double((long long)lane_u64((uint64_t)__double_as_longlong(v), j));
}

__global__ __launch_bounds__(64 * LM_WAVES) void lm_dev_kernel(
    const int64_t *__restrict__ hyp, long long N, int T, const int64_t *__restrict__ labels, int n_lm,
    const isc_lm_slot *__restrict__ slots, const int64_t *__restrict__ lm_off, const int64_t *__restrict__ lm_capacity,
    const int32_t *__restrict__ lm_order, int V, int eos_word, int unk_as_word, int64_t sos, int64_t eos,
    double *__restrict__ score, int32_t *__restrict__ n_scored, int32_t *__restrict__ n_oov,
    double *__restrict__ tok_logp) {
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    const long long r = (long long)blockIdx.x * LM_WAVES + wave;
    if (r >= N) return;                                   // (the whole wave leaves: nothing below waits for it)

    const long long lab = labels ? labels[r] : 0;         // (the same in every lane)
    if (lab < 0 || lab >= n_lm) {                         // no such model: no table is read
        if (lane == 0) {
            score[r] = __longlong_as_double(0x7ff8000000000000LL);
            if (n_scored) n_scored[r] = -1;
            if (n_oov) n_oov[r] = 0;
        }
        if (tok_logp && lane < T + 2) tok_logp[r * (T + 2) + lane] = 0.0;
        return;
    }
    const isc_lm_slot *__restrict__ table = slots + lm_off[lab];
    const uint64_t mask = (uint64_t)lm_capacity[lab] - 1;
    const int order = __builtin_amdgcn_readfirstlane(lm_order[lab]);

    // ---- normalise as cider_dev_kernel does: drop a leading <SOS>, cut at the first <EOS>, append <EOS>.  Lanes >= T hold
    // <EOS>, so the first <EOS> at or behind `start` always exists (T <= 62) and is the appended one when the row has none.
    const int64_t tok = lane < T ? hyp[r * T + lane] : eos;
    const int start = (int64_t)lane_u64((uint64_t)tok, 0) == sos ? 1 : 0;
    const unsigned long long at_eos = __ballot(lane >= start && tok == eos);
    const int L = __builtin_amdgcn_readfirstlane(__ffsll((long long)at_eos) - 1 - start + 1);      // 1 .. T + 1 words
    // scored positions: 'word' - the L words (<EOS> among them, as a word), then </s>; 'end' - the <EOS> becomes </s>
    const int P = eos_word ? L + 1 : L;                   // 1 .. T + 2 <= 64
    // the 16-bit key field of a word is id + 1; an id outside [0, V) becomes the "no word" id
    const int field0 = (int)((tok >= 0 && tok < V ? tok : ISC_LM_NONE(V)) + 1);
    const int moved = __shfl(field0, (start + lane) & 63);                    // word `lane` of the normalised row
    const int wf = lane < P - 1 ? moved : (int)(ISC_LM_EOS(V) + 1);
    // f[d]: the word d places in front of the lane's own (d = 0); in front of word 0 stands <s>, in front of that nothing
    uint64_t f[ISC_CIDER_MAX_ORDER];
    f[0] = (uint64_t)(uint32_t)wf;
#pragma unroll
    for (int d = 1; d < ISC_CIDER_MAX_ORDER; ++d) {
        const int g = __shfl(wf, (lane - d) & 63);
        f[d] = (uint64_t)(uint32_t)(lane - d >= 0 ? g : (int)(ISC_LM_BOS(V) + 1));
    }
    const int ctx = order - 1 < lane + 1 ? order - 1 : lane + 1;             // words of context this position has
    const bool active = lane < P;

    // ---- the back-off walk, from the longest context to the empty one
    double acc = 0.0, val = 0.0;
    bool found = false;
#pragma unroll
    for (int len = ISC_CIDER_MAX_ORDER - 1; len >= 0; --len) {
        if (active && !found && len <= ctx) {
            uint64_t kc = 0;                              // the context: its oldest word in field 0
#pragma unroll
            for (int j = 0; j < len; ++j) kc |= f[len - j] << (16 * j);
            const uint64_t kw = kc | (f[0] << (16 * len));
            const isc_lm_slot hit = isc_lm_find(table, mask, kw);
            if (hit.key) {
                val = (double)hit.logp + acc;
                found = true;
            } else if (len > 0) {
                const isc_lm_slot c = isc_lm_find(table, mask, kc);
                if (c.key) acc += (double)c.backoff;
            }
        }
    }
    const bool oov = active && !found;                    // no unigram
    if (oov && unk_as_word) {
        const isc_lm_slot u = isc_lm_find(table, mask, (uint64_t)(ISC_LM_UNK(V) + 1));
        if (u.key) {
            val = (double)u.logp + acc;
            found = true;
        }
    }
    const bool scored = active && found;
    if (!scored) val = 0.0;

    const int cnt_scored = __popcll(__ballot(scored));
    const int cnt_oov = __popcll(__ballot(oov));
    double s = 0.0;
    for (int j = 0; j < P; ++j) s += lm_lane_f64(val, j);
    if (lane == 0) {
        score[r] = s;
        if (n_scored) n_scored[r] = cnt_scored;
        if (n_oov) n_oov[r] = cnt_oov;
    }
    if (tok_logp && lane < T + 2) tok_logp[r * (T + 2) + lane] = val;
}

extern "C" int isc_lm_dev_score(const int64_t *hyp, int64_t N, int T, const int64_t *labels, int n_lm, const void *slots,
                                const int64_t *lm_off, const int64_t *lm_capacity, const int32_t *lm_order, int V,
                                int eos_mode, int unk_as_word, int64_t sos_id, int64_t eos_id, double *score,
                                int32_t *n_scored, int32_t *n_oov, double *tok_logp, void *stream) {
    if (!hyp || !slots || !lm_off || !lm_capacity || !lm_order || !score) return ISC_E_NULL;
    if (N < 1 || T < 1 || T > ISC_LM_MAX_T || n_lm < 1 || V < 1 || V > ISC_LM_MAX_VOCAB) return ISC_E_SHAPE;
    if (eos_mode < 0 || eos_mode > 1) return ISC_E_SHAPE;
    const int64_t blocks = (N + LM_WAVES - 1) / LM_WAVES;
    if (blocks > 0x7fffffffLL) return ISC_E_SHAPE;
    hipLaunchKernelGGL(lm_dev_kernel, dim3((unsigned)blocks), dim3(64 * LM_WAVES), 0, (hipStream_t)stream, hyp,
                       (long long)N, T, labels, n_lm, (const isc_lm_slot *)slots, lm_off, lm_capacity, lm_order, V,
                       eos_mode == 0 ? 1 : 0, unk_as_word ? 1 : 0, sos_id, eos_id, score, n_scored, n_oov, tok_logp);
    ISC_LAUNCH_CHECK();
    return ISC_OK;
}
