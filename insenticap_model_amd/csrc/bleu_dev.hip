// BLEU on the device (isc_bleu_dev_score): what csrc/cider.cpp bleu_stats / bleu_scores do for one hypothesis, done by
// one wave64 in the form of cider_dev_kernel.  Lane i owns word i of the normalised hypothesis (L <= 64 words) and, per
// order k, the k-gram that starts there.  Everything a lane needs from another lane travels through cross-lane reads - no
// LDS, no workspace, no atomics, no barrier: the four waves of a workgroup are independent.  The statistics are integers
// (the host's, exactly); the float tail - a dozen operations, one pow per order, one exp - is computed wave-uniformly in
// the order of bleu_scorer.py:233-242 and stored by one lane.
#include "common.h"
#include "cider_key.h"

#define BLEU_WAVES 4      // hypotheses per workgroup

__global__ __launch_bounds__(64 * BLEU_WAVES) void bleu_dev_kernel(
    const int64_t *__restrict__ hyp, long long N, int T, int row_div, const int32_t *__restrict__ img_ent_off,
    const uint64_t *__restrict__ ref_keys, const int32_t *__restrict__ ref_counts,
    const int32_t *__restrict__ img_cap_off, const int32_t *__restrict__ ref_lens, int order, int64_t sos, int64_t eos,
    double *__restrict__ scores, int32_t *__restrict__ stats) {
#pragma clang fp contract(off)
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    const long long r = (long long)blockIdx.x * BLEU_WAVES + wave;
    if (r >= N) return;                                   // (the whole wave leaves: nothing below waits for it)

    // ---- normalise: drop a leading <SOS>, cut at the first <EOS>, append <EOS>.  Lanes >= T hold <EOS>, so the first
    // <EOS> at or behind `start` always exists (T <= 63) and is the appended one when the row has none.
    const int64_t tok = lane < T ? hyp[r * T + lane] : eos;
    const int start = (int64_t)lane_u64((uint64_t)tok, 0) == sos ? 1 : 0;
    const unsigned long long at_eos = __ballot(lane >= start && tok == eos);
    const int L = __builtin_amdgcn_readfirstlane(__ffsll((long long)at_eos) - 1 - start + 1);      // testlen: 1 .. T + 1
    const int field0 = (int)isc_cider_field(tok, 0);      // 16 bits: this lane's token as field 0 of a key

    // ---- keys: key[o] = the (o + 1)-gram that starts at word `lane`, 0 where it would run past the last word
    uint64_t key[ISC_CIDER_MAX_ORDER];
#pragma unroll
    for (int o = 0; o < ISC_CIDER_MAX_ORDER; ++o) {
        const uint64_t f = (uint64_t)(uint32_t)__shfl(field0, (start + lane + o) & 63);      // word lane + o
        const uint64_t head = o ? key[o - 1] : 0;
        key[o] = (lane + o < L && (o == 0 || head)) ? (head | (f << (16 * o))) : 0;
    }

    // ---- count of the lane's k-gram among the positions, and whether the lane is its first occurrence
    int tf[ISC_CIDER_MAX_ORDER];
    bool first[ISC_CIDER_MAX_ORDER];
#pragma unroll
    for (int o = 0; o < ISC_CIDER_MAX_ORDER; ++o) tf[o] = 0, first[o] = key[o] != 0;
    for (int j = 0; j < L; ++j) {
#pragma unroll
        for (int o = 0; o < ISC_CIDER_MAX_ORDER; ++o) {
            const uint64_t kj = lane_u64(key[o], j);      // (read by every lane: in front of the lane's own test)
            const bool same = key[o] != 0 && kj == key[o];
            tf[o] += same ? 1 : 0;
            if (same && j < lane) first[o] = false;
        }
    }

    // ---- the largest count of the lane's k-grams in one reference of the row's image: the image's cooked entries come in
    // 64 at a time, one per lane, and are handed round (keys of different orders differ: one walk serves the four orders)
    const long long img = r / row_div;
    const int a = __builtin_amdgcn_readfirstlane(img_ent_off[5 * img]);
    const int b = __builtin_amdgcn_readfirstlane(img_ent_off[5 * img + 4]);
    int rmax[ISC_CIDER_MAX_ORDER] = {0, 0, 0, 0};
    for (int base = a; base < b; base += 64) {
        const int mine = base + lane;
        const uint64_t rk = mine < b ? ref_keys[mine] : 0;
        const int rc = mine < b ? ref_counts[mine] : 0;
        const int cnt = b - base < 64 ? b - base : 64;
        for (int j = 0; j < cnt; ++j) {
            const uint64_t kq = lane_u64(rk, j);
            const int cq = __builtin_amdgcn_readlane(rc, j);
#pragma unroll
            for (int o = 0; o < ISC_CIDER_MAX_ORDER; ++o)
                if (kq == key[o]) rmax[o] = cq;               // (key[o] == 0 matches nothing: no entry has key 0)
        }
    }

    // ---- correct[o]: the clipped counts of the distinct k-grams, an integer sum over the lanes
    int clip[ISC_CIDER_MAX_ORDER], correct[ISC_CIDER_MAX_ORDER];
#pragma unroll
    for (int o = 0; o < ISC_CIDER_MAX_ORDER; ++o) {
        clip[o] = first[o] ? (tf[o] < rmax[o] ? tf[o] : rmax[o]) : 0;
        correct[o] = 0;
    }
    for (int j = 0; j < L; ++j) {
#pragma unroll
        for (int o = 0; o < ISC_CIDER_MAX_ORDER; ++o) correct[o] += __builtin_amdgcn_readlane(clip[o], j);
    }

    // ---- the "closest" reference length: min((abs(l - testlen), l)) over the image's references, a tie takes the shorter
    const int c0 = __builtin_amdgcn_readfirstlane(img_cap_off[img]);
    const int c1 = __builtin_amdgcn_readfirstlane(img_cap_off[img + 1]);
    int best_d = 0x7fffffff, reflen = 0;
    for (int c = c0; c < c1; ++c) {
        const int l = __builtin_amdgcn_readfirstlane(ref_lens[c]);
        const int d = l > L ? l - L : L - l;
        if (d < best_d || (d == best_d && l < reflen)) best_d = d, reflen = l;
    }

    // ---- the float tail (bleu_scorer.py:233-242), the same in every lane
    const double small = 1e-9, tiny = 1e-15;
    double s[ISC_CIDER_MAX_ORDER];
    int guess[ISC_CIDER_MAX_ORDER];
    double bleu = 1.0;
#pragma unroll
    for (int k = 0; k < ISC_CIDER_MAX_ORDER; ++k) {
        guess[k] = L - k > 0 ? L - k : 0;
        bleu *= ((double)correct[k] + tiny) / ((double)guess[k] + small);
        s[k] = pow(bleu, 1.0 / (double)(k + 1));
    }
    const double ratio = ((double)L + tiny) / ((double)reflen + small);
    if (ratio < 1) {
        const double pen = exp(1 - 1 / ratio);
#pragma unroll
        for (int k = 0; k < ISC_CIDER_MAX_ORDER; ++k) s[k] *= pen;
    }
    if (lane == 0) {
        if (order == 0) {
#pragma unroll
            for (int k = 0; k < ISC_CIDER_MAX_ORDER; ++k) scores[4 * r + k] = s[k];
        } else {
            scores[r] = order == 1 ? s[0] : order == 2 ? s[1] : order == 3 ? s[2] : s[3];
        }
        if (stats) {
            int32_t *st = stats + 10 * r;
            st[0] = L;
            st[1] = reflen;
#pragma unroll
            for (int k = 0; k < ISC_CIDER_MAX_ORDER; ++k) st[2 + k] = guess[k], st[6 + k] = correct[k];
        }
    }
}

extern "C" int isc_bleu_dev_score(const int64_t *hyp, int64_t N, int T, int row_div, const int32_t *img_ent_off,
                                  const uint64_t *ref_keys, const int32_t *ref_counts, const int32_t *img_cap_off,
                                  const int32_t *ref_lens, int64_t n_img, int order, int64_t sos_id, int64_t eos_id,
                                  double *scores, int32_t *stats, void *stream) {
    if (!hyp || !img_ent_off || !ref_keys || !ref_counts || !img_cap_off || !ref_lens || !scores) return ISC_E_NULL;
    if (N < 1 || T < 1 || T > 63 || row_div < 1 || order < 0 || order > ISC_CIDER_MAX_ORDER) return ISC_E_SHAPE;
    if (n_img < 1 || (N - 1) / row_div >= n_img) return ISC_E_SHAPE;      // every row's image has a reference range
    const int64_t blocks = (N + BLEU_WAVES - 1) / BLEU_WAVES;
    if (blocks > 0x7fffffffLL) return ISC_E_SHAPE;
    hipLaunchKernelGGL(bleu_dev_kernel, dim3((unsigned)blocks), dim3(64 * BLEU_WAVES), 0, (hipStream_t)stream, hyp,
                       (long long)N, T, row_div, img_ent_off, ref_keys, ref_counts, img_cap_off, ref_lens, order, sos_id,
                       eos_id, scores, stats);
    ISC_LAUNCH_CHECK();
    return ISC_OK;
}
