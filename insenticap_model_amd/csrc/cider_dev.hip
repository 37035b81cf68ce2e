// CIDEr-D on the device (isc_cider_dev_score): what csrc/cider.cpp score_one does for one hypothesis, done by one wave64.
// Lane i owns position i of the normalised hypothesis (L <= 64 words) and, per order k, the k-gram that starts there.
// Everything a lane needs from another lane travels through cross-lane reads - no LDS, no workspace, no atomics, no
// barrier: the four waves of a workgroup are independent.  Every sum runs over the lanes in ascending order, which is
// the host's first-occurrence order (a k-gram that occurred before contributes an exact +0.0), and over the references
// in ascending order: two runs give the same bits, and only exp, sqrt and the division can differ from the host's.
#include "common.h"
#include "cider_key.h"

#define CIDER_WAVES 4      // hypotheses per workgroup

// Value of `v` in lane j, j wave-uniform (lane_u64: cider_key.h).
__device__ __forceinline__ double lane_f64(double v, int j) {
    return __longlong_as_double((long long)lane_u64((uint64_t)__double_as_longlong(v), j));
}

// log(max(1, df)) of `key`, 0.0 when the table does not hold it.  At most `mask + 1` probes: a table without an empty
// slot (a damaged one) ends the walk as "absent".
__device__ __forceinline__ double cider_log_df(const isc_cider_slot *__restrict__ table, uint64_t mask, uint64_t key) {
    uint64_t s = isc_cider_hash(key) & mask;
    for (uint64_t p = 0; p <= mask; ++p) {
        const isc_cider_slot slot = table[s];
        if (slot.key == key) return slot.log_df;
        if (slot.key == 0) break;
        s = (s + 1) & mask;
    }
    return 0.0;
}

__global__ __launch_bounds__(64 * CIDER_WAVES) void cider_dev_kernel(
    const int64_t *__restrict__ hyp, long long N, int T, int row_div, const isc_cider_slot *__restrict__ table,
    uint64_t mask, const int32_t *__restrict__ img_cap_off, const int32_t *__restrict__ ord_off,
    const double *__restrict__ ref_norms, const double *__restrict__ ref_length, const uint64_t *__restrict__ ref_keys,
    const double *__restrict__ ref_vals, int n, double two_sigma2, double ref_len, int64_t sos, int64_t eos,
    double *__restrict__ scores) {
#pragma clang fp contract(off)
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    const long long r = (long long)blockIdx.x * CIDER_WAVES + wave;
    if (r >= N) return;                                   // (the whole wave leaves: nothing below waits for it)

    // ---- normalise (cider.cpp normalise): drop a leading <SOS>, cut at the first <EOS>, append <EOS>.  Lanes >= T hold
    // <EOS>, so the first <EOS> at or behind `start` always exists (T <= 63) and is the appended one when the row has none.
    const int64_t tok = lane < T ? hyp[r * T + lane] : eos;
    const int start = (int64_t)lane_u64((uint64_t)tok, 0) == sos ? 1 : 0;
    const unsigned long long at_eos = __ballot(lane >= start && tok == eos);
    const int L = __builtin_amdgcn_readfirstlane(__ffsll((long long)at_eos) - 1 - start + 1);      // 1 .. T + 1 words
    const int field0 = (int)isc_cider_field(tok, 0);      // 16 bits: this lane's token as field 0 of a key

    // ---- keys: key[o] = the (o + 1)-gram that starts at word `lane`, 0 where it would run past the last word
    uint64_t key[ISC_CIDER_MAX_ORDER];
#pragma unroll
    for (int o = 0; o < ISC_CIDER_MAX_ORDER; ++o) {
        const uint64_t f = (uint64_t)(uint32_t)__shfl(field0, (start + lane + o) & 63);      // word lane + o
        const uint64_t head = o ? key[o - 1] : 0;
        key[o] = (o < n && lane + o < L && (o == 0 || head)) ? (head | (f << (16 * o))) : 0;
    }

    // ---- precook: tf of the lane's k-gram among the positions, and whether the lane is its first occurrence
    double tf[ISC_CIDER_MAX_ORDER];
    bool first[ISC_CIDER_MAX_ORDER];
#pragma unroll
    for (int o = 0; o < ISC_CIDER_MAX_ORDER; ++o) tf[o] = 0.0, first[o] = key[o] != 0;
    for (int j = 0; j < L; ++j) {
#pragma unroll
        for (int o = 0; o < ISC_CIDER_MAX_ORDER; ++o) {
            const uint64_t kj = lane_u64(key[o], j);      // (read by every lane: in front of the lane's own test)
            const bool same = key[o] != 0 && kj == key[o];
            tf[o] += same ? 1.0 : 0.0;
            if (same && j < lane) first[o] = false;
        }
    }

    // ---- counts2vec: x = tf (ref_len - d) per distinct k-gram (one probe walk each), per-order norms, bigram `length`
    double x[ISC_CIDER_MAX_ORDER], sq[ISC_CIDER_MAX_ORDER], nh[ISC_CIDER_MAX_ORDER];
#pragma unroll
    for (int o = 0; o < ISC_CIDER_MAX_ORDER; ++o) {
        x[o] = 0.0;
        if (first[o]) x[o] = tf[o] * (ref_len - cider_log_df(table, mask, key[o]));
        sq[o] = x[o] * x[o];
        nh[o] = 0.0;
    }
    const double tf2 = first[1] ? tf[1] : 0.0;
    double len_h = 0.0;
    for (int j = 0; j < L; ++j) {
#pragma unroll
        for (int o = 0; o < ISC_CIDER_MAX_ORDER; ++o) nh[o] += lane_f64(sq[o], j);
        len_h += lane_f64(tf2, j);
    }
#pragma unroll
    for (int o = 0; o < ISC_CIDER_MAX_ORDER; ++o) nh[o] = sqrt(nh[o]);

    // ---- the references of the row's image, ascending
    const long long img = r / row_div;
    const int c0 = __builtin_amdgcn_readfirstlane(img_cap_off[img]);
    const int c1 = __builtin_amdgcn_readfirstlane(img_cap_off[img + 1]);
    double score[ISC_CIDER_MAX_ORDER] = {0.0, 0.0, 0.0, 0.0};
    for (int c = c0; c < c1; ++c) {
        const int a = __builtin_amdgcn_readfirstlane(ord_off[5 * (long long)c]);
        const int b = __builtin_amdgcn_readfirstlane(ord_off[5 * (long long)c + 4]);
        // the reference's value of the lane's k-grams: its entries come in 64 at a time, one per lane, and are handed round
        // (keys of different orders differ, so one walk over all of the reference's entries serves the four orders)
        double rv[ISC_CIDER_MAX_ORDER] = {0.0, 0.0, 0.0, 0.0};
        for (int base = a; base < b; base += 64) {
            const int mine = base + lane;
            const uint64_t rk = mine < b ? ref_keys[mine] : 0;
            const double rx = mine < b ? ref_vals[mine] : 0.0;
            const int cnt = b - base < 64 ? b - base : 64;
            for (int j = 0; j < cnt; ++j) {
                const uint64_t kq = lane_u64(rk, j);
                const double vq = lane_f64(rx, j);
#pragma unroll
                for (int o = 0; o < ISC_CIDER_MAX_ORDER; ++o)
                    if (kq == key[o]) rv[o] = vq;         // (key[o] == 0 matches nothing: no entry has key 0)
            }
        }
        double term[ISC_CIDER_MAX_ORDER], val[ISC_CIDER_MAX_ORDER];
#pragma unroll
        for (int o = 0; o < ISC_CIDER_MAX_ORDER; ++o) {
            term[o] = first[o] ? fmin(x[o], rv[o]) * rv[o] : 0.0;      // clipped (ciderD_scorer.py:164)
            val[o] = 0.0;
        }
        for (int j = 0; j < L; ++j) {
#pragma unroll
            for (int o = 0; o < ISC_CIDER_MAX_ORDER; ++o) val[o] += lane_f64(term[o], j);
        }
        const double delta = len_h - ref_length[c];
        const double pen = exp(-(delta * delta) / two_sigma2);
#pragma unroll
        for (int o = 0; o < ISC_CIDER_MAX_ORDER; ++o) {
            const double nr = ref_norms[4 * (long long)c + o];
            if (nh[o] != 0 && nr != 0) val[o] /= (nh[o] * nr);
            val[o] *= pen;
            score[o] += val[o];
        }
    }
    double s = 0.0;
#pragma unroll
    for (int o = 0; o < ISC_CIDER_MAX_ORDER; ++o)
        if (o < n) s += score[o];
    s /= (double)n;
    s /= (double)(c1 - c0);
    if (lane == 0) scores[r] = s * 10.0;
}

extern "C" int isc_cider_dev_score(const int64_t *hyp, int64_t N, int T, int row_div, const void *table, int64_t capacity,
                                   const int32_t *img_cap_off, int64_t n_img, const int32_t *ord_off,
                                   const double *ref_norms, const double *ref_length, const uint64_t *ref_keys,
                                   const double *ref_vals, int n, double sigma, double ref_len, int64_t sos_id,
                                   int64_t eos_id, double *scores, void *stream) {
    if (!hyp || !table || !img_cap_off || !ord_off || !ref_norms || !ref_length || !ref_keys || !ref_vals || !scores)
        return ISC_E_NULL;
    if (N < 1 || T < 1 || T > 63 || row_div < 1 || n < 1 || n > ISC_CIDER_MAX_ORDER) return ISC_E_SHAPE;
    if (capacity < 2 || (capacity & (capacity - 1))) return ISC_E_SHAPE;
    if (n_img < 1 || (N - 1) / row_div >= n_img) return ISC_E_SHAPE;      // every row's image has a reference range
    const int64_t blocks = (N + CIDER_WAVES - 1) / CIDER_WAVES;
    if (blocks > 0x7fffffffLL) return ISC_E_SHAPE;
    hipLaunchKernelGGL(cider_dev_kernel, dim3((unsigned)blocks), dim3(64 * CIDER_WAVES), 0, (hipStream_t)stream, hyp,
                       (long long)N, T, row_div, (const isc_cider_slot *)table, (uint64_t)capacity - 1, img_cap_off,
                       ord_off, ref_norms, ref_length, ref_keys, ref_vals, n, 2 * sigma * sigma, ref_len, sos_id,
                       eos_id, scores);
    ISC_LAUNCH_CHECK();
    return ISC_OK;
}
