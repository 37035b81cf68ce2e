// Sentiment-word reward on the device (isc_sw_reward, isc_sw_decay): the reference's get_senti_words_reward
// (self_critical/utils.py:154-166) and the decay of the used words (models/decoder.py:174-176) on a dense lexicon table -
// weights float64 [n_labels, V] and state uint8 [n_labels, V] (0 = not in the lexicon, 1 = in it, 2 = in it and used since
// the last decay).  One wave64 per row, lanes stride over the positions; one random 1-byte read per position and an 8-byte
// read per hit.  No LDS, no atomics, no workspace, no barrier: the waves of a workgroup are independent.  The marks are
// plain vector stores of the constant 2 - many lanes and rows may store it to the same byte, nothing is read-modify-written.
#include "common.h"

#pragma clang fp contract(off)

#define SW_WAVES 4      // rows per workgroup

__global__ __launch_bounds__(64 * SW_WAVES) void sw_reward_kernel(
    const int64_t *__restrict__ tok, long long N, int T, const int64_t *__restrict__ labels, int n_labels, int V,
    const double *__restrict__ weights, uint8_t *state, float flag, float *reward_io, int accumulate,
    double *__restrict__ reward64, int32_t *__restrict__ row_hits, int mark) {
#pragma clang fp contract(off)
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    const long long r = (long long)blockIdx.x * SW_WAVES + wave;
    if (r >= N) return;                                   // (the whole wave leaves: nothing below waits for it)

    const long long lab = labels[r];                      // (the same in every lane)
    if (lab < 0 || lab >= n_labels) {                     // no such lexicon: no table is read, nothing is marked
        for (int j = lane; j < T; j += 64) {
            if (reward_io) reward_io[r * T + j] = __int_as_float(0x7fc00000);
            if (reward64) reward64[r * T + j] = __longlong_as_double(0x7ff8000000000000LL);
        }
        if (row_hits && lane == 0) row_hits[r] = -1;
        return;
    }
    const size_t base = (size_t)lab * (size_t)V;
    int hits = 0;
    for (int j0 = 0; j0 < T; j0 += 64) {                  // (uniform trip count: the ballot below sees every lane)
        const int j = j0 + lane;
        const bool active = j < T;
        const int64_t id = active ? tok[r * T + j] : -1;  // compared as a 64-bit integer before it becomes an index
        bool hit = false;
        double w = 0.0;
        if (id >= 0 && id < V) {
            const size_t at = base + (size_t)id;
            if (state[at] != 0) {
                hit = true;
                w = weights[at];
                if (mark) state[at] = 2;
            }
        }
        hits += __popcll(__ballot(hit));
        if (active) {
            if (reward64) reward64[r * T + j] = w;
            if (reward_io) {
                const float wf = (float)w;                // rounded once
                // accumulate: the product is rounded to float32 before the addition - plain operators under this file's
                // `fp contract(off)` (the __fmul_rn / __fadd_rn of the HIP headers are plain operators compiled under the
                // headers' own contraction mode: inlined here they were fused into one v_fma_f32)
                if (accumulate) {
                    const float p = flag * wf;
                    reward_io[r * T + j] = reward_io[r * T + j] + p;
                } else {
                    reward_io[r * T + j] = wf;
                }
            }
        }
    }
    if (row_hits && lane == 0) row_hits[r] = hits;
}

__global__ __launch_bounds__(256) void sw_decay_kernel(double *__restrict__ weights, uint8_t *__restrict__ state,
                                                       long long n, double factor) {
    const long long stride = (long long)gridDim.x * blockDim.x;
    for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += stride)
        if (state[i] == 2) {
            weights[i] = weights[i] * factor;
            state[i] = 1;
        }
}

extern "C" int isc_sw_reward(const int64_t *tok, int64_t N, int T, const int64_t *labels, int n_labels, int V,
                             const double *weights, uint8_t *state, double flag, float *reward_io, int accumulate,
                             double *reward64, int32_t *row_hits, int mark, void *stream) {
    if (!tok || !labels || !weights || !state) return ISC_E_NULL;
    if (N < 1 || T < 1 || n_labels < 1 || V < 1) return ISC_E_SHAPE;
    const int64_t blocks = (N + SW_WAVES - 1) / SW_WAVES;
    if (blocks > 0x7fffffffLL) return ISC_E_SHAPE;
    hipLaunchKernelGGL(sw_reward_kernel, dim3((unsigned)blocks), dim3(64 * SW_WAVES), 0, (hipStream_t)stream, tok,
                       (long long)N, T, labels, n_labels, V, weights, state, (float)flag, reward_io, accumulate ? 1 : 0,
                       reward64, row_hits, mark ? 1 : 0);
    ISC_LAUNCH_CHECK();
    return ISC_OK;
}

extern "C" int isc_sw_decay(double *weights, uint8_t *state, int64_t n, double factor, void *stream) {
    if (!weights || !state) return ISC_E_NULL;
    if (n < 1) return ISC_E_SHAPE;
    int64_t blocks = (n + 255) / 256;
    if (blocks > 1024) blocks = 1024;                     // (grid-stride beyond that)
    hipLaunchKernelGGL(sw_decay_kernel, dim3((unsigned)blocks), dim3(256), 0, (hipStream_t)stream, weights, state,
                       (long long)n, factor);
    ISC_LAUNCH_CHECK();
    return ISC_OK;
}
