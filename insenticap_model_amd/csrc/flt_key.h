// The rank key of the filtered sampling (temperature / top-k / top-p): ONE definition, read by the forward that decides a
// row's kept set (pointwise.hip: rollout_finalize_filtered_body) and by the backward that differentiates the sampled
// distribution's log-probability (backward.hip: logsoftmax_bwd_raw_filtered_kernel).  Both must agree on every bit of it:
// the backward re-derives "v is kept" from the saved boundary key K* alone.
#pragma once

typedef unsigned long long isc_u64;

// ids a row may not choose at one step (isc_decode_constraints: 8 caller ids, <EOS> under min_len, the previous token)
#define ISC_CON_MAX 10

// K = (descending image of x : id): larger x -> smaller K, equal x -> the smaller id first; all keys of a row distinct.
__device__ __forceinline__ isc_u64 flt_key(float x, int i) {
    unsigned b = __float_as_uint(x);
    if (b == 0x80000000u) b = 0u;                                     // -0 ranks with +0
    const unsigned dk = (b & 0x80000000u) ? b : (~b & 0x7fffffffu);   // larger x -> smaller dk
    return ((isc_u64)dk << 32) | (unsigned)i;
}
