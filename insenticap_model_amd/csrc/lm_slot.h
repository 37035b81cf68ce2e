// The slot of the n-gram language-model tables and the ids of the special words: ONE definition, included by cider.cpp
// (g++: fills the tables, host scorer isc_lm_score) and by lm_dev.hip (hipcc: isc_lm_dev_score).  The key of an n-gram
// and its hash are cider_key.h's, unchanged: field j holds id_j + 1, the OLDEST word of the n-gram in field 0.
//
// With a vocabulary of V words (ids 0 .. V - 1) the words an ARPA file adds take the ids behind it:
//   <s> = V, </s> = V + 1, <unk> = V + 2, and V + 3 = "no word": what a token id outside [0, V) becomes - no table ever
// holds it, so it matches nothing and cannot alias a special.  V + 3 <= ISC_CIDER_MAX_ID, hence V <= 65531.
#ifndef INSENTICAP_LM_SLOT_H
#define INSENTICAP_LM_SLOT_H

#include "cider_key.h"

#define ISC_LM_MAX_VOCAB (ISC_CIDER_MAX_ID - 3)      /* 65531 */
#define ISC_LM_MAX_T 62                              /* T + 2 scored positions (eos_mode 'word') fit 64 lanes */
#define ISC_LM_BOS(V) ((int64_t)(V))
#define ISC_LM_EOS(V) ((int64_t)(V) + 1)
#define ISC_LM_UNK(V) ((int64_t)(V) + 2)
#define ISC_LM_NONE(V) ((int64_t)(V) + 3)

/* One slot: 16 bytes.  key == 0: empty.  logp / backoff: the ARPA decimals (log10) rounded once to float32; an n-gram
 * without a back-off weight holds +0.0. */
typedef struct {
    uint64_t key;
    float logp;
    float backoff;
} isc_lm_slot;

/* The slot of `key` among the `mask + 1` slots at `table` (linear probing from the key's home slot, wrapping inside this
 * range), or a slot with key 0 when the table does not hold it.  At most mask + 1 probes: a table without an empty slot
 * (a damaged one) ends the walk as "absent". */
ISC_CIDER_HD isc_lm_slot isc_lm_find(const isc_lm_slot *table, uint64_t mask, uint64_t key) {
    uint64_t s = isc_cider_hash(key) & mask;
    for (uint64_t p = 0; p <= mask; ++p) {
        const isc_lm_slot slot = table[s];
        if (slot.key == key) return slot;
        if (slot.key == 0) break;
        s = (s + 1) & mask;
    }
    isc_lm_slot none;
    none.key = 0, none.logp = 0.0f, none.backoff = 0.0f;
    return none;
}

#endif
