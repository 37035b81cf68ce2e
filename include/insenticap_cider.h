/*
 * insenticap_cider.h - C ABI of libinsenticap_cider.so: native CIDEr-D reward for the
 * self-critical RL step (host side of the hot path).
 *
 * Replaces the pure-Python scorer the reference calls once per RL iteration:
 *   self_critical/utils.py:11-21   _array_to_str      (strip <SOS>, cut at first <EOS>, append <EOS>)
 *   self_critical/utils.py:38-53   get_ciderd_scorer  (document frequencies over all GT captions)
 *   self_critical/utils.py:56-83   get_self_critical_reward
 *   self_critical/cider/pyciderevalcap/ciderD/ciderD_scorer.py:13-28,52-64,120-192
 * Token ids are used directly as n-gram symbols (the reference joins them into strings and
 * splits them again). All arithmetic is fp64 in the reference's order of operations, so scores
 * agree to the last bits; scoring is multi-threaded over hypotheses.
 *
 * Captions are passed flattened: `tokens` holds all ids back to back, caption c is
 * tokens[cap_off[c] .. cap_off[c+1]), image i owns captions [img_off[i] .. img_off[i+1]).
 */
#ifndef INSENTICAP_CIDER_H
#define INSENTICAP_CIDER_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef struct isc_cider isc_cider;

/* Build the document-frequency table from the ground-truth captions of all images
 * (CiderScorer.update_df). n = max n-gram order (4), sigma = length-penalty width (6.0). */
isc_cider *isc_cider_create(const int64_t *tokens, const int64_t *cap_off, const int64_t *img_off,
                            int64_t n_imgs, int64_t sos_id, int64_t eos_id, int n, double sigma);
void isc_cider_destroy(isc_cider *h);

/* Number of images and distinct n-grams in the document-frequency table (diagnostics). */
int64_t isc_cider_num_images(const isc_cider *h);
int64_t isc_cider_num_ngrams(const isc_cider *h);

/* CIDEr-D score of n_hyp hypotheses (hyp[i*hyp_stride .. +T), raw roll-out rows) against their
 * own reference captions (flattened like above, hypothesis i owns captions
 * [ref_img_off[i] .. ref_img_off[i+1])).  scores_out[n_hyp] (already x10, mean over refs).
 * Returns 0, or -1 on a null pointer, -2 on a hypothesis without references. */
int isc_cider_score(const isc_cider *h, const int64_t *hyp, int64_t n_hyp, int64_t T,
                    int64_t hyp_stride, const int64_t *ref_tokens, const int64_t *ref_cap_off,
                    const int64_t *ref_img_off, double *scores_out, int n_threads);

/* ---- What the device scorer (isc_cider_dev_score, include/insenticap_hip.h) reads, prepared here.
 * The n-gram key, its hash and the 16-byte slot {uint64 key, double log_df} are defined once, in
 * csrc/cider_key.h: field j (16 bits) of a key holds id_j + 1, unused fields hold 0, key 0 = empty
 * slot.  Every id must lie in [0, 65534]: where one does not, the functions below return -3. */

/* log(number of images), the maximal order n and sigma of the scorer.  0, or -1 on a null pointer. */
int isc_cider_params(const isc_cider *h, double *ref_len, int *n, double *sigma);

/* The document frequencies as an open-addressing array with linear probing: home slot
 * isc_cider_hash(key) & (capacity - 1), log_df = log(max(1, df)) (the `d` of counts2vec).
 * isc_cider_table_capacity: the smallest power of two >= max(16, 2 x isc_cider_num_ngrams).
 * isc_cider_table_fill writes `capacity` slots; any power of two above the number of n-grams is
 * taken (tests fill a tighter table).  0, -1 null pointer, -2 bad capacity, -3 id out of range. */
int64_t isc_cider_table_capacity(const isc_cider *h);
int isc_cider_table_fill(const isc_cider *h, void *slots, int64_t capacity);

/* Cooked captions: for each of n_caps captions (flattened as above) its distinct n-grams in the
 * scorer's first-occurrence order - all 1-grams by position, then the 2-grams, ... - as keys[] and
 * the tf-idf vals[] of counts2vec, back to back over the captions; ord_off[5 c + o] = index of
 * caption c's first entry of order o + 1, ord_off[5 c + 4] = one past its last; norms[4 c + o]
 * and length[c] as counts2vec forms them - the values the host scorer uses, bit for bit.
 * isc_cider_cook_size returns the number of entries, isc_cider_cook_fill fills and returns it;
 * negative: -1 null pointer, -2 more than 2^31 - 1 entries, -3 id out of range. */
int64_t isc_cider_cook_size(const isc_cider *h, const int64_t *tokens, const int64_t *cap_off,
                            int64_t n_caps);
int64_t isc_cider_cook_fill(const isc_cider *h, const int64_t *tokens, const int64_t *cap_off,
                            int64_t n_caps, uint64_t *keys, double *vals, int32_t *ord_off,
                            double *norms, double *length);

/* ---- BLEU, the reference's other self-critical scorer (self_critical/bleu/bleu.py, bleu_scorer.py).
 * It keeps no document frequencies, hence no handle.  Rows and references are normalised as above
 * (_array_to_str); per row the integer statistics of cook_refs / cook_test (bleu_scorer.py:38-86):
 *   testlen; reflen = the "closest" reference length, min((abs(l - testlen), l)) - a tie takes the
 *   shorter; guess[k] = max(0, testlen - k); correct[k] = sum over the row's distinct (k+1)-grams of
 *   min(count in the row, max over the image's references of the count in that reference);
 * and the four per-sentence scores in compute_score's order of operations (bleu_scorer.py:233-242):
 * the running product of (correct + 1e-15) / (guess + 1e-9), ** (1 / (k + 1)), and, where
 * ratio = (testlen + 1e-15) / (reflen + 1e-9) < 1, *= exp(1 - 1 / ratio).  fp64, no contraction.
 *   hyp: n_hyp rows of T ids, row r at hyp + r * hyp_stride, belongs to image r / row_div;
 *   the references flattened as for isc_cider_score, n_imgs images (ref_img_off has n_imgs + 1);
 *   scores4 [n_hyp, 4] = BLEU-1 .. BLEU-4; stats [n_hyp, 10] int32 = testlen, reflen, guess[0..3],
 *   correct[0..3], or NULL.
 * Up to n_threads threads, each image's references cooked once; the result does not depend on the
 * thread count.  0, -1 null pointer, -2 an image (that owns a row) without references, -4 bad shape
 * (n_hyp < 1, row_div < 1, fewer than ceil(n_hyp / row_div) images). */
int isc_bleu_score(const int64_t *hyp, int64_t n_hyp, int64_t T, int64_t hyp_stride,
                   const int64_t *ref_tokens, const int64_t *ref_cap_off, const int64_t *ref_img_off,
                   int64_t n_imgs, int64_t row_div, int64_t sos_id, int64_t eos_id, int n_threads,
                   double *scores4, int32_t *stats);

/* ONE image's references (n_caps captions, flattened as above) cooked for the device scorer
 * (isc_bleu_dev_score): the distinct n-grams over all of them as csrc/cider_key.h keys with their
 * largest count in one reference, grouped by order - within an order: references ascending, first
 * occurrence within a reference - ent_off[o] = first entry of order o + 1, ent_off[4] = the number of
 * entries; ref_lens[c] = words of caption c after normalisation.  isc_bleu_cook_size returns the
 * number of entries, isc_bleu_cook_fill fills and returns it; negative: -1 null pointer, -2 more than
 * 2^31 - 1 entries, -3 id out of [0, 65534]. */
int64_t isc_bleu_cook_size(const int64_t *tokens, const int64_t *cap_off, int64_t n_caps,
                           int64_t sos_id, int64_t eos_id);
int64_t isc_bleu_cook_fill(const int64_t *tokens, const int64_t *cap_off, int64_t n_caps,
                           int64_t sos_id, int64_t eos_id, uint64_t *keys, int32_t *counts,
                           int32_t *ent_off, int32_t *ref_lens);

/* ---- n-gram language models (per-sentiment ARPA models of order <= 4: the `ppl` metric and the LM reward of
 * self_critical/utils.py:86-100).  An ARPA file is parsed in Python (rewards.read_arpa); here its n-grams arrive as
 * csrc/cider_key.h keys - the OLDEST word in field 0 - with logp and backoff already rounded to float32 (a missing
 * back-off weight is +0.0).  With V vocabulary words, <s>, </s>, <unk> are the ids V, V + 1, V + 2 and V + 3 is "no
 * word" (what a token outside [0, V) becomes; no table holds it): V <= 65531.  Slot (csrc/lm_slot.h, 16 bytes):
 * {uint64 key; float logp; float backoff}, key 0 = empty; home slot isc_cider_hash(key) & (capacity - 1), linear probing.
 *
 * isc_lm_table_capacity(n): the smallest power of two >= max(16, 2 n).  isc_lm_table_fill writes `capacity` slots; any
 * power of two above n is taken (tests fill a tighter table; one slot at least stays empty).  0, -1 null pointer, -2 bad
 * capacity, -3 a key 0, -5 a duplicate key. */
int64_t isc_lm_table_capacity(int64_t n);
int isc_lm_table_fill(const uint64_t *keys, const float *logp, const float *backoff, int64_t n, void *slots,
                      int64_t capacity);

/* Host scorer: the inputs and outputs of isc_lm_dev_score (include/insenticap_hip.h), all in host memory, plus n_slots,
 * the length of the slot array.  Several models lie in ONE slot array, model l in lm_off[l] .. lm_off[l] + lm_capacity[l]
 * with order lm_order[l]; a probe wraps inside its own model's range.  Row r (hyp + r T, normalised as isc_cider_score
 * normalises) is scored by model labels[r] (labels == NULL: model 0):
 *   eos_mode 0 ('word'): the <EOS> id is scored as a word, then </s>;  1 ('end'): the <EOS> becomes </s>;
 *   the value of a word after its context (the last order - 1 words, starting at <s>): from the longest context c to the
 *   empty one - c.w in the table: (double)logp(c.w) + acc; otherwise acc += (double)backoff(c) where c is in the table,
 *   and the oldest word of c is dropped; acc starts at 0.0.  A word without a unigram is out of vocabulary: with
 *   unk_as_word and an <unk> unigram it scores logp(<unk>) + acc, otherwise it is skipped (value 0.0, not in n_scored);
 *   score[r] = the float64 sum of the values over the positions in ascending order (log10); n_scored[r], n_oov[r] (or
 *   NULL); tok_logp [N, T + 2] (or NULL): the value per position, 0.0 where skipped and behind the sentence.
 * A label outside [0, n_lm): score NaN, n_scored -1, n_oov 0.  Up to min(n_threads, 16) threads; the result does not
 * depend on their number and equals the device scorer's in bits.
 * 0, -1 null pointer, -2 a bad table description (capacity no power of two >= 2, a range outside the slot array, an order
 * outside [1, 4]), -4 bad shape (N < 1, T < 1, n_lm < 1, V outside [1, 65531], eos_mode outside {0, 1}). */
int isc_lm_score(const int64_t *hyp, int64_t N, int64_t T, const int64_t *labels, int n_lm, const void *slots,
                 int64_t n_slots, const int64_t *lm_off, const int64_t *lm_capacity, const int32_t *lm_order, int V,
                 int eos_mode, int unk_as_word, int64_t sos_id, int64_t eos_id, double *score, int32_t *n_scored,
                 int32_t *n_oov, double *tok_logp, int n_threads);

#ifdef __cplusplus
}
#endif
#endif
