// Back-off n-gram language models on the host (include/insenticap_cider.h, "n-gram language models"): the tables the
// device scorer reads (isc_lm_table_fill) and the host scorer (isc_lm_score) - the same walk as csrc/lm_dev.hip, position
// by position: float32 -> float64 conversions and float64 additions in a fixed order, so host and device agree in bits.
// The definition (DESIGN.md "Per-sentiment n-gram language models") is restated without tables in tests/_lm_ref.py.
#include <algorithm>
#include <cmath>
#include <cstdint>
#include <limits>
#include <thread>
#include <vector>

#include "../../include/insenticap_cider.h"
#include "lm_slot.h"

extern "C" int64_t isc_lm_table_capacity(int64_t n) {
    if (n < 0) return -1;
    int64_t cap = 16;
    while (cap < 2 * n) cap <<= 1;
    return cap;
}

extern "C" int isc_lm_table_fill(const uint64_t *keys, const float *logp, const float *backoff, int64_t n,
                                 void *slots_out, int64_t capacity) {
    isc_lm_slot *slots = (isc_lm_slot *)slots_out;
    if (!slots || n < 0 || (n > 0 && (!keys || !logp || !backoff))) return -1;
    if (capacity < 2 || (capacity & (capacity - 1)) || capacity <= n) return -2;      // (one slot at least stays empty)
    const uint64_t mask = (uint64_t)capacity - 1;
    for (int64_t i = 0; i < capacity; ++i) slots[i].key = 0, slots[i].logp = 0.0f, slots[i].backoff = 0.0f;
    for (int64_t i = 0; i < n; ++i) {
        if (keys[i] == 0) return -3;
        uint64_t s = isc_cider_hash(keys[i]) & mask;
        while (slots[s].key) {
            if (slots[s].key == keys[i]) return -5;      // a duplicate
            s = (s + 1) & mask;
        }
        slots[s].key = keys[i];
        slots[s].logp = logp[i];
        slots[s].backoff = backoff[i];
    }
    return 0;
}

namespace {

struct LmArgs {
    const isc_lm_slot *slots;
    const int64_t *off, *cap;
    const int32_t *order;
    int n_lm, V, eos_word, unk_as_word;
    int64_t sos, eos;
};

// One row: what one wave of lm_dev_kernel does.  `w` is scratch for the fields (id + 1) of the scored words.
static void lm_score_row(const LmArgs &A, const int64_t *row, int64_t T, int64_t lab, std::vector<uint64_t> &w, double *score,
                         int32_t *n_scored, int32_t *n_oov, double *tok_logp) {
    if (tok_logp)
        for (int64_t i = 0; i < T + 2; ++i) tok_logp[i] = 0.0;
    if (lab < 0 || lab >= A.n_lm) {
        *score = std::numeric_limits<double>::quiet_NaN();
        if (n_scored) *n_scored = -1;
        if (n_oov) *n_oov = 0;
        return;
    }
    const isc_lm_slot *table = A.slots + A.off[lab];
    const uint64_t mask = (uint64_t)A.cap[lab] - 1;
    const int order = A.order[lab];
    // normalise: drop a leading <SOS>, cut at the first <EOS>, append <EOS>; then 'word': the <EOS> id stays a word and
    // </s> follows, 'end': the <EOS> becomes </s>
    w.clear();
    for (int64_t i = (T > 0 && row[0] == A.sos) ? 1 : 0; i < T && row[i] != A.eos; ++i) w.push_back((uint64_t)row[i]);
    if (A.eos_word) w.push_back((uint64_t)A.eos);
    for (auto &x : w) {
        const int64_t id = (int64_t)x;
        x = (uint64_t)((id >= 0 && id < A.V ? id : ISC_LM_NONE(A.V)) + 1);
    }
    w.push_back((uint64_t)(ISC_LM_EOS(A.V) + 1));
    const int64_t P = (int64_t)w.size();
    const uint64_t bos = (uint64_t)(ISC_LM_BOS(A.V) + 1);
    double s = 0.0;
    int scored = 0, oov = 0;
    for (int64_t i = 0; i < P; ++i) {
        const int ctx = (int)std::min<int64_t>(order - 1, i + 1);
        double acc = 0.0, val = 0.0;
        bool found = false;
        for (int len = ctx; len >= 0 && !found; --len) {
            uint64_t kc = 0;
            for (int j = 0; j < len; ++j) {
                const int64_t at = i - len + j;               // (-1: <s>)
                kc |= (at >= 0 ? w[at] : bos) << (16 * j);
            }
            const uint64_t kw = kc | (w[i] << (16 * len));
            const isc_lm_slot hit = isc_lm_find(table, mask, kw);
            if (hit.key) {
                val = (double)hit.logp + acc;
                found = true;
            } else if (len > 0) {
                const isc_lm_slot c = isc_lm_find(table, mask, kc);
                if (c.key) acc += (double)c.backoff;
            }
        }
        if (!found) {
            ++oov;
            if (A.unk_as_word) {
                const isc_lm_slot u = isc_lm_find(table, mask, (uint64_t)(ISC_LM_UNK(A.V) + 1));
                if (u.key) {
                    val = (double)u.logp + acc;
                    found = true;
                }
            }
        }
        if (!found) val = 0.0;
        scored += found ? 1 : 0;
        s += val;
        if (tok_logp) tok_logp[i] = val;
    }
    *score = s;
    if (n_scored) *n_scored = scored;
    if (n_oov) *n_oov = oov;
}

}  // namespace

extern "C" int isc_lm_score(const int64_t *hyp, int64_t N, int64_t T, const int64_t *labels, int n_lm, const void *slots,
                            int64_t n_slots, const int64_t *lm_off, const int64_t *lm_capacity, const int32_t *lm_order,
                            int V, int eos_mode, int unk_as_word, int64_t sos_id, int64_t eos_id, double *score,
                            int32_t *n_scored, int32_t *n_oov, double *tok_logp, int n_threads) {
    if (!hyp || !slots || !lm_off || !lm_capacity || !lm_order || !score) return -1;
    if (N < 1 || T < 1 || n_lm < 1 || V < 1 || V > ISC_LM_MAX_VOCAB || eos_mode < 0 || eos_mode > 1) return -4;
    for (int l = 0; l < n_lm; ++l) {      // every model's range lies inside the slot array: a probe cannot leave it
        const int64_t c = lm_capacity[l];
        if (c < 2 || (c & (c - 1)) || lm_off[l] < 0 || lm_off[l] > n_slots - c) return -2;
        if (lm_order[l] < 1 || lm_order[l] > ISC_CIDER_MAX_ORDER) return -2;
    }
    const LmArgs A = {(const isc_lm_slot *)slots, lm_off, lm_capacity, lm_order, n_lm, V, eos_mode == 0 ? 1 : 0,
                      unk_as_word ? 1 : 0, sos_id, eos_id};
    if (n_threads < 1) n_threads = 1;
    if (n_threads > 16) n_threads = 16;
    if ((int64_t)n_threads > N) n_threads = (int)N;
    auto work = [&](int tid) {
        std::vector<uint64_t> w;
        for (int64_t r = tid; r < N; r += n_threads)
            lm_score_row(A, hyp + r * T, T, labels ? labels[r] : 0, w, score + r, n_scored ? n_scored + r : nullptr,
                         n_oov ? n_oov + r : nullptr, tok_logp ? tok_logp + r * (T + 2) : nullptr);
    };
    if (n_threads == 1) {
        work(0);
    } else {
        std::vector<std::thread> th;
        for (int t = 0; t < n_threads; ++t) th.emplace_back(work, t);
        for (auto &t : th) t.join();
    }
    return 0;
}
