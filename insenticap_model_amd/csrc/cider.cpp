// Native CIDEr-D (host C++), see include/insenticap_cider.h.  Exact fp64 port of the scorer the
// reference runs in pure Python once per RL iteration (ciderD_scorer.py:120-192), keeping its
// order of operations: n-grams are visited in first-occurrence order (Python dict insertion
// order: all 1-grams by position, then 2-grams, ...), per-order norms and clipped dot products are
// accumulated in that order, the four per-order similarities are summed over the references in
// reference order, then mean over n, / #refs, * 10.
#include <cmath>
#include <cstdint>
#include <algorithm>
#include <cstring>
#include <thread>
#include <unordered_map>
#include <vector>

#include "../../include/insenticap_cider.h"
#include "cider_key.h"

namespace {

struct NGram {
    int64_t w[4];
    int n;  // order 1..4
    bool operator==(const NGram &o) const {
        if (n != o.n) return false;
        for (int i = 0; i < n; ++i)
            if (w[i] != o.w[i]) return false;
        return true;
    }
};
struct NGramHash {
    size_t operator()(const NGram &g) const {
        uint64_t h = 0x9E3779B97F4A7C15ull * (uint64_t)g.n;
        for (int i = 0; i < g.n; ++i) {
            h ^= (uint64_t)g.w[i] + 0x9E3779B97F4A7C15ull + (h << 6) + (h >> 2);
            h *= 0xBF58476D1CE4E5B9ull;
        }
        return (size_t)(h ^ (h >> 31));
    }
};

// Small open-addressing index over the n-grams of ONE caption (<= a few hundred entries); buffers
// are reused across captions so the scoring loop performs no heap allocation.
struct LocalIndex {
    std::vector<int> slot;   // -1 = empty, else index into keys
    size_t mask = 0;
    void reset(size_t n_items) {
        size_t cap = 64;
        while (cap < 4 * n_items) cap <<= 1;
        if (slot.size() != cap) slot.assign(cap, -1);
        else std::fill(slot.begin(), slot.end(), -1);
        mask = cap - 1;
    }
    // returns the position of g in keys, or -1 (and, if `insert_as` >= 0, records it)
    int find(const std::vector<NGram> &keys, const NGram &g, int insert_as) {
        size_t h = NGramHash()(g) & mask;
        for (;;) {
            const int s = slot[h];
            if (s < 0) {
                if (insert_as >= 0) slot[h] = insert_as;
                return -1;
            }
            if (keys[s] == g) return s;
            h = (h + 1) & mask;
        }
    }
};

// counts in first-occurrence order (precook, ciderD_scorer.py:13-28)
struct Cooked {
    std::vector<NGram> keys;
    std::vector<double> tf;
    LocalIndex index;
};

// _array_to_str (self_critical/utils.py:11-21): drop a leading <SOS>, stop at the first <EOS>, append <EOS>
static void normalise(const int64_t *arr, int64_t len, int64_t sos, int64_t eos, std::vector<int64_t> &out) {
    out.clear();
    int64_t i = 0;
    if (len > 0 && arr[0] == sos) i = 1;
    for (; i < len; ++i) {
        if (arr[i] == eos) break;
        out.push_back(arr[i]);
    }
    out.push_back(eos);
}

static void precook(const std::vector<int64_t> &words, int n, Cooked &c) {
    c.keys.clear();
    c.tf.clear();
    const int64_t L = (int64_t)words.size();
    c.index.reset((size_t)(n * L));
    for (int k = 1; k <= n; ++k)
        for (int64_t i = 0; i + k <= L; ++i) {
            NGram g;
            g.n = k;
            for (int j = 0; j < 4; ++j) g.w[j] = j < k ? words[i + j] : 0;
            const int at = c.index.find(c.keys, g, (int)c.keys.size());
            if (at < 0) {
                c.keys.push_back(g);
                c.tf.push_back(1.0);
            } else {
                c.tf[at] += 1.0;
            }
        }
}

struct Vec {  // counts2vec result; keys / index live in the Cooked it was built from
    std::vector<double> val;
    double norm[4];
    double length;
};

struct Scratch {  // per-thread buffers
    std::vector<int64_t> words;
    Cooked hyp, ref;
    Vec vh, vr;
};

}  // namespace

struct isc_cider {
    std::unordered_map<NGram, double, NGramHash> df;
    double ref_len;
    int64_t n_imgs, sos, eos;
    int n;
    double sigma;

    void counts2vec(const Cooked &c, Vec &v) const {
        v.val.resize(c.keys.size());
        for (int i = 0; i < 4; ++i) v.norm[i] = 0.0;
        v.length = 0.0;
        for (size_t i = 0; i < c.keys.size(); ++i) {
            const NGram &g = c.keys[i];
            auto it = df.find(g);
            const double d = std::log(std::fmax(1.0, it == df.end() ? 0.0 : it->second));
            const int o = g.n - 1;
            const double x = c.tf[i] * (ref_len - d);
            v.val[i] = x;
            v.norm[o] += std::pow(x, 2);
            if (o == 1) v.length += c.tf[i];  // "length" counts bigrams (ciderD_scorer.py:142-143)
        }
        for (int i = 0; i < 4; ++i) v.norm[i] = std::sqrt(v.norm[i]);
    }

    double score_one(Scratch &S, const int64_t *hyp, int64_t T, const int64_t *rtok, const int64_t *rcap,
                     int64_t c0, int64_t c1) const {
        normalise(hyp, T, sos, eos, S.words);
        precook(S.words, n, S.hyp);
        counts2vec(S.hyp, S.vh);
        double score[4] = {0, 0, 0, 0};
        for (int64_t c = c0; c < c1; ++c) {
            normalise(rtok + rcap[c], rcap[c + 1] - rcap[c], sos, eos, S.words);
            precook(S.words, n, S.ref);
            counts2vec(S.ref, S.vr);
            const double delta = S.vh.length - S.vr.length;
            double val[4] = {0, 0, 0, 0};
            for (size_t i = 0; i < S.hyp.keys.size(); ++i) {
                const int o = S.hyp.keys[i].n - 1;
                const int at = S.ref.index.find(S.ref.keys, S.hyp.keys[i], -1);
                const double r = at < 0 ? 0.0 : S.vr.val[at];
                val[o] += std::fmin(S.vh.val[i], r) * r;  // clipped (ciderD_scorer.py:164)
            }
            const double pen = std::pow(M_E, -(delta * delta) / (2 * sigma * sigma));
            for (int o = 0; o < n; ++o) {
                if (S.vh.norm[o] != 0 && S.vr.norm[o] != 0) val[o] /= (S.vh.norm[o] * S.vr.norm[o]);
                val[o] *= pen;
                score[o] += val[o];
            }
        }
        double s = 0.0;
        for (int o = 0; o < n; ++o) s += score[o];
        s /= (double)n;
        s /= (double)(c1 - c0);
        return s * 10.0;
    }
};

extern "C" isc_cider *isc_cider_create(const int64_t *tokens, const int64_t *cap_off, const int64_t *img_off,
                                       int64_t n_imgs, int64_t sos_id, int64_t eos_id, int n, double sigma) {
    if (!tokens || !cap_off || !img_off || n_imgs <= 0 || n < 1 || n > 4) return nullptr;
    isc_cider *h = new isc_cider();
    h->n_imgs = n_imgs; h->sos = sos_id; h->eos = eos_id; h->n = n; h->sigma = sigma;
    h->ref_len = std::log((double)n_imgs);
    std::vector<int64_t> words;
    Cooked ck;
    for (int64_t i = 0; i < n_imgs; ++i) {
        // every n-gram counts once per image, whichever of its references contain it (compute_doc_freq)
        std::unordered_map<NGram, char, NGramHash> seen;
        for (int64_t c = img_off[i]; c < img_off[i + 1]; ++c) {
            normalise(tokens + cap_off[c], cap_off[c + 1] - cap_off[c], sos_id, eos_id, words);
            precook(words, n, ck);
            for (const NGram &g : ck.keys) seen.emplace(g, 1);
        }
        for (auto &kv : seen) h->df[kv.first] += 1.0;
    }
    return h;
}

extern "C" void isc_cider_destroy(isc_cider *h) { delete h; }
extern "C" int64_t isc_cider_num_images(const isc_cider *h) { return h ? h->n_imgs : 0; }
extern "C" int64_t isc_cider_num_ngrams(const isc_cider *h) { return h ? (int64_t)h->df.size() : 0; }

extern "C" int isc_cider_score(const isc_cider *h, const int64_t *hyp, int64_t n_hyp, int64_t T,
                               int64_t hyp_stride, const int64_t *ref_tokens, const int64_t *ref_cap_off,
                               const int64_t *ref_img_off, double *scores_out, int n_threads) {
    if (!h || !hyp || !ref_tokens || !ref_cap_off || !ref_img_off || !scores_out) return -1;
    for (int64_t i = 0; i < n_hyp; ++i)
        if (ref_img_off[i + 1] <= ref_img_off[i]) return -2;
    if (n_threads < 1) n_threads = 1;
    if ((int64_t)n_threads > n_hyp) n_threads = (int)n_hyp;
    auto work = [&](int tid) {
        Scratch S;
        for (int64_t i = tid; i < n_hyp; i += n_threads)
            scores_out[i] = h->score_one(S, hyp + i * hyp_stride, T, ref_tokens, ref_cap_off, ref_img_off[i],
                                         ref_img_off[i + 1]);
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

// ------------------------------------------------------------------ exports for the device scorer (csrc/cider_dev.hip)
// The device scores a hypothesis from two things the host prepares with the functions above: the document-frequency
// table as an open-addressing array of (key, log df) slots, and the references "cooked" - their distinct n-grams in
// first-occurrence order with the tf-idf values, norms and length counts2vec forms.  Keys and hash: cider_key.h.
static bool key_of(const NGram &g, uint64_t *key) {
    for (int j = 0; j < g.n; ++j)
        if (g.w[j] < 0 || g.w[j] > ISC_CIDER_MAX_ID) return false;
    *key = isc_cider_key(g.w, g.n);
    return true;
}

extern "C" int isc_cider_params(const isc_cider *h, double *ref_len, int *n, double *sigma) {
    if (!h || !ref_len || !n || !sigma) return -1;
    *ref_len = h->ref_len; *n = h->n; *sigma = h->sigma;
    return 0;
}

extern "C" int64_t isc_cider_table_capacity(const isc_cider *h) {
    if (!h) return -1;
    int64_t cap = 16;
    while (cap < 2 * (int64_t)h->df.size()) cap <<= 1;
    return cap;
}

extern "C" int isc_cider_table_fill(const isc_cider *h, void *slots_out, int64_t capacity) {
    isc_cider_slot *slots = (isc_cider_slot *)slots_out;
    if (!h || !slots) return -1;
    if (capacity < 2 || (capacity & (capacity - 1)) || capacity <= (int64_t)h->df.size()) return -2;
    const uint64_t mask = (uint64_t)capacity - 1;
    for (int64_t i = 0; i < capacity; ++i) slots[i].key = 0, slots[i].log_df = 0.0;
    for (const auto &kv : h->df) {
        uint64_t key;
        if (!key_of(kv.first, &key)) return -3;
        uint64_t s = isc_cider_hash(key) & mask;
        while (slots[s].key) s = (s + 1) & mask;          // (an empty slot exists: capacity > number of n-grams)
        slots[s].key = key;
        slots[s].log_df = std::log(std::fmax(1.0, kv.second));
    }
    return 0;
}

// One pass over `n_caps` captions; with keys == nullptr only the number of entries is counted.
static int64_t cook(const isc_cider *h, const int64_t *tokens, const int64_t *cap_off, int64_t n_caps, uint64_t *keys,
                    double *vals, int32_t *ord_off, double *norms, double *length) {
    Scratch S;
    int64_t at = 0;
    for (int64_t c = 0; c < n_caps; ++c) {
        normalise(tokens + cap_off[c], cap_off[c + 1] - cap_off[c], h->sos, h->eos, S.words);
        precook(S.words, h->n, S.ref);
        const int64_t m = (int64_t)S.ref.keys.size();
        if (at + m > 0x7fffffffLL) return -2;
        if (keys) {
            h->counts2vec(S.ref, S.vr);
            int32_t *off = ord_off + 5 * c;
            int order = 0;                                // precook lists all 1-grams, then all 2-grams, ...
            off[0] = (int32_t)at;
            for (int64_t i = 0; i < m; ++i) {
                if (!key_of(S.ref.keys[i], keys + at + i)) return -3;
                while (order < S.ref.keys[i].n - 1) off[++order] = (int32_t)(at + i);
                vals[at + i] = S.vr.val[i];
            }
            while (order < 4) off[++order] = (int32_t)(at + m);
            for (int o = 0; o < 4; ++o) norms[4 * c + o] = S.vr.norm[o];
            length[c] = S.vr.length;
        } else {
            uint64_t key;
            for (int64_t i = 0; i < m; ++i)
                if (!key_of(S.ref.keys[i], &key)) return -3;
        }
        at += m;
    }
    return at;
}

extern "C" int64_t isc_cider_cook_size(const isc_cider *h, const int64_t *tokens, const int64_t *cap_off, int64_t n_caps) {
    if (!h || !tokens || !cap_off || n_caps < 0) return -1;
    return cook(h, tokens, cap_off, n_caps, nullptr, nullptr, nullptr, nullptr, nullptr);
}

extern "C" int64_t isc_cider_cook_fill(const isc_cider *h, const int64_t *tokens, const int64_t *cap_off, int64_t n_caps,
                                       uint64_t *keys, double *vals, int32_t *ord_off, double *norms, double *length) {
    if (!h || !tokens || !cap_off || n_caps < 0 || !keys || !vals || !ord_off || !norms || !length) return -1;
    return cook(h, tokens, cap_off, n_caps, keys, vals, ord_off, norms, length);
}

// ------------------------------------------------------------------------------------------------------------- BLEU
// The reference's other self-critical scorer (self_critical/bleu/bleu_scorer.py), on the same normalised rows.  Its
// statistics are integers - testlen, the "closest" reference length, guess[k] = max(0, testlen - k) and correct[k] =
// the sum over the row's distinct (k+1)-grams of min(count in the row, max over the references of the count there)
// (cook_refs / cook_test, :38-86) - and the four scores follow compute_score's order of operations (:233-242).
namespace {

// The distinct n-grams over ALL references of one image with their largest count in one reference (cook_refs'
// `maxcounts`), in insertion order: references ascending, within one the order of precook; and the reference lengths.
struct RefMax {
    std::vector<NGram> keys;
    std::vector<int32_t> count;
    std::vector<int32_t> lens;
    LocalIndex index;
};

struct BleuScratch {
    std::vector<int64_t> words;
    Cooked one;
    RefMax ref;
};

static void cook_image(BleuScratch &S, const int64_t *tokens, const int64_t *cap_off, int64_t c0, int64_t c1,
                       int64_t sos, int64_t eos) {
    RefMax &R = S.ref;
    R.keys.clear();
    R.count.clear();
    R.lens.clear();
    size_t total = 0;
    for (int64_t c = c0; c < c1; ++c) total += (size_t)(cap_off[c + 1] - cap_off[c]) + 1;
    R.index.reset(4 * total);
    for (int64_t c = c0; c < c1; ++c) {
        normalise(tokens + cap_off[c], cap_off[c + 1] - cap_off[c], sos, eos, S.words);
        precook(S.words, 4, S.one);
        R.lens.push_back((int32_t)S.words.size());
        for (size_t i = 0; i < S.one.keys.size(); ++i) {
            const int32_t cnt = (int32_t)S.one.tf[i];
            const int at = R.index.find(R.keys, S.one.keys[i], (int)R.keys.size());
            if (at < 0) {
                R.keys.push_back(S.one.keys[i]);
                R.count.push_back(cnt);
            } else if (cnt > R.count[at]) {
                R.count[at] = cnt;
            }
        }
    }
}

// stats10: testlen, reflen, guess[0..3], correct[0..3]
static void bleu_stats(BleuScratch &S, const int64_t *hyp, int64_t T, int64_t sos, int64_t eos, int32_t *st) {
    normalise(hyp, T, sos, eos, S.words);
    precook(S.words, 4, S.one);
    const int32_t testlen = (int32_t)S.words.size();
    int32_t best_d = 0, reflen = 0;
    for (size_t c = 0; c < S.ref.lens.size(); ++c) {      // min((abs(l - testlen), l)): a tie takes the shorter
        const int32_t l = S.ref.lens[c], d = l > testlen ? l - testlen : testlen - l;
        if (c == 0 || d < best_d || (d == best_d && l < reflen)) best_d = d, reflen = l;
    }
    st[0] = testlen;
    st[1] = reflen;
    for (int k = 0; k < 4; ++k) st[2 + k] = testlen - k > 0 ? testlen - k : 0, st[6 + k] = 0;
    for (size_t i = 0; i < S.one.keys.size(); ++i) {
        const int at = S.ref.index.find(S.ref.keys, S.one.keys[i], -1);
        if (at < 0) continue;
        const int32_t cnt = (int32_t)S.one.tf[i];
        st[6 + S.one.keys[i].n - 1] += cnt < S.ref.count[at] ? cnt : S.ref.count[at];
    }
}

// bleu_scorer.py:233-242 on one row's statistics
static void bleu_scores(const int32_t *st, double *out4) {
    const double small = 1e-9, tiny = 1e-15;
    double bleu = 1.0;
    for (int k = 0; k < 4; ++k) {
        bleu *= ((double)st[6 + k] + tiny) / ((double)st[2 + k] + small);
        out4[k] = std::pow(bleu, 1.0 / (double)(k + 1));
    }
    const double ratio = ((double)st[0] + tiny) / ((double)st[1] + small);
    if (ratio < 1) {
        const double pen = std::exp(1 - 1 / ratio);
        for (int k = 0; k < 4; ++k) out4[k] *= pen;
    }
}

}  // namespace

extern "C" int isc_bleu_score(const int64_t *hyp, int64_t n_hyp, int64_t T, int64_t hyp_stride,
                              const int64_t *ref_tokens, const int64_t *ref_cap_off, const int64_t *ref_img_off,
                              int64_t n_imgs, int64_t row_div, int64_t sos_id, int64_t eos_id, int n_threads,
                              double *scores4, int32_t *stats) {
    if (!hyp || !ref_tokens || !ref_cap_off || !ref_img_off || !scores4) return -1;
    if (n_hyp < 1 || T < 0 || row_div < 1 || n_imgs < 1 || (n_hyp - 1) / row_div >= n_imgs) return -4;
    const int64_t used = (n_hyp - 1) / row_div + 1;      // images that own a row
    for (int64_t i = 0; i < used; ++i)
        if (ref_img_off[i + 1] <= ref_img_off[i]) return -2;
    if (n_threads < 1) n_threads = 1;
    if ((int64_t)n_threads > used) n_threads = (int)used;
    auto work = [&](int tid) {      // an image's references are cooked once for its row_div rows
        BleuScratch S;
        int32_t st[10];
        for (int64_t i = tid; i < used; i += n_threads) {
            cook_image(S, ref_tokens, ref_cap_off, ref_img_off[i], ref_img_off[i + 1], sos_id, eos_id);
            const int64_t r1 = std::min(n_hyp, (i + 1) * row_div);
            for (int64_t r = i * row_div; r < r1; ++r) {
                bleu_stats(S, hyp + r * hyp_stride, T, sos_id, eos_id, st);
                bleu_scores(st, scores4 + 4 * r);
                if (stats) std::memcpy(stats + 10 * r, st, sizeof(st));
            }
        }
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

// One image's references cooked for the device (csrc/bleu_dev.hip): with keys == nullptr only the entries are counted.
static int64_t bleu_cook(const int64_t *tokens, const int64_t *cap_off, int64_t n_caps, int64_t sos, int64_t eos,
                         uint64_t *keys, int32_t *counts, int32_t *ent_off, int32_t *ref_lens) {
    BleuScratch S;
    cook_image(S, tokens, cap_off, 0, n_caps, sos, eos);
    const int64_t m = (int64_t)S.ref.keys.size();
    if (m > 0x7fffffffLL) return -2;
    int64_t at = 0;
    for (int o = 0; o < 4; ++o) {                             // grouped by order, insertion order within one
        if (keys) ent_off[o] = (int32_t)at;
        for (int64_t i = 0; i < m; ++i) {
            if (S.ref.keys[i].n != o + 1) continue;
            uint64_t key;
            if (!key_of(S.ref.keys[i], &key)) return -3;
            if (keys) keys[at] = key, counts[at] = S.ref.count[i];
            ++at;
        }
    }
    if (keys) {
        ent_off[4] = (int32_t)at;
        for (int64_t c = 0; c < n_caps; ++c) ref_lens[c] = S.ref.lens[c];
    }
    return at;
}

extern "C" int64_t isc_bleu_cook_size(const int64_t *tokens, const int64_t *cap_off, int64_t n_caps, int64_t sos_id,
                                      int64_t eos_id) {
    if (!tokens || !cap_off || n_caps < 0) return -1;
    return bleu_cook(tokens, cap_off, n_caps, sos_id, eos_id, nullptr, nullptr, nullptr, nullptr);
}

extern "C" int64_t isc_bleu_cook_fill(const int64_t *tokens, const int64_t *cap_off, int64_t n_caps, int64_t sos_id,
                                      int64_t eos_id, uint64_t *keys, int32_t *counts, int32_t *ent_off,
                                      int32_t *ref_lens) {
    if (!tokens || !cap_off || n_caps < 0 || !keys || !counts || !ent_off || !ref_lens) return -1;
    return bleu_cook(tokens, cap_off, n_caps, sos_id, eos_id, keys, counts, ent_off, ref_lens);
}
