"""The cases the host scorer (tests/test_lm_host.py, CPU) and the device kernel (tests/test_gpu_lm_kernels.py) are both held
to the fp64 restatement with (tests/_lm_ref.py), in bits.  A case: ARPA texts by label, V, eos_mode, unk_as_word, table
capacities (None: the default), <SOS> / <EOS>, raw rows and labels (None: no label array).  Built once and cached; the
restatement's result is computed once per case and shared."""
import numpy as np

import _lm_ref as R
from insenticap_model_amd import rewards

SOS, EOS = 1, 2
_cache = {}


def case(name, texts, V, hyps, labels=None, mode='word', unk=True, caps=None, sos=SOS, eos=EOS):
    return dict(name=name, texts=list(texts), V=V, hyps=np.ascontiguousarray(hyps, dtype=np.int64),
                labels=None if labels is None else np.ascontiguousarray(labels, dtype=np.int64), mode=mode, unk=unk,
                caps=caps, sos=sos, eos=eos)


def host_set(c):
    lms = [rewards.NgramLM.from_arpa(t, c['V']) for t in c['texts']]
    return rewards.NgramLMSet(lms, c['V'], c['mode'], c['unk'], sos=c['sos'], eos=c['eos'], capacities=c['caps'])


def models(c):
    return [R.parse_arpa(t, c['V'])[:2] for t in c['texts']]


def expected(c):
    """(score, n_scored, n_oov, tok_logp) of the restatement, computed once per case."""
    if 'want' not in c:
        c['want'] = R.score_rows(models(c), c['hyps'], c['labels'], c['V'], c['sos'], c['eos'], c['mode'], c['unk'])
    return c['want']


def traces(c):
    """The set of (levels, contexts present, how) over every scored position of the case."""
    seen = set()
    ms = models(c)
    for r, row in enumerate(c['hyps']):
        lab = 0 if c['labels'] is None else int(c['labels'][r])
        if 0 <= lab < len(ms):
            t = []
            R.score_row(ms[lab][1], ms[lab][0], row, c['V'], c['sos'], c['eos'], c['mode'], c['unk'], trace=t)
            seen.update(t)
    return seen


def same_bits(got, want, what):
    """score / n_scored / n_oov / tok_logp equal in bits (a NaN score equals a NaN score)."""
    names = ('score', 'n_scored', 'n_oov', 'tok_logp')
    for g, w, n in zip(got, want, names):
        g, w = np.asarray(g), np.asarray(w)
        assert g.shape == w.shape and g.dtype == w.dtype, (what, n, g.shape, w.shape, g.dtype, w.dtype)
        if g.dtype == np.float64:
            nan = np.isnan(w)
            assert np.array_equal(np.isnan(g), nan), (what, n)
            g, w = np.where(nan, 0.0, g).view(np.int64), np.where(nan, 0.0, w).view(np.int64)
        assert np.array_equal(g, w), (what, n, g, w)


HAND4 = """
\\data\\
ngram 1=8
ngram 2=4
ngram 3=4
ngram 4=2

\\1-grams:
-99\t<s>\t-0.1
-1.0\t</s>
-2.0\t<unk>
-0.5\t4\t-0.11
-0.6\t5\t-0.12
-0.7\t6\t-0.13
-0.8\t7\t-0.14
-0.9\t8\t-0.15

\\2-grams:
-0.2\t<s> 4\t-0.21
-0.3\t4 5\t-0.22
-0.4\t5 6\t-0.23
-0.45\t6 7\t-0.24

\\3-grams:
-0.1\t<s> 4 5\t-0.31
-0.15\t4 5 6\t-0.32
-0.17\t5 6 7\t-0.33
-0.19\t4 5 8

\\4-grams:
-0.05\t<s> 4 5 6
-0.06\t4 5 6 7

\\end\\
"""


def _text(seed, V, order, **kw):
    return R.write_arpa(R.random_lm(seed, V, order, **kw))


def _tight(seed, V, n):
    """An order-3 random model of exactly n n-grams - all unigrams, the rest halved between bigrams and trigrams - for a
    table of capacity n + 1 = a power of two: one empty slot, chains that run long and wrap past the end.
    -> (ARPA text, the n-grams)."""
    g = R.random_lm(seed, V, 3, n_words=10, per_order=n)
    u = len(g[1])
    keep = {1: g[1], 2: g[2][:(n - u) // 2], 3: g[3][:n - u - (n - u) // 2]}
    assert sum(len(v) for v in keep.values()) == n
    return R.write_arpa(keep), keep


def _home_slot_words(V, capacity, count, home=0):
    """`count` word ids whose unigram key has home slot `home` in a table of `capacity` slots (splitmix64 as cider_key.h)."""
    M = (1 << 64) - 1
    out = []
    for w in range(3, V):
        k = w + 1
        k ^= k >> 30
        k = k * 0xBF58476D1CE4E5B9 & M
        k ^= k >> 27
        k = k * 0x94D049BB133111EB & M
        k ^= k >> 31
        if k & (capacity - 1) == home:
            out.append(w)
            if len(out) == count:
                return out
    raise AssertionError('no such words')


def build():
    if 'cases' in _cache:
        return _cache['cases']
    cs = []
    V = 40
    three = [_text(s, V, 3) for s in (11, 12, 13)]
    grams3 = R.random_lm(11, V, 3)
    # N x T: one row, a full workgroup, a partial last one, three workgroups; one token, a few, all 64 lanes in 'word' mode
    for N in (1, 4, 5, 9):
        for T in (1, 5, 62):
            rng = np.random.default_rng(100 * N + T)
            cs.append(case('shape N=%d T=%d' % (N, T), three, V, R.walk_rows(grams3, N, T, V, SOS, EOS, seed=N * 7 + T),
                           labels=rng.integers(0, 3, size=N)))
    # T = 62 without <EOS> and without <SOS>: 62 words + <EOS> + </s> = 64 scored positions
    plain = [w for w in R.model_words(grams3) if w not in (SOS, EOS)]
    full = np.asarray([plain[(i * 5) % len(plain)] for i in range(62)])[None, :]
    cs.append(case('64 positions', three, V, full, labels=[0]))
    # orders 1 to 4, with and without <unk>, both unk_as_word values, both eos_modes
    for order in (1, 2, 3, 4):
        for with_unk in (True, False):
            g = R.random_lm(20 + order, V, order, with_unk=with_unk)
            rows = R.walk_rows(g, 24, 10, V, SOS, EOS, seed=30 + order, p_oov=0.15)
            for unk in (True, False):
                for mode in ('word', 'end'):
                    cs.append(case('order %d unk-in-model %d unk_as_word %d %s' % (order, with_unk, unk, mode),
                                   [R.write_arpa(g)], V, rows, mode=mode, unk=unk))
    # the hand-built order-4 model: a hit at full order, back-off through one, two and three levels with the contexts
    # present and absent, an OOV as the scored word and in later contexts, <EOS> at position 0, a leading <SOS>, garbage
    # behind the <EOS>, ids >= V and negative ones
    hand = [[4, 5, 6, 7, 8, EOS, 9, 9], [8, 7, 6, EOS, 4, 5, 6, 7], [4, 5, 8, EOS, 0, 0, 0, 0],
            [8, 5, 6, 7, EOS, 39, 39, 39], [4, 5, 6, 7, 4, 5, 6, 7], [EOS, 4, 5, 6, 7, 8, 4, 5],
            [SOS, 4, 5, 6, 7, EOS, 4, 4], [SOS, EOS, 4, 5, 6, 7, 8, 4], [4, 9, 5, 6, 7, EOS, 0, 0],
            [4, 5, 9, 9, 6, 7, 8, EOS], [4, 5, 40, 6, 7, -1, 6, 7], [4, 5, 2 ** 40, 6, -2 ** 40, 7, EOS, 1],
            [4, 5, 43, 6, 41, 42, 7, EOS], [6, 7, 8, 4, 5, 6, 7, EOS], [5, 6, 7, 8, EOS, 4, 5, 6],
            [SOS, SOS, 4, 5, EOS, 6, 7, 8]]
    for unk in (True, False):
        for mode in ('word', 'end'):
            cs.append(case('hand4 unk_as_word %d %s' % (unk, mode), [HAND4], V, hand, mode=mode, unk=unk))
    # tables at their tightest capacity: 63 n-grams in 64 slots, 127 in 128
    for n, seed in ((63, 41), (127, 42)):
        t, g = _tight(seed, V, n)
        cs.append(case('tight %d' % n, [t], V, R.walk_rows(g, 16, 12, V, SOS, EOS, seed=seed), caps=[n + 1]))
    # two models adjacent in the slot array: the first one full but for one slot (its chains wrap at ITS end, in front of
    # the second one's first slot), the second one's unigrams all at home slot 0 - the start of its range
    Vb = 4000
    words_b = _home_slot_words(Vb, 16, 9)
    lm_b = R.random_lm(52, Vb, 2, per_order=3, with_unk=False, words=words_b)
    text_a, lm_a = _tight(51, Vb, 63)
    rows_a, rows_b = R.walk_rows(lm_a, 4, 8, Vb, SOS, EOS, seed=51), R.walk_rows(lm_b, 4, 8, Vb, SOS, EOS, seed=52)
    cs.append(case('adjacent', [text_a, R.write_arpa(lm_b)], Vb, np.concatenate([rows_a, rows_b, rows_a]),
                   labels=[0, 0, 0, 0, 1, 1, 1, 1, 1, 1, 0, 0], caps=[64, 16]))
    # four rows of one workgroup on three labels; labels out of range; no label array
    rows = R.walk_rows(grams3, 8, 9, V, SOS, EOS, seed=61)
    cs.append(case('one workgroup, three labels', three, V, rows[:4], labels=[2, 0, 1, 2]))
    cs.append(case('labels out of range', three, V, rows, labels=[0, -1, 3, 1, 2 ** 33, 2, -2 ** 40, 0]))
    cs.append(case('no labels', three, V, rows, labels=None))
    # V = 65531 with the largest id in use; 65531 .. 65534 as TOKENS are no words (never the specials they would alias)
    Vm = rewards.LM_MAX_VOCAB
    big = R.random_lm(71, Vm, 3, words=[5, 77, 30000, 65000, 65529, 65530])
    rows = R.walk_rows(big, 12, 8, Vm, SOS, EOS, seed=71)
    rows[0, :5] = [65530, 65531, 65532, 65533, 65534]
    rows[1, :4] = [65530, 65530, 65535, 65536]
    for unk in (True, False):
        cs.append(case('V = 65531 unk_as_word %d' % unk, [R.write_arpa(big)], Vm, rows, unk=unk))
    _cache['cases'] = cs
    return cs


def named(name):
    return [c for c in build() if c['name'] == name][0]
