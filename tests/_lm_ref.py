"""The back-off n-gram language model of DESIGN.md ("Per-sentiment n-gram language models") restated in fp64 Python: a
dictionary from id tuples to (logp, backoff), no hash table of its own and no key packing.  The library's host scorer
(isc_lm_score) and the device kernel (isc_lm_dev_score) are held to it IN BITS: every stored value is the ARPA decimal
read as a Python float and rounded once to float32, and a sentence score is a chain of float64 additions in one order.

Also here: a seeded generator of random models (orders 1 to 4, with and without <unk>, contexts deliberately absent as
in a pruned model), an ARPA writer, and rows that walk a model's n-grams.

No KenLM or SRILM binary has been available: agreement with those programs' printed numbers is not measured; the
yardstick is the ARPA back-off definition."""
import numpy as np

BOS, EOS_W, UNK = '<s>', '</s>', '<unk>'


def f32(x):
    """The one rounding of a stored value: Python float -> float32 (returned as the float64 that holds it)."""
    return float(np.float32(float(x)))


def specials(V):
    return {BOS: V, EOS_W: V + 1, UNK: V + 2}


def parse_arpa(text, V, word2idx=None):
    """-> (order, {ids tuple: (logp, backoff)}, n_dropped).  Words map through word2idx when given, else as decimal ids;
    <s>, </s>, <unk> are V, V + 1, V + 2; an n-gram with a word outside the vocabulary is dropped and counted."""
    sp = specials(V)

    def wid(w):
        if w in sp:
            return sp[w]
        if word2idx is not None:
            i = word2idx.get(w)
        else:
            i = int(w) if w.isdigit() else None
        return i if i is not None and 0 <= i < V else None
    table, order, dropped, k = {}, 0, 0, 0
    for line in text.splitlines():
        line = line.strip()
        if not line or line.startswith('ngram ') or line == '\\data\\':
            continue
        if line == '\\end\\':
            break
        if line.startswith('\\') and line.endswith('-grams:'):
            k = int(line[1:-len('-grams:')])
            order = max(order, k)
            continue
        parts = line.split()
        assert k >= 1 and len(parts) in (k + 1, k + 2), line
        ids = tuple(wid(w) for w in parts[1:k + 1])
        if any(i is None for i in ids):
            dropped += 1
            continue
        assert ids not in table, line
        table[ids] = (f32(parts[0]), f32(parts[k + 1]) if len(parts) == k + 2 else 0.0)
    return order, table, dropped


def normalise(row, sos, eos):
    """utils._array_to_str as a list of ids: drop a leading <SOS>, cut at the first <EOS>, append <EOS>."""
    row = [int(x) for x in row]
    if row and row[0] == sos:
        row = row[1:]
    out = []
    for w in row:
        if w == eos:
            break
        out.append(w)
    return out + [eos]


def score_row(table, order, row, V, sos, eos, eos_mode='word', unk_as_word=True, trace=None):
    """-> (score, n_scored, n_oov, [value per position]) of one raw row.  `trace`: a list that receives per position
    (back-off levels walked, contexts among them that the table held, 'hit' | 'unk' | 'skip')."""
    words = normalise(row, sos, eos)
    if eos_mode == 'end':
        words = words[:-1]
    else:
        assert eos_mode == 'word'
    none = V + 3
    seq = [w if 0 <= w < V else none for w in words] + [V + 1]
    hist = [V] + seq                                   # hist[i + 1] = seq[i]; <s> in front
    total, n_scored, n_oov, vals = 0.0, 0, 0, []
    for i, w in enumerate(seq):
        ctx = tuple(hist[max(0, i + 1 - (order - 1)):i + 1]) if order > 1 else ()
        acc, val, found = 0.0, 0.0, False
        levels, present, how = 0, 0, 'hit'
        while True:
            if ctx + (w,) in table:
                val, found = table[ctx + (w,)][0] + acc, True
                break
            if not ctx:
                break
            levels += 1
            if ctx in table:
                acc += table[ctx][1]
                present += 1
            ctx = ctx[1:]
        if not found:
            n_oov += 1
            how = 'skip'
            if unk_as_word and (V + 2,) in table:
                val, found, how = table[(V + 2,)][0] + acc, True, 'unk'
        if trace is not None:
            trace.append((levels, present, how))
        if found:
            n_scored += 1
        else:
            val = 0.0
        vals.append(val)
        total += val
    return total, n_scored, n_oov, vals


def score_rows(models, hyps, labels, V, sos, eos, eos_mode='word', unk_as_word=True):
    """models: list of (order, table) by label.  -> score float64 [N], n_scored int32 [N], n_oov int32 [N], tok_logp
    float64 [N, T + 2]; a label outside the list: NaN, -1, 0, zeros."""
    hyps = np.asarray(hyps)
    N, T = hyps.shape
    score, ns, no = np.zeros(N), np.zeros(N, dtype=np.int32), np.zeros(N, dtype=np.int32)
    tok = np.zeros((N, T + 2))
    for r in range(N):
        lab = 0 if labels is None else int(labels[r])
        if not 0 <= lab < len(models):
            score[r], ns[r] = np.nan, -1
            continue
        order, table = models[lab]
        score[r], ns[r], no[r], vals = score_row(table, order, hyps[r], V, sos, eos, eos_mode, unk_as_word)
        tok[r, :len(vals)] = vals
    return score, ns, no, tok


# ------------------------------------------------------------------------------------------------ random models
def random_lm(seed, V, order, n_words=12, per_order=40, with_unk=True, words=None):
    """A seeded random model: {order k: [(word strings tuple, logp string, backoff string or None)]}.  Half of the
    k-grams extend a (k - 1)-gram of the model, the others are drawn freely - their contexts are mostly ABSENT, as in a
    pruned model; about a third of the eligible n-grams carry no back-off weight."""
    rng = np.random.default_rng(seed)
    if words is None:
        words = sorted(int(x) for x in rng.choice(V, size=min(n_words, V), replace=False))
    W = [str(w) for w in words]

    def lp():
        return '%.6f' % -float(rng.uniform(0.05, 4.0))

    def bo(last):
        return None if last == EOS_W or rng.random() < 0.33 else '%.6f' % -float(rng.uniform(0.0, 1.5))
    grams = {1: [((BOS,), '-99', '%.6f' % -float(rng.uniform(0.1, 1.0))), ((EOS_W,), lp(), None)]}
    if with_unk:
        grams[1].append(((UNK,), lp(), None))
    for w in W:
        grams[1].append(((w,), lp(), bo(w) if order > 1 else None))
    for k in range(2, order + 1):
        seen, out = set(), []
        prev = [g[0] for g in grams[k - 1] if g[0][-1] != EOS_W and g[0] != (UNK,)]
        for _ in range(per_order * 4):
            if len(out) >= per_order:
                break
            if prev and rng.random() < 0.5:
                head = prev[int(rng.integers(len(prev)))]
            else:
                head = tuple((BOS if j == 0 and rng.random() < 0.25 else W[int(rng.integers(len(W)))]) for j in range(k - 1))
            last = EOS_W if rng.random() < 0.2 else W[int(rng.integers(len(W)))]
            g = head + (last,)
            if g in seen:
                continue
            seen.add(g)
            out.append((g, lp(), bo(last) if k < order else None))
        grams[k] = out
    return grams


def write_arpa(grams):
    lines = ['', '\\data\\'] + ['ngram %d=%d' % (k, len(grams[k])) for k in sorted(grams)] + ['']
    for k in sorted(grams):
        lines.append('\\%d-grams:' % k)
        for g, logp, backoff in grams[k]:
            lines.append('\t'.join([logp, ' '.join(g)] + ([backoff] if backoff is not None else [])))
        lines.append('')
    lines.append('\\end\\')
    return '\n'.join(lines) + '\n'


def model_words(grams):
    return sorted(int(g[0][0]) for g in grams[1] if g[0][0] not in (BOS, EOS_W, UNK))


def walk_rows(grams, N, T, V, sos, eos, seed, p_follow=0.7, p_oov=0.1):
    """N raw rows of T ids that mostly follow the model's n-grams (so full-order hits and every back-off depth occur), with
    out-of-vocabulary words mixed in; a third carry a leading <SOS>, a fifth no <EOS>; garbage behind the <EOS>."""
    rng = np.random.default_rng(seed)
    words = model_words(grams)
    inside = set(words)
    others = [w for w in range(V) if w not in inside and w not in (sos, eos)] or words
    nxt = {}
    for k in grams:
        for g, _, _ in grams[k]:
            if k >= 2 and g[-1] != EOS_W:
                nxt.setdefault(g[:-1], []).append(int(g[-1]))
    rows = np.zeros((N, T), dtype=np.int64)
    for r in range(N):
        length = T if r % 5 == 4 else int(rng.integers(0, T + 1))
        seq, hist = [], [BOS]
        for _ in range(length):
            w = None
            if rng.random() < p_follow:
                for c in range(min(3, len(hist)), 0, -1):
                    cand = nxt.get(tuple(hist[-c:]))
                    if cand:
                        w = cand[int(rng.integers(len(cand)))]
                        break
            if w is None:
                w = others[int(rng.integers(len(others)))] if rng.random() < p_oov else words[int(rng.integers(len(words)))]
            seq.append(w)
            hist.append(str(w))
        if r % 3 == 1:
            seq = [sos] + seq
        seq = seq[:T]
        if len(seq) < T:
            seq.append(eos)
        while len(seq) < T:                              # garbage behind the <EOS>
            seq.append(int(rng.integers(0, V)))
        rows[r] = seq
    return rows
