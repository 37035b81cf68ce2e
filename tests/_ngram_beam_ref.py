"""The beam search's two controls restated on the oracle: no n-gram twice in a caption (`no_repeat_ngram`), no <EOS>
before `min_len` words.  The reference has neither control, so the yardstick of test_ngram_beam_ref_host.py (CPU) and
of the GPU tests is this file: `ban_list` is the rule, `beam_search` is oracle.captioner_oracle.beam_search's candidate
loop driven by oracle.step with the rule's ids at -inf next to the reference's own masks (captioner.py:394-399).

Rule.  A live candidate has generated words w[0..L) (<SOS> is not among them; L == t at step t).  With n >= 1 and
L >= n - 1 let pre = w[L-n+1 .. L) (empty for n = 1): for every position j in [n-1, L) with w[j-n+1 .. j) == pre the id
w[j] is banned.  With t < min_len, eos is banned.  The list is ordered: one entry per matching j, ascending, duplicates
kept, then eos - at most T entries."""
import torch

import _senti_beam as SB
import _widths as Wd

T = Wd.T
WIDTH_SETS = ('h_wide', 'all_differ', 'h_768')
IMAGES = (0, 1, 2)                    # label = image index
CONTROLS = ((2, 0, 1, 3), (3, 8, 1, 3), (3, 0, 0, 5), (1, 10, 0, 2))       # (n, min_len, decoding_constraint, beam)
MARGIN = SB.MARGIN
ALL_CASES = tuple((name, img, c) for name in WIDTH_SETS for img in IMAGES for c in CONTROLS)
# neighbouring final scores of the fp64 run closer than MARGIN (1.81e-3): a rounding of the device could swap two beams
TOO_CLOSE = (('h_wide', 0, (3, 0, 0, 5)),)
CASES = tuple(c for c in ALL_CASES if c not in TOO_CLOSE)
# one image under several (rotated) labels, Captioner.sample_sentiments: SENTI_IMAGE under every label, beam-3 controls
SENTI_IMAGE = 1
SENTI_CONTROLS = CONTROLS[:2]
SENTI_CASES = tuple((name, SENTI_IMAGE, c, label) for name in WIDTH_SETS for c in SENTI_CONTROLS for label in (0, 1, 2))
_cache = {}


def ban_list(words, n, t, min_len, eos):
    """The ordered ban list of a candidate with the generated words `words` at step t."""
    w, L, out = list(words), len(words), []
    if n >= 1 and L >= n - 1:
        pre = w[L - n + 1:L]
        for j in range(n - 1, L):
            if w[j - n + 1:j] == pre:
                out.append(w[j])
    if t < min_len:
        out.append(eos)
    return out


def beam_search(p, ids, idx2word, fc_feat, att_feat, senti_words=None, senti_label=None, beam_size=3,
                decoding_constraint=1, max_seq_len=16, no_repeat_ngram=0, min_len=0):
    """oracle.beam_search with the two controls.  Returns (captions, scores, id_sequences, binds): `binds` counts the
    (step, candidate) pairs whose top-`beam_size` ids the controls changed."""
    from oracle import captioner_oracle as O
    fc = fc_feat.reshape(1, -1)
    att = att_feat.reshape(1, -1, att_feat.shape[-1])
    if senti_words is not None:
        P = O.prologue(p, ids, 'beam', fc, att, None, senti_words.reshape(1, -1), senti_label)
    else:
        P = O.prologue(p, ids, 'beam', fc, att, None, None, None)
    cands = [(O.init_state(p, 1), 0.0, ids.sos, [])]
    binds = 0
    for t in range(max_seq_len):
        nxt = []
        all_ended = True
        for (state, score, last, words) in cands:
            if t > 0 and last == ids.eos:
                nxt.append((state, score, last, words))
                continue
            all_ended = False
            it = torch.tensor([last], dtype=torch.long)
            logp, st, _ = O.step(p, it, state, P.fc_e, P.att_e, P.p_att, P.words_e, P.p_words, P.label_e)
            logp = logp.detach().squeeze(0).clone()
            if ids.pad != ids.eos:
                logp[ids.pad] = O.NEG_INF
                logp[ids.sos] = O.NEG_INF
                logp[ids.unk] = O.NEG_INF
            if decoding_constraint:
                logp[last] = O.NEG_INF
            free = torch.sort(logp, descending=True)[1][:beam_size].tolist()
            for b in ban_list(words, no_repeat_ngram, t, min_len, ids.eos):
                logp[b] = O.NEG_INF
            vals, idx = torch.sort(logp, descending=True)
            binds += idx[:beam_size].tolist() != free
            for k in range(beam_size):
                nxt.append((st, score + float(vals[k]), int(idx[k]), words + [int(idx[k])]))
        cands = sorted(nxt, key=lambda c: c[1], reverse=True)[:beam_size]
        if all_ended:
            break
    caps = [' '.join(idx2word[i] for i in c[3] if i != ids.eos) for c in cands]
    return caps, [c[1] for c in cands], [c[3] for c in cands], binds


def run(name, image, control, dtype=torch.float64, label=None):
    """The restatement on `image` of width set `name` under sentiment `label` (default: the image index); cached."""
    n, min_len, dc, beam = control
    label = image if label is None else label
    key = (name, image, control, dtype, label)
    if key not in _cache:
        from oracle import captioner_oracle as O
        st, w, d, _ = Wd.setup(name)
        with torch.no_grad():
            _cache[key] = beam_search(O.to_params(w, dtype=dtype), Wd.oracle_ids(), Wd.idx2word(),
                                      Wd.cpu(d, 'fc_feats', dtype=dtype)[image], Wd.cpu(d, 'att_feats', dtype=dtype)[image],
                                      Wd.cpu(d, 'senti_words')[image], torch.tensor([label]), beam, dc, T, n, min_len)
    return _cache[key]


def repeated_ngrams(words, n):
    """How many n-grams of `words` occurred earlier in it."""
    seen, rep = set(), 0
    for j in range(len(words) - n + 1):
        g = tuple(words[j:j + n])
        rep += g in seen
        seen.add(g)
    return rep


def score_gap(scores):
    """Smallest distance between neighbouring final scores."""
    return min(abs(a - b) for a, b in zip(scores, scores[1:])) if len(scores) > 1 else float('inf')
