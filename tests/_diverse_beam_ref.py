"""Diverse beam search (beam groups with a Hamming penalty, Vijayakumar et al. 2016) restated in plain Python: the
yardstick of tests/test_diverse_beam_ref_host.py (CPU), of the kernel tests of tests/test_gpu_diverse_beam_kernels.py and of
the end-to-end tests of tests/test_gpu_diverse_beam.py.  The reference has no such search.  Lists and Python floats;
nothing here imports insenticap_model_amd.beam.

Definition.  `beam` rows per search, G groups of bp = beam / G ranks; group g owns ranks g bp .. (g + 1) bp - 1.  Step t
handles the groups in this order.  Group g's candidates, in insertion order: its parents by rank - an ended one
(t > 0, last word == eos) carried as ONE candidate, a live one contributing its children in the row's order (log-prob
descending, ties to the smaller id); at t == 0 the group's first row alone.  key = (s_parent + logp) - lam * c, c = how
many candidates selected at this step by the groups in front appended the same token (a carried candidate appended none
and its key is its score); one fp64 add, one multiply, one subtract - Python floats do exactly that.  The group keeps
the first bp of a stable descending sort by key.  The stored score is the un-augmented sum.

`select_step` is that rule over children lists of ANY length: the whole vocabulary (the definition) or the row's best
`beam` (what the kernels read).  That the two agree is the containment property the host tests check."""
import numpy as np
import torch

import _ngram_beam_ref as NB
import _widths as Wd

NEG = float('-inf')
MARGIN = Wd.MARGIN


def order_row(logp):
    """A row of log-probs (masked words at -inf) -> [(logp, id)] of the WHOLE vocabulary: descending, ties to the smaller id."""
    lp = [float(v) for v in logp]
    return [(lp[i], i) for i in sorted(range(len(lp)), key=lambda i: (-lp[i], i))]


def select_step(parents, G, lam, t, eos, trace=None):
    """One step of one search.  parents: `beam` entries (score, last word, children) by rank, children = [(logp, id)] in the
    row's order (any length >= the group width; ignored for an ended parent).  Returns (new, all_ended, gaps):
    new       `beam` entries (score, token, parent rank, carried) group-major, by selection order inside a group;
    all_ended every candidate of every group was a carried one (the search latches);
    gaps      per group: the smallest distance between neighbouring keys from the best down to the first rejected one (the
              last selected / first rejected gap and the order of the selected; inf where the keys are -inf or none is
              rejected).
    trace (a list): receives every group's ranked candidates (key, score, token, parent rank, carried)."""
    beam = len(parents)
    assert G >= 1 and beam % G == 0 and lam >= 0.0
    bp = beam // G
    new, chosen, gaps, all_ended = [], [], [], True
    for g in range(G):
        cand = []                                          # (key, score, token, parent rank, carried)
        for k in ([g * bp] if t == 0 else range(g * bp, (g + 1) * bp)):
            score, last, children = parents[k]
            if t > 0 and last == eos:
                cand.append((float(score), float(score), int(last), k, True))
                continue
            all_ended = False
            for lp, w in children:
                s = float(score) + float(lp)
                cand.append((s - lam * float(chosen.count(int(w))), s, int(w), k, False))
        ranked = sorted(cand, key=lambda c: c[0], reverse=True)          # stable: insertion order decides ties
        assert len(ranked) >= bp
        if trace is not None:
            trace.append(ranked)
        # (the selected keys among themselves as well: two of them changing places would re-order the group's rows)
        gaps.append(min([ranked[j][0] - ranked[j + 1][0] for j in range(min(bp, len(ranked) - 1)) if ranked[j][0] > NEG]
                        or [float('inf')]))
        picked = ranked[:bp]
        chosen += [c[2] for c in picked if not c[4]]       # behind the group: the groups in front are what counts
        new += [(c[1], c[2], c[3], c[4]) for c in picked]
    return new, all_ended, gaps


def truncate(parents, beam):
    """The same parents with every row cut to its raw top-`beam`: what the kernels see."""
    return [(s, last, children[:beam]) for (s, last, children) in parents]


# ------------------------------------------------------------------------------------------------ the kernels' step
def merge_groups_ref(top_val, top_idx, score_in, last_in, words_in, len_in, done, t, T, eos, beam, G, lam):
    """isc_beam_merge_groups / isc_beam_select_groups, one step for every search: _beam_ref.merge_ref's dictionary (score,
    last, words, length, done, parent, gather, live_inc).  At t == 0 group g's parent is the row g * bp as it stands."""
    n_img = len(done)
    rows = n_img * beam
    out = dict(score=[float(s) for s in score_in], last=[int(w) for w in last_in], words=[list(map(int, w)) for w in words_in],
               length=[int(n) for n in len_in], done=[int(bool(x)) for x in done], parent=list(range(rows)),
               gather=[r + rows for r in range(rows)], live_inc=0)
    for i in range(n_img):
        base = i * beam
        if done[i]:
            continue
        parents = [(float(score_in[base + k]), int(last_in[base + k]),
                    [(float(top_val[base + k][j]), int(top_idx[base + k][j])) for j in range(beam)]) for k in range(beam)]
        new, all_ended, _ = select_step(parents, G, lam, t, eos)
        for r, (score, word, k, carried) in enumerate(new):
            dst, par = base + r, base + k
            n = int(len_in[par])
            words = list(map(int, words_in[par]))
            if not carried and n < T:
                words[n] = word
            out['score'][dst], out['last'][dst], out['words'][dst] = score, word, words
            out['length'][dst] = n + (0 if carried else 1)
            out['parent'][dst], out['gather'][dst] = par, par + rows if carried else par
        if all_ended:
            out['done'][i] = 1
        else:
            out['live_inc'] += 1
    return out


# ------------------------------------------------------------------------------------------------ the driver on the oracle
def beam_search(p, ids, idx2word, fc_feat, att_feat, senti_words, senti_label, beam, decoding_constraint, max_seq_len,
                G, lam, no_repeat_ngram=0, min_len=0, full=True):
    """The definition driven by oracle.captioner_oracle.step (one batch-1 step per live parent, the reference's masks,
    _ngram_beam_ref.ban_list's ids at -inf).  full: every row contributes its WHOLE vocabulary (the definition); False: its
    best `beam` (the kernels' form).  Returns (captions, scores, id_sequences, min_gap): group-major results, and the
    smallest selected / rejected key gap over every (step, group)."""
    from oracle import captioner_oracle as O
    fc = fc_feat.reshape(1, -1)
    att = att_feat.reshape(1, -1, att_feat.shape[-1])
    P = O.prologue(p, ids, 'beam', fc, att, None, senti_words.reshape(1, -1), senti_label)
    cands = [(O.init_state(p, 1), 0.0, ids.sos, []) for _ in range(beam)]           # every row starts alike
    min_gap = float('inf')
    for t in range(max_seq_len):
        parents, states = [], []
        for k, (state, score, last, words) in enumerate(cands):
            if (t > 0 and last == ids.eos) or (t == 0 and k > 0):
                parents.append((score, last, parents[0][2] if t == 0 else None))     # (t == 0: every row decodes the same step)
                states.append(states[0] if t == 0 else state)
                continue
            logp, st, _ = O.step(p, torch.tensor([last], dtype=torch.long), state, P.fc_e, P.att_e, P.p_att, P.words_e,
                                 P.p_words, P.label_e)
            logp = logp.detach().squeeze(0).clone()
            if ids.pad != ids.eos:
                logp[ids.pad] = logp[ids.sos] = logp[ids.unk] = O.NEG_INF
            if decoding_constraint:
                logp[last] = O.NEG_INF
            for b in NB.ban_list(words, no_repeat_ngram, t, min_len, ids.eos):
                logp[b] = O.NEG_INF
            children = order_row(logp.tolist())
            parents.append((score, last, children if full else children[:beam]))
            states.append(st)
        new, all_ended, gaps = select_step(parents, G, lam, t, ids.eos)
        min_gap = min([min_gap] + gaps)
        cands = [(cands[k][0] if carried else states[k], score, word, cands[k][3] + ([] if carried else [word]))
                 for (score, word, k, carried) in new]
        if all_ended:
            break
    caps = [' '.join(idx2word[i] for i in c[3] if i != ids.eos) for c in cands]
    return caps, [c[1] for c in cands], [c[3] for c in cands], min_gap


# ------------------------------------------------------------------------------------------------ the end-to-end cases
WIDTH_SET = 'h_wide'                  # H != A, few-row step and fused gate eligible (tests/_widths.py)
TRIGRAM = (3, 6)                      # (no_repeat_ngram, min_len) of the "with controls" runs
# name: (model, kind, (image, label) searches in result order, beam, G, lambda); 'tiny' = conftest.CASES['tiny'].  Chosen on
# the CPU among images x labels x lambda in {0.5, 1}: every (step, group) of the fp64 run, with and without TRIGRAM, keeps
# its neighbouring keys down to the first rejected one more than MARGIN apart (test_diverse_beam_ref_host.py asserts it).
CASES = {
    'tiny_one': ('tiny', 'one', ((0, 0),), 6, 3, 0.5),
    'tiny_batch': ('tiny', 'batch', ((0, 0), (1, 0), (3, 1)), 6, 3, 0.5),
    'tiny_senti': ('tiny', 'senti', ((1, 2), (1, 0)), 4, 2, 0.5),
    'wide_one': (WIDTH_SET, 'one', ((1, 1),), 6, 3, 0.5),
    'wide_batch': (WIDTH_SET, 'batch', ((1, 1), (2, 2), (4, 1)), 6, 3, 0.5),
    'wide_senti': (WIDTH_SET, 'senti', ((4, 2), (4, 0)), 4, 2, 0.5),
}
_models, _runs = {}, {}


def model(name):
    """(settings, weights, inputs, T, V) of 'tiny' (conftest.CASES) or of a width set."""
    if name not in _models:
        if name == 'tiny':
            from conftest import case_setup
            c, st, w, d, _ = case_setup('tiny')
            _models[name] = (st, w, d, c['T'], c['V'])
        else:
            st, w, d, _ = Wd.setup(name)
            _models[name] = (st, w, d, Wd.T, Wd.V)
    return _models[name]


def model_ids(name):
    from insenticap_model_amd import synth
    from oracle import captioner_oracle as O
    i2w = synth.make_idx2word(model(name)[4])
    return i2w, O.Ids(i2w, synth.SENTIMENT_CATEGORIES)


def run(name, image, label, beam, G, lam, dc=1, control=(0, 0), dtype=torch.float64, full=True):
    """The driver on `image` of model `name` under sentiment `label`; cached."""
    key = (name, image, label, beam, G, lam, dc, control, dtype, full)
    if key not in _runs:
        from oracle import captioner_oracle as O
        st, w, d, T_, _ = model(name)
        i2w, ids = model_ids(name)
        with torch.no_grad():
            _runs[key] = beam_search(O.to_params(w, dtype=dtype), ids, i2w, Wd.cpu(d, 'fc_feats', dtype=dtype)[image],
                                     Wd.cpu(d, 'att_feats', dtype=dtype)[image], Wd.cpu(d, 'senti_words')[image],
                                     torch.tensor([label]), beam, dc, T_, G, lam, control[0], control[1], full)
    return _runs[key]


def expected(case, control=(0, 0), dtype=torch.float64, full=True):
    """The driver's (captions, scores, ids, min_gap) of every search of a case, in result order."""
    name, _, pairs, beam, G, lam = CASES[case]
    return [run(name, i, l, beam, G, lam, 1, control, dtype, full) for (i, l) in pairs]


def dyadic_rows(rng, rows, V, unit=0.25, lo=-6.0, hi=0.0):
    """[rows][V] 'log-probs' on a lattice of `unit` in [lo, hi]: sums and penalties with lam a multiple of `unit` are exact,
    so a penalised and an un-penalised key tie exactly."""
    return (rng.integers(int(lo / unit), int(hi / unit) + 1, size=(rows, V)) * unit).astype(np.float64).tolist()
