"""Width sets with rnn_hid_dim, att_hid_dim and feat_emb_dim different from each other, shared by test_widths_host.py,
test_gpu_widths.py and the few-row kernel tests of test_gpu_rows.py.  Every other end-to-end test builds its model from
synth.TINY_SETTINGS (all 32) or synth.DEFAULT_SETTINGS (all 512), where a wrong symbol in the plumbing (a buffer sized A
where E is read, a leading dimension H where H + E + W is meant) cannot be seen.

  h_wide        H != A with the few-row step and the fused gate still eligible (A == E == W)
  all_differ    E, H, A all different, A smallest: neither the few-row step nor the fused gate
  a_wide        A largest
  h_768         rows_lstm's two units per wave (6 to 7 K-slices, one column group)
  h_1024_e_288  10 K-slices against the 8 the few-row LSTM keeps in flight, a ragged 256 + 32 slice, A = 288 in the row scan

The seeds are chosen on the CPU (test_widths_host.py asserts what the GPU tests rest on: every live greedy step has a
top-1 / top-2 margin above 2e-3 in the fp64 oracle, fp32 and fp64 oracle agree on tokens and beams)."""
import numpy as np
import torch

from insenticap_model_amd import synth

V, R, T, B = 300, 7, 10, 9
S2S_B = 5
MARGIN = 2e-3


def _st(we, f, fa, h, a):
    return dict(word_emb_dim=we, fc_feat_dim=f, att_feat_dim=fa, feat_emb_dim=we, dropout_p=0.5, rnn_hid_dim=h,
                att_hid_dim=a)


WIDTHS = {
    'h_wide': dict(settings=_st(32, 96, 160, 64, 32), wseed=4, in_seed=6, rows_step=True),
    'all_differ': dict(settings=_st(64, 128, 160, 96, 32), wseed=4, in_seed=6, rows_step=False),
    'a_wide': dict(settings=_st(32, 64, 96, 64, 96), wseed=4, in_seed=6, rows_step=False),
    'h_768': dict(settings=_st(32, 64, 64, 768, 32), wseed=3, in_seed=5, rows_step=True),
    'h_1024_e_288': dict(settings=_st(288, 64, 64, 1024, 288), wseed=3, in_seed=5, rows_step=True),
}
SMALL = ('h_wide', 'all_differ', 'a_wide')
LARGE = ('h_768', 'h_1024_e_288')
ELIGIBLE = tuple(k for k, v in WIDTHS.items() if v['rows_step'])

H_WIDE, H_768, H_1024_E_288 = (WIDTHS[k]['settings'] for k in ('h_wide', 'h_768', 'h_1024_e_288'))

_cache = {}


def setup(name):
    """(settings, weights, inputs of B rows, seq2seq inputs of S2S_B rows) of a width set; built once."""
    if name not in _cache:
        c = WIDTHS[name]
        st = c['settings']
        _cache[name] = (st, synth.make_weights(V, st, seed=c['wseed']),
                        synth.make_inputs(B, V, st, regions=R, seq_len=T, seed=c['in_seed']),
                        synth.make_inputs(S2S_B, V, st, regions=R, seq_len=T, seed=c['in_seed'] + 1))
    return _cache[name]


def idx2word():
    return synth.make_idx2word(V)


def oracle_ids():
    from oracle import captioner_oracle as O
    return O.Ids(idx2word(), synth.SENTIMENT_CATEGORIES)


def cpu(d, key, rows=None, dtype=None):
    x = torch.from_numpy(np.ascontiguousarray(np.asarray(d[key])[:rows]))
    return x.to(dtype) if dtype is not None and x.is_floating_point() else x


RL_KEYS = ('fc_feats', 'att_feats', 'cpt_words', 'senti_words', 'senti_labels')


def oracle_greedy(name, rows=B, dtype=torch.float64):
    """The oracle's greedy roll-out of the first `rows` rows: (seq, logprobs, masks, P, weights, margins), cached."""
    key = ('greedy', name, rows, dtype)
    if key not in _cache:
        from oracle import captioner_oracle as O
        st, w, d, _ = setup(name)
        with torch.no_grad():
            _cache[key] = O.forward_rl(O.to_params(w, dtype=dtype), oracle_ids(), *[cpu(d, k, rows, dtype) for k in RL_KEYS],
                                       T, 1)
    return _cache[key]


def oracle_beams(name, image, dtype=torch.float64, beam=3):
    """The oracle's beam search (decoding_constraint = 1, T steps, sentiment words) of one image: (captions, scores,
    ids), cached."""
    key = ('beam', name, image, dtype, beam)
    if key not in _cache:
        from oracle import captioner_oracle as O
        st, w, d, _ = setup(name)
        with torch.no_grad():
            _cache[key] = O.beam_search(O.to_params(w, dtype=dtype), oracle_ids(), idx2word(),
                                        cpu(d, 'fc_feats', dtype=dtype)[image], cpu(d, 'att_feats', dtype=dtype)[image],
                                        cpu(d, 'senti_words')[image], cpu(d, 'senti_labels')[image:image + 1], beam, 1, T)
    return _cache[key]


def fused_gate_eligible(st, rows, max_rows=768):
    """The condition under which Captioner._prologue builds the gate tables for an inference call of `rows` rows."""
    A, E, W = st['att_hid_dim'], st['feat_emb_dim'], st['word_emb_dim']
    return 0 < rows <= max_rows and A == E == W and A <= 1024
