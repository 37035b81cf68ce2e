"""CPU checks of the beam search's controls (no_repeat_ngram, min_len): the restatement of tests/_ngram_beam_ref.py
against the oracle and against its own rule - what the GPU tests of test_gpu_ngram_beam.py rest on - and the C layout
of what the controls added to the library's interface."""
import ctypes
import os
import subprocess

import pytest
import torch

import _ngram_beam_ref as NB
import _widths as Wd
from conftest import ROOT
from insenticap_model_amd import _lib, ops


def test_ban_list_rule():
    a, b, c, eos = 5, 6, 7, 2
    assert NB.ban_list([], 3, 0, 0, eos) == []
    assert NB.ban_list([], 1, 0, 2, eos) == [eos]
    assert NB.ban_list([a], 3, 1, 0, eos) == []                       # L < n - 1
    assert NB.ban_list([a, a], 3, 2, 0, eos) == []                    # L == n - 1: pre = (a, a), no j yet
    assert NB.ban_list([a, a, a, a, a], 1, 5, 0, eos) == [a] * 5
    assert NB.ban_list([a, a, a, a, a], 2, 5, 0, eos) == [a] * 4
    assert NB.ban_list([a, a, a, a, a], 4, 5, 0, eos) == [a] * 2
    assert NB.ban_list([a, b, a, b, a, b], 2, 6, 0, eos) == [a, a]    # pre = (b): b -> a at j = 2 and 4 (duplicates kept)
    assert NB.ban_list([a, b, a, b, a], 2, 5, 6, eos) == [b, b, eos]  # pre = (a): a -> b twice, then <EOS> (t < min_len)
    assert NB.ban_list([a, b, c, a, b], 3, 5, 0, eos) == [c]
    assert NB.ban_list([a, b, c], 2, 3, 3, eos) == []                 # t == min_len: <EOS> allowed


@pytest.mark.parametrize('name', NB.WIDTH_SETS)
def test_controls_off_equal_the_oracle(name):
    """no_repeat_ngram = 0 and min_len = 0: the restatement is oracle.beam_search, ids and scores."""
    for image in NB.IMAGES:
        for beam, dc in ((3, 1), (5, 0)):
            caps, scores, ids, binds = NB.run(name, image, (0, 0, dc, beam))
            from oracle import captioner_oracle as O
            st, w, d, _ = Wd.setup(name)
            with torch.no_grad():
                ref = O.beam_search(O.to_params(w, dtype=torch.float64), Wd.oracle_ids(), Wd.idx2word(),
                                    Wd.cpu(d, 'fc_feats', dtype=torch.float64)[image],
                                    Wd.cpu(d, 'att_feats', dtype=torch.float64)[image], Wd.cpu(d, 'senti_words')[image],
                                    torch.tensor([image]), beam, dc, NB.T)
            assert (caps, scores, ids) == tuple(ref) and binds == 0


@pytest.mark.parametrize('case', NB.ALL_CASES, ids=lambda c: '%s-%d-%s' % (c[0], c[1], '_'.join(map(str, c[2]))))
def test_rule_holds_and_precisions_agree(case):
    name, image, (n, min_len, dc, beam) = case
    caps, scores, ids, binds = NB.run(name, image, case[2])
    eos = Wd.oracle_ids().eos
    assert len(ids) == beam
    for words in ids:
        assert NB.repeated_ngrams(words, n) == 0, words
        assert len(words) >= min_len or len(words) == NB.T, words
        if len(words) < NB.T:
            assert words[-1] == eos
        assert eos not in words[:min(min_len, len(words))]
    c32, s32, i32, _ = NB.run(name, image, case[2], dtype=torch.float32)
    assert i32 == ids and c32 == caps
    assert max(abs(a - b) for a, b in zip(s32, scores)) <= 1e-5        # (measured: <= 3.1e-6)


def test_case_list_conditions():
    """Every kept case has neighbouring final scores at least MARGIN apart (the one dropped case has not); the controls
    change some step's top-`beam` in at least 30 of the kept cases."""
    bound = 0
    for case in NB.CASES:
        caps, scores, ids, binds = NB.run(case[0], case[1], case[2])
        assert NB.score_gap(scores) >= NB.MARGIN, (case, NB.score_gap(scores))
        bound += binds > 0
    assert len(NB.CASES) == 35 and bound >= 30, bound
    for case in NB.TOO_CLOSE:
        assert NB.score_gap(NB.run(case[0], case[1], case[2])[1]) < NB.MARGIN


def test_sentiment_cases_are_decided():
    """The (image, label) searches of the sample_sentiments tests - labels other than the image index - are held to the
    same conditions: the rule, fp32 == fp64 ids, neighbouring final scores at least MARGIN apart."""
    for name, image, control, label in NB.SENTI_CASES:
        caps, scores, ids, _ = NB.run(name, image, control, label=label)
        assert NB.run(name, image, control, torch.float32, label=label)[2] == ids
        assert NB.score_gap(scores) >= NB.MARGIN, (name, image, control, label)
        assert all(NB.repeated_ngrams(w, control[0]) == 0 and (len(w) >= control[1] or len(w) == NB.T) for w in ids)
    per_label = {(n, c): [NB.run(n, i, c, label=l)[2] for (n2, i, c2, l) in NB.SENTI_CASES if (n2, c2) == (n, c)]
                 for (n, _, c, _) in NB.SENTI_CASES}
    assert any(len({str(x) for x in v}) == 3 for v in per_label.values())       # (the label reaches the captions)


def test_extended_struct_layouts_match_c(tmp_path):
    """sizeof / offsetof of isc_beam_ngram_ban_args and isc_rows_ban against their ctypes mirrors.  isc_rows_ext itself did
    not grow (tests/test_senti_beam_host.py pins its size): the few-row step's list travels next to it."""
    prog = r'''
#include <stdio.h>
#include <stddef.h>
#include "insenticap_hip.h"
int main(void) {
  printf("%zu %zu %zu %zu %zu %zu %zu\n", sizeof(isc_rows_ext), offsetof(isc_rows_ext, live_in),
         offsetof(isc_rows_ext, fin_prev), offsetof(isc_rows_ext, fin_unfinished_out), sizeof(isc_rows_ban),
         offsetof(isc_rows_ban, cnt), offsetof(isc_rows_ban, ld));
  printf("%zu %zu %zu %zu %zu %zu %zu %zu\n", sizeof(isc_beam_ngram_ban_args), offsetof(isc_beam_ngram_ban_args, t),
         offsetof(isc_beam_ngram_ban_args, min_len), offsetof(isc_beam_ngram_ban_args, eos_id),
         offsetof(isc_beam_ngram_ban_args, words), offsetof(isc_beam_ngram_ban_args, ban_cnt),
         offsetof(isc_beam_ngram_ban_args, ban_ld), offsetof(isc_beam_ngram_ban_args, live_in));
  return 0;
}
'''
    cfile, exe = str(tmp_path / 'layout.c'), str(tmp_path / 'layout')
    open(cfile, 'w').write(prog)
    subprocess.check_call(['gcc', '-I', os.path.join(ROOT, 'include'), cfile, '-o', exe])
    got = [int(x) for x in subprocess.check_output([exe]).decode().split()]
    R, G, RB = _lib.RowsExt, _lib.BeamNgramBanArgs, _lib.RowsBan
    exp = [ctypes.sizeof(R), R.live_in.offset, R.fin_prev.offset, R.fin_unfinished_out.offset, ctypes.sizeof(RB),
           RB.cnt.offset, RB.ld.offset,
           ctypes.sizeof(G), G.t.offset, G.min_len.offset, G.eos_id.offset, G.words.offset, G.ban_cnt.offset,
           G.ban_ld.offset, G.live_in.offset]
    assert got == exp
    assert R.fin_unfinished_out.offset == 96 and ctypes.sizeof(R) == 104        # as before the controls


def test_ngram_ban_refusals_without_a_gpu():
    """isc_beam_ngram_ban / isc_beam_topk_banned refuse bad arguments on the host, before any launch."""
    lib = _lib.load()
    assert lib.isc_beam_ngram_ban(None, None) == -1
    g = _lib.BeamNgramBanArgs()
    g.rows, g.T, g.t, g.no_repeat_ngram, g.min_len, g.ban_ld = 3, 10, 0, 3, 0, 10
    assert lib.isc_beam_ngram_ban(ctypes.byref(g), None) == -1            # null tables
    g.words = g.len = g.ban_ids = g.ban_cnt = 4096                        # (never dereferenced: refused first)
    for field, bad in (('no_repeat_ngram', -1), ('no_repeat_ngram', 5), ('min_len', -1), ('min_len', 11), ('t', -1),
                       ('t', 10), ('ban_ld', 9), ('rows', 0), ('T', 0), ('T', 257)):
        keep = getattr(g, field)
        setattr(g, field, bad)
        assert lib.isc_beam_ngram_ban(ctypes.byref(g), None) == -2, (field, bad)
        setattr(g, field, keep)
    assert lib.isc_beam_topk_banned(4096, 16, 4096, 4096, 1, 1, 16, 2, 4096, 0, 1, 3, 1, 1, None, None, 10, 4096, 4096,
                                    None) == -1
    x, b, p = _lib.RowsExt(), _lib.RowsBan(), _lib.StepPlan()
    x.beam = 3
    assert lib.isc_rows_step_banned_fwd(ctypes.byref(p), ctypes.byref(x), None, None) == -1
    assert lib.isc_rows_step_banned_fwd(ctypes.byref(p), ctypes.byref(x), ctypes.byref(b), None) == -1       # null ids / cnt
    b.ids = b.cnt = 4096
    assert lib.isc_rows_step_banned_fwd(ctypes.byref(p), ctypes.byref(x), ctypes.byref(b), None) == -2       # ld < 1
    b.ld, x.beam = 10, 0
    assert lib.isc_rows_step_banned_fwd(ctypes.byref(p), ctypes.byref(x), ctypes.byref(b), None) == -2       # no candidates
    assert lib.isc_beam_topk_banned(4096, 16, 4096, 4096, 1, 1, 16, 2, 4096, 0, 1, 3, 1, 1, 4096, 4096, 0, 4096, 4096,
                                    None) == -2


def test_control_values_are_checked_on_the_host():
    ok = dict(max_seq_len=10, vocab_size=300, beam=3, device_merge=True)
    assert ops.check_beam_controls(0, 0, **ok) == (0, 0)
    assert ops.check_beam_controls(3, 8, **ok) == (3, 8)
    assert ops.check_beam_controls(4, 10, **ok) == (4, 10)
    for n, m in ((5, 0), (-1, 0), (2.0, 0), (True, 0), (None, 0), ('2', 0), (0, 11), (0, -1), (0, 1.5), (0, False)):
        with pytest.raises(ValueError):
            ops.check_beam_controls(n, m, **ok)
    with pytest.raises(ValueError, match='vocabulary'):
        ops.check_beam_controls(2, 0, max_seq_len=10, vocab_size=17, beam=3, device_merge=True)
    assert ops.check_beam_controls(2, 0, max_seq_len=10, vocab_size=18, beam=3, device_merge=True) == (2, 0)
    with pytest.raises(ValueError, match='not built'):
        ops.check_beam_controls(2, 0, max_seq_len=10, vocab_size=300, beam=3, device_merge=False)
    with pytest.raises(ValueError, match='not built'):
        ops.check_beam_controls(0, 4, max_seq_len=10, vocab_size=300, beam=9, device_merge=True)
    # isc_beam_ngram_ban tests up to 256 positions: a longer search with a control on is refused here, not at its first launch
    assert ops.check_beam_controls(3, 256, max_seq_len=256, vocab_size=300, beam=3, device_merge=True) == (3, 256)
    with pytest.raises(ValueError, match='not built'):
        ops.check_beam_controls(3, 0, max_seq_len=257, vocab_size=300, beam=3, device_merge=True)
    # the defaults ask nothing of the vocabulary, the merge or the length
    assert ops.check_beam_controls(0, 0, max_seq_len=300, vocab_size=5, beam=9, device_merge=False) == (0, 0)


def test_bad_controls_raise_before_anything_touches_the_device():
    """A captioner whose parameters live on the CPU cannot search (the product has no CPU path): a bad control value is
    still a ValueError, i.e. it is checked in front of everything else; good values reach the usual loud failure."""
    from insenticap_model_amd import Captioner, synth
    V, st = 64, synth.TINY_SETTINGS
    cap = Captioner(synth.make_idx2word(V), synth.SENTIMENT_CATEGORIES, st).eval()
    d = synth.make_inputs(1, V, st, regions=5, seq_len=8, seed=1)
    fc, att, sw = (torch.from_numpy(d[k]) for k in ('fc_feats', 'att_feats', 'senti_words'))
    lab = torch.tensor([1])
    for kw in (dict(no_repeat_ngram=5), dict(no_repeat_ngram=1.0), dict(min_len=9), dict(min_len=-1), dict(no_repeat_ngram='3')):
        with pytest.raises(ValueError):
            cap.sample_batch(fc, att, sw, lab, 3, 1, 8, **kw)
        with pytest.raises(ValueError):
            cap.sample(fc[0], att[0], sw[0], lab, 3, 1, 8, **kw)
        with pytest.raises(ValueError):
            cap.sample_sentiments(fc, att, sw, torch.tensor([[0, 1]]), 3, 1, 8, **kw)
    with pytest.raises(ValueError, match='vocabulary'):
        cap.sample_batch(fc, att, sw, lab, 3, 1, 57, no_repeat_ngram=2)         # 64 <= 57 + 4 + 3
    with pytest.raises(ValueError, match='not built'):
        cap.sample_batch(fc, att, sw, lab, 9, 1, 8, min_len=2)
    with pytest.raises(Exception) as e:
        cap.sample_batch(fc, att, sw, lab, 3, 1, 8, no_repeat_ngram=3, min_len=4)
    assert not isinstance(e.value, (ValueError, TypeError))
