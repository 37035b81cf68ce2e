"""CPU checks of the roll-out's token constraints: the fp64 reference loop of tests/_constraint_ref.py against the
oracle's beam search (constrained greedy IS beam 1), min_len, the special-token rule when pad_id == eos_id, and the
ValueErrors of the public API - raised with CPU tensors, before any library call."""
import numpy as np
import pytest
import torch

import _constraint_ref as cref
from insenticap_model_amd import Captioner, synth
from oracle import captioner_oracle as O

setup, T = cref.setup, cref.T


_CACHE = {}


def case(V):
    if V not in _CACHE:
        st, w, i2w, prm, oid, ins = setup(V)
        con = cref.rollout(prm, oid, ins, T, 1, suppress_special=True, decoding_constraint=1)
        beams = []
        with torch.no_grad():
            for b in range(8):
                beams.append(O.beam_search(prm, oid, i2w, ins[0][b], ins[1][b], ins[3][b], ins[4][b:b + 1], beam_size=1,
                                           decoding_constraint=1, max_seq_len=T))
        _CACHE[V] = (prm, oid, ins, i2w, con, beams)
    return _CACHE[V]


@pytest.mark.parametrize('V', [64, 200])
def test_constrained_greedy_is_beam_1(V):
    prm, oid, ins, i2w, con, beams = case(V)
    for b, (_, scores, ids) in enumerate(beams):
        n = int(con['masks'][b].sum())
        assert con['seq'][b, :n].tolist() == ids[0], b
        assert abs((con['logprobs'][b] * con['masks'][b]).sum() - scores[0]) <= 1e-12 * max(1, n), b
    # the rules hold on every live position
    live = con['masks'] > 0
    assert not np.isin(con['seq'][live], [oid.pad, oid.sos, oid.unk]).any()
    prev = np.concatenate([np.full((8, 1), oid.sos), con['seq'][:, :-1]], 1)
    assert (con['seq'][live] != prev[live]).all()
    # ... and the plain greedy roll-out breaks them
    plain = cref.rollout(prm, oid, ins, T, 1)
    pl = plain['masks'] > 0
    pprev = np.concatenate([np.full((8, 1), oid.sos), plain['seq'][:, :-1]], 1)
    unk, rep = int((plain['seq'][pl] == oid.unk).sum()), int((plain['seq'][pl] == pprev[pl]).sum())
    print('V=%d: plain greedy emits <UNK> %d times and repeats its input %d times in %d live positions' % (
        V, unk, rep, int(pl.sum())))
    assert unk > 0 and rep > 0


@pytest.mark.parametrize('V', [64, 200])
def test_min_len_bans_eos_until_then(V):
    prm, oid, ins, i2w, con, _ = case(V)
    m4 = cref.rollout(prm, oid, ins, T, 1, suppress_special=True, decoding_constraint=1, min_len=4)
    assert (m4['masks'].sum(1) >= 5).all()            # (the first <EOS> can stand at t = 4: five live positions)
    assert not (m4['seq'][:, :4] == oid.eos).any()
    short = con['masks'].sum(1) < 4
    if short.any():                                   # rows that ended early now run on
        assert (m4['masks'].sum(1)[short] > con['masks'].sum(1)[short]).all()
    # t = min_len allows <EOS> again
    ok = cref.allowed(V, oid, 7, 4, True, 1, 4)
    assert ok[oid.eos] and not cref.allowed(V, oid, 7, 3, True, 1, 4)[oid.eos]
    assert not ok[7] and not ok[oid.unk] and ok.sum() == V - 4


def test_special_rule_is_off_when_pad_is_eos():
    class NoSos:
        pad = eos = sos = 0
        unk = 1
    ok = cref.allowed(10, NoSos, 5, 0, suppress_special=True, decoding_constraint=1)
    assert ok[0] and ok[1] and not ok[5] and ok.sum() == 9
    # the public API follows: without <SOS> in the vocabulary pad_id == eos_id, and suppress_special bans nothing
    i2w = ['<PAD>', '<UNK>'] + ['w%d' % i for i in range(2, 40)]
    cap = Captioner(i2w, synth.SENTIMENT_CATEGORIES, synth.TINY_SETTINGS)
    assert cap.pad_id == cap.eos_id
    assert cap._decode_constraints(True, 0, 0, T) is None
    c = cap._decode_constraints(True, 1, 2, T)
    assert (c.n_ban, c.no_repeat, c.first_id, c.min_len) == (0, 1, cap.sos_id, 2)


def test_the_struct_of_a_usual_vocabulary():
    cap = Captioner(synth.make_idx2word(64), synth.SENTIMENT_CATEGORIES, synth.TINY_SETTINGS)
    assert cap._decode_constraints(False, 0, 0, T) is None
    c = cap._decode_constraints(True, 1, 3, T)
    assert list(c.ban_ids[:c.n_ban]) == [cap.pad_id, cap.sos_id, cap.unk_id]
    assert (c.no_repeat, c.first_id, c.min_len) == (1, cap.sos_id, 3)


@pytest.mark.parametrize('kw', [dict(min_len=-1), dict(min_len=T + 1), dict(min_len=2.5), dict(min_len=True),
                                dict(suppress_special='yes'), dict(suppress_special=2), dict(decoding_constraint=2),
                                dict(decoding_constraint=None), dict(decoding_constraint=0.5)])
def test_bad_values_raise_before_the_device_is_touched(kw):
    st, w, i2w, prm, oid, ins = setup(64, torch.float32)
    cap = Captioner(i2w, synth.SENTIMENT_CATEGORIES, st).eval()          # CPU parameters, CPU tensors
    for sample_max in (0, 1):
        with pytest.raises(ValueError):
            cap.forward_rl(*ins, T, sample_max, **kw)
        with pytest.raises(ValueError):
            cap(*ins, T, sample_max, mode='rl', **kw)
    with pytest.raises(ValueError):
        cap.sample_captions(*ins, n=2, max_seq_len=T, **kw)


def test_replay_excludes_a_constraint():
    st, w, i2w, prm, oid, ins = setup(64, torch.float32)
    cap = Captioner(i2w, synth.SENTIMENT_CATEGORIES, st).eval()
    replay = torch.zeros(8, T, dtype=torch.long)
    for kw in (dict(suppress_special=True), dict(decoding_constraint=1), dict(min_len=1)):
        with pytest.raises(ValueError, match='_replay'):
            cap.forward_rl(*ins, T, 0, _replay=replay, **kw)
