"""What test_gpu_widths.py and the width cases of test_gpu_rows.py rest on, asserted on the CPU for every width set of
tests/_widths.py: the fp64 oracle's greedy roll-out has no near-tie (the trusted prefix is every live step), its fp32
and fp64 arithmetic agree on tokens and beams, beam scores are well separated, the oracle's own fp32 gradients lie within
a third of the gradient bound of its fp64 ones; the product's constructor takes every set, refuses what it documents, and
its two selectors (few-row step, fused gate) say for each set what the table says."""
import numpy as np
import pytest
import torch

import _widths as Wd
from conftest import trusted_prefix
from insenticap_model_amd import Captioner, synth
from test_gpu_train_sizes import GRAD_RTOL, _oracle_iteration

NAMES = list(Wd.WIDTHS)


@pytest.mark.parametrize('name', NAMES)
def test_greedy_rollout_has_no_near_tie_and_fp32_equals_fp64(name):
    seq, lp, mk, _, _, margins = Wd.oracle_greedy(name)
    live = int(mk.sum())
    n = trusted_prefix(margins.numpy(), mk.numpy(), Wd.MARGIN)
    covered = sum(int(mk[b, :n[b]].sum()) for b in range(Wd.B))
    print('%s: live steps %d, smallest margin %.2e' % (name, live, float(margins[mk > 0].min())))
    assert live >= 60 and covered == live and (n == Wd.T).all()          # trusted share 1.0
    seq32, lp32, mk32, _, _, _ = Wd.oracle_greedy(name, dtype=torch.float32)
    assert torch.equal(seq32, seq) and torch.equal(mk32.double(), mk)
    live_m = mk[:, :lp.shape[1]] > 0                                     # (the oracle stops once every row has ended)
    assert lp32.shape == lp.shape and float((lp32.double() - lp)[live_m].abs().max()) <= 2.5e-6
    # the few-row cases decode the first 4 and 7 rows alone: rows are independent
    for rows in (4, 7):
        s = Wd.oracle_greedy(name, rows=rows)[0]
        assert torch.equal(s, seq[:rows])


@pytest.mark.parametrize('name', NAMES)
def test_beams_are_well_separated_and_fp32_equals_fp64(name):
    for image in range(Wd.B):
        _, s64, i64 = Wd.oracle_beams(name, image)
        _, s32, i32 = Wd.oracle_beams(name, image, dtype=torch.float32)
        assert i32 == i64 and len(i64) == 3, (name, image)
        assert len({tuple(x) for x in i64}) == 3
        gaps = np.abs(np.diff(np.asarray(s64)))
        assert (gaps > Wd.MARGIN).all(), (name, image, gaps)
        np.testing.assert_allclose(s32, s64, atol=1e-4)


@pytest.mark.parametrize('name', Wd.SMALL)
def test_fp32_oracle_gradients_within_a_third_of_the_bound(name):
    st, w, d, s2s = Wd.setup(name)
    l32, g32, _ = _oracle_iteration(w, Wd.V, d, s2s)
    l64, g64, _ = _oracle_iteration(w, Wd.V, d, s2s, dtype=torch.float64)
    assert len(g64) == 32 and set(g32) == set(g64)
    np.testing.assert_allclose(l32, l64, rtol=1e-5)
    worst = 0.0
    for k, ref in g64.items():
        scale = np.abs(ref).max()
        if scale < 1e-12:
            continue
        worst = max(worst, float(np.abs(g32[k] - ref).max() / scale))
    print('%s: worst fp32-oracle gradient error %.2e of the tensor max' % (name, worst))
    assert worst <= GRAD_RTOL / 3


@pytest.mark.parametrize('name', NAMES)
def test_constructor_takes_the_set_and_state_dict_has_the_reference_shapes(name):
    st = Wd.WIDTHS[name]['settings']
    cap = Captioner(Wd.idx2word(), synth.SENTIMENT_CATEGORIES, st)
    sd = cap.state_dict()
    shapes = synth.param_shapes(Wd.V, st)
    assert list(sd) == list(shapes)
    for k, shape in shapes.items():
        assert tuple(sd[k].shape) == tuple(shape), k
    dims = {st[k] for k in ('feat_emb_dim', 'rnn_hid_dim', 'att_hid_dim')}
    assert len(dims) >= 2                              # the point of the set: not all widths equal


def test_constructor_refusals():
    st = dict(Wd.WIDTHS['all_differ']['settings'])
    with pytest.raises(ValueError):
        Captioner(Wd.idx2word(), synth.SENTIMENT_CATEGORIES, dict(st, word_emb_dim=st['feat_emb_dim'] + 32))
    for key in ('rnn_hid_dim', 'att_hid_dim', 'att_feat_dim', 'fc_feat_dim'):
        with pytest.raises(ValueError):
            Captioner(Wd.idx2word(), synth.SENTIMENT_CATEGORIES, dict(st, **{key: st[key] + 16}))
    with pytest.raises(ValueError):                    # W == E, both no multiple of 32
        Captioner(Wd.idx2word(), synth.SENTIMENT_CATEGORIES, dict(st, word_emb_dim=48, feat_emb_dim=48))


class _GateTables:
    """Stand-in for a prologue's result: the gate tables exist exactly where Captioner._prologue would build them."""

    def __init__(self, st, rows):
        self.gate_Gc = self.gate_Gs = object() if Wd.fused_gate_eligible(st, rows) else None


@pytest.mark.parametrize('name', NAMES)
def test_few_row_step_and_fused_gate_eligibility_is_the_tables(name):
    c = Wd.WIDTHS[name]
    st = c['settings']
    cap = Captioner(Wd.idx2word(), synth.SENTIMENT_CATEGORIES, st)
    assert Wd.fused_gate_eligible(st, Wd.B) == c['rows_step']
    assert Wd.fused_gate_eligible(st, Captioner.GATE_FUSED_MAX_ROWS) == c['rows_step']
    assert not Wd.fused_gate_eligible(st, Captioner.GATE_FUSED_MAX_ROWS + 1)
    for rows in (1, 4, 7, 8):
        assert cap._rows_step_ok(rows, _GateTables(st, rows)) == c['rows_step'], rows
    assert not cap._rows_step_ok(9, _GateTables(st, 9))
    # with the tables present the widths alone decide (all_differ, a_wide: A != E)
    both = _GateTables(Wd.H_WIDE, 4)
    assert cap._rows_step_ok(4, both) == c['rows_step']
    cap.rows_step = False
    assert not cap._rows_step_ok(4, both)
