"""Host side of the differentiable filtered roll-out (no GPU): the row formula against torch autograd, the new entry points
in the header and in the built library, and the CPU facts of every case tests/test_gpu_filtered_rl.py runs."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

import _filtered_rl_ref as FR
import _sample_filter_ref as ref
from insenticap_model_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.parametrize('tau', [0.5, 1.0, 2.5])
@pytest.mark.parametrize('top_k,top_p,banned', [(0, 1.0, ()), (5, 1.0, ()), (0, 0.8, ()), (8, 0.9, (0, 1, 3, 17)), (1, 1.0, ())])
def test_row_formula_is_the_autograd_of_the_filtered_log_softmax(tau, top_k, top_p, banned):
    """d log q(tok) / d x = (1 / tau)([v == tok] - [v in K] q_v) equals torch float64 autograd of
    log_softmax(x[K] / tau)[tok], for every token of the kept set; columns outside K are exactly zero; top_k = 1: the
    whole row is exactly zero."""
    rng = np.random.default_rng(int(tau * 10) + top_k)
    x = 3.0 * rng.standard_normal(97)
    x[17] = x.max() + 1.0                                  # a banned id inside the top ranks
    kept = FR.kept_ids(x, tau, top_k, top_p, banned)
    assert not set(kept) & set(banned)
    for tok in kept[:: max(1, len(kept) // 4)]:
        xt = torch.tensor(x, dtype=torch.float64, requires_grad=True)
        kt = torch.from_numpy(np.sort(kept))
        torch.log_softmax(xt[kt] / tau, dim=0)[int(np.nonzero(np.sort(kept) == tok)[0][0])].backward()
        got = FR.row_grad(x, tau, kept, int(tok), banned)
        np.testing.assert_allclose(got, xt.grad.numpy(), rtol=0, atol=1e-14)
        outside = np.setdiff1d(np.arange(97), kept)
        assert (got[outside] == 0.0).all()
        if top_k == 1:
            assert (got == 0.0).all()


def test_header_declares_and_library_exports_the_new_entry_points():
    hdr = open(os.path.join(ROOT, 'include', 'insenticap_hip.h')).read()
    for name in ('isc_logsoftmax_bwd_raw_filtered', 'isc_rollout_finalize_saved'):
        assert re.search(r'\bint\s+%s\s*\(' % name, hdr), name
        assert name in _lib.SIGNATURES
    assert 'isc_filter_saved' in hdr
    lib = ctypes.CDLL(_lib.LIB_PATH)
    for name in ('isc_logsoftmax_bwd_raw_filtered', 'isc_rollout_finalize_saved'):
        assert hasattr(lib, name), name
    # the existing structs keep their layout (the saved arrays travel in a struct of their own)
    assert ctypes.sizeof(_lib.SampleFilter) == 24 and ctypes.sizeof(_lib.DecodeConstraints) == 88
    assert ctypes.sizeof(_lib.FilterSaved) == 32


def test_flt_key_has_one_definition_shared_by_forward_and_backward():
    csrc = os.path.join(ROOT, 'insenticap_model_amd', 'csrc')
    defs = [f for f in sorted(os.listdir(csrc)) if re.search(r'isc_u64\s+flt_key\s*\(', open(os.path.join(csrc, f)).read())]
    assert defs == ['flt_key.h']
    for f in ('pointwise.hip', 'backward.hip'):
        src = open(os.path.join(csrc, f)).read()
        assert '#include "flt_key.h"' in src and 'flt_key(' in src


def test_reference_key_orders_like_the_reference_ranking():
    rng = np.random.default_rng(0)
    x = rng.standard_normal(200).astype(np.float32)
    x[10] = x[150] = x[42]                                   # ties: the smaller id first
    x[5], x[6] = 0.0, -0.0
    order = np.argsort(FR.flt_key(x, np.arange(200)), kind='stable')
    assert np.array_equal(order, ref.ranking(x.astype(np.float64)))


def test_filtered_call_with_gradients_must_ask_for_the_sampling_logprobs():
    """Without return_sampling_logprobs a filtered call with gradients is refused before the device (ValueError); with it
    the call is valid - on CPU tensors it gets as far as the library's loud error.  Default controls need no flag."""
    from insenticap_model_amd import Captioner, synth
    cap = Captioner(synth.make_idx2word(64), synth.SENTIMENT_CATEGORIES, synth.TINY_SETTINGS).train()
    d = synth.make_inputs(2, 64, synth.TINY_SETTINGS, regions=6, seq_len=4, seed=0)
    a = [torch.from_numpy(d[k]) for k in ('fc_feats', 'att_feats', 'cpt_words', 'senti_words', 'senti_labels')]
    for kw in (dict(temperature=0.7), dict(top_k=5), dict(top_p=0.9)):
        for group in (dict(), dict(captions_per_image=3)):
            with pytest.raises(ValueError, match='return_sampling_logprobs'):
                cap.forward_rl(*a, 4, 0, **kw, **group)
            with pytest.raises(_lib.HipLibraryError):
                cap.forward_rl(*a, 4, 0, return_sampling_logprobs=True, **kw, **group)
    for kw in (dict(), dict(return_sampling_logprobs=True), dict(_uniforms=torch.zeros(2, 4)),
               dict(generator=torch.Generator())):
        with pytest.raises(_lib.HipLibraryError):
            cap.forward_rl(*a, 4, 0, **kw)


CASES = [(name, n, m) for name in FR.CONTROLS for n in (1, 3) for m in (False, True)]


@pytest.fixture(scope='module')
def facts():
    return {c: FR.case_facts(*c) for c in CASES}


@pytest.mark.parametrize('case', CASES, ids=lambda c: '%s-n%d-%s' % (c[0], c[1], 'masks' if c[2] else 'nodrop'))
def test_cpu_facts_of_a_gpu_case(facts, case):
    """The fp32 and the fp64 oracle roll-out of the case draw the same tokens from the same kept set at every executed
    (row, step), no draw is within 2e-6 of a CDF boundary (RowCheck.near_boundary), and at least five steps run: the GPU
    test skips nothing and relaxes nothing."""
    ok, o = facts[case]
    assert ok and o['steps'] >= 5
    flt, cons = FR.split_controls(FR.CONTROLS[case[0]])
    if cons:          # the constraints bite: a banned id would have been kept otherwise somewhere
        assert all(len(f['ban']) >= 3 for f in o['facts'].values())


def test_the_gpu_cases_cover_the_edges(facts):
    """Among the cases: a row that ends at step 1, a step behind the early break, a top-k-bound and a top-p-bound live step."""
    outs = [o for _, o in facts.values()]
    assert any(bool((o['mk'].sum(1) == 2).any()) for o in outs)
    assert any(o['steps'] < FR.T for o in outs)
    live = [f['bound'] for o in outs for f in o['facts'].values() if f['live']]
    assert 'k' in live and 'p' in live
