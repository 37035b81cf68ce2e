"""CPU-only checks of the filtered sampler (temperature / top-k / top-p): the entry point is declared, exported and
bound; the ctypes struct matches the C layout; the public signatures; argument checks raise before any device work; and
the fp64 reference sampler the GPU tests compare against (tests/_sample_filter_ref.py) obeys its own definition."""
import ctypes
import inspect
import os
import re
import subprocess

import numpy as np
import pytest
import torch

import _sample_filter_ref as ref
from conftest import ROOT
from insenticap_model_amd import Captioner, _build, _lib, ops, synth

NAME = 'isc_rollout_finalize_filtered'


def declared_functions():
    src = open(os.path.join(ROOT, 'include', 'insenticap_hip.h')).read()
    src = re.sub(r'/\*.*?\*/', '', src, flags=re.S)
    return sorted(set(re.findall(r'\b(isc_[a-z0-9_]+)\s*\(', src)))


def test_entry_point_is_declared_exported_and_bound():
    assert NAME in declared_functions()
    lib = ctypes.CDLL(_build.build())
    assert hasattr(lib, NAME)
    res, args = _lib.SIGNATURES[NAME]
    assert res is ctypes.c_int and len(args) == 3
    assert args[0]._type_ is _lib.RolloutStep and args[1]._type_ is _lib.SampleFilter


def test_sample_filter_struct_layout_matches_c(tmp_path):
    prog = r'''
#include <stdio.h>
#include <stddef.h>
#include "insenticap_hip.h"
int main(void) {
  printf("%zu %zu %zu %zu %zu %zu\n", sizeof(isc_sample_filter), offsetof(isc_sample_filter, temperature),
         offsetof(isc_sample_filter, top_k), offsetof(isc_sample_filter, top_p),
         offsetof(isc_sample_filter, sampling_logprobs), sizeof(isc_rollout_step));
  return 0;
}
'''
    cfile, exe = str(tmp_path / 'layout.c'), str(tmp_path / 'layout')
    open(cfile, 'w').write(prog)
    subprocess.check_call(['gcc', '-I', os.path.join(ROOT, 'include'), cfile, '-o', exe])
    got = [int(x) for x in subprocess.check_output([exe]).decode().split()]
    F = _lib.SampleFilter
    assert got == [ctypes.sizeof(F), F.temperature.offset, F.top_k.offset, F.top_p.offset, F.sampling_logprobs.offset,
                   ctypes.sizeof(_lib.RolloutStep)]


def test_library_rejects_bad_controls_before_any_launch():
    lib = _lib.load()
    st, f = _lib.RolloutStep(), _lib.SampleFilter()
    assert lib.isc_rollout_finalize_filtered(None, ctypes.byref(f), None) == -1
    assert lib.isc_rollout_finalize_filtered(ctypes.byref(st), None, None) == -1
    # every pointer "set" (never dereferenced: the call returns on the argument check), a plausible geometry
    for k in ('part_max', 'part_sum', 'part_idx', 'logits', 'sample_u', 'seq', 'seq_logprobs', 'seq_masks', 'unfinished',
              'alive', 'emb'):
        setattr(st, k, 4096)
    st.B, st.V, st.T, st.t, st.n_tile, st.W, st.ld_logits = 2, 64, 4, 0, 1, 32, 64
    for tau, k, p in [(0.0, 0, 1.0), (-1.0, 0, 1.0), (float('nan'), 0, 1.0), (float('inf'), 0, 1.0), (1.0, -1, 1.0),
                      (1.0, 0, 0.0), (1.0, 0, -0.5), (1.0, 0, float('nan'))]:
        f.temperature, f.top_k, f.top_p = tau, k, p
        assert lib.isc_rollout_finalize_filtered(ctypes.byref(st), ctypes.byref(f), None) == -2, (tau, k, p)


def test_public_signatures():
    sig = inspect.signature(Captioner.forward_rl).parameters
    want = [('temperature', 1.0), ('top_k', 0), ('top_p', 1.0), ('generator', None), ('return_sampling_logprobs', False),
            ('_uniforms', None)]
    names = list(sig)
    for name, default in want:
        assert name in sig and sig[name].default == default, name
        assert names.index(name) > names.index('_masks')           # after the existing arguments
    sc = inspect.signature(Captioner.sample_captions).parameters
    assert list(sc)[:12] == ['self', 'fc_feats', 'att_feats', 'cpt_words', 'senti_words', 'senti_labels', 'n', 'max_seq_len',
                             'temperature', 'top_k', 'top_p', 'generator']
    assert (sc['n'].default, sc['max_seq_len'].default, sc['temperature'].default, sc['top_k'].default,
            sc['top_p'].default, sc['generator'].default) == (1, 16, 1.0, 0, 1.0, None)
    assert callable(ops.rollout_finalize_filtered)


def _cpu_call():
    cap = Captioner(synth.make_idx2word(64), synth.SENTIMENT_CATEGORIES, synth.TINY_SETTINGS).eval()
    d = synth.make_inputs(2, 64, synth.TINY_SETTINGS, regions=6, seq_len=4, seed=0)
    a = [torch.from_numpy(d[k]) for k in ('fc_feats', 'att_feats', 'cpt_words', 'senti_words', 'senti_labels')]
    return cap, a


@pytest.mark.parametrize('kw', [dict(temperature=0.0), dict(temperature=-0.5), dict(temperature=float('nan')),
                                dict(temperature=float('inf')), dict(top_k=-1), dict(top_p=0.0), dict(top_p=-0.1),
                                dict(top_p=float('nan'))])
def test_out_of_domain_controls_raise_value_error(kw):
    """... on CPU parameters, without a GPU: the checks run before any device work (a valid call on CPU parameters
    raises HipLibraryError, tests/test_abi_and_host.py)."""
    cap, a = _cpu_call()
    with torch.no_grad():
        with pytest.raises(ValueError):
            cap.forward_rl(*a, 4, 0, **kw)
        with pytest.raises(ValueError):
            cap.sample_captions(*a, n=2, max_seq_len=4, **kw)
    with pytest.raises(ValueError):
        ops.check_sample_filter(kw.get('temperature', 1.0), kw.get('top_k', 0), kw.get('top_p', 1.0))


@pytest.mark.parametrize('kw', [dict(temperature=0.7), dict(top_k=5), dict(top_p=0.9), dict(return_sampling_logprobs=True),
                                dict(_uniforms=torch.zeros(2, 4))])
def test_controls_with_greedy_decoding_raise(kw):
    cap, a = _cpu_call()
    with torch.no_grad():
        with pytest.raises(ValueError):
            cap.forward_rl(*a, 4, 1, **kw)


def test_filtered_sampling_with_gradients_raises():
    cap, a = _cpu_call()
    assert cap._needs_grad()
    with pytest.raises(ValueError, match='inference-only'):
        cap.forward_rl(*a, 4, 0, top_p=0.9)
    with pytest.raises(ValueError):
        cap.sample_captions(*a, n=0)


# ----------------------------------------------------------------------------- the reference sampler itself
def _rows(seed, B=24, V=97):
    g = np.random.default_rng(seed)
    return 4.0 * g.standard_normal((B, V)), g.random(B)


def test_reference_top_k_1_and_vanishing_top_p_are_the_arg_max():
    x, u = _rows(1)
    for b in range(x.shape[0]):
        for uu in (0.0, 1e-9, u[b], 0.999999):
            assert ref.draw(x[b], uu, 1.3, 1, 1.0) == int(x[b].argmax())
            assert ref.draw(x[b], uu, 0.7, 0, 1e-12) == int(x[b].argmax())
        assert ref.kept_count(x[b], 1.0, 0, 1.0) == x.shape[1] and ref.kept_count(x[b], 1.0, 500, 1.0) == x.shape[1]


def test_reference_kept_sets_are_nested_in_k_and_p():
    x, _ = _rows(2)
    for b in range(x.shape[0]):
        order = ref.ranking(x[b])
        prev = 0
        for k in (1, 2, 5, 20, 96, 97, 0):
            n = ref.kept_count(x[b], 0.9, k, 1.0, order)
            assert n >= prev and (n == k if 0 < k < 97 else n == 97)
            prev = n
        prev = 0
        for p in (1e-6, 0.1, 0.5, 0.9, 0.99, 0.999999, 1.0):
            n = ref.kept_count(x[b], 1.2, 0, p, order)
            assert n >= prev >= 0 and n >= 1
            prev = n
            # top-p after top-k: a prefix of the top-k prefix, and never longer than top-p alone
            assert ref.kept_count(x[b], 1.2, 10, p, order) <= min(10, n)
        # the defining inequality, on one case
        w = ref.masses(x[b], 1.2)[order]
        n = ref.kept_count(x[b], 1.2, 0, 0.9, order)
        assert w[:n - 1].sum() < 0.9 * w.sum() <= w[:n].sum() + 1e-15


def test_reference_orders_ties_by_the_smaller_id():
    x = np.array([1.0, 3.0, 3.0, -2.0, 3.0, 1.0, 0.0, -0.0])
    assert ref.ranking(x).tolist() == [1, 2, 4, 0, 5, 6, 7, 3]
    assert sorted(ref.kept_set(x, 1.0, 2, 1.0).tolist()) == [1, 2]                 # id 4 ties with them and loses
    assert sorted(ref.kept_set(x, 1.0, 4, 1.0).tolist()) == [0, 1, 2, 4]
    # three equal masses e^0 in front: 1/3 of the kept mass each; the prefix ends with the rank whose predecessors reach p
    W = 3 + 2 * np.exp(-2.0) + 2 * np.exp(-3.0) + np.exp(-5.0)
    assert ref.kept_count(x, 1.0, 0, 1.5 / W) == 2 and ref.kept_count(x, 1.0, 0, 2.5 / W) == 3
    # the draw walks the kept ids in vocabulary order
    assert [ref.draw(x, u, 1.0, 3, 1.0) for u in (0.0, 0.33, 0.34, 0.66, 0.67, 0.99)] == [1, 1, 2, 2, 4, 4]
    # temperature does not reorder
    assert ref.ranking(x / 0.3).tolist() == ref.ranking(x).tolist()


def test_reference_row_check_accepts_its_own_draw():
    x, u = _rows(3, B=40, V=130)
    strict = 0
    for b in range(x.shape[0]):
        rc = ref.RowCheck(x[b], u[b], 1.3, 50, 0.9)
        assert rc.n_lo <= rc.n <= rc.n_hi <= 50 and rc.n_hi - rc.n_lo <= 1
        tok = rc.ref_token()
        assert rc.token_ok(tok) and tok in ref.kept_set(x[b], 1.3, 50, 0.9)
        outside = [i for i in range(130) if i not in set(rc.order[:rc.n_hi].tolist())]
        assert not rc.token_ok(outside[0])
        strict += rc.strict
        lp = rc.sampling_logprob(tok)
        w = ref.masses(x[b], 1.3)
        assert abs(lp - np.log(w[tok] / w[rc.order[:rc.n]].sum())) < 1e-12
    assert strict >= 38
