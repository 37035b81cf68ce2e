"""Host side of teacher-forced XE training on n captions per image (no GPU): forward_xe's argument checks, the caption
collate with `captions_per_image`, the ctypes layout and host-side refusals of the entry points that learned row_div /
group, and the premise that the order of the caption rows is free (the XE loss masks by row)."""
import ctypes
import os
import subprocess

import numpy as np
import pytest
import torch

from insenticap_model_amd import Captioner, _lib, data, synth, train

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
E_SHAPE = -2
V, ST = 64, synth.TINY_SETTINGS


def make():
    return Captioner(synth.make_idx2word(V), synth.SENTIMENT_CATEGORIES, ST)


def cpu_inputs(I=2, n=3, T=4, labels='row'):
    img = synth.make_inputs(I, V, ST, regions=6, seq_len=T, seed=0)
    row = synth.make_inputs(I * n, V, ST, regions=1, seq_len=T, seed=1)
    lab = row['senti_labels'] if labels == 'row' else img['senti_labels']
    return [torch.from_numpy(x) for x in (img['fc_feats'], img['att_feats'], img['cpt_words'], row['captions'], lab)]


# ------------------------------------------------------------------------------------------------ forward_xe's checks
@pytest.mark.parametrize('n', [0, -2, 2.0, 1.5, '3', None, True])
@pytest.mark.parametrize('grad', [False, True])
def test_captions_per_image_must_be_a_positive_integer(n, grad):
    cap = make()
    with torch.set_grad_enabled(grad), pytest.raises(ValueError, match='captions_per_image must be an integer >= 1'):
        cap.forward_xe(*cpu_inputs(), 0.0, captions_per_image=n)
    with torch.set_grad_enabled(grad), pytest.raises(ValueError, match='captions_per_image must be an integer >= 1'):
        cap(*cpu_inputs(), 0.0, mode='xe', captions_per_image=n)


def test_row_and_label_counts_are_checked_before_the_device():
    """Every refusal is a ValueError raised on CPU tensors and CPU parameters: a call that got as far as the device
    would raise HipLibraryError here (tests/test_abi_and_host.py::test_product_fails_loudly_on_cpu)."""
    cap = make()
    fc, att, cpt, caps, lab = cpu_inputs(I=2, n=3)
    for grad in (False, True):
        with torch.set_grad_enabled(grad):
            with pytest.raises(ValueError, match='caption rows'):
                cap.forward_xe(fc, att, cpt, caps[:5], lab, 0.0, captions_per_image=3)
            with pytest.raises(ValueError, match='caption rows'):
                cap.forward_xe(fc, att, cpt, caps, lab, 0.0, captions_per_image=2)
            with pytest.raises(ValueError, match='senti_labels'):
                cap.forward_xe(fc, att, cpt, caps, lab[:4], 0.0, captions_per_image=3)
            # [I*n] and [I] labels pass the checks: the call goes on to the device, where CPU parameters are the
            # library's loud error
            for labels in (lab, lab[:2]):
                with pytest.raises(_lib.HipLibraryError):
                    cap.forward_xe(fc, att, cpt, caps, labels, 0.0, captions_per_image=3)


def test_captions_per_image_1_is_the_plain_call():
    cap = make()
    fc, att, cpt, caps, lab = cpu_inputs(I=2, n=1)
    assert Captioner._check_group_xe(1, fc, caps[:1], lab[:7]) == 1           # (n = 1 adds no refusal)
    with pytest.raises(_lib.HipLibraryError):
        cap.forward_xe(fc, att, cpt, caps, lab, 0.0, captions_per_image=1)


def test_the_merged_step_and_the_training_wrapper_refuse_or_pass_it_on():
    """mode='xe_seq2seq' with n > 1 is a ValueError (out of scope); train.xe_forward_backward takes the keyword, checks
    it and refuses the merged route for it - all before the device."""
    cap = make()
    fc, att, cpt, caps, lab = cpu_inputs(I=2, n=3)
    s = synth.make_inputs(4, V, ST, regions=1, seq_len=4, seed=2)
    s_args = [torch.from_numpy(s[k]) for k in ('captions', 'cpt_words', 'senti_words', 'senti_labels')]
    with pytest.raises(ValueError, match='xe_seq2seq'):
        cap(fc, att, cpt, caps, lab, 0.0, *s_args, mode='xe_seq2seq', captions_per_image=3)
    fact = (fc, att, caps, [3] * 6, cpt)
    with pytest.raises(ValueError, match='captions_per_image must be an integer >= 1'):
        train.xe_forward_backward(cap, None, None, None, fact, lab, captions_per_image=0)
    with pytest.raises(ValueError, match='merged'):
        train.xe_forward_backward(cap, None, None, None, fact, lab, pair=True, captions_per_image=3)
    with pytest.raises(_lib.HipLibraryError):          # accepted: on to the un-merged XE unroll (CPU parameters)
        train.xe_forward_backward(cap, None, None, None, fact, lab, captions_per_image=3)


# ------------------------------------------------------------------------------------------------ the collate
def _dataset():
    """Four images with 5, 2, 7 and 1 captions of different lengths (dataloader.py's CaptionDataset items)."""
    rng = np.random.default_rng(3)
    items = []
    for u, n_caps in enumerate((5, 2, 7, 1)):
        caps = [[1] + rng.integers(4, V, size=int(rng.integers(2, 12))).tolist() + [2] for _ in range(n_caps)]
        items.append(('img%d' % u, rng.random(8, dtype=np.float32) + u, rng.random((3, 8), dtype=np.float32) + u, caps,
                      rng.integers(4, V, size=int(rng.integers(1, 7))).tolist()))
    return items


@pytest.mark.parametrize('n', [1, 3, 5])
@pytest.mark.parametrize('width', [None, 'full', 4])
def test_caption_collate_with_captions_per_image(n, width):
    ds = _dataset()
    kw = dict(pad_index=0, max_seq_len=10, num_concepts=5, caption_width=width)
    fns, fc, att, (caps, lengths), cpts = data.create_collate_fn('caption', captions_per_image=n, **kw)(ds)
    I = len(ds)
    assert tuple(fc.shape) == (I, 8) and tuple(att.shape) == (I, 3, 8) and tuple(cpts.shape) == (I, 5)
    assert caps.shape[0] == I * n == len(lengths) == len(fns)
    for i, (fn, f, a, cs, cp) in enumerate(ds):
        assert np.array_equal(fc[i].numpy(), f) and np.array_equal(att[i].numpy(), a)       # each image once, in order
        assert cpts[i].tolist() == (cp + [0] * 5)[:5]
        for j in range(n):
            want = cs[j % len(cs)][:10]                  # the first n captions, cycled from the first
            r = i * n + j
            assert fns[r] == fn and lengths[r] == len(want) - 1
            assert caps[r, :len(want)].tolist() == want and not caps[r, len(want):].any()
    # the default collate's rows of the same captions, up to the documented permutation (image-major instead of
    # sorted by length): the same multiset of (fn, caption, length, features) rows
    picked = [(fn, f, a, [cs[j % len(cs)] for j in range(n)], cp) for fn, f, a, cs, cp in ds]
    fns0, fc0, att0, (caps0, lengths0), cpts0 = data.create_collate_fn('caption', **kw)(picked)
    assert caps0.shape == caps.shape
    key = lambda f, c, l, x: (f, tuple(c.tolist()), l, float(x.sum()))
    rows = sorted(key(fns[r], caps[r], lengths[r], fc[r // n]) for r in range(I * n))
    rows0 = sorted(key(fns0[r], caps0[r], lengths0[r], fc0[r]) for r in range(I * n))
    assert rows == rows0


def test_caption_collate_group_composes_with_dedup_stores_and_the_loader(tmp_path):
    ds = _dataset()
    ref = data.create_collate_fn('caption', captions_per_image=3)(ds)
    dd = data.create_collate_fn('caption', captions_per_image=3, dedup=True)(ds)           # dedup: nothing left to do
    assert torch.equal(ref[1], dd[1]) and torch.equal(ref[2], dd[2]) and torch.equal(ref[3][0], dd[3][0])
    fns = [x[0] for x in ds]
    path = str(tmp_path / 'fc.npy')
    data.FeatureStore.write(path, fns, np.stack([x[1] for x in ds]), dtype=np.float16)
    store = data.FeatureStore(path)
    st = data.create_collate_fn('caption', captions_per_image=3)([(x[0], store[x[0]], x[2], x[3], x[4]) for x in ds])
    assert st[1].dtype == torch.float16 and tuple(st[1].shape) == (4, 8)
    loader = data.get_caption_dataloader({x[0]: x[1] for x in ds}, {x[0]: x[2] for x in ds}, {x[0]: x[3] for x in ds},
                                         {x[0]: x[4] for x in ds}, 0, 16, 5, batch_size=2, shuffle=False,
                                         captions_per_image=2)
    batches = list(loader)
    assert len(batches) == 2 and all(b[1].shape[0] == 2 and b[3][0].shape[0] == 4 for b in batches)
    with pytest.raises(ValueError, match='captions_per_image'):
        data.create_collate_fn('caption', captions_per_image=0)
    with pytest.raises(ValueError, match='captions_per_image'):
        data.create_collate_fn('scs', captions_per_image=2)


# ------------------------------------------------------------------------------------------------ library, host side
def test_group_entry_points_and_row_div_are_refused_on_the_host():
    """ISC_E_SHAPE from the entry points' checks, before any launch - no GPU needed: rows % row_div != 0 and a dP / dV
    to accumulate into with row_div > 1; rows % group != 0 and n*T beyond the LDS image; isc_step_bwd with row_div and
    the merged step's pair_rows_c."""
    lib = _lib.load()
    assert lib.isc_abi_version() >= 2
    buf = (ctypes.c_float * 64)()
    a = ctypes.addressof(buf)
    s = _lib.ScanBwdProblem()
    s.P = s.V = s.q = s.w = s.alpha = s.dout = s.dq = s.dw_rows = s.de_out = a
    s.R, s.A, s.D, s.rows, s.row_div = 1, 4, 4, 4, 3
    assert lib.isc_attn_scan_bwd(ctypes.byref(s), 1, 4, None) == E_SHAPE                # 4 % 3
    s.rows, s.row_div, s.dP = 6, 3, a
    assert lib.isc_attn_scan_bwd(ctypes.byref(s), 1, 6, None) == E_SHAPE                # dP with row_div
    s.dP, s.dV = None, a
    assert lib.isc_attn_scan_bwd(ctypes.byref(s), 1, 6, None) == E_SHAPE                # dV with row_div
    assert lib.isc_attn_dv_from_alpha_group(a, 4, 1, a, 4, 3, 2, 1, 4, a, 0, None) == E_SHAPE      # 4 % 3
    assert lib.isc_attn_dv_from_alpha_group(a, 4, 1, a, 4, 0, 2, 1, 4, a, 0, None) == E_SHAPE      # group 0
    assert lib.isc_attn_dv_from_alpha_group(a, 4, 1, a, 4, 4, 3751, 1, 4, a, 0, None) == E_SHAPE   # 15004 terms
    assert lib.isc_attn_dp_from_de_group(a, a, None, a, a, 4, 3, 2, 1, 4, a, None) == E_SHAPE
    assert lib.isc_attn_dp_from_de_group(a, a, None, a, a, 4, 4, 3751, 1, 4, a, None) == E_SHAPE
    bp = _lib.StepBwdPlan()
    bp.rows, bp.row_div, bp.att_e, bp.words_e, bp.pair_rows_c = 6, 3, a, a, 2
    assert lib.isc_step_bwd(ctypes.byref(bp), None) == E_SHAPE
    bp.pair_rows_c, bp.rows = 0, 7
    assert lib.isc_step_bwd(ctypes.byref(bp), None) == E_SHAPE


def test_ctypes_layout_of_the_new_fields_matches_the_header(tmp_path):
    prog = r'''
#include <stdio.h>
#include <stddef.h>
#include "insenticap_hip.h"
int main(void) {
  printf("%zu %zu %zu %zu %zu\n", offsetof(isc_scan_bwd_problem, row_div), sizeof(isc_scan_bwd_problem),
         offsetof(isc_step_bwd_plan, row_div), sizeof(isc_step_bwd_plan), offsetof(isc_step_plan, pre_rows));
  return 0;
}
'''
    cfile, exe = str(tmp_path / 'layout.c'), str(tmp_path / 'layout')
    open(cfile, 'w').write(prog)
    subprocess.check_call(['gcc', '-I', os.path.join(ROOT, 'include'), cfile, '-o', exe])
    got = [int(x) for x in subprocess.check_output([exe]).decode().split()]
    L = _lib
    assert got == [L.ScanBwdProblem.row_div.offset, ctypes.sizeof(L.ScanBwdProblem), L.StepBwdPlan.row_div.offset,
                   ctypes.sizeof(L.StepBwdPlan), L.StepPlan.pre_rows.offset]
    assert L.ScanBwdProblem.row_div.offset == L.ScanBwdProblem.rows.offset + 4           # (the former padding word)
    assert L.StepBwdPlan.row_div.offset == L.StepBwdPlan.de_s.offset + 8                 # appended
    assert L.StepPlan.pre_rows.offset == L.StepPlan.row_div.offset + 4
    assert L.ScanBwdProblem().row_div == 0 and L.StepBwdPlan().row_div == 0 and L.StepPlan().pre_rows == 0


# ------------------------------------------------------------------------------------------------ the order is free
def test_xe_loss_of_image_major_rows_equals_the_loss_of_length_sorted_rows():
    """The premise of leaving the rows image-major: the oracle's XE loss (float64) of the expanded batch in image-major
    order equals the loss of the same rows sorted by length, as the reference's collate orders them, to 1e-12."""
    from oracle import captioner_oracle as O
    I, n, T = 3, 4, 8
    img = synth.make_inputs(I, V, ST, regions=6, seq_len=T, seed=5)
    row = synth.make_inputs(I * n, V, ST, regions=1, seq_len=T, seed=6)
    p = O.to_params(synth.make_weights(V, ST, seed=1), dtype=torch.float64)
    ids = O.Ids(synth.make_idx2word(V), synth.SENTIMENT_CATEGORIES)
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a))
    rep = lambda a: t(a).repeat_interleave(n, 0)
    fc, att, cpt = rep(img['fc_feats']).double(), rep(img['att_feats']).double(), rep(img['cpt_words'])
    caps, lab, lens = t(row['captions']), t(row['senti_labels']), [int(x) for x in row['lengths']]
    assert lens != sorted(lens, reverse=True)

    def loss(order):
        o = torch.as_tensor(order)
        logp, _, _ = O.forward_xe(p, ids, fc[o], att[o], cpt[o], caps[o], lab[o])
        return float(O.xe_criterion(logp, caps[o][:, 1:], [lens[i] for i in order]))
    by_length = sorted(range(I * n), key=lambda i: -lens[i])
    assert abs(loss(list(range(I * n))) - loss(by_length)) <= 1e-12
