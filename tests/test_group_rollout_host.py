"""Host side of captions_per_image (no GPU): forward_rl's argument checks, the ISC_E_SHAPE rejections of the three entry
points that learned row_div / pre_div, and the ctypes layout of the three new fields against the C header."""
import ctypes
import os
import subprocess

import pytest
import torch

from insenticap_model_amd import Captioner, _lib, synth

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
E_SHAPE = -2


def make():
    return Captioner(synth.make_idx2word(64), synth.SENTIMENT_CATEGORIES, synth.TINY_SETTINGS)


def cpu_inputs(B=2, T=4):
    d = synth.make_inputs(B, 64, synth.TINY_SETTINGS, regions=6, seq_len=T, seed=0)
    return [torch.from_numpy(d[k]) for k in ('fc_feats', 'att_feats', 'cpt_words', 'senti_words', 'senti_labels')]


@pytest.mark.parametrize('n', [0, -2, 2.0, 1.5, '3', None, True])
def test_captions_per_image_must_be_a_positive_integer(n):
    cap = make().eval()
    with torch.no_grad(), pytest.raises(ValueError, match='captions_per_image'):
        cap.forward_rl(*cpu_inputs(), 4, 0, captions_per_image=n)


def test_grouped_call_refuses_greedy_training_gradients_and_masks_before_the_device():
    """Every refusal is a ValueError raised on CPU tensors: a call that got as far as the device would raise
    HipLibraryError here (tests/test_abi_and_host.py::test_product_fails_loudly_on_cpu)."""
    a = cpu_inputs()
    cap = make().eval()
    with torch.no_grad():
        with pytest.raises(ValueError, match='sample_max=0'):
            cap.forward_rl(*a, 4, 1, captions_per_image=3)
        with pytest.raises(ValueError, match='_masks'):
            cap.forward_rl(*a, 4, 0, captions_per_image=3, _masks={})
    with pytest.raises(ValueError, match='inference-only'):           # gradients enabled
        cap.forward_rl(*a, 4, 0, captions_per_image=3)
    cap.train()
    with torch.no_grad(), pytest.raises(ValueError, match='inference-only'):
        cap.forward_rl(*a, 4, 0, captions_per_image=3)
    with pytest.raises(ValueError):                                   # sample_captions hands the same checks on
        make().sample_captions(*a, n=0, share_image=True)


@pytest.mark.parametrize('sample_max', [0, 1])
def test_captions_per_image_1_is_accepted_wherever_the_call_is_valid_today(sample_max):
    """n = 1 adds no refusal - greedy, training mode, gradients and masks included - and the call goes where it goes
    today: on CPU parameters that is the library's loud error, not a ValueError."""
    a = cpu_inputs()
    cap = make()
    assert cap._check_captions_per_image(1, 1, {'fc': None}) == 1      # greedy, masks, train mode, gradients on
    cap.eval()
    for kw in (dict(), dict(captions_per_image=1)):
        with torch.no_grad(), pytest.raises(_lib.HipLibraryError):
            cap.forward_rl(*a, 4, sample_max, **kw)
    with pytest.raises(_lib.HipLibraryError):                          # gradients enabled
        cap.forward_rl(*a, 4, sample_max, captions_per_image=1)
    import numpy as np
    with torch.no_grad():
        assert cap._check_captions_per_image(np.int64(4), 0, None) == 4    # integer types other than int


def _fake(n_floats=0):
    return ctypes.c_void_p(0x10000 + 16 * n_floats)     # a non-null, 16-byte aligned address that is never read


def test_entry_points_reject_ragged_groups_and_excluded_combinations():
    """rows % row_div != 0 and the combinations a grouped step excludes return ISC_E_SHAPE on the host, before any
    launch (no device here: a launch would fail otherwise)."""
    lib = _lib.load()
    # isc_attn_scan_fwd
    s = _lib.ScanProblem()
    s.P = s.V = s.q = s.w = s.out = _fake()
    s.R, s.A, s.D = 6, 32, 32
    s.row_div = 3
    assert lib.isc_attn_scan_fwd(ctypes.byref(s), 1, 7, None) == E_SHAPE          # 7 rows in groups of 3
    s.rows = 8
    assert lib.isc_attn_scan_fwd(ctypes.byref(s), 1, 9, None) == E_SHAPE          # the problem's own row count
    s.rows, s.row_div, s.R = 0, 2, 20000
    assert lib.isc_attn_scan_fwd(ctypes.byref(s), 1, 8, None) == E_SHAPE          # scores beyond the LDS budget
    # isc_lstm_fwd
    l = _lib.LstmProblem()
    l.seg[0].A = l.seg[0].W = _fake()
    l.seg[0].lda = l.seg[0].ldw = l.seg[0].K = 32
    l.nseg, l.M, l.H = 1, 7, 32
    l.c_prev = l.h_out = l.c_out = l.pre = _fake()
    l.pre_div = 3
    assert lib.isc_lstm_fwd(ctypes.byref(l), None) == E_SHAPE                     # 7 rows, 3 per image
    l.M, l.pre, l.b_ih, l.b_hh = 6, None, _fake(), _fake()
    assert lib.isc_lstm_fwd(ctypes.byref(l), None) == E_SHAPE                     # pre_div without `pre`
    # isc_step_fwd
    p = _lib.StepPlan()
    p.rows, p.H, p.E, p.A, p.W, p.V, p.R, p.Mw = 7, 32, 32, 32, 32, 64, 6, 3
    p.att_e = p.words_e = _fake()
    p.row_div = 3
    assert lib.isc_step_fwd(ctypes.byref(p), None) == E_SHAPE                     # 7 rows, 3 per image
    p.rows = 6
    p.gate_Gc = p.gate_Gs = _fake()
    assert lib.isc_step_fwd(ctypes.byref(p), None) == E_SHAPE                     # fused gate scan
    p.gate_Gc = p.gate_Gs = None
    p.pair_rows_c = 3
    p.v = _fake()
    p.s = ctypes.c_void_p(p.v + 3 * 32 * 4)
    assert lib.isc_step_fwd(ctypes.byref(p), None) == E_SHAPE                     # merged training step


def test_new_fields_match_the_c_layout(tmp_path):
    prog = r'''
#include <stdio.h>
#include <stddef.h>
#include "insenticap_hip.h"
int main(void) {
  printf("%zu %zu %zu %zu %zu %zu\n", offsetof(isc_scan_problem, row_div), sizeof(isc_scan_problem),
         offsetof(isc_lstm_problem, pre_div), sizeof(isc_lstm_problem),
         offsetof(isc_step_plan, row_div), sizeof(isc_step_plan));
  printf("%zu %zu %zu\n", sizeof(((isc_scan_problem *)0)->row_div), sizeof(((isc_lstm_problem *)0)->pre_div),
         sizeof(((isc_step_plan *)0)->row_div));
  return 0;
}
'''
    cfile, exe = str(tmp_path / 'fields.c'), str(tmp_path / 'fields')
    open(cfile, 'w').write(prog)
    subprocess.check_call(['gcc', '-I', os.path.join(ROOT, 'include'), cfile, '-o', exe])
    got = [int(x) for x in subprocess.check_output([exe]).decode().split()]
    L = _lib
    assert got == [L.ScanProblem.row_div.offset, ctypes.sizeof(L.ScanProblem),
                   L.LstmProblem.pre_div.offset, ctypes.sizeof(L.LstmProblem),
                   L.StepPlan.row_div.offset, ctypes.sizeof(L.StepPlan),
                   L.ScanProblem.row_div.size, L.LstmProblem.pre_div.size, L.StepPlan.row_div.size]
    # appended: every field the parent had keeps its offset (the new ones sit behind the parent's last field)
    assert L.ScanProblem.row_div.offset == L.ScanProblem.row_ids_ld.offset + 8
    assert L.LstmProblem.pre_div.offset == L.LstmProblem.splitk_ws_floats.offset + 8
    assert L.StepPlan.row_div.offset == L.StepPlan.pair_rows_c.offset + 8
    # zero = today's behaviour: a fresh struct asks for nothing new
    assert L.ScanProblem().row_div == 0 and L.LstmProblem().pre_div == 0 and L.StepPlan().row_div == 0
