"""One image under several sentiment labels (Captioner.sample_sentiments): what the GPU tests rest on, on the CPU.

(a) the oracle's beam searches of tests/_senti_beam.py - width sets h_wide / all_differ / h_768, images 0-2, labels 0-2,
beam 2 and 3 - are decided: the fp32 and the fp64 oracle agree on every id sequence, the three labels give three
different results per image (so a wrong label index cannot pass the GPU tests), and the final scores of neighbouring
beams differ by more than MARGIN = 2e-3 (smallest gap found: 0.0103, all_differ, image 1, beam 3); the same for the
beam-4 searches of the 8-row few-row case;
(b) argument errors are ValueErrors raised before anything touches the device (the model here lives on the CPU: a call
that got past its checks would fail differently);
(c) the two new ABI fields sit in former pad slots: offsets and struct sizes, header against ctypes."""
import ctypes
import os
import subprocess

import pytest
import torch

import _senti_beam as SB
import _widths as Wd
from insenticap_model_amd import Captioner, _lib, synth

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.parametrize('name', SB.WIDTH_SETS)
def test_oracle_searches_are_decided(name):
    smallest = None
    for beam in SB.BEAMS:
        for image in SB.IMAGES:
            results = []
            for label in SB.LABELS:
                caps64, sc64, ids64 = SB.oracle(name, image, label, beam, torch.float64)
                _, _, ids32 = SB.oracle(name, image, label, beam, torch.float32)
                assert ids32 == ids64, (name, image, label, beam)
                assert len(sc64) == beam
                for a, b in zip(sc64[:-1], sc64[1:]):
                    gap = abs(a - b)
                    smallest = gap if smallest is None else min(smallest, gap)
                    assert gap > SB.MARGIN, (name, image, label, beam, gap)
                results.append(tuple(tuple(x) for x in ids64))
            assert len(set(results)) == len(SB.LABELS), (name, image, beam)     # three labels, three results
    print('smallest score gap, %s: %.4f' % (name, smallest))


@pytest.mark.parametrize('name', ['h_wide', 'h_768'])
def test_oracle_beam4_of_the_few_row_case_is_decided(name):
    """1 image x 2 labels x beam 4 (8 rows, the few-row step): image 1 under labels 1 and 2."""
    results = []
    for label in (1, 2):
        _, sc64, ids64 = SB.oracle(name, 1, label, 4, torch.float64)
        assert SB.oracle(name, 1, label, 4, torch.float32)[2] == ids64
        gaps = [abs(a - b) for a, b in zip(sc64[:-1], sc64[1:])]
        print('%s label %d beam 4: smallest score gap %.4f' % (name, label, min(gaps)))
        assert min(gaps) > SB.MARGIN
        results.append(tuple(tuple(x) for x in ids64))
    assert results[0] != results[1]


def test_rotated_labels_differ_from_group_index():
    lab = SB.rotated_labels(3)
    assert lab.shape == (3, 3) and sorted(lab[1].tolist()) == [0, 1, 2]
    assert any(lab[i, s] != s for i in range(3) for s in range(3))


def _cpu_cap():
    st, w, d, _ = Wd.setup('h_wide')
    cap = Captioner(Wd.idx2word(), synth.SENTIMENT_CATEGORIES, st)
    cap.load_state_dict({k: torch.from_numpy(v) for k, v in w.items()})
    return cap.eval(), d


def test_argument_errors_before_the_device():
    cap, d = _cpu_cap()
    fc, att, sw = Wd.cpu(d, 'fc_feats', 2), Wd.cpu(d, 'att_feats', 2), Wd.cpu(d, 'senti_words', 2)
    lab = SB.rotated_labels(2)
    M = sw.shape[1]
    bad = [
        (dict(senti_labels=lab[0]), r'senti_labels must be an integer tensor \[I, S\]'),                 # [S], not [I, S]
        (dict(senti_labels=SB.rotated_labels(3)), r'senti_labels must be an integer tensor \[I, S\]'),  # another I
        (dict(senti_labels=None), r'senti_labels must be an integer tensor \[I, S\]'),
        (dict(senti_labels=lab.float()), 'integer category ids'),
        (dict(senti_labels=lab + 1), 'outside the 3 sentiment categories'),
        (dict(senti_labels=lab - 1), 'outside the 3 sentiment categories'),
        (dict(senti_words=sw[0]), r'senti_words must be \[I, M\]'),                                        # a third shape
        (dict(senti_words=sw.reshape(2, 1, M).expand(2, 2, M)), r'senti_words must be \[I, M\]'),         # [I, 2, M], S = 3
        (dict(senti_words=None), r'senti_words must be \[I, M\]'),
        (dict(beam_size=9), 'at most 8 beams per search'),
        (dict(beam_size=0), 'beam_size must be an integer >= 1'),
        (dict(beam_size=True), 'beam_size must be an integer >= 1'),
    ]
    for change, msg in bad:
        kw = dict(senti_words=sw, senti_labels=lab, beam_size=3)
        kw.update(change)
        with pytest.raises(ValueError, match=msg):
            cap.sample_sentiments(fc, att, kw['senti_words'], kw['senti_labels'], kw['beam_size'], 1, Wd.T)
    with pytest.raises(ValueError, match='several labels per image: sample_sentiments'):
        cap.sample_batch(fc, att, sw, lab, 3, 1, Wd.T)


def test_grouped_rollout_label_count_errors():
    cap, d = _cpu_cap()
    args = [Wd.cpu(d, k, 2) for k in Wd.RL_KEYS[:4]]
    with torch.no_grad():
        for labels in (torch.zeros(5, dtype=torch.int64), torch.zeros(3, 2, dtype=torch.int64),
                       torch.zeros(1, dtype=torch.int64)):
            with pytest.raises(ValueError, match='one label per image .2. or per caption row'):
                cap.forward_rl(*args, labels, Wd.T, 0, captions_per_image=3)
    # the differentiable form keeps its refusal of per-row labels, and its wording
    cap.train()
    try:
        with pytest.raises(ValueError, match='with gradients: senti_labels must hold one label per image'):
            cap.forward_rl(*args, torch.zeros(2, 3, dtype=torch.int64), Wd.T, 0, captions_per_image=3)
    finally:
        cap.eval()


def test_detector_sentiment_names_checked_before_the_device():
    from insenticap_model_amd import Detector
    st, _, d, _ = Wd.setup('h_wide')
    det = Detector(Wd.idx2word(), Wd.T, synth.SENTIMENT_CATEGORIES, {'cap_lr': 4e-4}, dict(st, **synth.HELPER_SETTINGS))
    fc, att, sw = Wd.cpu(d, 'fc_feats', 1)[0], Wd.cpu(d, 'att_feats', 1)[0], Wd.cpu(d, 'senti_words', 1)
    for names, msg in ((['cheerful'], 'is not one of the sentiment categories'), ([], 'non-empty list'),
                       ('positive', 'non-empty list'), (['positive', 'positive'], 'named twice')):
        with pytest.raises(ValueError, match=msg):
            det.sample_sentiments(fc, att, sw, names)
    with pytest.raises(ValueError, match='needs set_concept_detector'):
        det.sample_sentiments(fc, att, None, ['positive'])


def test_new_abi_fields_sit_in_the_pad_slots(tmp_path):
    prog = r'''
#include <stdio.h>
#include <stddef.h>
#include "insenticap_hip.h"
int main(void) {
  printf("%zu %zu %zu %zu %zu\n", offsetof(isc_step_plan, senti_div), offsetof(isc_step_plan, pair_rows_c),
         offsetof(isc_step_plan, row_div), offsetof(isc_step_plan, pre_rows), sizeof(isc_step_plan));
  printf("%zu %zu %zu %zu %zu\n", offsetof(isc_rows_ext, senti_div), offsetof(isc_rows_ext, row_div),
         offsetof(isc_rows_ext, live_in), offsetof(isc_rows_ext, fin_unfinished_out), sizeof(isc_rows_ext));
  printf("%zu %zu\n", offsetof(isc_scan_gate_args, G), sizeof(isc_scan_gate_args));
  return 0;
}
'''
    cfile, exe = str(tmp_path / 'layout.c'), str(tmp_path / 'layout')
    open(cfile, 'w').write(prog)
    subprocess.check_call(['gcc', '-I', os.path.join(ROOT, 'include'), cfile, '-o', exe])
    got = [int(x) for x in subprocess.check_output([exe]).decode().split()]
    P, X, G = _lib.StepPlan, _lib.RowsExt, _lib.ScanGateArgs
    assert got == [P.senti_div.offset, P.pair_rows_c.offset, P.row_div.offset, P.pre_rows.offset, ctypes.sizeof(P),
                   X.senti_div.offset, X.row_div.offset, X.live_in.offset, X.fin_unfinished_out.offset, ctypes.sizeof(X),
                   G.G.offset, ctypes.sizeof(G)]
    # former pad slots: right behind pair_rows_c / row_div, nothing moved (sizes as before the fields had names)
    assert P.senti_div.offset == P.pair_rows_c.offset + 4 and P.row_div.offset == P.senti_div.offset + 4
    assert X.senti_div.offset == X.row_div.offset + 4 and X.live_in.offset == X.senti_div.offset + 4
    assert (ctypes.sizeof(P), ctypes.sizeof(X)) == (720, 104)
