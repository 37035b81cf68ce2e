#!/usr/bin/env python3
"""What the beam search's controls cost (no_repeat_ngram, min_len: Captioner.sample_batch and the calls built on it).

DEFAULT_SETTINGS, V = 10000, T = 20 steps (<EOS> out of reach: every search runs all its steps), 36 regions, beam 5,
served from the captured graphs, one process.  Each figure is the median (min - max) over REPS >= 11 repetitions of the
wall time of one call that ends in its read-back, CALLS calls per repetition, the variants alternating inside every
repetition:
  plain     the call without the keywords (what a build without the controls runs as well: run this file on it for (a));
  off       no_repeat_ngram = 0, min_len = 0 spelled out;
  trigram   no_repeat_ngram = 3, min_len = 8 - one isc_beam_ngram_ban launch per step plus the list in the candidate masks;
for one image (the few-row step, ONE graph) and for 64 images (general kernels, graphs of four steps).  The last lines
give the controls' cost per decode step.
    python tools/beam_controls_probe.py [reps] [calls]"""
import inspect
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch

from insenticap_model_amd import Captioner, synth

V, T, R, BEAM = 10000, 20, 36, 5
REPS = max(int(sys.argv[1]), 11) if len(sys.argv) > 1 else 11
CALLS = int(sys.argv[2]) if len(sys.argv) > 2 else 10
dev = torch.device('cuda:0')
st = synth.DEFAULT_SETTINGS
cap = Captioner(synth.make_idx2word(V), synth.SENTIMENT_CATEGORIES, st)
cap.load_state_dict({k: torch.from_numpy(v) for k, v in synth.make_weights(V, st).items()})
cap.to(dev).eval()
cap.eos_id = -7                                              # nobody ends early: T steps per search, in every variant
cap.enable_beam_graphs(True, max_graphs=8)
d = {k: torch.from_numpy(np.asarray(v)).to(dev) for k, v in synth.make_inputs(64, V, st, regions=R, seq_len=T, seed=3).items()}
HAS = 'no_repeat_ngram' in inspect.signature(cap.sample_batch).parameters


def compare(title, variants):
    for _, f in variants:
        for _ in range(3):                                   # first sight, capture, replay
            f()
    times = {name: [] for name, _ in variants}
    for _ in range(REPS):
        for name, f in variants:
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(CALLS):
                f()
            torch.cuda.synchronize()
            times[name].append((time.perf_counter() - t0) / CALLS * 1e3)
    print(title)
    for name, _ in variants:
        x = times[name]
        print('    %-44s %8.3f ms  (%.3f - %.3f)' % (name, statistics.median(x), min(x), max(x)))
    return {k: statistics.median(v) for k, v in times.items()}


with torch.no_grad():
    print('REPS %d, CALLS %d per repetition; median (min - max) ms per call; controls %s' %
          (REPS, CALLS, 'built' if HAS else 'not in this build'))
    for images in (1, 64):
        ins = [d[k][:images] for k in ('fc_feats', 'att_feats', 'senti_words', 'senti_labels')]
        variants = [('plain', lambda ins=ins: cap.sample_batch(*ins, BEAM, 1, T))]
        if HAS:
            variants += [('off (0, 0)', lambda ins=ins: cap.sample_batch(*ins, BEAM, 1, T, no_repeat_ngram=0, min_len=0)),
                         ('trigram blocking + min_len 8', lambda ins=ins: cap.sample_batch(*ins, BEAM, 1, T, no_repeat_ngram=3,
                                                                                            min_len=8))]
        m = compare('%d image%s x beam %d, T = %d, from the graph%s' % (images, '' if images == 1 else 's', BEAM, T,
                                                                      '' if images == 1 else 's'), variants)
        if HAS:
            print('    controls on - plain: %+.1f us per search, %+.2f us per step' %
                  ((m['trigram blocking + min_len 8'] - m['plain']) * 1e3, (m['trigram blocking + min_len 8'] - m['plain']) * 1e3 / T))
            ids = cap.sample_batch(*ins, BEAM, 1, T, no_repeat_ngram=3, min_len=8)[2]
            rep = sum(len(w) - 2 - len({tuple(w[j:j + 3]) for j in range(len(w) - 2)}) for img in ids for w in img)
            ids0 = cap.sample_batch(*ins, BEAM, 1, T)[2]
            rep0 = sum(len(w) - 2 - len({tuple(w[j:j + 3]) for j in range(len(w) - 2)}) for img in ids0 for w in img)
            print('    repeated trigrams in the returned candidates: %d plain, %d under the control' % (rep0, rep))
