#!/usr/bin/env python3
"""What sharing an image among its searches costs or saves (Captioner.sample_sentiments, sample_batch(share_image=True)).

DEFAULT_SETTINGS, V = 10000, T = 20 steps (<EOS> out of reach: every search runs all its steps), 36 regions, one process.
Each figure is the median (min - max) over REPS >= 9 repetitions of the wall time of one call that ends in its read-back
(a host clock around work that ends in a device synchronise), CALLS calls per repetition, the variants of a comparison
alternating inside every repetition:
  (a) one image: S graph-served `sample` calls against ONE `sample_sentiments` call, S x beam = 2 x 3 (few-row step, one
      graph) and 3 x 3 (9 rows: the general kernels);
  (b) 64 images x beam 5: sample_batch with share_image off and on;
  (c) 64 images x 3 sentiments x beam 3: sample_sentiments against sample_batch on inputs repeated 3 times;
  (d) peak device memory of one eager call of (b) and (c) above what is allocated before it.
    python tools/senti_beam_probe.py [reps] [calls]"""
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch

from insenticap_model_amd import Captioner, synth

V, T, R = 10000, 20, 36
REPS = max(int(sys.argv[1]), 9) if len(sys.argv) > 1 else 11
CALLS = int(sys.argv[2]) if len(sys.argv) > 2 else 10
dev = torch.device('cuda:0')
st = synth.DEFAULT_SETTINGS
cap = Captioner(synth.make_idx2word(V), synth.SENTIMENT_CATEGORIES, st)
cap.load_state_dict({k: torch.from_numpy(v) for k, v in synth.make_weights(V, st).items()})
cap.to(dev).eval()
cap.eos_id = -7                                              # nobody ends early: T steps per search, in every variant
cap.enable_beam_graphs(True, max_graphs=8)
d = {k: torch.from_numpy(np.asarray(v)).to(dev) for k, v in synth.make_inputs(64, V, st, regions=R, seq_len=T, seed=3).items()}
fc, att, sw = d['fc_feats'], d['att_feats'], d['senti_words']


def labels(I, S):
    return torch.tensor([[(i + s) % 3 for s in range(S)] for i in range(I)], dtype=torch.int64, device=dev)


def compare(title, variants):
    """variants: [(name, callable)]; every repetition times CALLS calls of each, in turn."""
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
        print('    %-58s %8.3f ms  (%.3f - %.3f)' % (name, statistics.median(x), min(x), max(x)))
    return {k: statistics.median(v) for k, v in times.items()}


def peak(f):
    """Peak device memory of one EAGER call above what was allocated before it, MB."""
    cap.enable_beam_graphs(False)
    f()
    torch.cuda.synchronize()
    base = torch.cuda.memory_allocated()
    torch.cuda.reset_peak_memory_stats()
    f()
    torch.cuda.synchronize()
    out = (torch.cuda.max_memory_allocated() - base) / 2 ** 20
    cap.enable_beam_graphs(True, max_graphs=8)
    return out


with torch.no_grad():
    print('REPS %d, CALLS %d per repetition; median (min - max) ms per call' % (REPS, CALLS))
    for S in (2, 3):
        lab = labels(1, S)
        singles = [lab[0, s:s + 1].contiguous() for s in range(S)]

        def separate(singles=singles):
            return [cap.sample(fc[0], att[0], sw[0], l, 3, 1, T) for l in singles]

        def together(lab=lab):
            return cap.sample_sentiments(fc[:1], att[:1], sw[:1], lab, 3, 1, T)
        compare('(a) one image, %d sentiments x beam 3 (%d rows: %s)' % (S, 3 * S, 'few-row step' if 3 * S <= 8 else 'general kernels'),
                [('%d graph-served sample calls' % S, separate), ('one sample_sentiments call', together)])
    lab64 = d['senti_labels']
    b_off = lambda: cap.sample_batch(fc, att, sw, lab64, 5, 1, T)
    b_on = lambda: cap.sample_batch(fc, att, sw, lab64, 5, 1, T, share_image=True)
    compare('(b) 64 images x beam 5 (320 rows)', [('sample_batch', b_off), ('sample_batch(share_image=True)', b_on)])
    lab3 = labels(64, 3)
    fc3, att3, sw3, labr = fc.repeat_interleave(3, 0), att.repeat_interleave(3, 0), sw.repeat_interleave(3, 0), lab3.reshape(-1)
    c_rep = lambda: cap.sample_batch(fc3, att3, sw3, labr, 3, 1, T)
    c_one = lambda: cap.sample_sentiments(fc, att, sw, lab3, 3, 1, T)
    compare('(c) 64 images x 3 sentiments x beam 3 (576 rows)',
            [('sample_batch on inputs repeated 3 times', c_rep), ('sample_sentiments', c_one)])
    print('(d) peak device memory of one eager call, MB above the allocation before it')
    for name, f in (('(b) sample_batch', b_off), ('(b) sample_batch(share_image=True)', b_on),
                    ('(c) sample_batch on repeated inputs', c_rep), ('(c) sample_sentiments', c_one)):
        print('    %-58s %8.1f MB' % (name, peak(f)))
