#!/usr/bin/env python3
"""What diverse beam search costs (beam_groups / diversity: Captioner.sample_batch and the calls built on it).

DEFAULT_SETTINGS, V = 10000, T = 20 steps (<EOS> out of reach: every search runs all its steps), 36 regions, served from
the captured graphs, one process.  Each figure is the median (min - max) over REPS >= 11 repetitions of the wall time of
one call that ends in its read-back, CALLS calls per repetition, the variants alternating inside every repetition:
  one image (the few-row step, ONE graph: the group loop is a chain of G rank rounds inside isc_beam_select_groups)
      beam 6 with G = 1 / 2 / 3 / 6, beam 8 with G = 1 / 4, diversity 0.5;
  64 images x beam 6 (general kernels, graphs of four steps: isc_beam_merge_groups)
      G = 1 / 3;
  the defaults: beam 5 without the keywords, one image and 64 images - the figures to hold against the same lines of a
      build without the feature (this file runs on such a build too and prints these lines only).
The "per step" lines give what the groups add to a decode step.
    python tools/diverse_beam_probe.py [reps] [calls]"""
import inspect
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch

from insenticap_model_amd import Captioner, synth

V, T, R, LAM = 10000, 20, 36, 0.5
REPS = max(int(sys.argv[1]), 11) if len(sys.argv) > 1 else 11
CALLS = int(sys.argv[2]) if len(sys.argv) > 2 else 10
dev = torch.device('cuda:0')
st = synth.DEFAULT_SETTINGS
cap = Captioner(synth.make_idx2word(V), synth.SENTIMENT_CATEGORIES, st)
cap.load_state_dict({k: torch.from_numpy(v) for k, v in synth.make_weights(V, st).items()})
cap.to(dev).eval()
cap.eos_id = -7                                              # nobody ends early: T steps per search, in every variant
cap.enable_beam_graphs(True, max_graphs=12)
d = {k: torch.from_numpy(np.asarray(v)).to(dev) for k, v in synth.make_inputs(64, V, st, regions=R, seq_len=T, seed=3).items()}
HAS = 'beam_groups' in inspect.signature(cap.sample_batch).parameters


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


def call(ins, beam, G=None):
    if G is None:
        return lambda: cap.sample_batch(*ins, beam, 1, T)
    return lambda: cap.sample_batch(*ins, beam, 1, T, beam_groups=G, diversity=LAM)


def distinct(ids):
    """Mean number of different first words among a search's captions."""
    return statistics.mean(len({w[0] for w in img}) for img in ids)


with torch.no_grad():
    print('REPS %d, CALLS %d per repetition; median (min - max) ms per call; beam groups %s' %
          (REPS, CALLS, 'built' if HAS else 'not in this build'))
    one = [d[k][:1] for k in ('fc_feats', 'att_feats', 'senti_words', 'senti_labels')]
    many = [d[k][:64] for k in ('fc_feats', 'att_feats', 'senti_words', 'senti_labels')]
    compare('defaults: 1 image x beam 5, T = %d, from the graph' % T, [('plain', call(one, 5))])
    compare('defaults: 64 images x beam 5, T = %d, from the graphs' % T, [('plain', call(many, 5))])
    if HAS:
        m = compare('1 image x beam 6, T = %d, from the graph' % T,
                    [('plain', call(one, 6))] + [('G = %d' % G, call(one, 6, G)) for G in (1, 2, 3, 6)])
        for G in (2, 3, 6):
            print('    G = %d - plain: %+.1f us per search, %+.2f us per step' %
                  (G, (m['G = %d' % G] - m['plain']) * 1e3, (m['G = %d' % G] - m['plain']) * 1e3 / T))
        m = compare('1 image x beam 8, T = %d, from the graph' % T,
                    [('plain', call(one, 8)), ('G = 4', call(one, 8, 4))])
        print('    G = 4 - plain: %+.1f us per search, %+.2f us per step' %
              ((m['G = 4'] - m['plain']) * 1e3, (m['G = 4'] - m['plain']) * 1e3 / T))
        m = compare('64 images x beam 6, T = %d, from the graphs' % T,
                    [('plain', call(many, 6)), ('G = 3', call(many, 6, 3))])
        print('    G = 3 - plain: %+.1f us per search, %+.2f us per step' %
              ((m['G = 3'] - m['plain']) * 1e3, (m['G = 3'] - m['plain']) * 1e3 / T))
        print('    different first words per search (64 images): %.2f plain, %.2f with G = 3'
              % (distinct(call(many, 6)()[2]), distinct(call(many, 6, 3)()[2])))
