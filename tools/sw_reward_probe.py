#!/usr/bin/env python3
"""What the sentiment-word reward costs, in ONE process: HIP events and host clocks, medians with their ranges, the forms
alternating, every step under a time limit (the process ends when one runs over).

Three lexicons of 600 of the V = 10000 words each, rows of T = 20 at random with about a fifth of the positions drawn
from the row's lexicon:
  * the kernel (isc_sw_reward, accumulating and marking, HIP events around the launch) at 512 and 2560 rows, the host
    function (rewards.get_senti_words_reward, a Python loop as in the reference) on the same rows, and whether the two
    agree in bits; isc_sw_decay + the copy that updates the dict;
  * the 512-image graph-served RL training iteration (the default fast path) with senti_words_flag 0 - the iteration as
    it was before the term existed - and 0.05;
  * the 512-image eager iteration (train_graphs = False) with the flag 0, 0.05 in 'device' form and 0.05 in 'host' form.
The numbers are reported, nothing is gated.

    python tools/sw_reward_probe.py [--reps 9] [--skip-detector] [--out FILE]
"""
import argparse
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch

from cider_dev_probe import DEV, IMAGES, T, V, load_helper, stats, step_limit
from insenticap_model_amd import rewards, synth
from insenticap_model_amd.detector import Detector

FLAG = 0.05


def lexicon(seed=11, words=600):
    rng = np.random.default_rng(seed)
    return {lab: {int(w): 1.0 for w in rng.choice(np.arange(4, V), size=words, replace=False)} for lab in range(3)}


def rows_of(lex, labels, seed):
    rng = np.random.default_rng(seed)
    rows = rng.integers(4, V, size=(len(labels), T)).astype(np.int64)
    for r, lab in enumerate(labels):
        own = np.fromiter(lex[int(lab)], dtype=np.int64)
        at = rng.random(T) < 0.2
        rows[r, at] = own[rng.integers(0, len(own), size=int(at.sum()))]
    return rows


def probe_kernel(a, lines, lex):
    table = rewards.SentimentWordWeights.from_dict(lex, V, 3, DEV)
    for N in (512, 2560):
        with step_limit(a.step_limit, 'kernel, N = %d' % N):
            labels = np.random.default_rng(N).integers(0, 3, size=N).astype(np.int64)
            rows = rows_of(lex, labels, seed=N)
            d_rows, d_labels = torch.from_numpy(rows).to(DEV), torch.from_numpy(labels).to(DEV)
            io = torch.zeros(N, T, dtype=torch.float32, device=DEV)
            r64 = torch.empty(N, T, dtype=torch.float64, device=DEV)
            table.reward(d_rows, d_labels, FLAG, io, False, r64)
            want, accur_w = rewards.get_senti_words_reward(rows, labels, lex)
            res = {'probe': 'kernel', 'N': N, 'T': T, 'V': V, 'reps': a.reps, 'paid_positions': int((want != 0).sum()),
                   'equal_in_bits': bool(np.array_equal(r64.cpu().numpy().view(np.int64), want.view(np.int64)) and
                                         np.array_equal(io.cpu().numpy(), want.astype(np.float32)))}
            kern, dev_wall, host_wall, decay = [], [], [], []
            for r in range(a.reps + 2):                                  # two warm-up rounds, the forms alternating
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                torch.cuda.synchronize()
                e0.record()
                table.reward(d_rows, d_labels, FLAG, io, True, r64)
                e1.record()
                torch.cuda.synchronize()
                w0 = time.perf_counter()
                table.reward(d_rows, d_labels, FLAG, io, True, r64)
                torch.cuda.synchronize()
                w1 = time.perf_counter()
                rewards.get_senti_words_reward(rows, labels, lex)
                w2 = time.perf_counter()
                table.decay(1.0)                                         # (factor 1: the states go back, the weights stay)
                table.update_dict(lex)
                w3 = time.perf_counter()
                if r >= 2:
                    kern.append(e0.elapsed_time(e1))
                    dev_wall.append((w1 - w0) * 1e3)
                    host_wall.append((w2 - w1) * 1e3)
                    decay.append((w3 - w2) * 1e3)
            res.update(device_kernel=stats(kern), device_launch_wait_wall=stats(dev_wall),
                       host_function_wall=stats(host_wall), decay_and_dict_update_wall=stats(decay))
            res['device_faster_beyond_spread'] = max(dev_wall) < min(host_wall)
            lines.append(json.dumps(res))
            print(lines[-1], flush=True)


def probe_detector(a, lines, lex):
    st = dict(synth.DEFAULT_SETTINGS, **synth.HELPER_SETTINGS)
    with step_limit(a.step_limit, 'building the detector'):
        det = Detector(synth.make_idx2word(V), T, synth.SENTIMENT_CATEGORIES, {'cap_lr': 4e-5}, st)
        det.captioner.load_state_dict({k: torch.from_numpy(v) for k, v in synth.make_weights(V, st, seed=0).items()})
        load_helper(det.senti_detector, 51)
        load_helper(det.sent_senti_cls, 52)
        det.to(DEV)
        t = torch.from_numpy
        s = synth.make_inputs(80, V, st, regions=1, seq_len=T, seed=72)
        scs = [((t(s['captions']), s['lengths']), t(s['cpt_words']), t(s['senti_words']), t(s['senti_labels']))]
        (b,), split = synth.make_rl_batches(1, IMAGES, V, st, grid=(6, 6), seq_len=T, seed=70)
        det.set_ciderd_scorer(split)
        det.set_sentiment_words(lex)
        det.senti_words_decay = 1.0                                      # (the same lexicon in every repetition)
        item = (b[0], t(b[1]).to(DEV), t(b[2]).to(DEV), (t(b[3][0]), b[3][1]), t(b[4]), t(b[5]), b[6])
    for graphs, forms in ((True, {'flag_0': (0.0, 'device'), 'flag_0.05_device': (FLAG, 'device')}),
                          (False, {'flag_0': (0.0, 'device'), 'flag_0.05_device': (FLAG, 'device'),
                                   'flag_0.05_host': (FLAG, 'host')})):
        det.train_graphs = graphs
        ev, wall, logged = {k: [] for k in forms}, {k: [] for k in forms}, {}
        with step_limit(a.step_limit, 'Detector.forward, train_graphs = %r' % graphs):
            for r in range(a.reps + 3):                                  # three warm-up rounds (two eager + the capture)
                for name, (flag, form) in forms.items():
                    det.senti_words_flag, det.senti_words_form = flag, form
                    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    torch.cuda.synchronize()
                    w0 = time.perf_counter()
                    e0.record()
                    out = det(([item], scs), 'fact', True)
                    e1.record()
                    torch.cuda.synchronize()
                    w1 = time.perf_counter()
                    logged[name] = out.get('senti_words_reward')
                    if r >= 3:
                        ev[name].append(e0.elapsed_time(e1))
                        wall[name].append((w1 - w0) * 1e3)
        res = {'probe': 'detector', 'form': 'graph_served_training_512' if graphs else 'eager_training_512',
               'images': IMAGES, 'V': V, 'T': T, 'reps': a.reps, 'logged_senti_words_reward': logged}
        if graphs:
            g = det._rl_graph
            res['graph'] = {'captures': g.captures, 'replays': g.replays, 'eager_steps': g.eager_steps}
        for name in forms:
            res[name] = {'events': stats(ev[name]), 'wall': stats(wall[name])}
            if name != 'flag_0':
                res['cost_median_wall_ms_' + name] = res[name]['wall']['median_ms'] - res['flag_0']['wall']['median_ms']
                res['slower_beyond_spread_' + name] = min(wall[name]) > max(wall['flag_0'])
        if not graphs:
            res['device_faster_than_host_beyond_spread'] = max(wall['flag_0.05_device']) < min(wall['flag_0.05_host'])
        lines.append(json.dumps(res))
        print(lines[-1], flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--reps', type=int, default=9)
    ap.add_argument('--step-limit', type=int, default=150, help='seconds per step')
    ap.add_argument('--skip-detector', action='store_true')
    ap.add_argument('--out', default=None)
    a = ap.parse_args()
    lines = []
    lex = lexicon()
    probe_kernel(a, lines, lex)
    if not a.skip_detector:
        probe_detector(a, lines, lex)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        open(a.out, 'w').write('\n'.join(lines) + '\n')


if __name__ == '__main__':
    main()
