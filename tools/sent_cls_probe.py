#!/usr/bin/env python3
"""The frozen sentence-sentiment classifier of the RL rewards: stock torch ops (nn.LSTM of the vendor library + a dozen
small launches - the parent behaviour, `native` off) against the native forward (isc_sent_cls_fwd, `native` on), in ONE
process, alternating.  T = 20, W = H = 512, V = 10000.

  classifier alone (rewards.get_cls_reward, device lengths, on_device=True), B = 512 and B = 2560 (512 x 5):
      host_us     host time to enqueue one call (perf_counter around the call, queue empty before it)
      device_us   device time of one call (HIP events around it)
      launches    kernels per call: the library's counter for the native path; a torch.profiler kernel count for both
                  (None where the profiler is not available)
  RL iteration (Detector.forward 'fact', training, served by RLTrainGraph, 512 images, 36 regions), native off / on / off /
  on: wall ms per iteration, median / min / max over --reps after the captures.

    python tools/sent_cls_probe.py [--reps 20] [--rl-reps 8] [--out FILE] [--no-rl]
"""
import argparse
import json
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch

from insenticap_model_amd import ops, synth
from insenticap_model_amd.detector import Detector
from insenticap_model_amd.helper_nets import SentenceSentimentClassifier
from insenticap_model_amd.rewards import get_cls_reward

V, T = 10000, 20
DEV = torch.device('cuda:0')


def load_helper(mod, seed):
    shapes = {k: tuple(v.shape) for k, v in mod.state_dict().items()}
    mod.load_state_dict({k: torch.from_numpy(v) for k, v in synth.make_module_weights(shapes, seed).items()})
    return mod.eval()


def spread(xs):
    return {'median': statistics.median(xs), 'min': min(xs), 'max': max(xs)}


def profiler_kernels(fn):
    """Device kernels one call launches, counted by torch.profiler; None when it cannot be had here."""
    try:
        from torch.profiler import ProfilerActivity, profile
        with profile(activities=[ProfilerActivity.CUDA]) as prof:
            fn()
            torch.cuda.synchronize()
        n = sum(1 for ev in prof.events() if str(ev.device_type).endswith('CUDA'))
        return n or None
    except Exception as exc:                     # measurement aid only
        print('torch.profiler unavailable: %r' % (exc,), file=sys.stderr)
        return None


def classifier_alone(B, reps, emit):
    st = dict(synth.DEFAULT_SETTINGS, **synth.HELPER_SETTINGS)
    net = load_helper(SentenceSentimentClassifier(synth.make_idx2word(V), synth.SENTIMENT_CATEGORIES, st), 52).to(DEV)
    rng = np.random.default_rng(7)
    seq = torch.from_numpy(rng.integers(0, V, (B, T)).astype(np.int64)).to(DEV)
    lens = torch.from_numpy(rng.integers(1, T + 1, B).astype(np.int32)).to(DEV)
    mk = (torch.arange(T, device=DEV).unsqueeze(0) < lens.unsqueeze(1)).float()
    labels = torch.from_numpy(rng.integers(0, 3, B).astype(np.int64)).to(DEV)

    def call(native):
        net.enable_native(native)
        return get_cls_reward(seq, mk, None, None, labels, net, sample_lens=lens, on_device=True)
    res = {'what': 'classifier', 'B': B, 'T': T, 'W': 512, 'H': 512, 'V': V, 'reps': reps}
    host = {False: [], True: []}
    devt = {False: [], True: []}
    for r in range(reps + 3):                    # three warm-up rounds (library algorithm search, workspaces)
        for native in (False, True):
            torch.cuda.synchronize()
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            t0 = time.perf_counter()
            e0.record()
            call(native)
            e1.record()
            t1 = time.perf_counter()
            torch.cuda.synchronize()
            if r >= 3:
                host[native].append((t1 - t0) * 1e6)
                devt[native].append(e0.elapsed_time(e1) * 1e3)
    a, b = call(False), call(True)
    res['max_abs_diff_native_vs_torch'] = float((a - b).abs().max())
    before = ops.sent_cls_launches()
    call(True)
    res['native'] = {'host_us': spread(host[True]), 'device_us': spread(devt[True]),
                     'launches_library_counter': ops.sent_cls_launches() - before}
    res['torch'] = {'host_us': spread(host[False]), 'device_us': spread(devt[False])}
    emit(res)
    res['torch']['launches_profiler'] = profiler_kernels(lambda: call(False))
    res['native']['launches_profiler'] = profiler_kernels(lambda: call(True))
    res['native_faster_beyond_spread'] = {k: res['native'][k]['max'] < res['torch'][k]['min'] for k in ('host_us', 'device_us')}
    emit(res, replace=True)
    net.enable_native(False)


def rl_iteration(reps, emit, images=512):
    st = dict(synth.DEFAULT_SETTINGS, **synth.HELPER_SETTINGS)
    det = Detector(synth.make_idx2word(V), T, synth.SENTIMENT_CATEGORIES, {'cap_lr': 4e-5}, st)
    det.captioner.load_state_dict({k: torch.from_numpy(v) for k, v in synth.make_weights(V, st, seed=0).items()})
    load_helper(det.senti_detector, 51)
    load_helper(det.sent_senti_cls, 52)
    det.to(DEV)
    t = torch.from_numpy
    s = synth.make_inputs(80, V, st, regions=1, seq_len=T, seed=72)
    scs = [((t(s['captions']), s['lengths']), t(s['cpt_words']), t(s['senti_words']), t(s['senti_labels']))]
    (b,), split = synth.make_rl_batches(1, images, V, st, grid=(6, 6), seq_len=T, seed=70)
    det.set_ciderd_scorer(split)
    item = (b[0], t(b[1]).to(DEV), t(b[2]).to(DEV), (t(b[3][0]), b[3][1]), t(b[4]), t(b[5]), b[6])

    def iteration():
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        det(([item], scs), 'fact', True)
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e3
    res = {'what': 'rl_iteration', 'images': images, 'regions': 36, 'T': T, 'V': V, 'reps': reps, 'rounds': []}
    for rnd, native in enumerate((False, True, False, True)):
        det.native_sentence_classifier = native
        for _ in range(4 if rnd == 0 else 2):    # warm-up: two eager iterations + the captures; later: the reward graph
            iteration()
        res['rounds'].append({'native': native, 'ms_per_iter': spread([iteration() for _ in range(reps)])})
    g = det._rl_graph
    res['graph_captures'], res['graph_replays'], res['cls_graph_captures'] = g.captures, g.replays, g.cls_captures
    off = [r['ms_per_iter'] for r in res['rounds'] if not r['native']]
    on = [r['ms_per_iter'] for r in res['rounds'] if r['native']]
    res['native_faster_beyond_spread'] = max(x['max'] for x in on) < min(x['min'] for x in off)
    res['median_off_over_on'] = statistics.median(x['median'] for x in off) / statistics.median(x['median'] for x in on)
    emit(res)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--reps', type=int, default=20)
    ap.add_argument('--rl-reps', type=int, default=8)
    ap.add_argument('--out', default=None)
    ap.add_argument('--no-rl', action='store_true')
    a = ap.parse_args()
    lines = []

    def emit(res, replace=False):
        if replace:
            lines.pop()
        lines.append(json.dumps(res))
        print(lines[-1], flush=True)
        if a.out:
            os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
            open(a.out, 'w').write('\n'.join(lines) + '\n')
    if not a.no_rl:
        rl_iteration(a.rl_reps, emit)
        torch.cuda.empty_cache()
    for B in (512, 2560):
        classifier_alone(B, a.reps, emit)
        torch.cuda.empty_cache()


if __name__ == '__main__':
    main()
