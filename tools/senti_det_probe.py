#!/usr/bin/env python3
"""The frozen image-sentiment detector: stock torch ops (permute + vendor-library fp32 convolutions + small launches on an
fp32 copy of the features - the parent behaviour, `native` off) against the native forward (isc_senti_det_fwd: implicit
GEMM on the split-f16 engine over the channels-last grid as stored, `native` on), in ONE process, alternating.
F = 2048, two convs, two FCs, k = 3.

  detector alone (SentimentDetector.sample_device; the torch path is handed `feats.float()` for float16 features, as
  Detector does), B = 1, 64, 512 at 6x6 and B = 1, 64 at 14x14, fp32 and float16 features:
      device_us   device time of one call (HIP events around it), median / min / max over --reps after the warm-up
      route       the library's launch kinds of one native call
  RL iteration (Detector.forward 'fact', training, 512 images, 6x6 regions, cache_image_sentiments = False), native
  off / on / off / on: wall ms per iteration.
  Detector.sample per image (beam 5, 6x6 regions; as tools/eval_loop_probe.py), native off / on: wall ms per image.

    python tools/senti_det_probe.py [--reps 20] [--rl-reps 8] [--out FILE] [--no-rl] [--no-sample]
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
from insenticap_model_amd.helper_nets import SentimentDetector

V, T = 10000, 20
DEV = torch.device('cuda:0')
ST = dict(synth.DEFAULT_SETTINGS, **synth.HELPER_SETTINGS)
SIZES = [(1, 6), (64, 6), (512, 6), (1, 14), (64, 14)]


def load_helper(mod, seed):
    shapes = {k: tuple(v.shape) for k, v in mod.state_dict().items()}
    mod.load_state_dict({k: torch.from_numpy(v) for k, v in synth.make_module_weights(shapes, seed).items()})
    return mod.eval()


def spread(xs):
    return {'median': statistics.median(xs), 'min': min(xs), 'max': max(xs)}


def detector_alone(net, B, g, f16, reps, emit):
    rng = np.random.default_rng(7)
    feats = torch.from_numpy(np.maximum(rng.standard_normal((B, g, g, 2048), dtype=np.float32), 0)).to(DEV)
    if f16:
        feats = feats.half()

    def call(native):
        net.enable_native(native)
        return net.sample_device(feats if native else (feats.float() if f16 else feats), 0.7)
    devt = {False: [], True: []}
    for r in range(reps + 3):                    # three warm-up rounds (vendor algorithm search, workspaces, the pack)
        for native in (False, True):
            torch.cuda.synchronize()
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            call(native)
            e1.record()
            torch.cuda.synchronize()
            if r >= 3:
                devt[native].append(e0.elapsed_time(e1) * 1e3)
    a, b = call(False), call(True)
    before = ops.senti_det_launches()
    call(True)
    now = ops.senti_det_launches()
    torch.cuda.synchronize()
    res = {'what': 'detector', 'B': B, 'grid': g, 'features': 'f16' if f16 else 'fp32', 'reps': reps,
           'torch': {'device_us': spread(devt[False])}, 'native': {'device_us': spread(devt[True])},
           'route': {k: now[k] - before[k] for k in now if now[k] != before[k]},
           'labels_equal': bool(torch.equal(a[0], b[0])), 'max_abs_score_diff': float((a[2] - b[2]).abs().max())}
    res['native_faster_beyond_spread'] = res['native']['device_us']['max'] < res['torch']['device_us']['min']
    res['native_slower_beyond_spread'] = res['native']['device_us']['min'] > res['torch']['device_us']['max']
    res['torch_over_native_median'] = res['torch']['device_us']['median'] / res['native']['device_us']['median']
    emit(res)
    net.enable_native(False)


def make_detector():
    det = Detector(synth.make_idx2word(V), T, synth.SENTIMENT_CATEGORIES, {'cap_lr': 4e-5}, ST)
    det.captioner.load_state_dict({k: torch.from_numpy(v) for k, v in synth.make_weights(V, ST, seed=0).items()})
    load_helper(det.senti_detector, 51)
    load_helper(det.sent_senti_cls, 52)
    return det.to(DEV)


def rl_iteration(reps, emit, images=512):
    det = make_detector()
    det.cache_image_sentiments = False
    t = torch.from_numpy
    s = synth.make_inputs(80, V, ST, regions=1, seq_len=T, seed=72)
    scs = [((t(s['captions']), s['lengths']), t(s['cpt_words']), t(s['senti_words']), t(s['senti_labels']))]
    (b,), split = synth.make_rl_batches(1, images, V, ST, grid=(6, 6), seq_len=T, seed=70)
    det.set_ciderd_scorer(split)
    item = (b[0], t(b[1]).to(DEV), t(b[2]).to(DEV), (t(b[3][0]), b[3][1]), t(b[4]), t(b[5]), b[6])

    def iteration():
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        det(([item], scs), 'fact', True)
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e3
    res = {'what': 'rl_iteration', 'images': images, 'regions': 36, 'cache_image_sentiments': False, 'reps': reps, 'rounds': []}
    for rnd, native in enumerate((False, True, False, True)):
        det.native_sentiment_detector = native
        for _ in range(4 if rnd == 0 else 2):    # warm-up: two eager iterations + the captures; later: pack, workspace
            iteration()
        res['rounds'].append({'native': native, 'ms_per_iter': spread([iteration() for _ in range(reps)])})
    off = [r['ms_per_iter'] for r in res['rounds'] if not r['native']]
    on = [r['ms_per_iter'] for r in res['rounds'] if r['native']]
    res['native_faster_beyond_spread'] = max(x['max'] for x in on) < min(x['min'] for x in off)
    res['median_off_over_on'] = statistics.median(x['median'] for x in off) / statistics.median(x['median'] for x in on)
    emit(res)


def sample_per_image(emit, n=32):
    det = make_detector().eval()
    d = synth.make_inputs(n, V, ST, regions=36, seq_len=T, seed=3)
    fc = torch.from_numpy(d['fc_feats']).to(DEV)
    att = torch.from_numpy(d['att_feats']).to(DEV).reshape(n, 6, 6, -1)
    sw = torch.from_numpy(d['senti_words']).to(DEV)
    res = {'what': 'Detector.sample', 'images': n, 'beam': 5, 'rounds': []}
    for native in (False, True, False, True):
        det.native_sentiment_detector = native
        for i in range(4):
            det.sample(fc[i], att[i], sw[i], 5, 1)
        ms = []
        for i in range(n):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            det.sample(fc[i], att[i], sw[i], 5, 1)
            torch.cuda.synchronize()
            ms.append((time.perf_counter() - t0) * 1e3)
        res['rounds'].append({'native': native, 'ms_per_image': spread(ms)})
    emit(res)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--reps', type=int, default=20)
    ap.add_argument('--rl-reps', type=int, default=8)
    ap.add_argument('--out', default=None)
    ap.add_argument('--no-rl', action='store_true')
    ap.add_argument('--no-sample', action='store_true')
    a = ap.parse_args()
    lines = []

    def emit(res):
        lines.append(json.dumps(res))
        print(lines[-1], flush=True)
        if a.out:
            os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
            open(a.out, 'w').write('\n'.join(lines) + '\n')
    net = load_helper(SentimentDetector(synth.SENTIMENT_CATEGORIES, ST), 51).to(DEV)
    for B, g in SIZES:
        for f16 in (False, True):
            detector_alone(net, B, g, f16, a.reps, emit)
            torch.cuda.empty_cache()
    del net
    if not a.no_sample:
        sample_per_image(emit)
        torch.cuda.empty_cache()
    if not a.no_rl:
        rl_iteration(a.rl_reps, emit)


if __name__ == '__main__':
    main()
