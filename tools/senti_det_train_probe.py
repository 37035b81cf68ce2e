#!/usr/bin/env python3
"""Training the image-sentiment detector (train_senti.py:78-85): the stock torch iteration (module forward through the
vendor's convolution library, CrossEntropyLoss, autograd, clip_gradient, Adam) against the native step
(train.senti_det_train_step: isc_senti_det_train_fwd / isc_senti_det_bwd, FusedClampAdam), in ONE process, alternating.
F = 2048, two convs, two FCs, k = 3, dropout 0.5, batch 80 at 14x14 and at 6x6.

  per size:   device_us  device time of one iteration (HIP events around it), median / min / max over --reps (>= 15)
                         after the warm-up           host_us  host time to enqueue one iteration
              launches   the library's launches of one native loss + backward (forward, backward, slab reduces)
  dw kernel:  isc_senti_det_dw alone at both layers' shapes: device_us, TFLOP/s (2 M Cout 9 Cin useful flops), and its share
              of the split-f16 engine's ceiling (three f16 MFMA products per useful one: a third of --f16-peak TFLOP/s).

    python tools/senti_det_train_probe.py [--reps 15] [--out FILE] [--f16-peak 2500]
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
from insenticap_model_amd.helper_nets import SentimentDetector
from insenticap_model_amd.optim import clip_gradient
from insenticap_model_amd.train import senti_det_loss_with_grad, senti_det_train_step

DEV = torch.device('cuda:0')
ST = dict(synth.DEFAULT_SETTINGS, **synth.HELPER_SETTINGS)
SIZES = [(80, 14), (80, 6)]


def spread(xs):
    return {'median': statistics.median(xs), 'min': min(xs), 'max': max(xs)}


def make_net(seed=51):
    net = SentimentDetector(synth.SENTIMENT_CATEGORIES, dict(ST, dropout_p=0.5))
    shapes = {k: tuple(v.shape) for k, v in net.state_dict().items()}
    net.load_state_dict({k: torch.from_numpy(v) for k, v in synth.make_module_weights(shapes, seed).items()})
    return net.to(DEV).train()


def timed(fn):
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    t0 = time.perf_counter()
    e0.record()
    fn()
    e1.record()
    host = (time.perf_counter() - t0) * 1e6
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) * 1e3, host


def training_step(B, g, reps, emit):
    rng = np.random.default_rng(7)
    feats = torch.from_numpy(np.maximum(rng.standard_normal((B, g, g, 2048), dtype=np.float32), 0)).to(DEV)
    labels = torch.from_numpy(rng.integers(0, 3, B)).to(DEV)
    nets = {False: make_net(), True: make_net()}
    opts = {False: nets[False].get_optim_criterion(4e-4), True: nets[True].get_optim_criterion(4e-4, fused=True)}

    def stock():
        net, (opt, crit) = nets[False], opts[False]
        pred, _ = net(feats)
        loss = crit(pred, labels)
        opt.zero_grad()
        loss.backward()
        clip_gradient(opt, 0.1)
        opt.step()

    def native():
        senti_det_train_step(nets[True], opts[True][0], feats, labels, 0.1)
    dev, host = {False: [], True: []}, {False: [], True: []}
    for r in range(reps + 3):                    # three warm-up rounds (vendor algorithm search, workspaces, allocator)
        for nat in (False, True):
            d, h = timed(native if nat else stock)
            if r >= 3:
                dev[nat].append(d)
                host[nat].append(h)
    before = ops.senti_det_bwd_launches()
    senti_det_loss_with_grad(nets[True], feats, labels).backward()
    now = ops.senti_det_bwd_launches()
    torch.cuda.synchronize()
    res = {'what': 'training_step', 'B': B, 'grid': g, 'reps': reps,
           'torch': {'device_us': spread(dev[False]), 'host_us': spread(host[False])},
           'native': {'device_us': spread(dev[True]), 'host_us': spread(host[True])},
           'launches': {k: now[k] - before[k] for k in now}}
    res['native_faster_beyond_spread'] = res['native']['device_us']['max'] < res['torch']['device_us']['min']
    res['native_slower_beyond_spread'] = res['native']['device_us']['min'] > res['torch']['device_us']['max']
    res['torch_over_native_median'] = res['torch']['device_us']['median'] / res['native']['device_us']['median']
    emit(res)


def dw_alone(B, g, reps, peak, emit):
    rng = np.random.default_rng(8)
    for Cin in (2048, 1024):
        Cout = Cin // 2
        x = torch.from_numpy(rng.standard_normal((B, g, g, Cin), dtype=np.float32)).to(DEV)
        dy = torch.from_numpy(rng.standard_normal((B * g * g, Cout), dtype=np.float32)).to(DEV)
        us = [timed(lambda: ops.senti_det_dw(dy, x, Cout))[0] for _ in range(reps + 3)][3:]
        flops = 2.0 * B * g * g * Cout * 9 * Cin
        tf = flops / (statistics.median(us) * 1e-6) / 1e12
        emit({'what': 'dw_kernel', 'B': B, 'grid': g, 'Cin': Cin, 'Cout': Cout, 'tiles': (9 * Cin // 128) * (Cout // 64),
              'device_us': spread(us), 'tflops': tf, 'engine_ceiling_tflops': peak / 3.0, 'share_of_ceiling': tf / (peak / 3.0)})


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--reps', type=int, default=15)
    ap.add_argument('--out', default=None)
    ap.add_argument('--f16-peak', type=float, default=2500.0, help='dense f16 MFMA peak of the device, TFLOP/s')
    a = ap.parse_args()
    a.reps = max(a.reps, 15)
    lines = []

    def emit(res):
        lines.append(json.dumps(res))
        print(lines[-1], flush=True)
        if a.out:
            os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
            open(a.out, 'w').write('\n'.join(lines) + '\n')
    for B, g in SIZES:
        training_step(B, g, a.reps, emit)
        torch.cuda.empty_cache()
        dw_alone(B, g, a.reps, a.f16_peak, emit)
        torch.cuda.empty_cache()


if __name__ == '__main__':
    main()
