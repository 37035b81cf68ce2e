#!/usr/bin/env python3
"""The concept detector's native path beside its stock torch ops, in ONE process, the forms alternating, HIP events and
host clocks, every step under a time limit (the process ends when one runs over).  Product widths 2048 / 1024 / 2000,
weights synth.make_module_weights, features U[0, 1).

  forward + top-5 at B = 1 (test_cpt.py), 100 (detect_concepts.py:35) and 4096: `sample_device` native against
      `enable_native(False)` - host enqueue time (a host clock around the call, no wait) and device time (HIP events);
      the largest |native - torch| probability and whether both pick the same concepts;
  one training iteration at B = 80 (opts.py:12): train.concept_train_step against model / MultiLabelClsLoss / backward /
      clip_gradient / FusedClampAdam on torch ops - wall time per iteration with a wait at its end;
  Detector.sample per image (beam 3) with the sentiment words derived on the device against words passed in.

The numbers are reported, nothing is gated.

    python tools/concept_probe.py [--reps 15] [--out FILE]
"""
import argparse
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch

from cider_dev_probe import DEV, stats, step_limit
from insenticap_model_amd import data, synth
from insenticap_model_amd.helper_nets import ConceptDetector
from insenticap_model_amd.optim import clip_gradient
from insenticap_model_amd.train import concept_train_step

F, H, C, NUM = 2048, 1024, 2000, 5


def model(dropout_p=0.5, seed=61):
    m = ConceptDetector(['c%d' % i for i in range(C)], dict(fc_feat_dim=F, concept_mid_him=H, dropout_p=dropout_p))
    w = synth.make_module_weights({n: tuple(v.shape) for n, v in m.state_dict().items()}, seed, gain=3.0)
    m.load_state_dict({n: torch.from_numpy(v) for n, v in w.items()})
    return m.to(DEV)


def timed(fn):
    """(host enqueue ms, device ms) of fn(): the stream is idle at the start; the host clock stops when fn returns."""
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    e0.record()
    fn()
    e1.record()
    t1 = time.perf_counter()
    torch.cuda.synchronize()
    return (t1 - t0) * 1e3, e0.elapsed_time(e1)


def probe_forward(a, lines):
    m = model().eval()
    rng = np.random.default_rng(3)
    for B in (1, 100, 4096):
        with step_limit(a.step_limit, 'forward + top-%d, B = %d' % (NUM, B)):
            x = torch.from_numpy(rng.random((B, F)).astype(np.float32)).to(DEV)
            forms = {'native': lambda: m.enable_native(True).sample_device(x, NUM),
                     'torch': lambda: m.enable_native(False).sample_device(x, NUM)}
            n_idx, n_sc, _ = forms['native']()
            t_idx, t_sc, _ = forms['torch']()
            res = {'probe': 'forward_top%d' % NUM, 'B': B, 'reps': a.reps,
                   'same_concepts': bool(torch.equal(n_idx, t_idx)),
                   'rows_with_other_concepts': int((n_idx != t_idx).any(dim=1).sum()),
                   'max_abs_score_diff': float((n_sc - t_sc).abs().max())}
            t = {k: ([], []) for k in forms}
            for r in range(a.reps + 3):                      # three warm-up rounds, the forms alternating
                for k, fn in forms.items():
                    host, dev = timed(fn)
                    if r >= 3:
                        t[k][0].append(host)
                        t[k][1].append(dev)
            for k in forms:
                res[k + '_host_enqueue'] = stats(t[k][0])
                res[k + '_device'] = stats(t[k][1])
            res['native_device_faster_beyond_spread'] = max(t['native'][1]) < min(t['torch'][1])
            res['native_host_faster_beyond_spread'] = max(t['native'][0]) < min(t['torch'][0])
            m.enable_native(True)
            lines.append(json.dumps(res))
            print(lines[-1], flush=True)


def probe_training(a, lines):
    B = 80
    with step_limit(a.step_limit, 'training iteration, B = %d' % B):
        rng = np.random.default_rng(4)
        x = torch.from_numpy(rng.random((B, F)).astype(np.float32)).to(DEV)
        y = torch.from_numpy((rng.random((B, C)) < 0.005).astype(np.int64)).to(DEV)
        nat, ref = model().train(), model().train()
        o_nat, _ = nat.get_optim_criterion(4e-4)
        o_ref, crit = ref.get_optim_criterion(4e-4)

        def native():
            return concept_train_step(nat, o_nat, x, y, 0.1)

        def stock():
            loss = crit(ref(x), y)
            o_ref.zero_grad()
            loss.backward()
            clip_gradient(o_ref, 0.1)
            o_ref.step()
            return loss.detach()
        forms = {'native': native, 'torch': stock}
        t = {k: [] for k in forms}
        for r in range(a.reps + 3):
            for k, fn in forms.items():
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                fn()
                torch.cuda.synchronize()
                if r >= 3:
                    t[k].append((time.perf_counter() - t0) * 1e3)
        res = {'probe': 'training_iteration', 'B': B, 'reps': a.reps, 'native_wall': stats(t['native']),
               'torch_wall': stats(t['torch']),
               'native_faster_beyond_spread': max(t['native']) < min(t['torch'])}
        lines.append(json.dumps(res))
        print(lines[-1], flush=True)


def probe_detector(a, lines):
    from insenticap_model_amd.detector import Detector
    with step_limit(a.step_limit, 'Detector.sample per image'):
        V = 10000
        st = dict(synth.DEFAULT_SETTINGS, **synth.HELPER_SETTINGS)
        idx2word = synth.make_idx2word(V)
        det = Detector(idx2word, 16, synth.SENTIMENT_CATEGORIES, {'cap_lr': 4e-5}, st)
        det.captioner.load_state_dict({k: torch.from_numpy(v) for k, v in synth.make_weights(V, st, seed=0).items()})
        for mod, seed in ((det.senti_detector, 51), (det.sent_senti_cls, 52)):
            shapes = {k: tuple(v.shape) for k, v in mod.state_dict().items()}
            mod.load_state_dict({k: torch.from_numpy(v) for k, v in synth.make_module_weights(shapes, seed).items()})
        det.to(DEV).eval()
        word2idx = {w: i for i, w in enumerate(idx2word)}
        cd = ConceptDetector(idx2word[100:100 + C], dict(fc_feat_dim=F, concept_mid_him=H, dropout_p=0.5))
        w = synth.make_module_weights({n: tuple(v.shape) for n, v in cd.state_dict().items()}, 61, gain=3.0)
        cd.load_state_dict({n: torch.from_numpy(v) for n, v in w.items()})
        cd.set_vocabulary(word2idx).to(DEV)
        rng = np.random.default_rng(5)
        sd = {c: [[idx2word[int(rng.integers(3000, 5000))], float(rng.random())] for _ in range(int(rng.integers(0, 40)))]
              for c in cd.idx2concept}
        table = data.SentimentWordTable(sd, word2idx, cd.idx2concept)
        det.set_concept_detector(cd, table)
        d = synth.make_inputs(8, V, st, regions=36, seq_len=16, seed=9, grid=(6, 6))
        fc = torch.from_numpy(d['fc_feats']).to(DEV)
        att = torch.from_numpy(d['att_feats']).to(DEV)
        words = [det.tag(fc[i:i + 1])[1][0].clone() for i in range(8)]
        same = all(det.sample(fc[i], att[i], None) == det.sample(fc[i], att[i], words[i]) for i in range(8))
        t = {'derived_on_device': [], 'words_passed_in': []}
        for r in range(a.reps + 2):
            for k in t:
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                for i in range(8):
                    det.sample(fc[i], att[i], None if k == 'derived_on_device' else words[i])
                if r >= 2:
                    t[k].append((time.perf_counter() - t0) * 1e3 / 8)
        res = {'probe': 'detector_sample_per_image', 'beam': 3, 'reps': a.reps, 'same_captions': bool(same),
               'derived_on_device_wall': stats(t['derived_on_device']), 'words_passed_in_wall': stats(t['words_passed_in'])}
        lines.append(json.dumps(res))
        print(lines[-1], flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--reps', type=int, default=15)
    ap.add_argument('--step-limit', type=int, default=150, help='seconds per step')
    ap.add_argument('--out', default=None)
    ap.add_argument('--skip-detector', action='store_true')
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit('concept_probe needs the GPU: there is nothing to time without one')
    lines = []
    probe_forward(a, lines)
    probe_training(a, lines)
    if not a.skip_detector:
        probe_detector(a, lines)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        open(a.out, 'w').write('\n'.join(lines) + '\n')


if __name__ == '__main__':
    main()
