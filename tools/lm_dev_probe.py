#!/usr/bin/env python3
"""What the n-gram language-model scorer costs, in ONE process: HIP events and host clocks, medians with their ranges, the
forms alternating, every step under a time limit (the process ends when one runs over).

Three order-3 models of about 10^6 synthetic n-grams each (V = 10000: every unigram, 4 x 10^5 bigrams, 6 x 10^5
trigrams, drawn at random; tables at the production capacity), rows of T = 20 built from the models' own trigrams with
random words mixed in, labels at random:
  * the kernel (isc_lm_dev_score, HIP events around the launch) at 1024 and 2560 rows;
  * the same rows through the host scorer (isc_lm_score) on 16 threads, wall time, and whether the two agree in bits;
  * the 512-image eager RL training iteration (train_graphs = False, device_cider on) with lm_flag 0 - the iteration as
    it was before the LM reward existed - and 0.1 on the device, and 0.1 through the host scorer.
The numbers are reported, nothing is gated.

    python tools/lm_dev_probe.py [--reps 9] [--skip-detector] [--out FILE]
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

SOS, EOS = 1, 2


def synthetic_lm(seed, n2=400000, n3=600000):
    """-> (NgramLM, its trigram ids [n, 3]): all V unigrams + <s>, </s>, <unk>, random bigrams and trigrams."""
    rng = np.random.default_rng(seed)

    def keys_of(ids):
        key = np.zeros(len(ids), dtype=np.uint64)
        for j in range(ids.shape[1]):
            key |= (ids[:, j] + 1).astype(np.uint64) << np.uint64(16 * j)
        return key
    uni = np.arange(V + 3, dtype=np.int64)[:, None]
    bi = np.unique(rng.integers(4, V, size=(n2, 2)), axis=0)
    tri = np.unique(rng.integers(4, V, size=(n3, 3)), axis=0)
    starts = np.unique(np.concatenate([np.full((2000, 1), V), rng.integers(4, V, size=(2000, 1))], axis=1), axis=0)
    ends = np.unique(np.concatenate([rng.integers(4, V, size=(2000, 1)), np.full((2000, 1), V + 1)], axis=1), axis=0)
    keys = np.concatenate([keys_of(x) for x in (uni, bi, starts, ends, tri)])
    n = len(keys)
    logp = -rng.uniform(0.05, 5.0, size=n).astype(np.float32)
    backoff = np.where(rng.random(n) < 0.7, -rng.uniform(0.0, 1.5, size=n), 0.0).astype(np.float32)
    backoff[len(keys) - len(tri):] = 0.0
    return rewards.NgramLM(3, V, keys, logp, backoff), tri


def rows_of(tris, labels, seed):
    rng = np.random.default_rng(seed)
    rows = np.full((len(labels), T), EOS, dtype=np.int64)
    for r, lab in enumerate(labels):
        tri = tris[lab]
        words = tri[rng.integers(0, len(tri), size=7)].reshape(-1)[:T].copy()
        noise = rng.random(T) < 0.15
        words[noise] = rng.integers(4, V, size=int(noise.sum()))
        n = int(rng.integers(5, T + 1))
        rows[r, :n] = words[:n]
    return rows


def probe_scoring(a, lines, lms, dev, tris):
    for N in (1024, 2560):
        with step_limit(a.step_limit, 'scoring, N = %d' % N):
            labels = np.random.default_rng(N).integers(0, 3, size=N).astype(np.int64)
            rows = rows_of(tris, labels, seed=N)
            d_rows, d_labels = torch.from_numpy(rows).to(DEV), torch.from_numpy(labels).to(DEV)
            outs = (torch.empty(N, dtype=torch.float64, device=DEV), torch.empty(N, dtype=torch.int32, device=DEV),
                    torch.empty(N, dtype=torch.int32, device=DEV))
            got = dev.score(d_rows, d_labels, out=outs[0], n_scored=outs[1], n_oov=outs[2])
            want = lms.score(rows, labels)
            res = {'probe': 'scoring', 'N': N, 'T': T, 'V': V, 'ngrams': [len(m) for m in lms.lms], 'reps': a.reps,
                   'slots': int(len(lms.slots)), 'host_threads': lms.n_threads,
                   'equal_in_bits': bool(np.array_equal(got[0].cpu().numpy().view(np.int64), want[0].view(np.int64)) and
                                         np.array_equal(got[1].cpu().numpy(), want[1])),
                   'mean_scored_positions': float(want[1].mean())}
            kern, dev_wall, host_wall = [], [], []
            for r in range(a.reps + 2):                                  # two warm-up rounds, the forms alternating
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                torch.cuda.synchronize()
                e0.record()
                dev.score(d_rows, d_labels, out=outs[0], n_scored=outs[1], n_oov=outs[2])
                e1.record()
                torch.cuda.synchronize()
                w0 = time.perf_counter()
                dev.score(d_rows, d_labels, out=outs[0], n_scored=outs[1], n_oov=outs[2])
                torch.cuda.synchronize()
                w1 = time.perf_counter()
                lms.score(rows, labels)
                w2 = time.perf_counter()
                if r >= 2:
                    kern.append(e0.elapsed_time(e1))
                    dev_wall.append((w1 - w0) * 1e3)
                    host_wall.append((w2 - w1) * 1e3)
            res.update(device_kernel=stats(kern), device_launch_wait_wall=stats(dev_wall),
                       host_16_threads_wall=stats(host_wall))
            res['device_faster_beyond_spread'] = max(dev_wall) < min(host_wall)
            lines.append(json.dumps(res))
            print(lines[-1], flush=True)


def probe_detector(a, lines, lms):
    st = dict(synth.DEFAULT_SETTINGS, **synth.HELPER_SETTINGS)
    with step_limit(a.step_limit, 'building the detector'):
        det = Detector(synth.make_idx2word(V), T, synth.SENTIMENT_CATEGORIES, {'cap_lr': 4e-5}, st)
        det.captioner.load_state_dict({k: torch.from_numpy(v) for k, v in synth.make_weights(V, st, seed=0).items()})
        load_helper(det.senti_detector, 51)
        load_helper(det.sent_senti_cls, 52)
        det.to(DEV)
        det.train_graphs, det.device_cider = False, True
        t = torch.from_numpy
        s = synth.make_inputs(80, V, st, regions=1, seq_len=T, seed=72)
        scs = [((t(s['captions']), s['lengths']), t(s['cpt_words']), t(s['senti_words']), t(s['senti_labels']))]
        (b,), split = synth.make_rl_batches(1, IMAGES, V, st, grid=(6, 6), seq_len=T, seed=70)
        det.set_ciderd_scorer(split)
        det.set_lms(lms)
        item = (b[0], t(b[1]).to(DEV), t(b[2]).to(DEV), (t(b[3][0]), b[3][1]), t(b[4]), t(b[5]), b[6])
    twin = det._device_lms
    forms = {'lm_flag_0': (0.0, twin), 'lm_flag_0.1_device': (0.1, twin), 'lm_flag_0.1_host': (0.1, lambda device, T_: None)}
    ev, wall = {k: [] for k in forms}, {k: [] for k in forms}
    with step_limit(a.step_limit, 'Detector.forward'):
        for r in range(a.reps + 2):                                      # two warm-up rounds, the forms alternating
            for name, (flag, lookup) in forms.items():
                det.lm_flag, det._device_lms = flag, lookup
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                torch.cuda.synchronize()
                w0 = time.perf_counter()
                e0.record()
                det(([item], scs), 'fact', True)
                e1.record()
                torch.cuda.synchronize()
                w1 = time.perf_counter()
                if r >= 2:
                    ev[name].append(e0.elapsed_time(e1))
                    wall[name].append((w1 - w0) * 1e3)
    res = {'probe': 'detector', 'form': 'eager_training_512', 'images': IMAGES, 'V': V, 'T': T, 'reps': a.reps,
           'host_threads': lms.n_threads}
    for name in forms:
        res[name] = {'events': stats(ev[name]), 'wall': stats(wall[name])}
    for name in ('lm_flag_0.1_device', 'lm_flag_0.1_host'):
        res['cost_median_wall_ms_' + name] = res[name]['wall']['median_ms'] - res['lm_flag_0']['wall']['median_ms']
    res['cost_beyond_spread_device'] = min(wall['lm_flag_0.1_device']) > max(wall['lm_flag_0'])
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
    with step_limit(a.step_limit, 'building the models'):
        built = [synthetic_lm(300 + i) for i in range(3)]
        lms = rewards.NgramLMSet([m for m, _ in built], V, 'word', True, sos=SOS, eos=EOS, n_threads=16)
        dev = lms.to_device(DEV)
        torch.cuda.synchronize()
    probe_scoring(a, lines, lms, dev, [tri for _, tri in built])
    if not a.skip_detector:
        probe_detector(a, lines, lms)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        open(a.out, 'w').write('\n'.join(lines) + '\n')


if __name__ == '__main__':
    main()
