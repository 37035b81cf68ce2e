#!/usr/bin/env python3
"""What the device CIDEr-D scorer (rewards.DeviceCiderD, Detector.device_cider) costs and gains, in ONE process, HIP
events and host clocks, the forms alternating, every step under a time limit (the process ends when one runs over).

(a) The scoring alone, on the same rows: DeviceCiderD.score (HIP events around the launch; and the host's wall time for
    pack_refs + score + wait, references cached) against CiderD.score_arrays at 16 threads (host wall time), for N = 1024
    (512 images, sample + greedy) and N = 2560 (512 images x 5 rows), T = 20, synth.make_cider_data(600, 10000, ...) -
    once with that corpus's own table and once with the table grown by --grow-images more images to a few million n-grams
    (what probing costs at COCO size); the table's bytes (16 B x capacity) are reported.
(b) Detector.forward with device_cider off and on (the same tree, the flag off = the path without this scorer): one
    'fact' evaluation batch of 512, one grouped 512 x 5 training iteration, one constrained n = 1 training iteration;
    V = 10000, T = 20, 36 regions, every form eager.  ms per call: HIP events around the call and the host's wall time.

    python tools/cider_dev_probe.py [--reps 7] [--grow-images 40000] [--skip-detector] [--out FILE]
"""
import argparse
import json
import os
import signal
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch

from insenticap_model_amd import rewards, synth
from insenticap_model_amd.detector import Detector

V, T, IMAGES = 10000, 20, 512
DEV = torch.device('cuda:0')


class step_limit:
    """A wall-clock limit for one step: when it runs out the process ends (nothing more is started on the device)."""

    def __init__(self, seconds, what):
        self.seconds, self.what = seconds, what

    def _over(self, *_):
        print('STEP OVER ITS TIME LIMIT (%d s): %s' % (self.seconds, self.what), flush=True)
        os._exit(124)

    def __enter__(self):
        signal.signal(signal.SIGALRM, self._over)
        signal.alarm(self.seconds)

    def __exit__(self, *exc):
        signal.alarm(0)
        return False


def stats(ts):
    return {'median_ms': statistics.median(ts), 'min_ms': min(ts), 'max_ms': max(ts)}


def grown_corpus(split, n_images, seed=11):
    """The corpus of make_cider_data plus n_images images of 5 Zipf-distributed captions each (drawn in one call)."""
    rng = np.random.default_rng(seed)
    ranks = np.arange(4, V)
    prob = 1.0 / (ranks - 3.0)
    prob /= prob.sum()
    lens = rng.integers(8, 19, size=n_images * 5)
    toks = rng.choice(ranks, size=int(lens.sum()), p=prob).tolist()
    caps, at = {}, 0
    for i in range(n_images):
        mine = []
        for L in lens[5 * i:5 * i + 5]:
            mine.append([1] + toks[at:at + L] + [2])
            at += L
        caps['extra%06d' % i] = mine
    return dict(split, extra=caps)


def probe_scoring(a, lines):
    split, fns, gt, sample, greedy = synth.make_cider_data(600, V, IMAGES, seq_len=T, seed=8)
    refs = [gt[f] for f in fns]
    five = np.ascontiguousarray(np.stack([sample, greedy, sample, greedy, sample], 1).reshape(IMAGES * 5, T))
    cases = {1024: (np.concatenate([sample, greedy]), refs * 2, list(fns) + [f + '#g' for f in fns], 1),
             2560: (five, refs, list(fns), 5)}
    for table_name, corpus in (('corpus', split), ('grown', grown_corpus(split, a.grow_images))):
        with step_limit(a.step_limit, 'building the %s scorer' % table_name):
            t0 = time.perf_counter()
            scorer = rewards.get_ciderd_scorer(corpus, 1, 2)
            scorer.n_threads = 16
            t1 = time.perf_counter()
            dev = scorer.to_device(DEV, V)
            torch.cuda.synchronize()
            t2 = time.perf_counter()
        for N, (rows, ref_lists, keys, row_div) in cases.items():
            with step_limit(a.step_limit, 'scoring N = %d, %s table' % (N, table_name)):
                d_rows = torch.from_numpy(rows).to(DEV)
                host_refs = [ref_lists[r // row_div] for r in range(N)]
                flat = scorer.flatten_refs(host_refs, keys=[keys[r // row_div] + '/%d' % (r % row_div) for r in range(N)])
                pack = dev.pack_refs(ref_lists, keys=keys)
                want = scorer.score_arrays(rows, None, flat)
                got = dev.score(d_rows, pack, row_div=row_div).cpu().numpy()
                err = float(np.abs(got - want).max())
                kern, dev_wall, host_wall = [], [], []
                for r in range(a.reps + 2):                              # two warm-up rounds, the forms alternating
                    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    torch.cuda.synchronize()
                    e0.record()
                    dev.score(d_rows, pack, row_div=row_div)
                    e1.record()
                    torch.cuda.synchronize()
                    w0 = time.perf_counter()
                    p2 = dev.pack_refs(ref_lists, keys=keys)
                    dev.score(d_rows, p2, row_div=row_div)
                    torch.cuda.synchronize()
                    w1 = time.perf_counter()
                    scorer.score_arrays(rows, None, flat)
                    w2 = time.perf_counter()
                    if r >= 2:
                        kern.append(e0.elapsed_time(e1))
                        dev_wall.append((w1 - w0) * 1e3)
                        host_wall.append((w2 - w1) * 1e3)
                res = {'probe': 'scoring', 'table': table_name, 'images_in_corpus': scorer.num_images,
                       'ngrams': scorer.num_ngrams, 'table_capacity': int(dev.table.shape[0]),
                       'table_bytes': int(dev.table.shape[0]) * 16, 'scorer_build_s': t1 - t0, 'table_upload_s': t2 - t1,
                       'N': N, 'T': T, 'row_div': row_div, 'reps': a.reps, 'max_abs_diff_vs_host': err,
                       'device_kernel': stats(kern), 'device_pack_score_wait_wall': stats(dev_wall),
                       'host_16_threads_wall': stats(host_wall), 'host_threads': scorer.n_threads}
                res['device_faster_beyond_spread'] = max(dev_wall) < min(host_wall)
                lines.append(json.dumps(res))
                print(lines[-1], flush=True)
        del dev, scorer
        torch.cuda.empty_cache()


def load_helper(mod, seed):
    shapes = {k: tuple(v.shape) for k, v in mod.state_dict().items()}
    mod.load_state_dict({k: torch.from_numpy(v) for k, v in synth.make_module_weights(shapes, seed).items()})
    return mod.eval()


def probe_detector(a, lines):
    st = dict(synth.DEFAULT_SETTINGS, **synth.HELPER_SETTINGS)
    with step_limit(a.step_limit, 'building the detector'):
        det = Detector(synth.make_idx2word(V), T, synth.SENTIMENT_CATEGORIES, {'cap_lr': 4e-5}, st)
        det.captioner.load_state_dict({k: torch.from_numpy(v) for k, v in synth.make_weights(V, st, seed=0).items()})
        load_helper(det.senti_detector, 51)
        load_helper(det.sent_senti_cls, 52)
        det.to(DEV)
        det.train_graphs = False
        t = torch.from_numpy
        s = synth.make_inputs(80, V, st, regions=1, seq_len=T, seed=72)
        scs = [((t(s['captions']), s['lengths']), t(s['cpt_words']), t(s['senti_words']), t(s['senti_labels']))]
        (b,), split = synth.make_rl_batches(1, IMAGES, V, st, grid=(6, 6), seq_len=T, seed=70)
        det.set_ciderd_scorer(split)
        det.ciderd_scorer.n_threads = 16
        item = (b[0], t(b[1]).to(DEV), t(b[2]).to(DEV), (t(b[3][0]), b[3][1]), t(b[4]), t(b[5]), b[6])
    forms = {'evaluation_512': dict(training=False, n=1, constraints=None),
             'grouped_512x5': dict(training=True, n=5, constraints=None),
             'constrained_512': dict(training=True, n=1,
                                     constraints=dict(suppress_special=True, decoding_constraint=1, min_len=3))}
    for name, f in forms.items():
        det.rl_samples_per_image, det.rollout_constraints = f['n'], f['constraints']
        data = ([item], scs) if f['training'] else ([item],)
        ev = {False: [], True: []}
        wall = {False: [], True: []}
        with step_limit(a.step_limit, 'Detector.forward, ' + name):
            for r in range(a.reps + 2):                                  # two warm-up rounds, the flag alternating
                for flag in (False, True):
                    det.device_cider = flag
                    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    torch.cuda.synchronize()
                    w0 = time.perf_counter()
                    e0.record()
                    det(data, 'fact', f['training'])
                    e1.record()
                    torch.cuda.synchronize()
                    w1 = time.perf_counter()
                    if r >= 2:
                        ev[flag].append(e0.elapsed_time(e1))
                        wall[flag].append((w1 - w0) * 1e3)
        res = {'probe': 'detector', 'form': name, 'images': IMAGES, 'rows': IMAGES * f['n'], 'V': V, 'T': T, 'reps': a.reps,
               'host_threads': det.ciderd_scorer.n_threads,
               'flag_off': {'events': stats(ev[False]), 'wall': stats(wall[False])},
               'flag_on': {'events': stats(ev[True]), 'wall': stats(wall[True])}}
        res['gain_median_wall_ms'] = res['flag_off']['wall']['median_ms'] - res['flag_on']['wall']['median_ms']
        res['on_faster_beyond_spread'] = max(wall[True]) < min(wall[False])
        lines.append(json.dumps(res))
        print(lines[-1], flush=True)
    det.device_cider, det.rl_samples_per_image, det.rollout_constraints = False, 1, None


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--reps', type=int, default=7)
    ap.add_argument('--grow-images', type=int, default=40000)
    ap.add_argument('--step-limit', type=int, default=150, help='seconds per step')
    ap.add_argument('--skip-detector', action='store_true')
    ap.add_argument('--out', default=None)
    a = ap.parse_args()
    lines = []
    probe_scoring(a, lines)
    if not a.skip_detector:
        probe_detector(a, lines)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        open(a.out, 'w').write('\n'.join(lines) + '\n')


if __name__ == '__main__':
    main()
