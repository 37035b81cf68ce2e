#!/usr/bin/env python3
"""Time and memory of one 'fact' RL training iteration on n sampled captions per image, in ONE process: Detector.forward
over one batch (roll-out(s), CIDEr-D + classifier rewards, XE and seq2seq unrolls, backward, clamp + Adam), training mode,
default dropout, V = 10000, T = 20, every form served eagerly.  Forms, alternating:
  grouped   Detector.rl_samples_per_image = n on the I images: the differentiable grouped roll-out
            (forward_rl captions_per_image=n), no greedy roll-out, the reward from isc_group_reward;
  repeated  the same iteration with the roll-out on inputs expanded with repeat_interleave(n, 0) and
            captions_per_image=1 (a wrapper on Captioner.forward_rl; XE / seq2seq stay on the I images);
  today     today's iteration (sampled + greedy roll-out, rl_samples_per_image = 1) on I*n images' worth of rows: the
            batch repeated n times, so its XE unroll runs on I*n rows as well.
Per I x n x regions it reports, for each form: ms per iteration (HIP events around the iteration; median, min, max over
--reps after two warm-ups) and torch.cuda.max_memory_allocated over one iteration; and the roll-out prologue's ms (events
around Captioner._prologue) on the I images and on the I*n repeated rows.

    python tools/group_rl_probe.py [--configs 128x5x36,512x5x36,128x5x196] [--reps 5] [--out FILE]
"""
import argparse
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch

from insenticap_model_amd import synth
from insenticap_model_amd.detector import Detector

V, T = 10000, 20
GRIDS = {36: (6, 6), 196: (14, 14)}


def timed(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    out = fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1), out


def load_helper(mod, seed):
    shapes = {k: tuple(v.shape) for k, v in mod.state_dict().items()}
    mod.load_state_dict({k: torch.from_numpy(v) for k, v in synth.make_module_weights(shapes, seed).items()})
    return mod.eval()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--configs', default='128x5x36,512x5x36,128x5x196')
    ap.add_argument('--reps', type=int, default=5)
    ap.add_argument('--out', default=None)
    a = ap.parse_args()
    dev = torch.device('cuda:0')
    st = dict(synth.DEFAULT_SETTINGS, **synth.HELPER_SETTINGS)
    det = Detector(synth.make_idx2word(V), T, synth.SENTIMENT_CATEGORIES, {'cap_lr': 4e-5}, st)
    det.captioner.load_state_dict({k: torch.from_numpy(v) for k, v in synth.make_weights(V, st, seed=0).items()})
    load_helper(det.senti_detector, 51)
    load_helper(det.sent_senti_cls, 52)
    det.to(dev)
    det.train_graphs = False                    # every form eagerly: the grouped iteration has no graph route
    cap = det.captioner
    plain_rl = cap.forward_rl

    def repeated_rl(*args, **kw):               # the grouped call on repeated inputs, captions_per_image = 1 rows
        n = kw.pop('captions_per_image', 1)
        if n > 1:
            args = [x.repeat_interleave(n, 0) for x in args[:5]] + list(args[5:])
        return plain_rl(*args, **kw)
    t = torch.from_numpy
    s = synth.make_inputs(80, V, st, regions=1, seq_len=T, seed=72)
    scs = [((t(s['captions']), s['lengths']), t(s['cpt_words']), t(s['senti_words']), t(s['senti_labels']))]
    lines = []
    for cfg in a.configs.split(','):
        I, n, R = (int(x) for x in cfg.split('x'))
        (b,), split = synth.make_rl_batches(1, I, V, st, grid=GRIDS[R], seq_len=T, seed=70)
        det.set_ciderd_scorer(split)
        item = (b[0], t(b[1]).to(dev), t(b[2]).to(dev), (t(b[3][0]), b[3][1]), t(b[4]), t(b[5]), b[6])
        rep = lambda x: x.repeat_interleave(n, 0)
        big = ([fn for fn in b[0] for _ in range(n)], rep(item[1]), rep(item[2]),
               (rep(item[3][0]), [int(l) for l in np.repeat(np.asarray(b[3][1]), n)]), rep(item[4]), rep(item[5]), b[6])

        def iteration(form):
            det.rl_samples_per_image = 1 if form == 'today' else n
            cap.forward_rl = repeated_rl if form == 'repeated' else plain_rl
            return det(([big if form == 'today' else item], scs), 'fact', True)
        forms = ('grouped', 'repeated', 'today')
        res = {'images': I, 'samples_per_image': n, 'rows': I * n, 'regions': R, 'V': V, 'T': T, 'reps': a.reps}
        times = {k: [] for k in forms}
        for r in range(a.reps + 2):                                      # two warm-up rounds
            for form in forms:
                ms, _ = timed(lambda: iteration(form))
                if r >= 2:
                    times[form].append(ms)
        for form in forms:
            ts = times[form]
            res[form] = {'ms_per_iter_median': statistics.median(ts), 'ms_per_iter_min': min(ts), 'ms_per_iter_max': max(ts)}
        torch.cuda.empty_cache()
        for form in forms:                                               # peak memory of one iteration
            torch.cuda.synchronize()
            torch.cuda.reset_peak_memory_stats()
            before = torch.cuda.memory_allocated()
            iteration(form)
            torch.cuda.synchronize()
            res[form]['max_memory_allocated_bytes'] = torch.cuda.max_memory_allocated()
            res[form]['resident_before_iter_bytes'] = before
        cap.forward_rl = plain_rl
        cap.train()
        labels = torch.zeros(I, dtype=torch.int64, device=dev)
        ins = (item[1], item[2].reshape(I, -1, item[2].shape[-1]), item[4].to(dev), item[5].to(dev), labels)
        with torch.no_grad():
            p = cap._p()
            for form, args in (('grouped', ins), ('repeated', [rep(x) for x in ins])):
                pro = [timed(lambda: cap._prologue(p, 'rl', *args, None))[0] for _ in range(4)][1:]
                res[form]['prologue_ms'] = statistics.median(pro)
        res['today']['prologue_ms'] = res['repeated']['prologue_ms']     # (the same rows; run twice there: sample + greedy)
        others = min(res['repeated']['ms_per_iter_min'], res['today']['ms_per_iter_min'])
        res['grouped_faster_beyond_spread'] = res['grouped']['ms_per_iter_max'] < others
        res['speedup_median_vs_repeated'] = res['repeated']['ms_per_iter_median'] / res['grouped']['ms_per_iter_median']
        res['speedup_median_vs_today'] = res['today']['ms_per_iter_median'] / res['grouped']['ms_per_iter_median']
        lines.append(json.dumps(res))
        print(lines[-1], flush=True)
        del big, item
        torch.cuda.empty_cache()
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        open(a.out, 'w').write('\n'.join(lines) + '\n')


if __name__ == '__main__':
    main()
