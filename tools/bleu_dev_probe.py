#!/usr/bin/env python3
"""What the device BLEU scorer (rewards.DeviceBleu) costs beside the host scorer, and beside CIDEr-D, in ONE process: HIP
events and host clocks, the forms alternating, every step under a time limit (the process ends when one runs over).

On the same rows - T = 20, 512 images of synth.make_cider_data(600, 10000, ...), N = 1024 (sample + greedy, one row per
image) and N = 2560 (512 images x 5 rows, row_div 5) - for BLEU and for CIDEr-D: the kernel (HIP events around the
launch), the host's wall time for pack_refs + launch + wait (references cached), and the host scorer on 16 threads (wall
time).  For BLEU also the largest relative difference of the four scores, device against host, and whether the integer
statistics are equal.  The numbers are reported, nothing is gated.

    python tools/bleu_dev_probe.py [--reps 9] [--out FILE]
"""
import argparse
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch

from cider_dev_probe import DEV, IMAGES, T, V, stats, step_limit
from insenticap_model_amd import rewards, synth


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--reps', type=int, default=9)
    ap.add_argument('--step-limit', type=int, default=150, help='seconds per step')
    ap.add_argument('--out', default=None)
    a = ap.parse_args()
    lines = []
    split, fns, gt, sample, greedy = synth.make_cider_data(600, V, IMAGES, seq_len=T, seed=8)
    refs = [gt[f] for f in fns]
    five = np.ascontiguousarray(np.stack([sample, greedy, sample, greedy, sample], 1).reshape(IMAGES * 5, T))
    cases = {1024: (np.concatenate([sample, greedy]), refs * 2, list(fns) + [f + '#g' for f in fns], 1),
             2560: (five, refs, list(fns), 5)}
    with step_limit(a.step_limit, 'building the scorers'):
        scorers = {'bleu': rewards.get_bleu_scorer(1, 2), 'ciderd': rewards.get_ciderd_scorer(split, 1, 2)}
        twins = {}
        for name, s in scorers.items():
            s.n_threads = 16
            twins[name] = s.to_device(DEV, V)
        torch.cuda.synchronize()
    for N, (rows, ref_lists, keys, row_div) in cases.items():
        d_rows = torch.from_numpy(rows).to(DEV)
        host_refs = [ref_lists[r // row_div] for r in range(N)]
        flat_keys = [keys[r // row_div] + '/%d' % (r % row_div) for r in range(N)]
        for name in ('bleu', 'ciderd'):
            scorer, dev = scorers[name], twins[name]
            with step_limit(a.step_limit, '%s, N = %d' % (name, N)):
                bleu = name == 'bleu'
                # the host scorer as the trainer calls it: BLEU cooks an image's references once for its row_div rows
                host_flat = (scorer.flatten_refs(ref_lists, keys=keys) if bleu else
                             scorer.flatten_refs(host_refs, keys=flat_keys))
                host_call = ((lambda: scorer.score_arrays(rows, None, host_flat, row_div=row_div)) if bleu else
                             (lambda: scorer.score_arrays(rows, None, host_flat)))
                pack = dev.pack_refs(ref_lists, keys=keys)
                res = {'probe': 'scoring', 'scorer': name, 'N': N, 'T': T, 'row_div': row_div, 'reps': a.reps,
                       'host_threads': scorer.n_threads}
                if bleu:
                    st = torch.empty(N, 10, dtype=torch.int32, device=DEV)
                    got = dev.score4(d_rows, pack, row_div=row_div, stats=st).cpu().numpy()
                    want = scorer.score4(rows, None, host_flat, row_div=row_div)
                    res['max_rel_diff_vs_host'] = float((np.abs(got - want) / np.abs(want)).max())
                    res['stats_equal'] = bool(np.array_equal(st.cpu().numpy(),
                                                             scorer.stats(rows, None, host_flat, row_div=row_div)))
                else:
                    got = dev.score(d_rows, pack, row_div=row_div).cpu().numpy()
                    res['max_abs_diff_vs_host'] = float(np.abs(got - host_call()).max())
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
                    host_call()
                    w2 = time.perf_counter()
                    if r >= 2:
                        kern.append(e0.elapsed_time(e1))
                        dev_wall.append((w1 - w0) * 1e3)
                        host_wall.append((w2 - w1) * 1e3)
                res.update(device_kernel=stats(kern), device_pack_score_wait_wall=stats(dev_wall),
                           host_16_threads_wall=stats(host_wall))
                res['device_faster_beyond_spread'] = max(dev_wall) < min(host_wall)
                lines.append(json.dumps(res))
                print(lines[-1], flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        open(a.out, 'w').write('\n'.join(lines) + '\n')


if __name__ == '__main__':
    main()
