#!/usr/bin/env python3
"""Time of the sampled roll-out with and without the sampling controls (temperature / top-k / top-p).

Inputs resident, eval mode, V = 10000, T = 20, 36 regions; HIP events around
  (a) forward_rl(sample_max=0) with default arguments - the plain sampled roll-out -,
  (b) the same with (temperature, top_k, top_p) = (0.8, 0, 0.9) and (1.0, 50, 1.0),
the configurations alternating inside one process.  On a tree without the controls only (a) is measured (that is how
the comparison point - (a) at the parent commit - is taken on the same machine).  Prints one JSON line per batch size.

    python tools/sample_filter_probe.py [--batches 4096,16384] [--reps 7] [--out FILE]
    rocprofv3 --kernel-trace --stats -d DIR -- python tools/sample_filter_probe.py --batches 16384 --reps 2
        (a run of its own: rollout_finalize_filtered_kernel's time per launch)

The bound the issue sets: per decode step (b) may exceed the PARENT's (a) by at most two passes over the [B, V] logits
at the HBM rate the attention scan reaches (6.0-6.6 TB/s): 2 * B * V * 4 bytes / 6.3 TB/s, 0.21 ms at B = 16384."""
import argparse
import inspect
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch

from insenticap_model_amd import Captioner, synth

V, R, T = 10000, 36, 20
CONTROLS = [(0.8, 0, 0.9), (1.0, 50, 1.0)]
SCAN_TBS = 6.3


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--batches', default='4096,16384')
    ap.add_argument('--reps', type=int, default=7)
    ap.add_argument('--out', default=None)
    a = ap.parse_args()
    dev = torch.device('cuda:0')
    st = synth.DEFAULT_SETTINGS
    cap = Captioner(synth.make_idx2word(V), synth.SENTIMENT_CATEGORIES, st)
    cap.load_state_dict({k: torch.from_numpy(v) for k, v in synth.make_weights(V, st, seed=0).items()})
    cap.to(dev).eval()
    has_controls = 'temperature' in inspect.signature(Captioner.forward_rl).parameters
    configs = [('plain', {})]
    if has_controls:
        configs += [('t%g_k%d_p%g' % c, dict(temperature=c[0], top_k=c[1], top_p=c[2])) for c in CONTROLS]
    lines = []
    for B in [int(x) for x in a.batches.split(',')]:
        d = synth.make_inputs(B, V, st, regions=R, seq_len=T, seed=5)
        ins = [torch.from_numpy(d[k]).to(dev) for k in ('fc_feats', 'att_feats', 'cpt_words', 'senti_words', 'senti_labels')]
        times = {name: [] for name, _ in configs}
        steps = {}
        with torch.no_grad():
            for rep in range(a.reps + 2):                       # two warm-up rounds
                for name, kw in configs:
                    torch.manual_seed(rep)
                    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    e0.record()
                    seq, lp, mk = cap.forward_rl(*ins, T, 0, **kw)
                    e1.record()
                    torch.cuda.synchronize()
                    if rep >= 2:
                        times[name].append(e0.elapsed_time(e1))
                    steps[name] = int(mk.sum(0).gt(0).sum().item())       # executed decode steps
        res = {'B': B, 'V': V, 'T': T, 'regions': R, 'reps': a.reps, 'has_controls': has_controls,
               'bound_ms_per_step_over_parent_plain': 2 * B * V * 4 / (SCAN_TBS * 1e12) * 1e3}
        for name, _ in configs:
            ts = times[name]
            res[name] = {'ms_per_call_median': statistics.median(ts), 'ms_per_call_min': min(ts), 'ms_per_call_max': max(ts),
                         'steps': steps[name], 'ms_per_step_median': statistics.median(ts) / max(steps[name], 1)}
        if has_controls:
            for name, _ in configs[1:]:
                res[name]['ms_per_step_over_plain_same_tree'] = (res[name]['ms_per_step_median']
                                                                 - res['plain']['ms_per_step_median'])
        lines.append(json.dumps(res))
        print(lines[-1], flush=True)
        del ins, d
        torch.cuda.empty_cache()
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        open(a.out, 'w').write('\n'.join(lines) + '\n')


if __name__ == '__main__':
    main()
