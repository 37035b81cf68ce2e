#!/usr/bin/env python3
"""Time of the roll-out with and without the beam search's token constraints.

Inputs resident, eval mode, V = 10000, T = 20, 36 regions; HIP events around forward_rl,
  plain greedy / plain sampled (no keywords: the launches of a tree without the constraints) and
  greedy / sampled under suppress_special=True, decoding_constraint=1, min_len=4,
  the sampled roll-out with (temperature, top_k, top_p) = (0.8, 50, 0.9) without and with the constraints,
the configurations alternating inside one process.  Prints one JSON line per batch size.

    python tools/constrained_rollout_probe.py [--batches 4096,16384] [--reps 7] [--out FILE]

The allowance: per executed decode step a constrained roll-out, greedy or sampled, may cost what the plain SAMPLED
roll-out costs (it already writes the step's logits) plus one pass over the [B, V] fp32 logits at the HBM rate the
attention scan reaches (6 TB/s): B * V * 4 bytes / 6 TB/s, 0.11 ms at B = 16384."""
import argparse
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch

from insenticap_model_amd import Captioner, synth

V, R, T = 10000, 36, 20
CONS = dict(suppress_special=True, decoding_constraint=1, min_len=4)
FILTER = dict(temperature=0.8, top_k=50, top_p=0.9)
SCAN_TBS = 6.0


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
    configs = [('plain_greedy', 1, {}), ('plain_sampled', 0, {}), ('constrained_greedy', 1, CONS),
               ('constrained_sampled', 0, CONS), ('plain_filtered', 0, FILTER),
               ('constrained_filtered', 0, dict(CONS, **FILTER))]     # (the filtered pair: reported, no allowance set)
    lines = []
    for B in [int(x) for x in a.batches.split(',')]:
        d = synth.make_inputs(B, V, st, regions=R, seq_len=T, seed=5)
        ins = [torch.from_numpy(d[k]).to(dev) for k in ('fc_feats', 'att_feats', 'cpt_words', 'senti_words', 'senti_labels')]
        times = {name: [] for name, _, _ in configs}
        steps = {}
        with torch.no_grad():
            for rep in range(a.reps + 2):                       # two warm-up rounds
                for name, sample_max, kw in configs:
                    torch.manual_seed(rep)
                    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    e0.record()
                    seq, lp, mk = cap.forward_rl(*ins, T, sample_max, **kw)
                    e1.record()
                    torch.cuda.synchronize()
                    if rep >= 2:
                        times[name].append(e0.elapsed_time(e1))
                    steps[name] = int(mk.sum(0).gt(0).sum().item())       # executed decode steps
        allowance = B * V * 4 / (SCAN_TBS * 1e12) * 1e3
        res = {'B': B, 'V': V, 'T': T, 'regions': R, 'reps': a.reps, 'constraints': CONS,
               'allowance_ms_per_step_over_plain_sampled': allowance}
        for name, _, _ in configs:
            ts = times[name]
            res[name] = {'ms_per_call_median': statistics.median(ts), 'ms_per_call_min': min(ts), 'ms_per_call_max': max(ts),
                         'steps': steps[name], 'ms_per_step_median': statistics.median(ts) / max(steps[name], 1)}
        for name in ('constrained_greedy', 'constrained_sampled'):
            over = res[name]['ms_per_step_median'] - res['plain_sampled']['ms_per_step_median']
            res[name]['ms_per_step_over_plain_sampled'] = over
            res[name]['within_allowance'] = bool(over <= allowance)
        res['constrained_filtered']['ms_per_step_over_plain_filtered'] = (
            res['constrained_filtered']['ms_per_step_median'] - res['plain_filtered']['ms_per_step_median'])
        lines.append(json.dumps(res))
        print(lines[-1], flush=True)
        del ins, d
        torch.cuda.empty_cache()
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        open(a.out, 'w').write('\n'.join(lines) + '\n')


if __name__ == '__main__':
    main()
