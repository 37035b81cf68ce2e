#!/usr/bin/env python3
"""Time and memory of n sampled captions per image: one grouped roll-out (forward_rl(captions_per_image=n) on the I
images) against today's form (the same call on inputs repeated with repeat_interleave(n, 0)), in ONE process.

Inputs resident, eval mode, V = 10000, T = 20, 36 regions of 2048, default sampling controls; the two forms alternate.
Per I x n it reports, for each form:
  * ms per roll-out (HIP events around the call; median, min, max over --reps) - the repeated form on inputs that were
    expanded beforehand, and the time of that expansion next to it;
  * prologue ms and the attention scan's us per step, from the per-kernel timer bench.py uses (ops.TIMER; one roll-out
    with the prologue armed, one with decode step --step armed);
  * torch.cuda.max_memory_allocated over one call, the images' inputs resident (the repeated form's call includes its
    expansion, as Captioner.sample_captions does it).
`grouped_faster_beyond_spread`: the slowest grouped repetition beat the fastest repeated one.

    python tools/group_rollout_probe.py [--configs 3277x5,2048x8,8192x2] [--reps 5] [--out FILE]
"""
import argparse
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch

from insenticap_model_amd import Captioner, ops, synth

V, R, T = 10000, 36, 20
BASE = 256          # distinct synthetic images; a batch tiles them (timing does not depend on the values)
KEYS = ('fc_feats', 'att_feats', 'cpt_words', 'senti_words', 'senti_labels')


def rep(xs, n):
    return [x.repeat_interleave(n, dim=0) for x in xs]


def timed(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    out = fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1), out


def kernel_times(call, step):
    """(prologue ms, scan us per step) of one form from the per-kernel timer."""
    res = []
    for arm in (-1, step):
        ops.TIMER.records = []
        ops.TIMER.arm_step = arm
        try:
            call()
            torch.cuda.synchronize()
            res.append(ops.TIMER.summary())
        finally:
            ops.TIMER.arm_step = None
            ops.TIMER.armed = False
            ops.TIMER.records = []
    pro = sum(d['total_ms'] for d in res[0].values() if d['phase'] == 'prologue')
    scan = sum(d['total_ms'] for k, d in res[1].items() if k.startswith('attn_scan')) * 1e3
    return pro, scan


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--configs', default='3277x5,2048x8,8192x2')
    ap.add_argument('--reps', type=int, default=5)
    ap.add_argument('--step', type=int, default=5, help='decode step whose kernels are timed')
    ap.add_argument('--out', default=None)
    a = ap.parse_args()
    dev = torch.device('cuda:0')
    st = synth.DEFAULT_SETTINGS
    cap = Captioner(synth.make_idx2word(V), synth.SENTIMENT_CATEGORIES, st)
    cap.load_state_dict({k: torch.from_numpy(v) for k, v in synth.make_weights(V, st, seed=0).items()})
    cap.to(dev).eval()
    d = synth.make_inputs(BASE, V, st, regions=R, seq_len=T, seed=5)
    base = [torch.from_numpy(d[k]).to(dev) for k in KEYS]
    lines = []
    for cfg in a.configs.split(','):
        I, n = (int(x) for x in cfg.split('x'))
        idx = torch.arange(I, device=dev) % BASE
        ins = [x[idx].contiguous() for x in base]
        forms = {'grouped': lambda: cap.forward_rl(*ins, T, 0, captions_per_image=n),
                 'repeated': lambda: cap.forward_rl(*big, T, 0)}
        times = {k: [] for k in forms}
        expand = []
        res = {'images': I, 'captions_per_image': n, 'rows': I * n, 'V': V, 'T': T, 'regions': R, 'reps': a.reps}
        with torch.no_grad():
            big = rep(ins, n)
            for r in range(a.reps + 1):                          # one warm-up round
                for name, fn in forms.items():
                    torch.manual_seed(r)
                    ms, _ = timed(fn)
                    if r >= 1:
                        times[name].append(ms)
            for name, fn in forms.items():
                pro, scan = kernel_times(fn, a.step)
                res[name] = {'prologue_ms': pro, 'scan_us_per_step': scan}
            del big
            for r in range(3):
                ms, big = timed(lambda: rep(ins, n))
                expand.append(ms)
                del big
            torch.cuda.empty_cache()
            for name in forms:                                   # peak memory of one call, the images' inputs resident
                torch.cuda.synchronize()
                torch.cuda.reset_peak_memory_stats()
                before = torch.cuda.memory_allocated()
                if name == 'grouped':
                    cap.forward_rl(*ins, T, 0, captions_per_image=n)
                else:
                    cap.forward_rl(*rep(ins, n), T, 0)
                torch.cuda.synchronize()
                res[name]['max_memory_allocated_bytes'] = torch.cuda.max_memory_allocated()
                res[name]['resident_before_call_bytes'] = before
                torch.cuda.empty_cache()
        for name in forms:
            ts = times[name]
            res[name].update(ms_per_rollout_median=statistics.median(ts), ms_per_rollout_min=min(ts),
                             ms_per_rollout_max=max(ts))
        res['repeat_interleave_ms'] = statistics.median(expand)
        res['speedup_median'] = res['repeated']['ms_per_rollout_median'] / res['grouped']['ms_per_rollout_median']
        res['grouped_faster_beyond_spread'] = res['grouped']['ms_per_rollout_max'] < res['repeated']['ms_per_rollout_min']
        lines.append(json.dumps(res))
        print(lines[-1], flush=True)
        del ins
        torch.cuda.empty_cache()
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        open(a.out, 'w').write('\n'.join(lines) + '\n')


if __name__ == '__main__':
    main()
