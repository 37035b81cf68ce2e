#!/usr/bin/env python3
"""Time of the differentiable filtered roll-out (self-critical RL under temperature / top-k / top-p), in ONE process,
forms alternating, HIP events, medians with ranges over --reps after two warm-up rounds.

  kernel     d logits over [B*T, V] = [512*20, 10000] rows of raw logits, every coefficient non-zero:
               raw        isc_logsoftmax_bwd_raw, one model pair (the kernel the unfiltered iteration runs);
               filtered   isc_logsoftmax_bwd_raw_filtered, the filtered term alone, every id kept (K* = all ones);
               both       isc_logsoftmax_bwd_raw_filtered, one model pair plus the filtered term.
             All three read 4 B and write 4 B per element: GB/s = 8 B * B*T*V / time.
  iteration  Captioner.forward_rl(sample_max=0) with gradients + REINFORCE loss + backward, training mode, default
             dimensions, V = 10000, T = 20, 36 regions, at I x n = 512 x 1 and 512 x 5 (captions_per_image):
               plain      default controls, loss on the model's log-probs;
               filtered   temperature 0.8, top_p 0.9, loss on the sampling log-probs.

    python tools/filtered_rl_probe.py [--reps 7] [--configs 512x1,512x5] [--skip-kernel] [--out FILE]
"""
import argparse
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch

from insenticap_model_amd import Captioner, ops, synth

V, T = 10000, 20


def timed(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    out = fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1), out


def summary(ts):
    return {'ms_median': statistics.median(ts), 'ms_min': min(ts), 'ms_max': max(ts)}


def alternate(forms, reps):
    times = {k: [] for k in forms}
    for r in range(reps + 2):                     # two warm-up rounds
        for k, fn in forms.items():
            ms, _ = timed(fn)
            if r >= 2:
                times[k].append(ms)
    return {k: summary(ts) for k, ts in times.items()}


def kernel_part(dev, reps, B=512):
    M, tau = B * T, 0.8
    g = torch.Generator(device=dev).manual_seed(0)
    raw = torch.randn(B, T, V, device=dev, generator=g) * 3.0
    nt = (V + 127) // 128
    xp = torch.nn.functional.pad(raw.view(M, V), (0, nt * 128 - V), value=float('-inf')).view(M, nt, 128)
    pm = xp.amax(2)
    ps = torch.exp(xp - pm.unsqueeze(2)).sum(2)
    del xp
    # statistics rows are time-major (t * B + b)
    pm, ps = (x.view(B, T, nt).transpose(0, 1).contiguous() for x in (pm, ps))
    ids = torch.randint(0, V, (B, T), device=dev, generator=g)
    coef = torch.randn(B, T, device=dev, generator=g)
    gmax = raw.amax(2)
    flt = dict(tok=ids, coef=coef.clone(), inv_tau=1.0 / tau, kstar=torch.full((B, T), -1, dtype=torch.int64, device=dev),
               gmax=gmax.contiguous(), logz=torch.logsumexp((raw - gmax.unsqueeze(2)) / tau, dim=2).contiguous(), ban=None)
    out = torch.empty(M, (V + 31) // 32 * 32, device=dev)
    args = (raw, T * V, V, B, T, V, pm, ps, B)
    forms = {'raw': lambda: ops.logsoftmax_bwd_raw(*args, [(ids, coef)], out),
             'filtered': lambda: ops.logsoftmax_bwd_raw_filtered(*args, [], flt, out),
             'both': lambda: ops.logsoftmax_bwd_raw_filtered(*args, [(ids, coef)], flt, out)}
    res = {'part': 'kernel', 'rows': M, 'V': V, 'reps': reps, **alternate(forms, reps)}
    for k in forms:
        res[k]['GBps_median'] = 8.0 * M * V / (res[k]['ms_median'] * 1e-3) / 1e9
    res['filtered_over_raw_median'] = res['filtered']['ms_median'] / res['raw']['ms_median']
    res['both_over_raw_median'] = res['both']['ms_median'] / res['raw']['ms_median']
    res['filtered_slower_beyond_spread'] = res['filtered']['ms_min'] > res['raw']['ms_max']
    res['both_slower_beyond_spread'] = res['both']['ms_min'] > res['raw']['ms_max']
    return res


def iteration_part(dev, reps, I, n):
    st = synth.DEFAULT_SETTINGS
    cap = Captioner(synth.make_idx2word(V), synth.SENTIMENT_CATEGORIES, st)
    cap.load_state_dict({k: torch.from_numpy(v) for k, v in synth.make_weights(V, st, seed=0).items()})
    cap.to(dev).train()
    b = synth.make_inputs(I, V, st, regions=36, seq_len=T, seed=3)
    ins = [torch.from_numpy(b[k]).to(dev) for k in ('fc_feats', 'att_feats', 'cpt_words', 'senti_words', 'senti_labels')]
    reward = torch.randn(I * n, T, device=dev)
    group = dict(captions_per_image=n) if n > 1 else {}

    def iteration(filtered):
        cap.zero_grad(set_to_none=True)
        if filtered:
            seq, lp, mk, slp = cap.forward_rl(*ins, T, 0, temperature=0.8, top_p=0.9, return_sampling_logprobs=True, **group)
            lp = slp
        else:
            seq, lp, mk = cap.forward_rl(*ins, T, 0, **group)
        (-(lp * mk * reward).sum() / mk.sum()).backward()
    res = {'part': 'iteration', 'images': I, 'samples_per_image': n, 'rows': I * n, 'V': V, 'T': T, 'reps': reps,
           **alternate({'plain': lambda: iteration(False), 'filtered': lambda: iteration(True)}, reps)}
    res['filtered_over_plain_median'] = res['filtered']['ms_median'] / res['plain']['ms_median']
    res['filtered_slower_beyond_spread'] = res['filtered']['ms_min'] > res['plain']['ms_max']
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--reps', type=int, default=7)
    ap.add_argument('--configs', default='512x1,512x5')
    ap.add_argument('--skip-kernel', action='store_true')
    ap.add_argument('--out', default=None)
    a = ap.parse_args()
    dev = torch.device('cuda:0')
    lines = []
    if not a.skip_kernel:
        lines.append(json.dumps(kernel_part(dev, a.reps)))
        print(lines[-1], flush=True)
        torch.cuda.empty_cache()
    for cfg in a.configs.split(','):
        I, n = (int(x) for x in cfg.split('x'))
        lines.append(json.dumps(iteration_part(dev, a.reps, I, n)))
        print(lines[-1], flush=True)
        torch.cuda.empty_cache()
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        open(a.out, 'w').write('\n'.join(lines) + '\n')


if __name__ == '__main__':
    main()
