#!/usr/bin/env python3
"""Time and memory of one XE training iteration on n captions per image, in ONE process: forward, XE + domain-alignment
losses, backward, clamp + Adam (train.xe_forward_backward + train.xe_update, no seq2seq batch: it is the same work in
every form).  Features resident, training mode, default dropout, V = 10000, T = 20.  Forms, alternating:
  grouped   forward_xe(captions_per_image=n) on the I images, caption rows image-major;
  repeated  today's eager form on inputs expanded beforehand with repeat_interleave(n, 0) (the expansion's time is
            reported beside it), rows image-major, full unroll;
  ragged    the repeated form with the rows sorted by length and `ragged_unroll` on - the fastest the tree had.
Per I x n x regions it reports, for each form: ms per iteration (HIP events; median, min, max over --reps) and
torch.cuda.max_memory_allocated over one iteration; and for grouped / repeated: the prologue's ms (events around
Captioner._prologue), the scan backward's us per step (isc_attn_scan_bwd alone on tensors of the iteration's geometry)
and the two reductions after the sweep with their us and their fraction of 8 TB/s over the bytes they must move.
`grouped_faster_beyond_spread`: the slowest grouped repetition beat the fastest repetition of both other forms.

    python tools/xe_group_probe.py [--configs 128x5x36,205x5x36,128x5x196] [--reps 5] [--out FILE]
"""
import argparse
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch

from insenticap_model_amd import Captioner, ops, synth, train

V, T = 10000, 20
HBM_BYTES_PER_S = 8e12


def timed(fn, n=1):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(n):
        out = fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / n, out


def kernel_probe(I, n, R, st, grouped, dev):
    """us of isc_attn_scan_bwd (one step) and of the two reductions after the sweep, at the iteration's geometry."""
    E, A, B = st['feat_emb_dim'], st['att_hid_dim'], I * n
    imgs = I if grouped else B
    g = torch.Generator(device=dev).manual_seed(0)
    rn = lambda *s: torch.randn(*s, device=dev, generator=g)
    P, Vv, w = rn(imgs, R, A), rn(imgs, R, E), rn(A) * 0.3
    q, dout, alpha = rn(T, B, A), rn(T, B, E), torch.softmax(rn(B, T, R), dim=-1)
    de, dq, dw = rn(T, B, R) * 0.1, torch.empty(B, A, device=dev), torch.zeros(B, A, device=dev)
    dP, dV = torch.empty(imgs, R, A, device=dev), torch.empty(imgs, R, E, device=dev)
    grp = n if grouped else 1
    prob = ops.scan_bwd_problem(P, Vv, q[3], w, alpha[:, 3], dout[3], None, None, dq, dw, 1, de_out=de[3], row_div=grp)
    out = {}
    for name, fn, nbytes in (
            ('scan_bwd_step', lambda: ops.attn_scan_bwd([prob], B), 4.0 * imgs * R * (A + E)),
            ('dv_from_alpha', lambda: ops.attn_dv_from_alpha(alpha, dout, dV, group=grp),
             4.0 * (B * T * (R + E) + imgs * R * E)),
            ('dp_from_de', lambda: ops.attn_dp_from_de(P, q, w, de, dP, group=grp),
             4.0 * (2 * imgs * R * A + B * T * (R + A)))):
        timed(fn, 3)
        us = [timed(fn, 10)[0] * 1e3 for _ in range(5)]
        out[name] = {'us_median': statistics.median(us), 'us_min': min(us), 'us_max': max(us), 'bytes': nbytes,
                     'fraction_of_8TBs': nbytes / (statistics.median(us) * 1e-6) / HBM_BYTES_PER_S}
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--configs', default='128x5x36,205x5x36,128x5x196')
    ap.add_argument('--reps', type=int, default=5)
    ap.add_argument('--out', default=None)
    a = ap.parse_args()
    dev = torch.device('cuda:0')
    st = synth.DEFAULT_SETTINGS
    cap = Captioner(synth.make_idx2word(V), synth.SENTIMENT_CATEGORIES, st)
    cap.load_state_dict({k: torch.from_numpy(v) for k, v in synth.make_weights(V, st, seed=0).items()})
    cap.to(dev).train()
    optim, xe_crit, da_crit = cap.get_optim_criterion(4e-4)
    lines = []
    for cfg in a.configs.split(','):
        I, n, R = (int(x) for x in cfg.split('x'))
        img = synth.make_inputs(I, V, st, regions=R, seq_len=T, seed=5)
        row = synth.make_inputs(I * n, V, st, regions=1, seq_len=T, seed=6)
        fc, att, cpt = (torch.from_numpy(img[k]).to(dev) for k in ('fc_feats', 'att_feats', 'cpt_words'))
        caps, labels = torch.from_numpy(row['captions']).to(dev), torch.from_numpy(row['senti_labels']).to(dev)
        lengths = [int(x) for x in row['lengths']]
        order = sorted(range(I * n), key=lambda i: -lengths[i])          # (stable: the reference's collate order)
        o = torch.as_tensor(order, device=dev)
        expand = lambda: [x.repeat_interleave(n, 0) for x in (fc, att, cpt)]
        big = expand()
        srt = [x[o].contiguous() for x in big]

        def iteration(form):
            cap.ragged_unroll = form == 'ragged'
            if form == 'grouped':
                fact, lab, kw = (fc, att, caps, lengths, cpt), labels, dict(captions_per_image=n)
            elif form == 'repeated':
                fact, lab, kw = (big[0], big[1], caps, lengths, big[2]), labels, {}
            else:
                fact, lab, kw = (srt[0], srt[1], caps[o], [lengths[i] for i in order], srt[2]), labels[o], {}
            vec = train.xe_forward_backward(cap, optim, xe_crit, da_crit, fact, lab, None, 0.0, **kw)
            train.xe_update(optim, 0.1)
            return vec
        forms = ('grouped', 'repeated', 'ragged')
        res = {'images': I, 'captions_per_image': n, 'rows': I * n, 'regions': R, 'V': V, 'T': T, 'reps': a.reps}
        times = {k: [] for k in forms}
        for r in range(a.reps + 2):                                      # two warm-up rounds
            for form in forms:
                ms, _ = timed(lambda: iteration(form))
                if r >= 2:
                    times[form].append(ms)
        for form in forms:
            ts = times[form]
            res[form] = {'ms_per_iter_median': statistics.median(ts), 'ms_per_iter_min': min(ts), 'ms_per_iter_max': max(ts)}
        res['repeat_interleave_ms'] = statistics.median([timed(expand)[0] for _ in range(3)])
        torch.cuda.empty_cache()
        for form in forms:                                               # peak memory of one iteration
            torch.cuda.synchronize()
            torch.cuda.reset_peak_memory_stats()
            before = torch.cuda.memory_allocated()
            iteration(form)
            torch.cuda.synchronize()
            res[form]['max_memory_allocated_bytes'] = torch.cuda.max_memory_allocated()
            res[form]['resident_before_iter_bytes'] = before
        cap.ragged_unroll = False
        with torch.no_grad():
            p = cap._p()
            for form, args, g in (('grouped', (fc, att, cpt, None, labels), n), ('repeated', (*big, None, labels), 1)):
                pro = [timed(lambda: cap._prologue(p, 'xe', *args, None, group=g))[0] for _ in range(4)][1:]
                res[form]['prologue_ms'] = statistics.median(pro)
                res[form]['kernels'] = kernel_probe(I, n, R, st, form == 'grouped', dev)
        others = min(res['repeated']['ms_per_iter_min'], res['ragged']['ms_per_iter_min'])
        res['grouped_faster_beyond_spread'] = res['grouped']['ms_per_iter_max'] < others
        res['speedup_median_vs_ragged'] = res['ragged']['ms_per_iter_median'] / res['grouped']['ms_per_iter_median']
        res['speedup_median_vs_repeated'] = res['repeated']['ms_per_iter_median'] / res['grouped']['ms_per_iter_median']
        lines.append(json.dumps(res))
        print(lines[-1], flush=True)
        del big, srt
        torch.cuda.empty_cache()
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        open(a.out, 'w').write('\n'.join(lines) + '\n')


if __name__ == '__main__':
    main()
