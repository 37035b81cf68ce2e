#!/usr/bin/env python3
"""The sentence-sentiment classifier's training iteration on the library's kernels beside the stock torch iteration, in ONE
process, the forms alternating, HIP events and host clocks, every step under a time limit (the process ends when one runs
over).  Product widths W = H = 512, V = 10 000, L = 17 (opts.py's max_seq_len), dropout 0.5, weights
synth.make_module_weights, lengths drawn in [1, L] with the first row full, sorted longest first as the collate hands them
over; B = 80 (the reference's batch) and B = 512.

  torch:   model.train(); criterion(model(caps, lengths)[0], labels); backward; clip_gradient; torch.optim.Adam.step -
           train_sent_senti_cls_rnn.py:118-125 on stock torch ops (vendor-library nn.LSTM, host lengths);
  native:  train.sent_cls_train_step with model.get_optim_and_crit(lr, fused=True) (FusedClampAdam), the same host lengths.

Per form: host enqueue time (a host clock around the iteration, no wait), device time (HIP events) and the launches of one
iteration (kernels and copies a torch.profiler trace of a single iteration records; None where the profiler gives none).
Three warm-up rounds, then --reps rounds.  The numbers are reported, nothing is gated.

    python tools/sent_cls_train_probe.py [--reps 15] [--out FILE]
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
from insenticap_model_amd import synth
from insenticap_model_amd.helper_nets import SentenceSentimentClassifier
from insenticap_model_amd.optim import clip_gradient
from insenticap_model_amd.train import sent_cls_train_step

W = H = 512
V, L, K, LR, CLIP = 10000, 17, 3, 4e-4, 0.1


def model(seed=52):
    st = dict(synth.DEFAULT_SETTINGS, **synth.HELPER_SETTINGS)
    st.update(word_emb_dim=W, rnn_hid_dim=H, dropout_p=0.5)
    m = SentenceSentimentClassifier(synth.make_idx2word(V), synth.SENTIMENT_CATEGORIES[:K], st)
    w = synth.make_module_weights({n: tuple(v.shape) for n, v in m.state_dict().items()}, seed)
    m.load_state_dict({n: torch.from_numpy(v) for n, v in w.items()})
    return m.to(DEV).train()


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


def launches(fn):
    """Device activities (kernels, copies, fills) one call of fn() issues, from a profiler trace; None when it has none."""
    try:
        from torch.profiler import ProfilerActivity, profile
        torch.cuda.synchronize()
        with profile(activities=[ProfilerActivity.CUDA]) as prof:
            fn()
            torch.cuda.synchronize()
        n = sum(1 for e in prof.events() if str(getattr(e, 'device_type', '')).endswith('CUDA'))
        return n or None
    except Exception as exc:                 # (a build without the tracer: the times are still worth having)
        print('launch count unavailable: %r' % (exc,), flush=True)
        return None


def probe(a, B, lines):
    with step_limit(a.step_limit, 'training iteration, B = %d' % B):
        rng = np.random.default_rng(6)
        lens = np.sort(rng.integers(1, L + 1, B))[::-1].copy()
        lens[0] = L
        tokens = rng.integers(4, V, (B, L)).astype(np.int64)
        tokens[np.arange(L)[None, :] >= lens[:, None]] = 0                   # <PAD> behind every length, as the collate pads
        labels = rng.integers(0, K, B).astype(np.int64)
        caps, lab, lengths = torch.from_numpy(tokens).to(DEV), torch.from_numpy(labels).to(DEV), [int(x) for x in lens]
        nat, ref = model(), model()
        o_nat, _ = nat.get_optim_and_crit(LR, fused=True)
        o_ref, crit = ref.get_optim_and_crit(LR)

        def native():
            return sent_cls_train_step(nat, o_nat, caps, lengths, lab, CLIP)

        def stock():
            loss = crit(ref(caps, lengths)[0], lab)
            o_ref.zero_grad()
            loss.backward()
            clip_gradient(o_ref, CLIP)
            o_ref.step()
            return loss.detach()
        forms = {'torch': stock, 'native': native}
        first = {k: float(fn()) for k, fn in forms.items()}                  # (different dropout draws: not comparable bits)
        t = {k: ([], []) for k in forms}
        for r in range(a.reps + 3):                                          # three warm-up rounds, the forms alternating
            for k, fn in forms.items():
                host, dev = timed(fn)
                if r >= 3:
                    t[k][0].append(host)
                    t[k][1].append(dev)
        res = {'probe': 'sent_cls_training_iteration', 'B': B, 'L': L, 'W': W, 'H': H, 'V': V, 'rows': B * L, 'reps': a.reps,
               'first_loss': first}
        for k in forms:
            res[k + '_host_enqueue'] = stats(t[k][0])
            res[k + '_device'] = stats(t[k][1])
            res[k + '_launches'] = launches(forms[k])
        res['native_device_faster_beyond_spread'] = max(t['native'][1]) < min(t['torch'][1])
        res['native_device_slower_beyond_spread'] = min(t['native'][1]) > max(t['torch'][1])
        res['native_host_faster_beyond_spread'] = max(t['native'][0]) < min(t['torch'][0])
        lines.append(json.dumps(res))
        print(lines[-1], flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--reps', type=int, default=15)
    ap.add_argument('--step-limit', type=int, default=120, help='seconds per step')
    ap.add_argument('--out', default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit('sent_cls_train_probe needs the GPU: there is nothing to time without one')
    lines = []
    for B in (80, 512):
        probe(a, B, lines)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        open(a.out, 'w').write('\n'.join(lines) + '\n')


if __name__ == '__main__':
    main()
