#!/usr/bin/env python3
"""Time of the roll-out's prologue with fp32 and with float16 region features of the same values.

Inputs resident, eval mode, V = 10000; per shape HIP events around
  * the prologue's att_embed launch [B R x 2048 x 512] (ops.TIMER's prologue arm, as bench.py times it),
  * the whole prologue (Captioner._prologue inside the roll-out's weights scope),
  * isc_f16_to_f32 of the [B R, 2048] batch alone - what "convert, then the fp32 path" adds in front of the fp32 launch,
with fp32 and float16 features alternating inside one process, two warm-up rounds, `--reps` timed rounds; medians and
the spread (min .. max) are printed as one JSON line per shape.  `--gemm` adds the three tile geometries of the large
split-f16 kernels at the GEMM level (ops.linear_fwd, K = 2048, N = 512: 64-row tile at M = 4096, 128-row at M = 8192,
256-row at M = 16384): native float16 rows against convert + fp32 rows.  On a tree without float16 features only the
fp32 side is measured (the comparison point: the parent commit on the same machine).

    python tools/f16_features_probe.py [--shapes 4096x36,16384x36,4096x196] [--reps 9] [--gemm] [--out FILE]

Rule for shipping: a geometry keeps the native form only if it is not slower there than
convert + fp32 by more than the run-to-run spread this probe reports."""
import argparse
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch

from insenticap_model_amd import Captioner, ops, synth

V, T = 10000, 20
HAS_F16 = hasattr(ops, 'f16_to_f32')


def timed(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    out = fn()
    e1.record()
    return e0, e1, out


def stats(xs):
    return {'median_ms': round(statistics.median(xs), 4), 'min_ms': round(min(xs), 4), 'max_ms': round(max(xs), 4)}


def prologue_times(cap, ins, att_name):
    """(att_embed ms, whole prologue ms) of one prologue with the timer armed."""
    p = cap._p()
    ops.TIMER.records.clear()
    ops.TIMER.armed, ops.TIMER.phase = True, 'prologue'
    try:
        with torch.no_grad(), ops.h3_weights_scope(cap._dev, key=cap._weights_key()):
            e0, e1, _ = timed(lambda: cap._prologue(p, 'rl', *ins, want_table='cached', words_table=True))
    finally:
        ops.TIMER.armed, ops.TIMER.phase = False, 'step'
    torch.cuda.synchronize()
    att = [r[1].elapsed_time(r[2]) for r in ops.TIMER.records if r[0] == att_name]
    ops.TIMER.records.clear()
    assert len(att) == 1, att_name
    return att[0], e0.elapsed_time(e1)


def probe_shape(cap, B, R, reps):
    dev = cap._dev
    st = synth.DEFAULT_SETTINGS
    d = synth.make_inputs(B, V, st, regions=R, seq_len=T, seed=5)
    fc, att = torch.from_numpy(d['fc_feats']).to(dev).half(), torch.from_numpy(d['att_feats']).to(dev).half()
    rest = [torch.from_numpy(d[k]).to(dev) for k in ('cpt_words', 'senti_words', 'senti_labels')]
    sides = {'fp32': [fc.float(), att.float()] + rest}
    if HAS_F16:
        sides['f16'] = [fc, att] + rest
    name = 'linear[%dx%dx%d]' % (B * R, st['feat_emb_dim'], att.shape[-1])
    t = {k: {'att_embed': [], 'prologue': []} for k in sides}
    conv = []
    lib = ops._lib.load()
    native = None
    for rep in range(reps + 2):
        for k, ins in sides.items():
            before = lib.isc_h3_f16a_launches() if HAS_F16 else 0
            a, w = prologue_times(cap, ins, name)
            if k == 'f16':
                native = lib.isc_h3_f16a_launches() - before
            if rep >= 2:
                t[k]['att_embed'].append(a)
                t[k]['prologue'].append(w)
        if HAS_F16:
            x = att.reshape(B * R, -1)
            out = torch.empty(x.shape, dtype=torch.float32, device=dev)
            e0, e1, _ = timed(lambda: ops.f16_to_f32(x, out))
            torch.cuda.synchronize()
            if rep >= 2:
                conv.append(e0.elapsed_time(e1))
            del out
    line = {'B': B, 'R': R, 'reps': reps, 'f16_native_launches_per_prologue': native}
    for k in t:
        line[k] = {m: stats(v) for m, v in t[k].items()}
    if conv:
        line['convert_att'] = stats(conv)
        line['convert_then_fp32_att_embed_median_ms'] = round(
            line['convert_att']['median_ms'] + line['fp32']['att_embed']['median_ms'], 4)
    return line


def probe_gemm(reps):
    dev = torch.device('cuda:0')
    K, N = 2048, 512
    g = torch.Generator().manual_seed(1)
    w, b = (torch.randn(N, K, generator=g) * K ** -0.5).to(dev), torch.randn(N, generator=g).to(dev)
    lib = ops._lib.load()
    lines = []
    for tile, M in (('64-row', 4096), ('128-row', 8192), ('256-row', 16384)):
        x16 = torch.randn(M, K, generator=g).half().to(dev)
        x32 = x16.float()
        out, tmp = torch.empty(M, N, device=dev), torch.empty(M, K, device=dev)
        forms = {'fp32': lambda: ops.linear_fwd([ops.linear_problem([(x32, w)], out, b, relu=True)])}
        if HAS_F16:
            forms['f16_native'] = lambda: ops.linear_fwd([ops.linear_problem([(x16, w)], out, b, relu=True)])
            forms['convert_then_fp32'] = lambda: (ops.f16_to_f32(x16, tmp),
                                                  ops.linear_fwd([ops.linear_problem([(tmp, w)], out, b, relu=True)]))
        t = {k: [] for k in forms}
        before = (lib.isc_h3_f16a_launches(), lib.isc_h3x_launches()) if HAS_F16 else None
        for rep in range(reps + 2):
            for k, fn in forms.items():
                e0, e1, _ = timed(fn)
                torch.cuda.synchronize()
                if rep >= 2:
                    t[k].append(e0.elapsed_time(e1))
        line = {'gemm': '%dx%dx%d' % (M, N, K), 'tile': tile, 'reps': reps}
        if HAS_F16:
            line['f16_native_launches'] = lib.isc_h3_f16a_launches() - before[0]
            line['h3x_launches'] = lib.isc_h3x_launches() - before[1]
        line.update({k: stats(v) for k, v in t.items()})
        lines.append(line)
    return lines


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--shapes', default='4096x36,16384x36,4096x196')
    ap.add_argument('--reps', type=int, default=9)
    ap.add_argument('--gemm', action='store_true')
    ap.add_argument('--out', default=None)
    a = ap.parse_args()
    dev = torch.device('cuda:0')
    st = synth.DEFAULT_SETTINGS
    cap = Captioner(synth.make_idx2word(V), synth.SENTIMENT_CATEGORIES, st)
    cap.load_state_dict({k: torch.from_numpy(v) for k, v in synth.make_weights(V, st, seed=0).items()})
    cap.to(dev).eval()
    lines = probe_gemm(a.reps) if a.gemm else []
    for shape in [s for s in a.shapes.split(',') if s]:
        B, R = (int(x) for x in shape.split('x'))
        lines.append(probe_shape(cap, B, R, a.reps))
        torch.cuda.empty_cache()
    for line in lines:
        print(json.dumps(line))
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, 'w') as f:
            for line in lines:
                f.write(json.dumps(line) + '\n')


if __name__ == '__main__':
    main()
