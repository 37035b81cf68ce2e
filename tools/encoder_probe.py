"""Image encoder: the stock torch ops against the native path (isc_encoder_fwd), in one process, alternating.

    python tools/encoder_probe.py [--reps 20] [--layers 3,4,23,3] [--width 64]

Per shape: HIP-event medians with their ranges for both paths (alternating, so clock and thermal drift hit both), the
native path's launch count and its TFLOP/s (2 * MACs of every convolution, the stem included), and the largest
difference of the two outputs.  Random weights: the time does not depend on them."""
import argparse
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from insenticap_model_amd import ops  # noqa: E402
from insenticap_model_amd.encoder import Encoder  # noqa: E402


def flops(layers, width, B, H, W):
    h, w = (H - 1) // 2 + 1, (W - 1) // 2 + 1
    total = B * h * w * width * 147
    h, w = (h - 2) // 2 + 1, (w - 2) // 2 + 1
    inpl = width
    for l, n in enumerate(layers):
        p = width << l
        for i in range(n):
            if l > 0 and i == 0:
                h, w = (h - 1) // 2 + 1, (w - 1) // 2 + 1
            m = B * h * w
            total += m * (inpl * p + 9 * p * p + p * 4 * p + (inpl * 4 * p if i == 0 else 0))
            inpl = 4 * p
    return 2.0 * total


def timed(fn, reps):
    out = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        out.append(a.elapsed_time(b))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--reps', type=int, default=20)
    ap.add_argument('--layers', default='3,4,23,3')
    ap.add_argument('--width', type=int, default=64)
    args = ap.parse_args()
    layers = tuple(int(n) for n in args.layers.split(','))
    dev = torch.device('cuda:0')
    torch.manual_seed(0)
    enc = Encoder(None, layers, args.width).to(dev).eval()
    print('%-14s %26s %26s %8s %9s %9s' % ('shape', 'stock ms (min..max)', 'native ms (min..max)', 'launches', 'TFLOP/s',
                                           'max diff'))
    for B, H, W in ((1, 224, 224), (1, 448, 448), (1, 480, 640), (16, 224, 224)):
        x = torch.randn(B, 3, H, W, device=dev)
        with torch.no_grad():
            run = {False: lambda: enc.enable_native(False).forward_batch(x, 14),
                   True: lambda: enc.enable_native(True).forward_batch(x, 14)}
            for on in (False, True, False, True):                                    # warm both (pack, workspaces, tuning)
                run[on]()
            torch.cuda.synchronize()
            before = ops.encoder_launches()
            a = run[True]()
            now = ops.encoder_launches()
            n_launch = sum(now[k] - before[k] for k in ('stem', 'pool', 'direct', 'split', 'reduce', 'tail'))
            b = run[False]()
            diff = max(float((a[0] - b[0]).abs().max()), float((a[1] - b[1]).abs().max()))
            t = {False: [], True: []}
            for _ in range(args.reps):
                for on in (False, True):
                    t[on] += timed(run[on], 1)
        med = {k: statistics.median(v) for k, v in t.items()}
        print('%-14s %10.3f (%7.3f..%7.3f) %10.3f (%7.3f..%7.3f) %8d %9.2f %9.2e' % (
            '%dx%dx%d' % (B, H, W), med[False], min(t[False]), max(t[False]), med[True], min(t[True]), max(t[True]),
            n_launch, flops(layers, args.width, B, H, W) / med[True] / 1e9, diff))


if __name__ == '__main__':
    main()
