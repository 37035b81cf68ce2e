"""fp64 numpy restatement of the frozen image-sentiment detector's forward and `sample` (helper_nets.SentimentDetector;
reference models/sentiment_detector.py:30-60), the cases of tests/test_gpu_senti_det.py and the comparison those tests
apply - shared with tests/test_senti_det_ref_host.py, which checks the restatement, the cases' margin conditions and that
the comparison notices a wrong reference, all on the CPU.

    x = conv_{n-1}(... conv_0(features) ...)   3x3, padding 1, cross-correlation, no non-linearity in between
    r = relu(x);  m[b,j,p] = bs[j] + r[b,p,:] . Ws[j,:];  z = FC(... FC(mean_p m) ...);  prob = softmax(z)
    maps[b,p] = sum_j prob_j m[b,j,p];  scores = max prob;  labels = arg-max, neu_idx where scores < float32(threshold)
"""
import numpy as np

INJECTIONS = ('tap_transposed', 'border_not_zeroed', 'mean_wrong_axis', 'relu_between')

# name -> C, B, h, w, n_convs, n_fcs, k, threshold.  Every conv's Cin must be a multiple of 32, so three convs need
# C = 128 (128 -> 64 -> 32 -> 16); every other case keeps the issue's C = 64 unless its line says otherwise.
CASES = {
    'baseline': dict(C=64, B=37, h=6, w=6),             # M = 1332: 21 row tiles, image boundaries inside tiles
    'grid_2x3': dict(C=64, B=4, h=2, w=3),
    'grid_1x1': dict(C=64, B=9, h=1, w=1),              # eight taps out of grid
    'grid_1x5': dict(C=64, B=9, h=1, w=5),
    'grid_5x1': dict(C=64, B=9, h=5, w=1),
    'c256_3x3': dict(C=256, B=6, h=3, w=3),             # more than two k-chunks per tap
    'c128_14x14': dict(C=128, B=5, h=14, w=14),         # 196 rows per image
    'one_image': dict(C=64, B=1, h=6, w=6),
    'product': dict(C=2048, B=3, h=6, w=6),             # product widths
    'convs_1': dict(C=64, B=37, h=6, w=6, n_convs=1),
    'convs_3': dict(C=128, B=37, h=6, w=6, n_convs=3),
    'fcs_0': dict(C=64, B=37, h=6, w=6, n_fcs=0),
    'fcs_1': dict(C=64, B=37, h=6, w=6, n_fcs=1),
    'k_2': dict(C=64, B=37, h=6, w=6, k=2),
    'k_8': dict(C=64, B=37, h=6, w=6, k=8),
    'thr_0': dict(C=64, B=37, h=6, w=6, threshold=0.0),
    'thr_2': dict(C=64, B=37, h=6, w=6, threshold=2.0),
}
DEFAULTS = dict(n_convs=2, n_fcs=2, k=3, threshold=0.7)
# feature seed per case: default_rng(7) unless the case misses a margin condition with it (the host test says which)
# (with 7: convs_1 threshold margin 0.0038, fcs_0 top-2 margin 0.0025, fcs_1 threshold margin 0.0035)
SEEDS = {'convs_1': 8, 'fcs_0': 13, 'fcs_1': 12}
WEIGHT_SEED, WEIGHT_GAIN = 51, 3.0
MARGIN = 5e-3                   # smallest fp64 top-2 probability margin and |score - threshold| of a case


def case(name):
    return dict(DEFAULTS, **CASES[name])


def categories(k):
    """k category names with 'neutral' among them (index 2, or 1 when k = 2)."""
    names = ['positive', 'negative', 'neutral'] + ['c%d' % i for i in range(3, 8)]
    return ['positive', 'neutral'] if k == 2 else names[:k]


def features(c, seed=7):
    """relu(N(0,1) + 1.5 profile_b), one N(0,1) channel profile per image: images differ in which channels are lit, so
    the labels differ between images (i.i.d. features give one label for all)."""
    rng = np.random.default_rng(seed)
    profile = rng.standard_normal((c['B'], 1, 1, c['C']))
    noise = rng.standard_normal((c['B'], c['h'], c['w'], c['C']))
    return np.maximum(noise + 1.5 * profile, 0.0).astype(np.float32)


def split_weights(w):
    """state_dict arrays -> ([(W [N,Cin,3,3], b)], (Ws [k,CL], bs), [(W [k,k], b)]), fp64."""
    convs, fcs = [], []
    i = 0
    while 'convs.conv_%d.weight' % i in w:
        convs.append((np.asarray(w['convs.conv_%d.weight' % i], np.float64), np.asarray(w['convs.conv_%d.bias' % i], np.float64)))
        i += 1
    i = 0
    while 'output.%d.weight' % i in w:
        fcs.append((np.asarray(w['output.%d.weight' % i], np.float64), np.asarray(w['output.%d.bias' % i], np.float64)))
        i += 1
    Ws = np.asarray(w['senti_conv.weight'], np.float64)
    return convs, (Ws.reshape(Ws.shape[0], -1), np.asarray(w['senti_conv.bias'], np.float64)), fcs


def conv3x3(x, W, b, inject=None):
    """x [B,h,w,Cin] -> [B,h,w,N]: out[b,y,x] = b + sum_{ky,kx} in[b, y+ky-1, x+kx-1, :] W[:, :, ky, kx]^T, zeros outside."""
    B, h, w, _ = x.shape
    pad = np.pad(x, ((0, 0), (1, 1), (1, 1), (0, 0)), mode='edge' if inject == 'border_not_zeroed' else 'constant')
    out = np.zeros((B, h, w, W.shape[0])) + b
    for ky in range(3):
        for kx in range(3):
            oy, ox = (kx, ky) if inject == 'tap_transposed' else (ky, kx)
            out += pad[:, oy:oy + h, ox:ox + w, :] @ W[:, :, ky, kx].T
    return out


def forward(w, feats, threshold, neu_idx, inject=None):
    """-> dict(conv_out [B*h*w, CL], logits [B,k], maps [B,h,w], scores [B], labels [B] int64, probs [B,k]), fp64."""
    convs, (Ws, bs), fcs = split_weights(w)
    x = np.asarray(feats, np.float64)
    B, h, wd, _ = x.shape
    for i, (W, b) in enumerate(convs):
        x = conv3x3(x, W, b, inject)
        if inject == 'relu_between' and i + 1 < len(convs):
            x = np.maximum(x, 0.0)
    r = np.maximum(x, 0.0)
    m = np.einsum('bhwc,jc->bjhw', r, Ws) + bs[None, :, None, None]
    z = m.mean(axis=(2, 3))
    if inject == 'mean_wrong_axis':                     # the image's [k][h w] maps read as [h w][k]
        z = m.reshape(B, h * wd, -1).mean(axis=1)
    for W, b in fcs:
        z = z @ W.T + b
    e = np.exp(z - z.max(axis=-1, keepdims=True))
    prob = e / e.sum(axis=-1, keepdims=True)
    maps = np.einsum('bj,bjhw->bhw', prob, m)
    scores = prob.max(axis=-1)
    labels = prob.argmax(axis=-1).astype(np.int64)
    labels = np.where(scores < np.float64(np.float32(threshold)), neu_idx, labels)
    return dict(conv_out=r.reshape(B * h * wd, -1), logits=z, maps=maps, scores=scores, labels=labels, probs=prob)


def top2_margin(prob):
    s = np.sort(prob, axis=-1)
    return float((s[:, -1] - s[:, -2]).min()) if prob.shape[1] > 1 else 1.0


def threshold_margin(scores, threshold):
    return float(np.abs(scores - np.float64(np.float32(threshold))).min())


VALUE_KEYS = ('conv_out', 'logits', 'maps', 'scores')


def bound(e, ref):
    """4 max(e, 2^-23 max|fp64|): e = the stock fp32 module's CPU error against the same fp64 reference."""
    return 4.0 * max(float(e), 2.0 ** -23 * float(np.abs(ref).max()))


def compare(got, ref, e, name='', keys=VALUE_KEYS, labels=True):
    """The GPU tests' comparison: every value output within bound(e, ref) of the fp64 reference, labels equal.  Prints
    each figure before it asserts."""
    for k in keys:
        err = float(np.abs(np.asarray(got[k], np.float64).reshape(ref[k].shape) - ref[k]).max())
        b = bound(e[k], ref[k])
        print('%s %s: err %.3g  torch-fp32-cpu err %.3g  bound %.3g  max|ref| %.3g' % (name, k, err, e[k], b, np.abs(ref[k]).max()))
        assert err <= b, (name, k, err, b)          # (a NaN fails it)
    if labels:
        assert np.array_equal(np.asarray(got['labels']), ref['labels']), (name, 'labels')


# ---- the exact case: lattice operands -------------------------------------------------------------------------------
def lattice_operands(c, seed=3):
    """Integer features in {0 .. 3}, conv weights in {0, +-1/2, +-1}, biases multiples of 1/2 in [-2, 2]; weight density
    chosen per layer so that an output's sum of magnitudes is about 256.  -> (state_dict arrays fp32, feats fp32)."""
    rng = np.random.default_rng([seed, c['C'], c['h'], c['w'], c['B']])
    C, k = c['C'], c['k']
    feats = (rng.integers(1, 4, (c['B'], c['h'], c['w'], C)) * (rng.random((c['B'], c['h'], c['w'], C)) < 0.5)).astype(np.float32)
    w = {}
    for i in range(c['n_convs']):
        Cin = C >> i
        d = min(1.0, 256.0 / (9 * Cin * 0.75))
        mag = rng.integers(1, 3, (Cin // 2, Cin, 3, 3)) * 0.5
        sign = rng.integers(0, 2, mag.shape) * 2 - 1
        w['convs.conv_%d.weight' % i] = (mag * sign * (rng.random(mag.shape) < d)).astype(np.float32)
        w['convs.conv_%d.bias' % i] = (rng.integers(-4, 5, Cin // 2) * 0.5).astype(np.float32)
    CL = C >> c['n_convs']
    w['senti_conv.weight'] = (rng.integers(-2, 3, (k, CL, 1, 1)) * 2.0 ** -8).astype(np.float32)
    w['senti_conv.bias'] = np.zeros(k, np.float32)
    for i in range(c['n_fcs']):
        w['output.%d.weight' % i] = np.eye(k, dtype=np.float32)
        w['output.%d.bias' % i] = np.zeros(k, np.float32)
    return w, feats


def lattice_expect(w, feats):
    """The post-ReLU conv output of lattice operands in fp64, with the exactness guarantee asserted from the operands
    (as _lattice.expect does): layer l's inputs are multiples of q_l = 2^-l bounded by A_l (the running sum of
    magnitudes), its weights and bias multiples of 1/2, so every term and every partial sum of an output, in any order
    over taps, chunks, MFMA terms and slabs, is a multiple of q_{l+1} = q_l / 2 bounded by A_{l+1} = conv(A_l, |W|) + |b|:
      * A_l < 2^11 q_l makes every input an f16 number: its hi plane is the value, its lo plane zero (both planes of a
        weight likewise), so the three-term product IS the product;
      * A_{l+1} < 2^24 q_{l+1} makes every partial sum an fp32 number: nothing ever rounds.
    """
    convs, _, _ = split_weights(w)
    x = np.asarray(feats, np.float64)
    A = np.abs(x)
    q = 1.0
    assert np.array_equal(x, np.round(x))
    for W, b in convs:
        assert np.array_equal(W * 2, np.round(W * 2)) and np.array_equal(b * 2, np.round(b * 2))
        assert np.abs(W).max() <= 1.0
        assert A.max() < 2.0 ** 11 * q, 'an input of magnitude %g is not an f16 number on the lattice of %g' % (A.max(), q)
        x = conv3x3(x, W, b)
        A = conv3x3(A, np.abs(W), np.abs(b))
        q *= 0.5
        assert A.max() < 2.0 ** 24 * q, 'a partial sum may round: sum of magnitudes %g' % A.max()
        assert np.array_equal(x / q, np.round(x / q))
    r = np.maximum(x, 0.0)
    r32 = r.astype(np.float32)
    assert np.array_equal(r32.astype(np.float64), r)
    return r32.reshape(-1, r.shape[-1])


# ---- cases: module, inputs, reference, the stock module's error - once per case, shared, read-only ---------------------
_REF = {}


def module(c, weights=None, gain=WEIGHT_GAIN):
    """(SentimentDetector in eval mode on the CPU, its state_dict arrays): synth.make_module_weights(shapes, 51, gain)."""
    import torch
    from insenticap_model_amd import synth
    from insenticap_model_amd.helper_nets import SentimentDetector
    st = dict(synth.TINY_SETTINGS, **synth.HELPER_SETTINGS)
    st.update(fc_feat_dim=c['C'], sentiment_convs_num=c['n_convs'], sentiment_fcs_num=c['n_fcs'])
    m = SentimentDetector(categories(c['k']), st)
    if weights is None:
        shapes = {n: tuple(v.shape) for n, v in m.state_dict().items()}
        weights = synth.make_module_weights(shapes, WEIGHT_SEED, gain=gain)
    m.load_state_dict({n: torch.from_numpy(np.ascontiguousarray(v)) for n, v in weights.items()})
    return m.eval(), weights


def stock_outputs(m, feats, threshold):
    """The stock torch module's outputs (in the dtype of its parameters) as fp64 arrays, keyed like forward()."""
    import torch
    x = torch.from_numpy(feats).to(next(m.parameters()).dtype)
    with torch.no_grad():
        logits, maps = m(x)
        labels, _, _, scores = m.sample(x, threshold)
        r = m.convs(x.permute(0, 3, 1, 2)).permute(0, 2, 3, 1)
    return dict(conv_out=r.reshape(-1, r.shape[-1]).double().numpy(), logits=logits.double().numpy(),
                maps=maps.double().numpy(), scores=scores.double().numpy(), labels=labels.numpy())


def reference(name):
    if name in _REF:
        return _REF[name]
    c = case(name)
    m, w = module(c)
    feats = features(c, SEEDS.get(name, 7))
    ref = forward(w, feats, c['threshold'], m.neu_idx)
    stock = stock_outputs(m, feats, c['threshold'])
    e = {k: float(np.abs(stock[k] - ref[k]).max()) for k in VALUE_KEYS}
    for v in list(ref.values()) + [feats]:
        v.setflags(write=False)
    _REF[name] = dict(c=c, m=m, w=w, feats=feats, ref=ref, e=e, stock=stock, neu_idx=m.neu_idx)
    return _REF[name]
