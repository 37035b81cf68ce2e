"""The shape cases of the image-sentiment detector's training tests, shared by tests/test_senti_det_train_ref_host.py (CPU:
the restatement against torch's double-precision autograd, and every case's input condition) and
tests/test_gpu_senti_det_train.py (the device against the restatement).  Each case's reference is computed once, shared
and read-only.

name -> dict(C, h, w, B[, n_convs, n_fcs, k]) and the feature seed.  The seed is the first one >= 7
(tests/_senti_det_train_ref.find_seed, at most 64 tries) at which no x2 element lies within 1e-5 of its tensor's largest
magnitude from zero in fp64, so fp32 and fp64 agree on every ReLU sign - the host test asserts both that the condition
holds and that the constant is that first seed.  These are the smallest shapes at which each index path can go wrong."""
import numpy as np
import torch

import _senti_det_ref as S
import _senti_det_train_ref as R
from insenticap_model_amd import synth
from insenticap_model_amd.helper_nets import SentimentDetector

DEFAULTS = dict(n_convs=2, n_fcs=2, k=3)
CASES = {
    'grid_1x1': (dict(C=64, h=1, w=1, B=3), 7),                 # every tap but the centre is out of grid
    'grid_1x5': (dict(C=64, h=1, w=5, B=2), 7),                 # a one-row grid
    'grid_5x1': (dict(C=64, h=5, w=1, B=2), 7),                 # a one-column grid
    'one_image': (dict(C=64, h=3, w=3, B=1), 7),
    'rows_75': (dict(C=64, h=5, w=5, B=3), 7),                  # a partial row tile, image borders inside a tile
    'rows_1332': (dict(C=64, h=6, w=6, B=37), 10),              # many contraction chunks, M not a multiple of 64
    'c128_14x14': (dict(C=128, h=14, w=14, B=2), 7),            # the reference's grid
    'convs_1': (dict(C=64, h=3, w=3, B=2, n_convs=1), 7),       # no hidden dX
    'convs_3': (dict(C=256, h=3, w=3, B=2, n_convs=3), 7),      # two dX
    'fcs_0': (dict(C=64, h=3, w=3, B=2, n_fcs=0), 7),
    'product': (dict(C=2048, h=3, w=3, B=2), 7),                # product widths and tile counts, 18 rows
}
# replayed keep-masks at p = 0.5 (default_rng(4), image 0 all kept); the seed is the first that meets the condition WITH them
MASKED = {'masked_75': (dict(C=64, h=5, w=5, B=3), 7), 'masked_14x14': (dict(C=128, h=14, w=14, B=2), 7)}
# tiny gradients: the case's weights with senti_conv and the FC weights times 2^-10, and the loss times 2^-6 - in fp64
# every |dx2| and |dx1| element is below 2^-24 (asserted by the host test)
TINY = {'tiny_75': 'rows_75', 'tiny_14x14': 'c128_14x14'}
TINY_WEIGHT, TINY_SCALE = 2.0 ** -10, 2.0 ** -6
WEIGHT_SEED, WEIGHT_GAIN = 53, 3.0
_REF = {}


def case(name):
    base = TINY.get(name, name)
    c, seed = (MASKED[base] if base in MASKED else CASES[base])
    return dict(DEFAULTS, **c), seed


def module(c, dropout_p=0.0, weights=None, tiny=False):
    """(SentimentDetector in train mode on the CPU, its state_dict arrays fp32)."""
    st = dict(synth.TINY_SETTINGS, **synth.HELPER_SETTINGS)
    st.update(fc_feat_dim=c['C'], sentiment_convs_num=c['n_convs'], sentiment_fcs_num=c['n_fcs'], dropout_p=dropout_p)
    m = SentimentDetector(S.categories(c['k']) if c['k'] > 1 else ['neutral'], st)
    if weights is None:
        shapes = {n: tuple(v.shape) for n, v in m.state_dict().items()}
        weights = synth.make_module_weights(shapes, WEIGHT_SEED, gain=WEIGHT_GAIN)
        if tiny:
            weights = {n: (v * np.float32(TINY_WEIGHT) if n.endswith('weight') and not n.startswith('convs.') else v)
                       for n, v in weights.items()}
    m.load_state_dict({n: torch.from_numpy(np.ascontiguousarray(v)) for n, v in weights.items()})
    return m.train(), weights


def keep_mask(c):
    """p = 0.5, image 0 all kept; uint8 [B,h,w,CL] channels-last."""
    rng = np.random.default_rng(4)
    keep = (rng.random((c['B'], c['h'], c['w'], c['C'] >> c['n_convs'])) < 0.5).astype(np.uint8)
    keep[0] = 1
    return keep


def inputs(c, seed):
    return S.features(c, seed), R.draw_labels(seed, c['B'], c['k'])


def cpu_error(m, feats, labels, L64, G64, keep=None, p=0.0, scale=1.0):
    """The stock fp32 module on the CPU against fp64: (e of the loss, {name: e of its gradient}, the fp32 gradients, the
    fp32 loss) - the yardstick's `e`."""
    m.zero_grad()
    loss = R.torch_loss(m, feats, labels, keep, p, scale)
    loss.backward()
    e = {n: float(np.abs(q.grad.double().numpy() - G64[n]).max()) for n, q in m.named_parameters()}
    return abs(float(loss.detach()) - L64), e, {n: q.grad.numpy().copy() for n, q in m.named_parameters()}, float(loss.detach())


def reference(name):
    if name in _REF:
        return _REF[name]
    c, seed = case(name)
    masked, tiny = name in MASKED, name in TINY
    p = 0.5 if masked else 0.0
    scale = TINY_SCALE if tiny else 1.0
    m, w = module(c, dropout_p=p, tiny=tiny)
    feats, labels = inputs(c, seed)
    keep = keep_mask(c) if masked else None
    L64, G64, aux = R.forward_backward(w, feats, labels, keep=keep, dropout_p=p, scale=scale)
    eL, eG, _, _ = cpu_error(m, feats, labels, L64, G64, keep, p, scale)
    for v in list(G64.values()) + [feats, labels]:
        v.setflags(write=False)
    _REF[name] = dict(c=c, seed=seed, w=w, feats=feats, labels=labels, keep=keep, p=p, scale=scale, loss=L64, grads=G64,
                      aux=aux, e_loss=eL, e_grads=eG, names=R.names(c['n_convs'], c['n_fcs']))
    return _REF[name]
