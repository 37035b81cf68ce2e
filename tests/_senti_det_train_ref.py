"""fp64 numpy restatement of one training iteration of the image-sentiment detector (helper_nets.SentimentDetector with
nn.CrossEntropyLoss; reference train_senti.py:78-83), forward and backward, with an optional replayed dropout keep-mask -
shared by tests/test_senti_det_train_ref_host.py (CPU: the restatement against double-precision torch autograd and the
reference's fixture, every case's input condition) and the GPU tests.

    x_i = conv_i(x_{i-1})  (3x3, padding 1, no non-linearity in between);  x2 = the last one
    r = relu(keep x2 / (1 - p));  m[b,j,p] = bs[j] + r[b,p,:] . Ws[j,:];  z = FC(... FC(mean_p m) ...)
    loss = scale mean_b (lse(z_b) - z_b[y_b])
"""
import numpy as np

import _senti_det_ref as S


def names(n_convs, n_fcs):
    """The parameter names in state_dict order."""
    out = []
    for i in range(n_convs):
        out += ['convs.conv_%d.weight' % i, 'convs.conv_%d.bias' % i]
    out += ['senti_conv.weight', 'senti_conv.bias']
    for i in range(n_fcs):
        out += ['output.%d.weight' % i, 'output.%d.bias' % i]
    return out


def flipped(W):
    """W [Cout,Cin,3,3] -> W' [Cin,Cout,3,3] with W'[ci,co,ky,kx] = W[co,ci,2-ky,2-kx]: conv3x3(dY, W') is the transposed
    convolution (padding 1)."""
    return np.ascontiguousarray(W.transpose(1, 0, 2, 3)[:, :, ::-1, ::-1])


def conv_dw(dy, x):
    """dW[co,ci,ky,kx] = sum_{b,y,x} dy[b,y,x,co] xin[b,y+ky-1,x+kx-1,ci], zeros outside the grid.  dy [B,h,w,Cout]."""
    B, h, w, Cin = x.shape
    pad = np.pad(x, ((0, 0), (1, 1), (1, 1), (0, 0)))
    dW = np.zeros((dy.shape[-1], Cin, 3, 3))
    d2 = dy.reshape(-1, dy.shape[-1])
    for ky in range(3):
        for kx in range(3):
            dW[:, :, ky, kx] = d2.T @ pad[:, ky:ky + h, kx:kx + w, :].reshape(-1, Cin)
    return dW


def forward_backward(w, feats, labels, keep=None, dropout_p=0.0, scale=1.0):
    """-> (loss, {name: gradient}, aux) in fp64.  keep: None or a 0/1 array [B,h,w,CL] (channels-last).
    aux: x (every conv output, the last = x2), r, logits, maps, dx (gradient of every conv output: dx[-1] = dx2)."""
    convs, (Ws, bs), fcs = S.split_weights(w)
    x = np.asarray(feats, np.float64)
    B, h, wd, _ = x.shape
    hw = h * wd
    xs = [x]
    for W, b in convs:
        xs.append(S.conv3x3(xs[-1], W, b))
    x2 = xs[-1]
    ms = 1.0 / (1.0 - dropout_p) if keep is not None else 1.0
    kp = np.asarray(keep, np.float64).reshape(x2.shape) if keep is not None else np.ones_like(x2)
    r = np.maximum(kp * x2 * ms, 0.0)
    m = np.einsum('bhwc,jc->bjhw', r, Ws) + bs[None, :, None, None]
    acts = [m.mean(axis=(2, 3))]
    for W, b in fcs:
        acts.append(acts[-1] @ W.T + b)
    z = acts[-1]
    mx = z.max(axis=-1, keepdims=True)
    e = np.exp(z - mx)
    prob = e / e.sum(axis=-1, keepdims=True)
    lse = mx[:, 0] + np.log(e.sum(axis=-1))
    y = np.asarray(labels, np.int64)
    loss = scale * float((lse - z[np.arange(B), y]).mean())
    maps = np.einsum('bj,bjhw->bhw', prob, m)

    g = prob.copy()
    g[np.arange(B), y] -= 1.0
    g *= scale / B
    G = {}
    for l in range(len(fcs) - 1, -1, -1):
        G['output.%d.weight' % l] = g.T @ acts[l]
        G['output.%d.bias' % l] = g.sum(axis=0)
        g = g @ fcs[l][0]
    dm = g / hw                                                     # [B,k]: d loss / d m[b,j,p], constant over p
    G['senti_conv.weight'] = np.einsum('bj,bc->jc', dm, r.sum(axis=(1, 2))).reshape(Ws.shape[0], -1, 1, 1)
    G['senti_conv.bias'] = g.sum(axis=0)
    dr = (dm @ Ws)[:, None, None, :]
    dx = dr * (kp * x2 > 0) * kp * ms
    dxs = [None] * len(convs)
    for i in range(len(convs) - 1, -1, -1):
        dxs[i] = dx
        G['convs.conv_%d.weight' % i] = conv_dw(dx, xs[i])
        G['convs.conv_%d.bias' % i] = dx.sum(axis=(0, 1, 2))
        if i > 0:
            dx = S.conv3x3(dx, flipped(convs[i][0]), 0.0)
    return loss, G, dict(x=xs[1:], r=r, logits=z, maps=maps, dx=dxs, prob=prob)


def relu_margin(aux):
    """The smallest |x2| relative to the largest: the ReLU signs of fp32 and fp64 agree when this is >= 1e-5."""
    x2 = aux['x'][-1]
    return float(np.abs(x2).min() / np.abs(x2).max())


def draw_labels(seed, B, k):
    """Every category in turn from a drawn start, then shuffled: more than one category whenever B > 1."""
    rng = np.random.default_rng([seed, 99])
    return rng.permutation((np.arange(B) + rng.integers(0, k)) % k).astype(np.int64)


def find_seed(make, start=7, tries=64):
    """The first seed >= start (at most `tries`) at which make(seed) -> aux keeps every x2 element 1e-5 of the largest
    magnitude away from zero."""
    for seed in range(start, start + tries):
        if relu_margin(make(seed)) >= 1e-5:
            return seed
    raise AssertionError('no seed in [%d, %d) meets the ReLU margin' % (start, start + tries))


def torch_loss(m, feats, labels, keep=None, dropout_p=0.0, scale=1.0):
    """The stock module's loss in the dtype of its parameters as a torch scalar with a graph: m(feats) and
    CrossEntropyLoss, or - with a keep-mask - the module's own layers with the mask in the dropout's place."""
    import torch
    import torch.nn as nn
    dt = next(m.parameters()).dtype
    x = torch.from_numpy(np.array(feats)).to(dt)
    y = torch.from_numpy(np.array(labels, np.int64))
    if keep is None:
        logits, _ = m(x)
    else:
        t = x.permute(0, 3, 1, 2)
        for mod in m.convs:
            if isinstance(mod, nn.Conv2d):
                t = mod(t)
        kp = torch.from_numpy(np.asarray(keep)).to(dt).reshape(x.shape[0], x.shape[1], x.shape[2], -1).permute(0, 3, 1, 2)
        t = torch.relu(t * kp / (1.0 - dropout_p))
        logits = m.output(m.senti_conv(t).mean(dim=(2, 3)))
    return nn.functional.cross_entropy(logits, y) * scale


def yardstick(got, ref, e):
    """-> (error, bound) with bound = 4 max(e, 2^-23 max|fp64|)."""
    ref = np.asarray(ref, np.float64)
    err = float(np.abs(np.asarray(got, np.float64).reshape(ref.shape) - ref).max())
    return err, 4.0 * max(float(e), 2.0 ** -23 * float(np.abs(ref).max()))
