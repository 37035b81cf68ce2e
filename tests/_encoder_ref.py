"""The image encoder restated from the operator definitions, in any dtype (fp64: the reference of the encoder tests; fp32:
the same arithmetic at the native precision), plus the cases, parameters and the yardstick the encoder tests share.

Everything here is NCHW torch on the CPU and uses no torch.nn.functional operator: test_encoder_ref_host.py holds each
piece to F.conv2d / F.batch_norm / F.max_pool2d(ceil_mode=True) / F.adaptive_avg_pool2d.

Yardstick (the project's, tests/test_gpu_senti_det.py):  |native - fp64| <= 4 * max(e, 2^-23 * max|fp64|), e = the stock
fp32 torch path's own error on the same inputs, run on the CPU - never taken from the code under test."""
import numpy as np
import torch

F64 = torch.float64
EPS = 1e-5
MEAN = (0.485, 0.456, 0.406)
STD = (0.229, 0.224, 0.225)


# ------------------------------------------------------------------ operators
def conv2d(x, w, stride=1, pad=0):
    """Cross-correlation: out[b, n, y, x] = sum_{c, ky, kx} w[n, c, ky, kx] xpad[b, c, y s + ky, x s + kx]."""
    B, C, H, W = x.shape
    N, _, R, S = w.shape
    xp = x.new_zeros(B, C, H + 2 * pad, W + 2 * pad)
    xp[:, :, pad:pad + H, pad:pad + W] = x
    Ho, Wo = (H + 2 * pad - R) // stride + 1, (W + 2 * pad - S) // stride + 1
    out = x.new_zeros(B, N, Ho, Wo)
    for ky in range(R):
        for kx in range(S):
            win = xp[:, :, ky:ky + stride * (Ho - 1) + 1:stride, kx:kx + stride * (Wo - 1) + 1:stride]
            out += torch.einsum('bchw,nc->bnhw', win, w[:, :, ky, kx])
    return out


def batch_norm(x, g, b, m, v, eps=EPS):
    """Eval mode: (x - mean) / sqrt(var + eps) * weight + bias, per channel."""
    s = lambda t: t.view(1, -1, 1, 1)
    return (x - s(m)) / torch.sqrt(s(v) + eps) * s(g) + s(b)


def fold(w, g, b, m, v, eps=EPS):
    """(w', b') in double: w' = w g / sqrt(v + eps), b' = b - m g / sqrt(v + eps)."""
    s = g.double() / torch.sqrt(v.double() + eps)
    return w.double() * s.view(-1, 1, 1, 1), b.double() - m.double() * s


def pool_out(n):
    """ceil((n - 3) / 2) + 1, the last window starting inside the input; None where the stock op refuses (n < 2)."""
    if n < 2:
        return None
    o = -(-(n - 3) // 2) + 1
    if (o - 1) * 2 >= n:
        o -= 1
    return o


def max_pool_ceil(x):
    """3x3, stride 2, pad 0, ceil mode: windows that overhang the edge are clipped."""
    B, C, H, W = x.shape
    Ho, Wo = pool_out(H), pool_out(W)
    if Ho is None or Wo is None:
        raise ValueError('max_pool_ceil: %dx%d has no output' % (H, W))
    out = x.new_empty(B, C, Ho, Wo)
    for i in range(Ho):
        for j in range(Wo):
            out[:, :, i, j] = x[:, :, 2 * i:min(2 * i + 3, H), 2 * j:min(2 * j + 3, W)].amax(dim=(2, 3))
    return out


def adaptive_avg(x, a):
    """out[i, j] = the mean over rows [floor(i h / a), ceil((i + 1) h / a)) and the same columns."""
    B, C, H, W = x.shape
    out = x.new_empty(B, C, a, a)
    for i in range(a):
        y0, y1 = (i * H) // a, -(-((i + 1) * H) // a)
        for j in range(a):
            x0, x1 = (j * W) // a, -(-((j + 1) * W) // a)
            out[:, :, i, j] = x[:, :, y0:y1, x0:x1].sum(dim=(2, 3)) / ((y1 - y0) * (x1 - x0))
    return out


def tail(x, a):
    """(fc [B, C] = mean over w, then over h; att [B, a, a, C])."""
    return x.sum(3).div(x.shape[3]).sum(2).div(x.shape[2]), adaptive_avg(x, a).permute(0, 2, 3, 1).contiguous()


def preprocess(image):
    """uint8 [H, W, 3] -> fp32 [3, H, W]: x / 255, then (x - mean) / std, every step in fp32 (encoder.py:29-37)."""
    x = torch.from_numpy(np.ascontiguousarray(image)).to(torch.float32) / 255.0
    return ((x - torch.tensor(MEAN)) / torch.tensor(STD)).permute(2, 0, 1).contiguous()


# ------------------------------------------------------------------ the network, from a state dict with torchvision's names
def forward(sd, layers, x, att_size, dtype=F64):
    """sd: state dict (conv1.weight, bn1.*, layer{l}.{i}.conv{1,2,3}.weight, .bn{1,2,3}.*, .downsample.{0,1}.*);
    x [B, 3, H, W] normalised -> (fc, att) in `dtype`.  Conv, then BN, unfolded."""
    p = {k: v.to(dtype) for k, v in sd.items() if v.is_floating_point()}
    bn = lambda t, n: batch_norm(t, p[n + '.weight'], p[n + '.bias'], p[n + '.running_mean'], p[n + '.running_var'])
    x = x.to(dtype)
    x = max_pool_ceil(bn(conv2d(x, p['conv1.weight'], 2, 3), 'bn1').clamp_min(0))
    for l, n in enumerate(layers):
        for i in range(n):
            q = 'layer%d.%d.' % (l + 1, i)
            s = 2 if (l > 0 and i == 0) else 1
            o = bn(conv2d(x, p[q + 'conv1.weight'], s, 0), q + 'bn1').clamp_min(0)
            o = bn(conv2d(o, p[q + 'conv2.weight'], 1, 1), q + 'bn2').clamp_min(0)
            o = bn(conv2d(o, p[q + 'conv3.weight'], 1, 0), q + 'bn3')
            idn = bn(conv2d(x, p[q + 'downsample.0.weight'], s, 0), q + 'downsample.1') if i == 0 else x
            x = (o + idn).clamp_min(0)
    return tail(x, att_size)


# ------------------------------------------------------------------ cases
def make_encoder(layers, width, seed):
    """Convolution weights: torch's default init; BN weight and variance U(0.5, 1.5), bias and mean U(-0.2, 0.2)."""
    from insenticap_model_amd.encoder import Encoder
    torch.manual_seed(seed)
    enc = Encoder(None, layers, width)
    g = torch.Generator().manual_seed(seed + 1)
    with torch.no_grad():
        for m in enc.modules():
            if isinstance(m, torch.nn.BatchNorm2d):
                n = m.weight.numel()
                m.weight.copy_(torch.rand(n, generator=g) + 0.5)
                m.running_var.copy_(torch.rand(n, generator=g) + 0.5)
                m.bias.copy_(torch.rand(n, generator=g) * 0.4 - 0.2)
                m.running_mean.copy_(torch.rand(n, generator=g) * 0.4 - 0.2)
    return enc.eval()


def make_image(H, W, seed, B=None):
    shape = (H, W, 3) if B is None else (B, H, W, 3)
    return np.random.default_rng(seed).integers(0, 256, shape, dtype=np.uint8)


NETS = {'n1111': ((1, 1, 1, 1), 32, 101), 'n2121': ((2, 1, 2, 1), 32, 102), 'full': ((3, 4, 23, 3), 64, 103)}
IMAGES = {'45x61': (45, 61, 201), '33x33': (33, 33, 202), '97x70': (97, 70, 203)}
_ENC, _REF = {}, {}


def encoder(net):
    if net not in _ENC:
        _ENC[net] = make_encoder(*NETS[net])
    return _ENC[net]


def bound(e, ref):
    return 4.0 * max(float(e), 2.0 ** -23 * float(np.abs(ref).max()))


def reference(net, image, att_size=6):
    """Per (net, image, att_size), computed once and left unchanged: the uint8 image, its `preprocess`, the fp64 (fc,
    att) and e = the stock fp32 module's error against it (the module itself, native off, on the CPU)."""
    key = (net, image, att_size)
    if key not in _REF:
        enc = encoder(net)
        H, W, seed = IMAGES[image]
        u8 = make_image(H, W, seed)
        x = preprocess(u8)
        layers = NETS[net][0]
        with torch.no_grad():
            fc64, att64 = forward(enc.resnet.state_dict(), layers, x.unsqueeze(0), att_size)
            fc32, att32 = enc._torch_batch(x.unsqueeze(0), att_size)
        ref = dict(fc=fc64[0].numpy(), att=att64[0].numpy())
        e = dict(fc=float(np.abs(fc32[0].double().numpy() - ref['fc']).max()),
                 att=float(np.abs(att32[0].double().numpy() - ref['att']).max()))
        _REF[key] = dict(u8=u8, x=x, ref=ref, e=e)
    return _REF[key]


def compare(got_fc, got_att, c, what):
    for k, got in (('fc', got_fc), ('att', got_att)):
        ref = c['ref'][k]
        assert got.shape == ref.shape, (what, k, got.shape, ref.shape)
        err, b = float(np.abs(got.astype(np.float64) - ref).max()), bound(c['e'][k], ref)
        print('%s %s: err %.3g, stock fp32 e %.3g, bound %.3g, max|ref| %.3g' % (what, k, err, c['e'][k], b,
                                                                                np.abs(ref).max()))
        assert err <= b, '%s %s: |native - fp64| = %.3g > %.3g (stock fp32 error %.3g)' % (what, k, err, b, c['e'][k])


# ------------------------------------------------------------------ im2col (the lattice tests of the convolution kernel)
def im2col(x, R, stride=1):
    """x [B, h, w, C] (channels-last, any dtype) -> rows [B ho wo, R R C], k = tap C + ci; R = 3: pad 1, stride 1, zeros
    outside the image's own grid; R = 1: pixel (y stride, x stride)."""
    B, h, w, C = x.shape
    if R == 1:
        return x[:, ::stride, ::stride, :].reshape(-1, C)
    xp = x.new_zeros(B, h + 2, w + 2, C)
    xp[:, 1:h + 1, 1:w + 1] = x
    return torch.cat([xp[:, ky:ky + h, kx:kx + w, :] for ky in range(3) for kx in range(3)], dim=3).reshape(B * h * w, 9 * C)
