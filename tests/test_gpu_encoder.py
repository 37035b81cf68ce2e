"""The whole image encoder on the device (isc_encoder_fwd / encoder.Encoder) against the fp64 restatement
tests/_encoder_ref.py.  pytest -m gpu.

Yardstick, applied to fc and att:  |native - fp64| <= 4 * max(e, 2^-23 * max|fp64|), e = the stock fp32 module's own
error on the same inputs, run on the CPU (never taken from the code under test).  Networks [1, 1, 1, 1] and [2, 1, 2, 1]
at width 32 on images 45x61, 33x33 (a 1x1 layer-4 grid) and 97x70; the full depth [3, 4, 23, 3] at width 64 on one 97x70
image (a 3x3 final grid), with the launch count by formula."""
import copy

import numpy as np
import pytest
import torch

import _encoder_ref as R
from insenticap_model_amd import data, ops, synth
from insenticap_model_amd.helper_nets import ConceptDetector

pytestmark = pytest.mark.gpu
DEV = torch.device('cuda:0')
_DEV_ENC = {}


def dev_encoder(net):
    if net not in _DEV_ENC:
        _DEV_ENC[net] = copy.deepcopy(R.encoder(net)).to(DEV).eval()
    return _DEV_ENC[net]


def kinds_delta(before):
    now = ops.encoder_launches()
    return {k: now[k] - before[k] for k in now}


def conv_list(layers, width):
    """(R, Cin) of every implicit-GEMM convolution, in launch order."""
    out, inpl = [], width
    for l, n in enumerate(layers):
        p = width << l
        for i in range(n):
            out += [(1, inpl), (3, p)] + ([(1, inpl)] if i == 0 else []) + [(1, p)]
            inpl = 4 * p
    return out


def conv_geometry(layers, width, H, W):
    """(R, Cin, N, rows of ONE image) of every implicit-GEMM convolution, in launch order."""
    h, w = ((H - 1) // 2 + 1 - 2) // 2 + 1, ((W - 1) // 2 + 1 - 2) // 2 + 1
    out, inpl = [], width
    for l, n in enumerate(layers):
        p = width << l
        for i in range(n):
            if l > 0 and i == 0:
                h, w = (h - 1) // 2 + 1, (w - 1) // 2 + 1
            out += [(1, inpl, p, h * w), (3, p, p, h * w)] + ([(1, inpl, 4 * p, h * w)] if i == 0 else []) + \
                   [(1, p, 4 * p, h * w)]
            inpl = 4 * p
    return out


def cost_rule(R_, Cin, N, M1):
    """The library's route, restated from its documentation: from ONE image's rows M1 - under 128 tiles of 64 x 128 the
    contraction splits until about 256 workgroups per image run, 32 shares at the most, every share >= 2 chunks."""
    nchunks = R_ * R_ * Cin // 32
    tiles = -(-M1 // 64) * -(-N // 128)
    if tiles >= 128:
        return 1
    return max(1, min(-(-256 // tiles), 32, nchunks // 2))


def expected_launches(layers):
    return dict(stem=1, pool=1, convs=3 * sum(layers) + 4, tail=1)


@pytest.mark.parametrize('image', list(R.IMAGES))
@pytest.mark.parametrize('net', ['n1111', 'n2121'])
def test_small_networks_vs_fp64(net, image):
    c = R.reference(net, image)
    enc = dev_encoder(net)
    layers = R.NETS[net][0]
    before = ops.encoder_launches()
    with torch.no_grad():
        fc, att = enc(c['x'].to(DEV), 6)
    d = kinds_delta(before)
    want = expected_launches(layers)
    assert (d['stem'], d['pool'], d['direct'] + d['split'], d['tail']) == (1, 1, want['convs'], 1)
    assert d['reduce'] == d['split'] and d['r1'] == 2 * sum(layers) + 4 and d['r3'] == sum(layers)
    assert fc.shape == (1024,) and att.shape == (6, 6, 1024)
    R.compare(fc.cpu().numpy(), att.cpu().numpy(), c, '%s %s' % (net, image))
    # the fused-normalisation path from the decoded pixels
    fc8, att8 = enc.encode_uint8(c['u8'], 6)
    R.compare(fc8.cpu().numpy(), att8.cpu().numpy(), c, '%s %s uint8' % (net, image))
    assert (c['ref']['fc'] != 0).any()
    ops.check_numerics()


@pytest.mark.parametrize('ksplit', [1, 3])
def test_both_routes_forced_through_the_whole_network(ksplit):
    c = R.reference('n2121', '45x61')
    enc = dev_encoder('n2121')
    before = ops.encoder_launches()
    fc, att = enc._native_batch(c['x'].permute(1, 2, 0).contiguous().unsqueeze(0).to(DEV), 6, ksplit=ksplit)
    d = kinds_delta(before)
    # a forced split is capped at the chunk count: the 1x1 convolutions over 32 channels have one chunk and stay direct
    chunks = [r * r * cin // 32 for r, cin in conv_list((2, 1, 2, 1), 32)]
    n_split = sum(1 for n in chunks if min(ksplit, n) > 1)
    assert len(chunks) == 3 * 6 + 4 and (n_split == 0 if ksplit == 1 else 0 < n_split < len(chunks))
    assert (d['direct'], d['split'], d['reduce']) == (len(chunks) - n_split, n_split, n_split)
    R.compare(fc[0].cpu().numpy(), att[0].cpu().numpy(), c, 'n2121 45x61 ksplit=%d' % ksplit)


def test_full_depth_vs_fp64_and_its_launch_count():
    c = R.reference('full', '97x70', att_size=14)
    enc = dev_encoder('full')
    layers = R.NETS['full'][0]
    before = ops.encoder_launches()
    enc.packed()
    assert kinds_delta(before)['pack'] == 3 * sum(layers) + 4 + 1
    before = ops.encoder_launches()
    with torch.no_grad():
        fc, att = enc(c['x'].to(DEV), 14)
    d = kinds_delta(before)
    assert fc.shape == (2048,) and att.shape == (14, 14, 2048) and ops.encoder_final_grid(97, 70) == (3, 3)
    convs = 3 * sum(layers) + 4
    assert (d['stem'], d['pool'], d['tail'], d['pack']) == (1, 1, 1, 0)
    assert d['direct'] + d['split'] == convs == 103 and d['reduce'] == d['split']
    # the launch count by formula: stem, pool, 3 per block, one downsample per layer, tail, and one reduce behind every
    # convolution the cost rule splits - worked out here from the 97x70 geometry, not read from the counters
    geo = conv_geometry(layers, 64, 97, 70)
    assert len(geo) == convs and geo[-1][3] == 9
    n_split = sum(1 for g in geo if cost_rule(*g) > 1)
    assert 0 < n_split < convs
    assert (d['direct'], d['split'], d['reduce']) == (convs - n_split, n_split, n_split)
    total = d['stem'] + d['pool'] + d['direct'] + d['split'] + d['reduce'] + d['tail']
    assert total == 1 + 1 + 3 * sum(layers) + 4 + 1 + n_split
    print('full depth: %d launches (%d direct, %d split + reduce)' % (total, d['direct'], d['split']))
    R.compare(fc.cpu().numpy(), att.cpu().numpy(), c, 'full 97x70')
    ops.check_numerics()


def test_forward_batch_equals_single_calls_in_bits_and_float16_copies():
    enc = dev_encoder('n2121')
    u8 = R.make_image(45, 61, 7, B=3)
    x = torch.stack([R.preprocess(i) for i in u8]).to(DEV)
    with torch.no_grad():
        fc, att, fc16, att16 = enc.forward_batch(x, 6, want_f16=True)
        for i in range(3):
            f1, a1 = enc(x[i], 6)
            assert torch.equal(f1, fc[i]) and torch.equal(a1, att[i])
        again = enc.forward_batch(x, 6)
    assert torch.equal(again[0], fc) and torch.equal(again[1], att)             # two runs, the same bits
    assert torch.equal(fc16, fc.half()) and torch.equal(att16, att.half())


def test_a_batch_takes_the_route_of_one_image_where_a_rule_over_the_batch_would_not():
    """213 x 213 gives layer 1 a 53 x 53 grid: 2809 rows, 44 row tiles per image - under the rule's 128-tile threshold -
    and 132 for three images, above it.  The route comes from one image's rows, so the batch splits the same
    convolutions into the same shares as a single call and every image keeps its bits."""
    enc = dev_encoder('n1111')
    geo = conv_geometry((1, 1, 1, 1), 32, 213, 213)
    assert geo[0][3] == 2809 and -(-2809 // 64) < 128 <= -(-3 * 2809 // 64)
    assert cost_rule(*geo[1]) > 1 and cost_rule(geo[1][0], geo[1][1], geo[1][2], 3 * geo[1][3]) == 1
    n_split = sum(1 for g in geo if cost_rule(*g) > 1)
    u8 = torch.from_numpy(R.make_image(213, 213, 11, B=3)).to(DEV)
    before = ops.encoder_launches()
    fc, att = enc.encode_uint8(u8, 6)
    d = kinds_delta(before)
    assert (d['direct'], d['split'], d['reduce']) == (len(geo) - n_split, n_split, n_split)
    for i in range(3):
        before = ops.encoder_launches()
        f1, a1 = enc.encode_uint8(u8[i], 6)
        d = kinds_delta(before)
        assert (d['direct'], d['split'], d['reduce']) == (len(geo) - n_split, n_split, n_split)
        assert torch.equal(f1, fc[i]) and torch.equal(a1, att[i])


def test_one_workspace_per_stream_whatever_the_number_of_image_sizes():
    enc = dev_encoder('n1111')
    ops._ENCODER_WS.clear()
    sizes = []
    for H, W in ((33, 33), (97, 70), (45, 61), (64, 48), (33, 40)):
        enc.encode_uint8(torch.zeros(H, W, 3, dtype=torch.uint8, device=DEV), 3)
        assert len(ops._ENCODER_WS) == 1
        sizes.append(next(iter(ops._ENCODER_WS.values())).numel())
    assert sizes == sorted(sizes) and sizes[1] == sizes[-1] > sizes[0]           # grown once, then reused
    c = R.reference('n1111', '33x33')                                            # and a smaller image in the larger workspace
    fc, att = enc.encode_uint8(c['u8'], 6)
    R.compare(fc.cpu().numpy(), att.cpu().numpy(), c, 'n1111 33x33 in a grown workspace')


def test_in_place_weight_changes_are_followed():
    enc = copy.deepcopy(dev_encoder('n1111'))
    c = R.reference('n1111', '33x33')
    x = c['x'].to(DEV)
    with torch.no_grad():
        fc0, _ = enc(x, 6)
        before = ops.encoder_launches()
        enc(x, 6)
        assert kinds_delta(before)['pack'] == 0                                  # packed once per weight version
        enc.resnet.layer4[0].bn3.running_var.mul_(4.0)
        enc.resnet.layer1[0].conv2.weight.mul_(0.5)
        before = ops.encoder_launches()
        fc1, att1 = enc(x, 6)
        assert kinds_delta(before)['pack'] == 1 + 3 * 4 + 4
    assert not torch.equal(fc0, fc1)
    host = copy.deepcopy(enc).cpu()
    with torch.no_grad():
        fc64, att64 = R.forward(host.resnet.state_dict(), (1, 1, 1, 1), c['x'].unsqueeze(0), 6)
        fc32, att32 = host._torch_batch(c['x'].unsqueeze(0), 6)
    cc = dict(ref=dict(fc=fc64[0].numpy(), att=att64[0].numpy()),
              e=dict(fc=float((fc32.double() - fc64).abs().max()), att=float((att32.double() - att64).abs().max())))
    R.compare(fc1.cpu().numpy(), att1.cpu().numpy(), cc, 'n1111 33x33 after in-place changes')


def test_hip_graph_capture_of_a_fixed_size_forward():
    enc = dev_encoder('n1111')
    packed = enc.packed()
    rng = np.random.default_rng(9)
    fresh = [torch.from_numpy(rng.integers(0, 256, (1, 45, 61, 3), dtype=np.uint8)).to(DEV) for _ in range(3)]
    eager = [tuple(t.clone() for t in ops.encoder_fwd(packed, x, (1, 1, 1, 1), 32, 6)) for x in fresh]
    static = fresh[0].clone()
    st = torch.cuda.Stream()
    st.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(st):
        ops.encoder_fwd(packed, static, (1, 1, 1, 1), 32, 6)                      # warm
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph, stream=st):
            got = ops.encoder_fwd(packed, static, (1, 1, 1, 1), 32, 6)
    torch.cuda.current_stream().wait_stream(st)
    torch.cuda.synchronize()
    for x, want in zip(fresh, eager):
        static.copy_(x)
        graph.replay()
        torch.cuda.synchronize()
        assert torch.equal(got[0], want[0]) and torch.equal(got[1], want[1])


def test_detector_sample_image_returns_the_captions_of_sample_on_the_encoders_outputs():
    from insenticap_model_amd.detector import Detector
    V, TN = 64, 8
    st = dict(synth.TINY_SETTINGS, **synth.HELPER_SETTINGS)
    st.update(fc_feat_dim=1024, att_feat_dim=1024)
    idx2word = synth.make_idx2word(V)
    det = Detector(idx2word, TN, synth.SENTIMENT_CATEGORIES, {'cap_lr': 4e-5}, st)
    det.captioner.load_state_dict({k: torch.from_numpy(v) for k, v in synth.make_weights(V, st, seed=1).items()})
    for mod, seed in ((det.senti_detector, 51), (det.sent_senti_cls, 52)):
        shapes = {k: tuple(v.shape) for k, v in mod.state_dict().items()}
        mod.load_state_dict({k: torch.from_numpy(v) for k, v in synth.make_module_weights(shapes, seed).items()})
        mod.eval()
    det.to(DEV)
    word2idx = {w: i for i, w in enumerate(idx2word)}
    idx2concept = ['w%d' % (10 + i) for i in range(20)]
    cd = ConceptDetector(idx2concept, dict(fc_feat_dim=1024, concept_mid_him=32, dropout_p=0.5))
    w = synth.make_module_weights({n: tuple(v.shape) for n, v in cd.state_dict().items()}, 53, gain=4.0)
    cd.load_state_dict({n: torch.from_numpy(v) for n, v in w.items()})
    cd.set_vocabulary(word2idx).to(DEV).eval()
    rng = np.random.default_rng(21)
    sd = {c: [['w%d' % int(rng.integers(30, 64)), float(rng.random())] for _ in range(int(rng.integers(1, 7)))]
          for c in idx2concept[:16]}
    det.set_concept_detector(cd, data.SentimentWordTable(sd, word2idx, idx2concept), num_concepts=5, num_sentiments=10)
    enc = dev_encoder('n1111')
    with pytest.raises(ValueError):
        det.sample_image(R.make_image(45, 61, 1), att_size=3)
    det.set_encoder(enc)
    assert not any('encoder' in k or 'resnet' in k for k in det.state_dict())
    u8 = R.make_image(45, 61, 1)
    fc, att = enc.encode_uint8(u8, 3)
    want = det.sample(fc, att, None, beam_size=3, decoding_constraint=1)
    got = det.sample_image(u8, beam_size=3, decoding_constraint=1, att_size=3)
    assert got == want and len(got[0]) >= 1
    # a `preprocess`ed tensor takes the fp32 stem, whose values equal the fused path's
    assert det.sample_image(enc.preprocess(u8), beam_size=3, decoding_constraint=1, att_size=3) == want
