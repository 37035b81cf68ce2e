"""The inner XE training step of the reference (train_xe.py:149-192) on the HIP path, optionally
data-parallel.  Batch tuple layouts are the reference collate functions' (dataloader.py:11-58):
  fact batch: (fns, fc_feats [B,F], att_feats [B,...,F], (caps [B,L], lengths), cpts [B,C])
  scs  batch: ((caps [80,L], lengths), cpts [80,C], sentis [80,10], senti_labels [80])
The sentence-sentiment classifier that labels the factual captions (train_xe.py:155-158) is a
frozen helper outside this path: the caller passes its arg-max as `xe_senti_labels`.
"""
import math

import torch

from . import dp, ops
from .optim import FusedClampAdam, clip_gradient


_SIDE_STREAMS = {}


def _side_stream(device):
    key = (device.type, device.index)
    if key not in _SIDE_STREAMS:
        from . import ops
        _SIDE_STREAMS[key] = ops.private_stream(device)
        # gradients of one parameter arrive from two streams by design
        warn_off = getattr(torch.autograd.graph, 'set_warn_on_accumulate_grad_stream_mismatch', None)
        if warn_off is not None:
            warn_off(False)
    return _SIDE_STREAMS[key]


def run_on_side_stream(device, fn, side=None):
    """fn() with its launches on the device's side stream, ordered after everything queued so far on the current
    stream; the current stream then waits for it.  Returns fn()'s tensor result (recorded on the current stream)."""
    main = torch.cuda.current_stream(device)
    side = side if side is not None else _side_stream(device)
    side.wait_stream(main)
    with torch.cuda.stream(side):
        out = fn()
    main.wait_stream(side)
    out.record_stream(main)
    return out


def _xe_loss(xe_crit, pred, target, lengths):
    """xe_crit(pred, target, lengths) (train_xe.py:164); `lengths` already on the device (a captured iteration's static
    input, validated by the caller): straight to the criterion's launch, no host-side max()."""
    if isinstance(lengths, torch.Tensor) and lengths.is_cuda:
        from .autograd import xe_criterion_with_grad
        return xe_criterion_with_grad(pred, target, lengths)
    return xe_crit(pred, target, lengths)


def xe_forward_backward(captioner, optim, xe_crit, da_crit, fact, xe_senti_labels, scs=None, ss_prob=0.0, arena=None,
                        weights3=None, overlap_unrolls=True, side_stream=None, pair=None, sink=None, captions_per_image=1):
    """`captions_per_image=n` > 1 (Captioner.forward_xe): `fact` holds fc / att / cpts once per image, [I, ...], and caps /
    lengths / `xe_senti_labels` per caption row, image-major [I*n] (data.create_collate_fn('caption',
    captions_per_image=n)); the step then takes the un-merged route - the XE unroll, and the seq2seq unroll on the side
    stream.  The domain-alignment loss is a mean over the I images (equal to the mean over rows: every image has n).
    train_xe.py:160-190 on device tensors: both unrolls, the three losses, backward.  `fact` = (fc, att, caps,
    lengths, cpts), `scs` = (caps, lengths, cpts, sentis, labels) or None; `weights3` = this rank's shares of the three
    global normalisers (XE tokens, seq2seq tokens, rows) as a device tensor (or a callable returning it, resolved after
    the unrolls' forward: dp_shares_async), or None (single process: graph untouched).  Returns the detached [xe, da, seq2seq] losses as one device tensor.  No collective, no host read:
    this is the part of an iteration that train_graph.XETrainGraph captures into a HIP graph."""
    fc_feats, att_feats, caps_tensor, lengths, cpts_tensor = fact
    device = fc_feats.device
    share = (lambda x, w: x * w) if weights3 is not None else (lambda x, w: x)
    if (isinstance(captions_per_image, bool) or not hasattr(captions_per_image, '__index__')
            or int(captions_per_image) < 1):
        raise ValueError('captions_per_image must be an integer >= 1, got %r' % (captions_per_image,))
    grouped = int(captions_per_image) > 1
    if grouped:
        if pair or sink is not None:
            raise ValueError('captions_per_image > 1 is not built for the merged xe_seq2seq step (pair / sink)')
        pair = False
    if pair is None:
        from .autograd_pair import use_pair
        pair = use_pair(captioner, False)
        if (pair and sink is None and getattr(captioner, 'pair_unrolls', None) is None
                and not (captioner.training and ss_prob > 0.0)        # (scheduled sampling keeps the full unroll)
                and captioner.ragged_applies(lengths)):
            pair = False               # (captioner.ragged_unroll: one chain per unroll, each on the rows inside their captions)
    pair = pair and scs is not None and device.type == 'cuda'
    # (token_logprobs: the unrolls hand the criterion log p(target) [B,T] - the [B,T,V] log-probs are never formed)
    if pair:
        # both unrolls through ONE step chain (Captioner.forward_xe_seq2seq / autograd_pair): the LSTM cells, the
        # classifier and every backward contraction run once over the 128 + 80 rows instead of once per unroll
        s_caps, s_lengths, s_cpts, s_sentis, s_labels = scs
        with captioner.token_logprobs():
            pred, pred2 = captioner(fc_feats, att_feats, cpts_tensor, caps_tensor, xe_senti_labels, ss_prob,
                                    s_caps, s_cpts, s_sentis, s_labels, ss_prob, mode='xe_seq2seq')
    else:
        with captioner.token_logprobs(), captioner.row_counts(lengths):
            kw = dict(captions_per_image=captions_per_image) if grouped else {}
            pred = captioner(fc_feats, att_feats, cpts_tensor, caps_tensor, xe_senti_labels, ss_prob, mode='xe', **kw)
    if callable(weights3):            # (dp_shares_async: the counts' all-reduce ran next to the unroll; wait for it here)
        weights3 = weights3()
    w_xe, w_s2s, w_rows = weights3.unbind(0) if weights3 is not None else (None, None, None)
    xe_bwd = share(_xe_loss(xe_crit, pred, caps_tensor[:, 1:], lengths), w_xe)
    da_bwd = share(da_crit(captioner.cpt_feats, captioner.fc_feats.detach()), w_rows)
    total = xe_bwd + da_bwd
    s2s_d = torch.zeros((), device=device)
    if pair:
        s2s = share(_xe_loss(xe_crit, pred2, s_caps[:, 1:], s_lengths), w_s2s)
        total = total + s2s
        s2s_d = s2s.detach()
    elif scs is not None:
        s_caps, s_lengths, s_cpts, s_sentis, s_labels = scs

        def seq2seq_unroll():
            with captioner.token_logprobs(), captioner.row_counts(s_lengths):
                pred2 = captioner(s_caps, s_cpts, s_sentis, s_labels, ss_prob, mode='seq2seq')
            return share(_xe_loss(xe_crit, pred2, s_caps[:, 1:], s_lengths), w_s2s)
        if overlap_unrolls and device.type == 'cuda':
            s2s = run_on_side_stream(device, seq2seq_unroll, side_stream)
        else:
            s2s = seq2seq_unroll()
        total = total + s2s
        s2s_d = s2s.detach()
    if arena is not None:
        arena.zero_()
    else:
        optim.zero_grad()
    if sink is not None and pair:
        # data-parallel, merged unrolls: the backward writes every gradient into its arena view and starts each bucket's
        # all-reduce as soon as the bucket is complete (dp.GradSink; autograd_pair._pair_backward)
        sink.begin()
        captioner._grad_sink = sink
        try:
            total.backward()
        finally:
            captioner._grad_sink = None
    else:
        total.backward()
    return torch.stack([xe_bwd.detach(), da_bwd.detach(), s2s_d])


def xe_update(optim, grad_clip):
    """train_xe.py:191-192: clamp (fused into the Adam launch) + step."""
    clip_gradient(optim, grad_clip)
    optim.step()


def loss_dict(vec3):
    out = dict(zip(('xe_loss', 'da_loss', 'seq2seq_loss'), vec3.unbind(0)))
    out['cap_loss'] = out['xe_loss'] + out['da_loss']
    out['all_loss'] = out['cap_loss'] + out['seq2seq_loss']
    return out


def dp_shares(lengths, s_lengths, rows, device, group):
    """Each loss term's share of ITS global normaliser (XE tokens, seq2seq tokens, rows): ONE 3-float all-reduce, built
    on the rank's GPU (RCCL moves device tensors only), before any compute depends on it."""
    local, glob = dp.global_counts([float(sum(lengths)), float(sum(s_lengths)) if s_lengths is not None else 0.0,
                                    float(rows)], device, group)
    return local / glob.clamp_min(1.0)


def dp_shares_async(lengths, s_lengths, rows, device, group):
    """dp_shares whose all-reduce does not hold the compute stream: returns a callable that waits for the reduction (on
    the then-current stream) and returns the shares - the eager step calls it after the unrolls' forward passes, where
    the first loss is scaled, so the collective's latency is behind ~2 ms of launches instead of in front of them."""
    local, glob, work = dp.global_counts([float(sum(lengths)), float(sum(s_lengths)) if s_lengths is not None else 0.0,
                                          float(rows)], device, group, asynchronous=True)

    def shares():
        if work is not None:
            work.wait()
        return local / glob.clamp_min(1.0)
    return shares


def xe_train_step(captioner, optim, xe_crit, da_crit, fact_batch, xe_senti_labels, scs_batch=None,
                  ss_prob=0.0, grad_clip=0.1, arena=None, group=None, device=None, overlap_unrolls=True, bucketed=True,
                  captions_per_image=1):
    """`captions_per_image`: xe_forward_backward's (a batch of the 'caption' collate with the same keyword).
    One iteration. Returns dict(xe_loss, da_loss, cap_loss, seq2seq_loss, all_loss) of 0-dim
    tensors (global values under DP).  `arena`: dp.GradArena when gradients are all-reduced.
    `overlap_unrolls`: the seq2seq unroll (80 text-only rows) runs on a side HIP stream.  It shares nothing
    with the XE unroll but the weights, and at these batch sizes both are chains of small launches that leave
    most of the chip idle; autograd replays each unroll's backward on the stream its forward ran on, so the
    two backward sweeps overlap as well.  Same numbers either way (two-operand gradient sums commute).
    (train_graph.XETrainGraph runs the same three phases from HIP graphs.)
    `bucketed` (with an arena and the merged unrolls): the gradient exchange goes out in four buckets from inside the
    backward pass, overlapped with its dW contractions, and clamp + Adam run per bucket behind each reduction
    (dp.GradSink); False = one flat all-reduce after the backward.  Same parameters after the step, bit for bit."""
    device = torch.device(device) if device is not None else next(captioner.parameters()).device
    _, fc_feats, att_feats, (caps_tensor, lengths), cpts_tensor = fact_batch[:5]
    fact = (ops.to_device(fc_feats, device), ops.to_device(att_feats, device), ops.to_device(caps_tensor, device), lengths,
            ops.to_device(cpts_tensor, device))
    xe_senti_labels = ops.to_device(xe_senti_labels, device)
    scs = None
    if scs_batch is not None:
        (s_caps, s_lengths), s_cpts, s_sentis, s_labels = scs_batch
        scs = (ops.to_device(s_caps, device), s_lengths, ops.to_device(s_cpts, device), ops.to_device(s_sentis, device),
               ops.to_device(s_labels, device))
    # data-parallel: taken whenever a process group exists (also a one-rank one: shares are then exactly 1.0), so the
    # single-GPU RCCL test crosses every branch an 8-rank run does
    dist_on = dp.distributed(group)
    weights3 = dp_shares_async(lengths, scs[1] if scs is not None else None, fact[0].shape[0], device, group) \
        if dist_on else None
    from .autograd_pair import use_pair
    sink = None
    if (arena is not None and bucketed and scs is not None and device.type == 'cuda' and use_pair(captioner, False)
            and isinstance(optim, FusedClampAdam) and captions_per_image == 1):
        sink = captioner.__dict__.get('_dp_sink')
        if sink is None or sink.arena is not arena or sink.group is not group:
            sink = captioner.__dict__['_dp_sink'] = dp.GradSink(captioner, arena, group)
    vec = xe_forward_backward(captioner, optim, xe_crit, da_crit, fact, xe_senti_labels, scs, ss_prob, arena, weights3,
                              overlap_unrolls, sink=sink, captions_per_image=captions_per_image)
    if sink is not None and sink.order:
        # the loss statistics: queued behind the buckets on the backend's stream, NOT waited for here - the compute stream
        # would otherwise stand behind every bucket's reduction before the first bucket's update
        vec, work = dp.all_reduce_async_(vec, group) if dist_on else (vec, None)
        sink.finish(optim, grad_clip)    # per bucket: wait for its reduction, clamp + Adam
        if work is not None:
            work.wait()
        return loss_dict(vec)
    if arena is not None:
        arena.all_reduce(group)          # one 88 MB sum over xGMI; clamp must see reduced grads
    if dist_on:                          # report global losses (sum of the pre-scaled locals): one 3-float all-reduce
        vec = dp.all_reduce_(vec, group)
    xe_update(optim, grad_clip)
    return loss_dict(vec)


# ---------------------------------------------------------------------------- concept detector (train_cpt.py:76-90)
class _ConceptLossFn(torch.autograd.Function):
    """Features to MultiLabelClsLoss in one node.  Forward: two isc_linear_fwd launches with ReLU (the second with the
    dropout keep-mask in its epilogue), the logits launch, isc_concept_loss - which also leaves dz = d loss / d logits.
    Backward: ops.gemm_bwd TN for the three dW and NN for the two dX, ops.relu_mask_bwd, ops.colsum_multi for the biases."""

    @staticmethod
    def forward(ctx, feats, targets, keep_mask, mask_scale, w0, b0, w2, b2, w5, b5):
        B, H, C_ = feats.shape[0], w0.shape[0], w5.shape[0]
        dev = feats.device
        h1 = torch.empty(B, H, dtype=torch.float32, device=dev)
        h2 = torch.empty(B, H, dtype=torch.float32, device=dev)
        z = torch.empty(B, C_, dtype=torch.float32, device=dev)
        ops.linear_fwd([ops.linear_problem([(feats, w0)], h1, bias0=b0, relu=True)])
        ops.linear_fwd([ops.linear_problem([(h1, w2)], h2, bias0=b2, relu=True, keep_mask=keep_mask,
                                           mask_scale=mask_scale)])
        ops.linear_fwd([ops.linear_problem([(h2, w5)], z, bias0=b5)])
        # dz is of the order 1 / (B C) - below the f16 normal range at any training size, where the split-f16 engine's
        # planes (the dW contractions of a batch that is a multiple of 32) keep bits relative to 2^-14, not to the element.
        # The sweep is linear in dz: it enters as dz S with S the power of two that brings S / (B C) into (2^-4, 2^-3],
        # and the parameter gradients leave times 1 / S - both exact, so the fp32 tiles give the unscaled bits.
        S = 2.0 ** (math.floor(math.log2(B * C_)) - 3)
        out3, dz = ops.concept_loss(z, targets, S, want_dz=True)
        ctx.save_for_backward(feats, h1, h2, dz, w2, w5)
        ctx.keep_mask, ctx.mask_scale, ctx.unscale = keep_mask, mask_scale, 1.0 / S
        ctx.terms = out3
        return out3[2].clone()

    @staticmethod
    def backward(ctx, g):
        feats, h1, h2, dz, w2, w5 = ctx.saved_tensors
        B, H, C_, F = feats.shape[0], w2.shape[0], w5.shape[0], feats.shape[1]
        dev = feats.device
        dz = dz * g                                          # (the caller's d loss: a device scalar, 1 in the step below)
        new = lambda *s: torch.empty(*s, dtype=torch.float32, device=dev)
        dw0, db0, dw2, db2, dw5, db5 = new(H, F), new(H), new(H, H), new(H), new(C_, H), new(C_)
        dh2, dp2, dh1, dp1 = new(B, H), new(B, H), new(B, H), new(B, H)
        ops.gemm_bwd([ops.gemm_problem([(dz, h2)], dw5, ops.TN)], ops.TN)
        ops.gemm_bwd([ops.gemm_problem([(dz, w5)], dh2, ops.NN)], ops.NN)
        ops.relu_mask_bwd(dh2, h2, dp2, ctx.keep_mask, ctx.mask_scale)     # (h2 = relu * mask * scale: > 0 where both let through)
        ops.gemm_bwd([ops.gemm_problem([(dp2, h1)], dw2, ops.TN)], ops.TN)
        ops.gemm_bwd([ops.gemm_problem([(dp2, w2)], dh1, ops.NN)], ops.NN)
        ops.relu_mask_bwd(dh1, h1, dp1)
        ops.gemm_bwd([ops.gemm_problem([(dp1, feats)], dw0, ops.TN)], ops.TN)
        ops.colsum_multi([(dz, [db5], False), (dp2, [db2], False), (dp1, [db0], False)])
        torch._foreach_mul_([dw0, db0, dw2, db2, dw5, db5], ctx.unscale)
        return None, None, None, None, dw0, db0, dw2, db2, dw5, db5


def concept_loss_with_grad(model, fc_feats, targets, _keep_mask=None):
    """MultiLabelClsLoss of model(fc_feats) against the 0/1 `targets` [B, C] (uint8 or int64, as the concept collate
    gives them) as a differentiable device scalar, on the library's kernels.  In train mode with dropout_p > 0 the
    uint8 keep-mask [B, mid] is drawn the way the captioner draws its masks (one bernoulli_ launch on torch's
    generator); `_keep_mask` replays a given one (tests).  Needs fc_feat_dim % 32 == concept_mid_him % 32 == 0 (the
    forward contractions) and a number of concepts that is a multiple of 4 (the backward contractions): ValueError
    otherwise - there is no quiet torch fallback; call model(fc_feats) with its criterion for such shapes."""
    ops.require_device(fc_feats, targets)
    w0, b0, w2, b2, w5, b5 = model.native_params()
    H, F = w0.shape
    C_ = w5.shape[0]
    if not ops.concept_shape_ok(F, H) or C_ % 4:
        raise ValueError('concept training step: fc_feat_dim (%d) and concept_mid_him (%d) must be multiples of 32 and '
                         'the number of concepts (%d) a multiple of 4' % (F, H, C_))
    if fc_feats.dtype == torch.float16:
        fc_feats = ops.f16_to_f32(fc_feats if fc_feats.stride(1) == 1 else fc_feats.contiguous())
    if fc_feats.stride(1) != 1 or fc_feats.stride(0) % 4 or fc_feats.data_ptr() % 16:
        fc_feats = fc_feats.contiguous()
    if targets.dtype not in (torch.uint8, torch.int64):
        targets = targets.to(torch.int64)
    targets = targets.contiguous()
    p = model.output[4].p
    keep, scale = None, 1.0
    if _keep_mask is not None:
        keep = _keep_mask.to(device=fc_feats.device, dtype=torch.uint8).reshape(fc_feats.shape[0], H).contiguous()
        scale = 1.0 / (1.0 - p) if p < 1.0 else 0.0
    elif model.training and p > 0.0:
        keep = torch.empty(fc_feats.shape[0], H, dtype=torch.uint8, device=fc_feats.device).bernoulli_(1.0 - p)
        scale = 1.0 / (1.0 - p) if p < 1.0 else 0.0
    return _ConceptLossFn.apply(fc_feats, targets, keep, scale, w0, b0, w2, b2, w5, b5)


def concept_train_step(model, optimizer, fc_feats, targets, grad_clip, _keep_mask=None):
    """One training iteration of train_cpt.py:79-89 on the device: loss (concept_loss_with_grad), backward, the
    elementwise clamp to +-grad_clip and Adam (one launch with a FusedClampAdam).  Returns the loss as a device scalar -
    the trainer decides when to read it.  Dropout follows the module's mode, as in the reference's loop
    (train_cpt.py:77): call model.train() first - `sample`, `sample_device` and Detector.tag leave the module in eval
    mode, and in eval mode this step draws no mask."""
    device = next(model.parameters()).device
    fc_feats, targets = ops.to_device(fc_feats, device), ops.to_device(targets, device)
    loss = concept_loss_with_grad(model, fc_feats, targets, _keep_mask)
    optimizer.zero_grad()
    loss.backward()
    clip_gradient(optimizer, grad_clip)
    optimizer.step()
    return loss.detach()


# ---------------------------------------------------------------------------- sentence classifier (train_sent_senti_cls_rnn.py:110-165)
class _SentClsLossFn(torch.autograd.Function):
    """Tokens to CrossEntropyLoss in one node.  Forward: ops.sent_cls_train_fwd (isc_sent_cls_train_fwd: the native
    forward's launch sequence with every intermediate kept, then isc_sent_cls_head_loss, which also leaves dz, d hid and the
    last layer's two gradients).  Backward: ops.sent_cls_bwd (isc_sent_cls_bwd: the whole reverse sweep in one call)."""

    @staticmethod
    def forward(ctx, tokens, lens, labels, masks, mask_scale, pad_id, *params):
        B, H = tokens.shape[0], params[2].shape[1]
        # dz is of the order 1 / B and the excitation's gradient carries a further 1 / H - below the f16 normal range at
        # any training size, where the split-f16 engine's planes keep bits relative to 2^-14, not to the element.  The
        # sweep is linear in dz (isc_lstm_bwd included): it runs on dz S with S the power of two that brings S / (B H)
        # into (2^-4, 2^-3], and the gradients leave times 1 / S - both exact.
        S = 2.0 ** (math.floor(math.log2(B * H)) - 3)
        st = ops.sent_cls_train_fwd(list(params), tokens, lens, labels, grad_scale=S, keep_masks=masks,
                                    mask_scale=mask_scale, pad_id=pad_id)
        ctx.state, ctx.unscale = st, 1.0 / S
        return st['loss'].reshape(()).clone()

    @staticmethod
    def backward(ctx, g):
        # (the last layer's two gradients are the forward's own tensors: unscaled out of place, so that a second backward
        #  through a retained graph starts from the same values; the other eleven are fresh from every sweep)
        grads = torch._foreach_mul(ops.sent_cls_bwd(ctx.state), g * ctx.unscale)      # g: the caller's d loss, a device scalar
        return (None,) * 6 + tuple(grads)


def _sent_cls_inputs(seqs, lengths):
    """(tokens [B, L] on the device, lens [B] int32 there) the way forward_native takes them: a device tensor of lengths
    is used as it is (L = the tensor's width, no host read), host ints give L = max(lengths)."""
    if torch.is_tensor(lengths) and lengths.is_cuda:
        return seqs, lengths.to(torch.int32).contiguous()
    lengths = [int(x) for x in lengths]
    return seqs[:, :max(lengths)], ops.upload(lengths, torch.int32, seqs.device)


def sent_cls_loss_with_grad(model, seqs, lengths, labels, _keep_masks=None):
    """nn.CrossEntropyLoss of model(seqs, lengths)[0] against `labels` [B] as a differentiable device scalar whose
    backward() fills the thirteen .grad, on the library's kernels.  seqs [B, L] int64 on the device (every entry a valid id;
    what stands behind a row's length changes no bit), lengths: host ints or a device tensor [B] (then nothing is read
    back).  In train mode with dropout_p > 0 the three uint8 keep-masks - embedding [L, B, W], LSTM output [L, B, H] (both
    time-major), head hidden layer [B, H] - are drawn the way the captioner draws its masks (bernoulli_ on torch's
    generator); `_keep_masks` replays given ones (tests).  Shapes: the native forward's (word_emb_dim % 32 == rnn_hid_dim
    % 32 == 0) and word_emb_dim <= 1024: ValueError otherwise - there is no quiet torch fallback; call model(seqs, lengths)
    with its criterion for such shapes."""
    ops.require_device(seqs, labels)
    params = model.native_params()
    (V, W), H = params[0].shape, params[2].shape[1]
    if not ops.sent_cls_train_shape_ok(W, H) or not 1 <= params[11].shape[0] <= 8:
        raise ValueError('sentence classifier training step: word_emb_dim (%d) and rnn_hid_dim (%d) must be multiples of 32, '
                         'word_emb_dim <= 1024 and 1..8 categories (%d)' % (W, H, params[11].shape[0]))
    if seqs.dim() != 2 or seqs.dtype != torch.int64:
        raise ValueError('seqs must be an int64 matrix [B, L]')
    tokens, lens = _sent_cls_inputs(seqs, lengths)
    if tokens.stride(1) != 1:
        tokens = tokens.contiguous()
    B, L = tokens.shape
    dev = tokens.device
    labels = labels.to(device=dev, dtype=torch.int64).contiguous()
    p = model.drop.p
    masks, scale = None, 1.0
    shapes = ((L * B, W), (L * B, H), (B, H))
    if _keep_masks is not None:
        masks = tuple(None if m is None else m.to(device=dev, dtype=torch.uint8).reshape(s).contiguous()
                      for m, s in zip(_keep_masks, shapes))
        scale = 1.0 / (1.0 - p) if p < 1.0 else 0.0
    elif model.training and p > 0.0:
        masks = tuple(torch.empty(s, dtype=torch.uint8, device=dev).bernoulli_(1.0 - p) for s in shapes)
        scale = 1.0 / (1.0 - p) if p < 1.0 else 0.0
    return _SentClsLossFn.apply(tokens, lens, labels, masks, scale, model.pad_id, *params)


def sent_cls_train_step(model, optimizer, seqs, lengths, labels, grad_clip):
    """One training iteration of train_sent_senti_cls_rnn.py:118-125 on the device: loss (sent_cls_loss_with_grad),
    backward, the elementwise clamp to +-grad_clip and Adam (one launch with a FusedClampAdam -
    model.get_optim_and_crit(lr, fused=True) - or torch.optim.Adam).  Returns the loss as a device scalar - the trainer
    decides when to read it.  Dropout follows the module's mode: call model.train() first (`sample` and
    sent_cls_evaluate leave the module in eval mode, and in eval mode this step draws no mask)."""
    device = next(model.parameters()).device
    seqs, labels = ops.to_device(seqs, device), ops.to_device(labels, device)
    loss = sent_cls_loss_with_grad(model, seqs, lengths, labels)
    optimizer.zero_grad()
    loss.backward()
    clip_gradient(optimizer, grad_clip)
    optimizer.step()
    return loss.detach()


@torch.no_grad()
def sent_cls_evaluate(model, loaders_by_category):
    """The validation pass of train_sent_senti_cls_rnn.py:128-165 on the native forward: `loaders_by_category` =
    {category: iterable of (labels [B], (caps [B, L], lengths))}.  The wrong predictions are counted on the device, one
    read-back per call.  -> {'all': {total_num, wrong_num, acc_rate}, 'by_category': {category: the same three}} with
    acc_rate = 100 - wrong_num / total_num * 100.  Leaves the module in eval mode, as `sample` does."""
    model.eval()
    device = next(model.parameters()).device
    names, totals, wrongs = [], [], []
    for senti, loader in loaders_by_category.items():
        total, wrong = 0, torch.zeros((), dtype=torch.int64, device=device)
        for labels, (caps, lengths) in loader:
            labels, caps = ops.to_device(labels, device), ops.to_device(caps, device)
            pred = model.forward_native(caps, lengths)[2]
            wrong += (pred.to(torch.int64) != labels).sum()
            total += int(labels.shape[0])
        names.append(senti)
        totals.append(total)
        wrongs.append(wrong)
    counts = torch.stack(wrongs).tolist() if wrongs else []
    rate = lambda w, t: 100 - w / t * 100
    by = {n: {'total_num': t, 'wrong_num': int(w), 'acc_rate': rate(int(w), t)} for n, t, w in zip(names, totals, counts)}
    t_all, w_all = sum(totals), sum(int(w) for w in counts)
    return {'all': {'total_num': t_all, 'wrong_num': w_all, 'acc_rate': rate(w_all, t_all)}, 'by_category': by}


# ---------------------------------------------------------------------------- image-sentiment detector (train_senti.py:68-108)
class _SentiDetLossFn(torch.autograd.Function):
    """Features to CrossEntropyLoss in one node.  Forward: ops.senti_det_train_fwd (isc_senti_det_train_fwd: the frozen
    forward's convolution launches with every intermediate kept, the tail and the head loss, which also leaves dz).
    Backward: ops.senti_det_bwd (isc_senti_det_bwd: the whole reverse sweep in one call; the small gradients meet the
    split-f16 planes times a power of two the sweep itself takes from their magnitude - no constant to choose here)."""

    @staticmethod
    def forward(ctx, feats, labels, keep, mask_scale, scale, *params):
        st = ops.senti_det_train_fwd(list(params), feats, labels, scale=scale, keep=keep, mask_scale=mask_scale)
        ctx.state = st
        # (the backward reads the parameters again - the flipped pack, the FC and senti_conv weights: saved as tensors, so
        #  that an in-place update between forward and backward raises autograd's version error)
        ctx.save_for_backward(*params)
        return st['loss'].reshape(())           # (a fresh tensor of this call: no copy)

    @staticmethod
    def backward(ctx, g):
        ctx.saved_tensors                        # (the version check)
        grads = torch._foreach_mul(ops.senti_det_bwd(ctx.state), g)      # g: the caller's d loss, a device scalar
        return (None,) * 5 + tuple(grads)


def _senti_det_feats(att_feats, device):
    """[B, h, w, F] fp32 contiguous on the device; float16 features are converted once per batch."""
    att_feats = ops.to_device(att_feats, device)
    if att_feats.dtype != torch.float32:
        att_feats = att_feats.to(torch.float32)
    return att_feats.contiguous()


def senti_det_loss_with_grad(model, att_feats, labels, _keep_mask=None, _scale=1.0):
    """nn.CrossEntropyLoss of model(att_feats)[0] against `labels` [B] as a differentiable device scalar whose backward()
    fills the .grad of every parameter, on the library's kernels.  att_feats [B, h, w, F] fp32 or float16 on the device,
    labels a device tensor or host ints.  In train mode with dropout_p > 0 the uint8 keep-mask [B, h, w, F >> convs]
    (channels-last) is drawn the way the captioner draws its masks (bernoulli_ on torch's generator); a label outside
    [0, categories) makes the loss and every gradient NaN (torch raises there; here nothing is read back); `_keep_mask` replays
    a given one and `_scale` multiplies the loss (tests).  Shapes: the native forward's (every conv's input width a multiple
    of 32, at most four convs and four FCs, 1..8 categories, h w <= 1024): ValueError otherwise - there is no quiet torch
    fallback; call model(att_feats) with its criterion for such shapes."""
    params = model.native_params()
    device = params[0].device
    att_feats = ops.to_device(att_feats, device)                # (a data.RowGather batch is expanded here)
    if att_feats.dim() != 4:
        raise ValueError('att_feats must be [B, h, w, F]')
    B, h, w, F = att_feats.shape
    n_convs = sum(1 for m in model.convs if isinstance(m, torch.nn.Conv2d))
    n_fcs, k = len(model.output), model.senti_conv.weight.shape[0]
    if not ops._lib.load().isc_senti_det_train_saved_bytes(B, h, w, F, n_convs, n_fcs) or not 1 <= k <= 8 or \
            model.convs[0].weight.shape[1] != F:
        raise ValueError('image-sentiment training step: [%d, %d, %d, %d] features with %d convs, %d FCs and %d categories '
                         'are outside the kernels (every conv input width a multiple of 32, h w <= 1024)'
                         % (B, h, w, F, n_convs, n_fcs, k))
    feats = _senti_det_feats(att_feats, device)
    if not torch.is_tensor(labels):
        labels = ops.upload([int(x) for x in labels], torch.int64, device)
    labels = ops.to_device(labels, device).to(torch.int64).contiguous()
    ops.require_device(feats, labels)
    p = model.convs.dropout.p
    CL = F >> n_convs
    keep, ms = None, 1.0
    if _keep_mask is not None:
        keep = _keep_mask.to(device=device, dtype=torch.uint8).reshape(B, h, w, CL).contiguous()
        ms = 1.0 / (1.0 - p) if p < 1.0 else 0.0
    elif model.training and p > 0.0:
        keep = torch.empty(B, h, w, CL, dtype=torch.uint8, device=device).bernoulli_(1.0 - p)
        ms = 1.0 / (1.0 - p) if p < 1.0 else 0.0
    return _SentiDetLossFn.apply(feats, labels, keep, ms, float(_scale), *params)


def senti_det_train_step(model, optimizer, att_feats, labels, grad_clip):
    """One training iteration of train_senti.py:78-85 on the device: loss (senti_det_loss_with_grad), backward, the
    elementwise clamp to +-grad_clip and Adam (one launch with a FusedClampAdam - model.get_optim_criterion(lr,
    fused=True) - or torch.optim.Adam).  Returns the loss as a device scalar - the trainer decides when to read it.
    Dropout follows the module's mode: call model.train() first (senti_det_evaluate and `sample` leave it in eval mode)."""
    loss = senti_det_loss_with_grad(model, att_feats, labels)
    optimizer.zero_grad()
    loss.backward()
    clip_gradient(optimizer, grad_clip)
    optimizer.step()
    return loss.detach()


@torch.no_grad()
def senti_det_evaluate(model, loader):
    """The test pass of train_senti.py:100-108 through sample_device (the native forward when the module's switch is on):
    `loader` yields (fns, att_feats, labels).  The correct predictions are counted on the device, one read-back per call.
    -> {'corr_num', 'all_num', 'corr_rate'}.  Leaves the module in eval mode, as `sample` does."""
    model.eval()
    device = next(model.parameters()).device
    corr, total = torch.zeros((), dtype=torch.int64, device=device), 0
    for _, att_feats, labels in loader:
        att_feats, labels = ops.to_device(att_feats, device), ops.to_device(labels, device)
        idx = model.sample_device(att_feats)[0]
        corr += (idx == labels.to(torch.int64)).sum()
        total += int(labels.shape[0])
    corr = int(corr)
    return {'corr_num': corr, 'all_num': total, 'corr_rate': corr / total if total else 0.0}


EVAL_PPL_SENTIS = ('positive', 'negative', 'neutral')      # eval_ppl.py:7


def eval_ppl(captions_file_prefix, data_type, lms, word2idx=None, sentis=EVAL_PPL_SENTIS):
    """eval_ppl.py's `compute_ppl` without SRILM: the perplexity of the result files train_rl.py:304-309 writes, per
    sentiment, under that sentiment's n-gram model -> {sentiment: ppl}, 0 where the file is missing or nothing was scored
    (as the reference's `except`).  `lms`: a rewards.NgramLMSet whose label l is the model of sentis[l].
      word2idx None: the id files `<prefix>_<senti>_<data_type>.txt` (ids, the <EOS> id last), for a set loaded from the
        *_id.kenlm.arpa files (eos_mode 'word');
      word2idx given: the word files `..._w.txt` (words, no <EOS>), for a set loaded from the *_w.sri files through the
        same word2idx (eos_mode 'end', unk_as_word False: SRILM's `ngram -ppl` without -unk skips unknown words).
    ppl = 10 ** (-sum score / sum n_scored) (rewards.lm_perplexity), SRILM's `ppl=` figure; host scorer, float64 sums.  An
    empty line is no sentence."""
    import os

    import numpy as np

    from .rewards import NgramLMSet, lm_perplexity
    if not isinstance(lms, NgramLMSet):
        raise ValueError('eval_ppl takes a rewards.NgramLMSet')
    if len(lms) < len(sentis):
        raise ValueError('eval_ppl: %d sentiments, %d language models' % (len(sentis), len(lms)))
    scores = {}
    for label, senti in enumerate(sentis):
        path = '%s_%s_%s%s.txt' % (captions_file_prefix, senti, data_type, '_w' if word2idx is not None else '')
        scores[senti] = 0
        if not os.path.exists(path):
            continue
        with open(path) as f:
            lines = [ln.split() for ln in f.read().splitlines() if ln.strip()]
        if not lines:
            continue
        if word2idx is not None:          # unknown words: an id no vocabulary holds; the row ends at an <EOS> no word is
            eos, sos = -1, -3
            rows = [[word2idx.get(w, -2) for w in ln] for ln in lines]
        else:                             # the lines carry their <EOS> id themselves
            eos = int(lines[0][-1]) if lms.eos is None else lms.eos
            sos = -3 if lms.sos is None else lms.sos
            rows = [[int(w) for w in ln] for ln in lines]
        T = max(len(r) for r in rows)
        hyps = np.full((len(rows), T), eos, dtype=np.int64)
        for i, r in enumerate(rows):
            hyps[i, :len(r)] = r
        labels = np.full(len(rows), label, dtype=np.int64)
        s, n_scored, n_oov = lms.score(hyps, labels, sos=sos, eos=eos)
        ppl = lm_perplexity(s, n_scored, n_oov, labels)[label]['ppl']
        scores[senti] = ppl if ppl == ppl else 0
    return scores
