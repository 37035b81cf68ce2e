"""fp64 numpy restatement of the sentence-sentiment classifier's training loss and gradients (sent_senti_cls.py:38-56 in
train mode + nn.CrossEntropyLoss, train_sent_senti_cls_rnn.py:118-123) - the yardstick of isc_sent_cls_train_fwd /
isc_sent_cls_bwd and of their two kernels.  Pure numpy: nothing of the package under test.

Packed semantics: a row of length n is the sequence of its first n tokens - what stands at or past position n reaches no
sum (the recurrence is causal and every gradient entering a position t >= n is zero).  Dropout: three optional 0/1
keep-masks, time-major like the device's - embedding [L, B, W], LSTM output [L, B, H], head hidden layer [B, H] - scaled by
1 / (1 - p).  padding_idx: the <PAD> row of the embedding receives no gradient, wherever <PAD> stands.

`torch_loss` is the stock torch module's forward with the same masks applied by hand (any dtype): the fp32 CPU run of it
gives the error scale `e`, the fp64 run checks this restatement."""
import numpy as np

NAMES = ('word_embed.0.weight', 'rnn.weight_ih_l0', 'rnn.weight_hh_l0', 'rnn.bias_ih_l0', 'rnn.bias_hh_l0',
         'excitation.0.weight', 'excitation.0.bias', 'excitation.2.weight', 'excitation.2.bias',
         'sent_senti_cls.0.weight', 'sent_senti_cls.0.bias', 'sent_senti_cls.3.weight', 'sent_senti_cls.3.bias')


def _f64(x):
    return np.asarray(x, dtype=np.float64)


def _sig(x):
    return 1.0 / (1.0 + np.exp(-x))


def draw_inputs(seed, V, B, L, k=3, pad_id=0):
    """The cases' draw order: tokens, lengths (lens[0] = L, lens[1] = 1), labels; <PAD> behind every length, and one <PAD>
    at a VALID position of the full row (padding_idx must hold there too).  -> (tokens [B, L] int64, lens, labels int64)."""
    rng = np.random.default_rng(seed)
    tokens = rng.integers(0, V, (B, L)).astype(np.int64)
    lens = rng.integers(1, L + 1, B)
    lens[0] = L
    if B > 1:
        lens[1] = 1
    labels = rng.integers(0, k, B).astype(np.int64)
    tokens[np.arange(L)[None, :] >= lens[:, None]] = pad_id
    tokens[0, min(1, L - 1)] = pad_id
    return tokens, [int(x) for x in lens], labels


def head_loss(hid, w3, b3, labels, g=1.0, dtype=np.float64):
    """The k-way head with its loss in the max-subtracted form, evaluated in `dtype` (fp32: the error scale of the kernel's
    own formula).  -> dict(logits, pred, loss_rows, loss, wrong, dz [B, k], dhid, dw3, db3)."""
    hid, w3, b3 = (np.asarray(a, dtype=dtype) for a in (hid, w3, b3))
    labels = np.asarray(labels)
    B = hid.shape[0]
    z = hid @ w3.T + b3
    m = z.max(axis=1, keepdims=True)
    ex = np.exp(z - m)
    se = ex.sum(axis=1, keepdims=True)
    rows = (m[:, 0] - z[np.arange(B), labels]) + np.log(se[:, 0])
    onehot = np.zeros_like(z)
    onehot[np.arange(B), labels] = 1
    dz = (ex / se - onehot) * dtype(g / B)
    pred = np.argmax(z, axis=1)
    return dict(logits=z, pred=pred, loss_rows=rows, loss=rows.sum(dtype=dtype) / dtype(B), wrong=int((pred != labels).sum()),
                dz=dz, dhid=dz @ w3, dw3=dz.T @ hid, db3=dz.sum(axis=0))


def pool_bwd(dfeats, e2, o, weights, lens, dtype=np.float64):
    """dfeats [B, H], e2 / o [L, B, H], weights [B, >= L] -> (de2, d_o [L, B, H], dw [B, L]); zeros at and past every length."""
    dfeats, e2, o, weights = (np.asarray(a, dtype=dtype) for a in (dfeats, e2, o, weights))
    L, B, H = e2.shape
    valid = (np.arange(L)[:, None] < np.asarray(lens)[None, :])                   # [L, B]
    dw = np.einsum('bh,tbh->tb', dfeats, o).astype(dtype) * valid
    s = dtype(1) / (dtype(1) + np.exp(-e2))
    de2 = (dw / dtype(H))[:, :, None] * (s * (dtype(1) - s)) * valid[:, :, None]
    d_o = weights[:, :L].T[:, :, None] * dfeats[None] * valid[:, :, None]
    return de2, d_o, dw.T.copy()


def forward_backward(sd, tokens, lens, labels, pad_id=0, masks=None, dropout_p=0.0):
    """-> (loss, {name: gradient}, aux) in fp64.  aux: logits, pred, weights [B, L], a_ex0 [L, B, H] (excitation.0's
    pre-activation) with `valid` [L, B], a_hid [B, H] (sent_senti_cls.0's) - the tensors of the input condition."""
    emb, w_ih, w_hh, b_ih, b_hh, e0w, e0b, e2w, e2b, c0w, c0b, c3w, c3b = (_f64(sd[n]) for n in NAMES)
    tokens = np.asarray(tokens)
    lens = np.asarray([int(x) for x in lens])
    labels = np.asarray(labels)
    B, H, W = tokens.shape[0], w_hh.shape[1], emb.shape[1]
    L = int(lens.max())
    tokens = tokens[:, :L]
    scale = 1.0 / (1.0 - dropout_p) if masks is not None else 1.0
    one = lambda m, shape: np.ones(shape) if m is None else _f64(m).reshape(shape) * scale
    mE, mO, mH = (one(m, s) for m, s in zip(masks or (None, None, None), ((L, B, W), (L, B, H), (B, H))))
    valid = (np.arange(L)[:, None] < lens[None, :]).astype(np.float64)            # [L, B]

    x = np.maximum(emb[tokens.T], 0.0) * mE                                       # [L, B, W]
    h, c = np.zeros((B, H)), np.zeros((B, H))
    hs, cs, gs = [], [], []
    for t in range(L):
        g = x[t] @ w_ih.T + b_ih + h @ w_hh.T + b_hh
        i, f, gg, og = _sig(g[:, :H]), _sig(g[:, H:2 * H]), np.tanh(g[:, 2 * H:3 * H]), _sig(g[:, 3 * H:])
        c = f * c + i * gg
        h = og * np.tanh(c)
        hs.append(h); cs.append(c); gs.append((i, f, gg, og))
    hs = np.stack(hs)                                                             # raw h [L, B, H]
    o = hs * mO * valid[:, :, None]
    a1 = o @ e0w.T + e0b
    e1 = np.maximum(a1, 0.0)
    s = _sig(e1 @ e2w.T + e2b)
    w = s.mean(axis=2) * valid                                                    # [L, B]
    feats = np.einsum('tb,tbh->bh', w, o)
    a_hid = feats @ c0w.T + c0b
    hid = np.maximum(a_hid, 0.0) * mH
    hl = head_loss(hid, c3w, c3b, labels)

    G = {NAMES[11]: hl['dw3'], NAMES[12]: hl['db3']}
    dphid = hl['dhid'] * mH * (a_hid > 0)
    G[NAMES[9]], G[NAMES[10]] = dphid.T @ feats, dphid.sum(axis=0)
    dfeats = dphid @ c0w
    dw = np.einsum('bh,tbh->tb', dfeats, o) * valid
    de2 = (dw / H)[:, :, None] * s * (1.0 - s)
    d_o = w[:, :, None] * dfeats[None]
    G[NAMES[7]], G[NAMES[8]] = np.einsum('tbi,tbj->ij', de2, e1), de2.sum(axis=(0, 1))
    de1 = (de2 @ e2w) * (a1 > 0)
    G[NAMES[5]], G[NAMES[6]] = np.einsum('tbi,tbj->ij', de1, o), de1.sum(axis=(0, 1))
    d_o = (d_o + de1 @ e0w) * valid[:, :, None]
    dh_out = d_o * mO
    dWih, dWhh, db = np.zeros_like(w_ih), np.zeros_like(w_hh), np.zeros(4 * H)
    demb = np.zeros_like(emb)
    dh_next, dc_next = np.zeros((B, H)), np.zeros((B, H))
    for t in range(L - 1, -1, -1):
        i, f, gg, og = gs[t]
        c_prev = cs[t - 1] if t else np.zeros((B, H))
        h_prev = hs[t - 1] if t else np.zeros((B, H))
        dh = dh_out[t] + dh_next
        tc = np.tanh(cs[t])
        dc = dh * og * (1.0 - tc * tc) + dc_next
        dg = np.concatenate([dc * gg * i * (1 - i), dc * c_prev * f * (1 - f), dc * i * (1 - gg * gg),
                             dh * tc * og * (1 - og)], axis=1)
        dWih += dg.T @ x[t]
        dWhh += dg.T @ h_prev
        db += dg.sum(axis=0)
        dx = (dg @ w_ih) * mE[t] * (emb[tokens[:, t]] > 0)
        for b in range(B):
            if tokens[b, t] != pad_id:
                demb[tokens[b, t]] += dx[b]
        dh_next, dc_next = dg @ w_hh, dc * f
    G[NAMES[0]], G[NAMES[1]], G[NAMES[2]], G[NAMES[3]], G[NAMES[4]] = demb, dWih, dWhh, db, db.copy()
    aux = dict(logits=hl['logits'], pred=hl['pred'], weights=w.T.copy(), a_ex0=a1, valid=valid, a_hid=a_hid, hid=hid,
               feats=feats, o=o, e2=e1 @ e2w.T + e2b, dfeats=dfeats)
    return float(hl['loss']), G, aux


def relu_margin(aux):
    """The input condition of a GPU case: the smallest |pre-activation| of excitation.0 at a valid position and of
    sent_senti_cls.0, each relative to its tensor's largest magnitude (a ReLU unit within 1e-5 of zero can flip between
    fp32 and fp64 and move a gradient by a whole term).  -> the smaller of the two ratios."""
    a1 = np.abs(aux['a_ex0'][aux['valid'] > 0])
    ah = np.abs(aux['a_hid'])
    return float(min(a1.min() / a1.max(), ah.min() / ah.max()))


def find_seed(sd, V, B, L, k=3, first=7, tries=64, floor=1e-5):
    for seed in range(first, first + tries):
        tokens, lens, labels = draw_inputs(seed, V, B, L, k)
        if relu_margin(forward_backward(sd, tokens, lens, labels)[2]) >= floor:
            return seed
    raise AssertionError('no seed in [%d, %d) meets the ReLU condition' % (first, first + tries))


def torch_loss(m, tokens, lens, labels, masks=None, dropout_p=0.0):
    """CrossEntropyLoss of the stock module's forward (helper_nets.SentenceSentimentClassifier layers, in the module's own
    dtype) with the keep-masks applied by hand.  -> (loss tensor, logits)."""
    import torch
    dt = m.rnn.weight_hh_l0.dtype
    tokens = torch.as_tensor(np.asarray(tokens))
    lens_t = torch.as_tensor(np.asarray([int(x) for x in lens]))
    L = int(lens_t.max())
    tokens = tokens[:, :L]
    B = tokens.shape[0]
    scale = 1.0 / (1.0 - dropout_p) if masks is not None else 1.0
    mk = lambda a, shape: 1.0 if a is None else torch.as_tensor(np.asarray(a)).reshape(shape).to(dt) * scale
    mE, mO, mH = masks or (None, None, None)
    x = torch.relu(m.word_embed[0](tokens)).transpose(0, 1) * mk(mE, (L, B, -1))              # [L, B, W]
    out, _ = m.rnn(x)
    valid = (torch.arange(L).unsqueeze(1) < lens_t.unsqueeze(0)).to(dt).unsqueeze(-1)          # [L, B, 1]
    out = out * valid * mk(mO, (L, B, -1))
    w = (m.excitation(out) * valid).mean(dim=-1)                                               # [L, B]
    feats = (w.unsqueeze(-1) * out).sum(dim=0)
    hid = torch.relu(m.sent_senti_cls[0](feats)) * mk(mH, (B, -1))
    logits = m.sent_senti_cls[3](hid)
    return torch.nn.functional.cross_entropy(logits, torch.as_tensor(np.asarray(labels))), logits


def yardstick(got, ref64, e):
    """The project's bound: max |got - fp64| <= 4 max(e, 2^-23 max |fp64|).  -> (err, bound)."""
    ref64 = _f64(ref64)
    err = float(np.max(np.abs(_f64(got) - ref64))) if ref64.size else 0.0
    return err, 4.0 * max(float(e), 2.0 ** -23 * float(np.max(np.abs(ref64))) if ref64.size else 0.0)
