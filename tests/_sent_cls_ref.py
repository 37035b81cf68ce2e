"""fp64 numpy restatement of the frozen sentence-sentiment classifier's eval-mode forward (sent_senti_cls.py:38-56 of the
reference, helper_nets.SentenceSentimentClassifier here) - the yardstick of the native forward (isc_sent_cls_fwd).

Packed semantics: a row of length n is the sequence of its first n tokens; nothing at or past position n is ever read.
Token weights are exactly 0 there, the arg-max takes the lowest index on ties, reward = weights where the prediction
equals the label and 0 elsewhere."""
import numpy as np

NAMES = ('word_embed.0.weight', 'rnn.weight_ih_l0', 'rnn.weight_hh_l0', 'rnn.bias_ih_l0', 'rnn.bias_hh_l0',
         'excitation.0.weight', 'excitation.0.bias', 'excitation.2.weight', 'excitation.2.bias',
         'sent_senti_cls.0.weight', 'sent_senti_cls.0.bias', 'sent_senti_cls.3.weight', 'sent_senti_cls.3.bias')


def _sig(x):
    return 1.0 / (1.0 + np.exp(-x))


def forward(sd, tokens, lens, labels=None, pad_to=None):
    """sd: {state_dict name: array}; tokens [B, >= max(lens)] ints; lens [B] ints >= 1.
    -> dict(logits [B,k], weights [B,T_out], feats [B,H], pred [B], reward [B,T_out] or None), all float64 / int64,
    T_out = pad_to or max(lens)."""
    p = [np.asarray(sd[n], dtype=np.float64) for n in NAMES]
    emb, w_ih, w_hh, b_ih, b_hh, e0w, e0b, e2w, e2b, c0w, c0b, c3w, c3b = p
    tokens = np.asarray(tokens)
    lens = [int(x) for x in lens]
    B, H = tokens.shape[0], w_hh.shape[1]
    T_out = int(pad_to) if pad_to is not None else max(lens)
    weights = np.zeros((B, T_out))
    feats = np.zeros((B, H))
    for b in range(B):
        h, c = np.zeros(H), np.zeros(H)
        for t in range(lens[b]):                              # the packed row: its own tokens and nothing else
            x = np.maximum(emb[int(tokens[b, t])], 0.0)
            g = w_ih @ x + b_ih + w_hh @ h + b_hh
            i, f, gg, o = _sig(g[:H]), _sig(g[H:2 * H]), np.tanh(g[2 * H:3 * H]), _sig(g[3 * H:])
            c = f * c + i * gg
            h = o * np.tanh(c)
            w = _sig(e2w @ np.maximum(e0w @ h + e0b, 0.0) + e2b).mean()
            weights[b, t] = w
            feats[b] += w * h
    logits = np.maximum(feats @ c0w.T + c0b, 0.0) @ c3w.T + c3b
    pred = np.argmax(logits, axis=1)                          # (first maximum: the lowest index on ties)
    reward = None
    if labels is not None:
        reward = np.where((pred == np.asarray(labels))[:, None], weights, 0.0)
    return dict(logits=logits, weights=weights, feats=feats, pred=pred.astype(np.int64), reward=reward)


def top2_margin(logits):
    s = np.sort(np.asarray(logits, dtype=np.float64), axis=1)
    return float((s[:, -1] - s[:, -2]).min())
