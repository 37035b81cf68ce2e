"""fp64 numpy restatement of the concept detector (concept_detector.py, train_cpt.py:79-89, preprocess.py:288-301): the
reference the kernels of csrc/concept.hip and the module's paths are held to.  Pure numpy / Python: no torch, nothing of
the package under test.

Parameters: a dict by the state_dict's names ('output.0.weight' ... 'output.5.bias')."""
import numpy as np

NAMES = ('output.0.weight', 'output.0.bias', 'output.2.weight', 'output.2.bias', 'output.5.weight', 'output.5.bias')


def _f64(x):
    return np.asarray(x, dtype=np.float64)


def sigmoid(z):
    z = _f64(z)
    with np.errstate(over='ignore'):
        return np.where(z >= 0, 1.0 / (1.0 + np.exp(-np.abs(z))), np.exp(-np.abs(z)) / (1.0 + np.exp(-np.abs(z))))


def softplus(x):
    x = _f64(x)
    return np.maximum(x, 0.0) + np.log1p(np.exp(-np.abs(x)))


def forward(params, feats, keep_mask=None, dropout_p=0.0):
    """-> dict(h1, h2 (behind ReLU and the optional inverted dropout), logits, probs), all fp64."""
    p = {k: _f64(v) for k, v in params.items()}
    x = _f64(feats)
    h1 = np.maximum(x @ p[NAMES[0]].T + p[NAMES[1]], 0.0)
    h2 = np.maximum(h1 @ p[NAMES[2]].T + p[NAMES[3]], 0.0)
    if keep_mask is not None:
        h2 = h2 * _f64(keep_mask) * (1.0 / (1.0 - dropout_p))
    z = h2 @ p[NAMES[4]].T + p[NAMES[5]]
    return {'h1': h1, 'h2': h2, 'logits': z, 'probs': sigmoid(z)}


def topk(logits, num):
    """The ordering rule of isc_concept_head: larger logit first, lower index on equal logits, -0.0 == +0.0, +-inf ordinary,
    NaN below every number (lower index first among NaNs).  -> int64 [B, num]."""
    z = np.asarray(logits)
    out = np.zeros((z.shape[0], num), dtype=np.int64)
    for b in range(z.shape[0]):
        row = z[b].astype(np.float64)
        nan = np.isnan(row)
        neg = np.where(nan, 0.0, -row)
        out[b] = np.lexsort((np.arange(row.size), neg, nan))[:num]       # last key first: NaN flag, -value, index
    return out


def topk_gap(logits, num):
    """Smallest difference between neighbours among the num + 1 largest logits of any row (num = C: among all)."""
    z = -np.sort(-_f64(logits), axis=1)
    k = min(num + 1, z.shape[1])
    return float(np.min(z[:, :k - 1] - z[:, 1:k])) if k > 1 else float('inf')


def hits(idx, targets):
    """(hits [B], n_true [B]): picked concepts that are set in the 0/1 matrix, and how many are set."""
    t = np.asarray(targets) != 0
    return np.asarray([int(t[b, idx[b]].sum()) for b in range(t.shape[0])]), t.sum(axis=1).astype(np.int64)


def loss(logits, targets, g=1.0):
    """-> (term of the set targets, term of the unset ones, loss, dz = (sigmoid(z) - t) g / (B C)), stable form."""
    z, t = _f64(logits), (np.asarray(targets) != 0).astype(np.float64)
    n = z.size
    t1 = float(np.sum(t * softplus(-z)) / n)
    t2 = float(np.sum((1.0 - t) * softplus(z)) / n)
    return t1, t2, t1 + t2, (sigmoid(z) - t) * (g / n)


def backward(params, feats, targets, keep_mask=None, dropout_p=0.0):
    """-> (loss, {name: gradient}) of MultiLabelClsLoss(forward(feats), targets), fp64."""
    p = {k: _f64(v) for k, v in params.items()}
    x = _f64(feats)
    f = forward(params, feats, keep_mask, dropout_p)
    _, _, L, dz = loss(f['logits'], targets)
    g = {NAMES[4]: dz.T @ f['h2'], NAMES[5]: dz.sum(axis=0)}
    dh2 = dz @ p[NAMES[4]]
    if keep_mask is not None:
        dh2 = dh2 * _f64(keep_mask) * (1.0 / (1.0 - dropout_p))
    dp2 = dh2 * ((f['h1'] @ p[NAMES[2]].T + p[NAMES[3]]) > 0)
    g[NAMES[2]], g[NAMES[3]] = dp2.T @ f['h1'], dp2.sum(axis=0)
    dp1 = (dp2 @ p[NAMES[2]]) * (f['h1'] > 0)
    g[NAMES[0]], g[NAMES[1]] = dp1.T @ x, dp1.sum(axis=0)
    return L, g


def adam_steps(params, grads_fn, n_steps, lr, clip, betas=(0.9, 0.999), eps=1e-8):
    """clip_gradient (elementwise clamp) + torch.optim.Adam, n_steps times; grads_fn(params) -> (loss, grads).
    -> (params after, [loss per step], [grads per step])."""
    p = {k: _f64(v).copy() for k, v in params.items()}
    m = {k: np.zeros_like(v) for k, v in p.items()}
    v2 = {k: np.zeros_like(v) for k, v in p.items()}
    losses, all_g = [], []
    for step in range(1, n_steps + 1):
        L, g = grads_fn(p)
        losses.append(L)
        all_g.append(g)
        for k in p:
            gk = np.clip(g[k], -clip, clip)
            m[k] = betas[0] * m[k] + (1 - betas[0]) * gk
            v2[k] = betas[1] * v2[k] + (1 - betas[1]) * gk * gk
            mhat = m[k] / (1 - betas[0] ** step)
            p[k] = p[k] - lr * mhat / (np.sqrt(v2[k]) / np.sqrt(1 - betas[1] ** step) + eps)
    return p, losses, all_g


def senti_words(concept_idx, lists, n_out, pad_id):
    """preprocess.py:288-301 + the collates' fill_(pad_index), restated by hand: `lists[c]` = [(word id, score), ...] of
    concept index c (missing / out of range: nothing).  Python floats are IEEE doubles and the sums run in list order, so
    this is bit for bit what the host pipeline computes.  -> int64 [B, n_out]."""
    out = np.full((len(concept_idx), n_out), pad_id, dtype=np.int64)
    for b, row in enumerate(concept_idx):
        sentis = []
        for c in row:
            c = int(c)
            if 0 <= c < len(lists):
                sentis.extend(lists[c])
        tmp = {}
        for w, s in sentis:
            tmp[w] = tmp.get(w, 0.0) + float(s)
        order = sorted(tmp.items(), key=lambda q: q[1], reverse=True)      # stable: ties keep first-occurrence order
        ids = [w for w, _ in order][:20][:n_out]
        out[b, :len(ids)] = ids
    return out


def yardstick(got, ref64, e):
    """The project's bound (tests/test_gpu_sent_cls.py): max |got - fp64| <= 4 max(e, 2^-23 max |fp64|).  -> (err, bound)."""
    ref64 = _f64(ref64)
    err = float(np.max(np.abs(_f64(got) - ref64))) if ref64.size else 0.0
    return err, 4.0 * max(float(e), 2.0 ** -23 * float(np.max(np.abs(ref64))) if ref64.size else 0.0)
