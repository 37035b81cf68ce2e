"""numpy restatement of the sentiment-word reward (include/insenticap_hip.h: isc_sw_reward, isc_sw_decay) and of what
rewards.senti_word_stats reports.  Test code only: written from the header's value rule, not from the kernel."""
import numpy as np

NAN32 = np.float32(np.nan)


def table(lexicon, V, n_labels):
    """{label: {word: weight}} -> (weights float64 [n_labels, V], state uint8 [n_labels, V])."""
    weights = np.zeros((n_labels, V), dtype=np.float64)
    state = np.zeros((n_labels, V), dtype=np.uint8)
    for lab, words in lexicon.items():
        for w, x in words.items():
            weights[lab, w] = x
            state[lab, w] = 1
    return weights, state


def reward(tok, labels, weights, state, flag=0.0, reward_io=None, accumulate=False, mark=True):
    """-> (reward_io float32 [N, T], reward64 float64 [N, T], row_hits int32 [N], state after the launch).  Position by
    position, as the header states it: an id is compared before it is an index; membership is the state."""
    tok, labels = np.asarray(tok, dtype=np.int64), np.asarray(labels, dtype=np.int64)
    N, T = tok.shape
    n_labels, V = weights.shape
    r64 = np.zeros((N, T), dtype=np.float64)
    r32 = np.zeros((N, T), dtype=np.float32) if reward_io is None else np.array(reward_io, dtype=np.float32)
    hits = np.zeros(N, dtype=np.int32)
    after = state.copy()
    f32 = np.float32(flag)
    for i in range(N):
        lab = int(labels[i])
        if not 0 <= lab < n_labels:
            r64[i], r32[i], hits[i] = np.nan, NAN32, -1
            continue
        for j in range(T):
            w, t = 0.0, int(tok[i, j])
            if 0 <= t < V and state[lab, t] != 0:
                w = weights[lab, t]
                hits[i] += 1
                if mark:
                    after[lab, t] = 2
            r64[i, j] = w
            wf = np.float32(w)
            # (two float32 roundings: the product, then the sum - numpy scalars do not fuse)
            r32[i, j] = np.float32(r32[i, j] + np.float32(f32 * wf)) if accumulate else wf
    return r32, r64, hits, after


def decay(weights, state, factor):
    """The reference's loop (decoder.py:174-176) on the marked words: Python floats, `w *= factor`."""
    weights, state = weights.copy(), state.copy()
    for lab, w in zip(*np.nonzero(state == 2)):
        x = float(weights[lab, w])
        x *= factor
        weights[lab, w] = x
        state[lab, w] = 1
    return weights, state


def accur(state_before, state_after):
    """{label: set of words} that a launch marked."""
    out = {}
    for lab, w in zip(*np.nonzero((state_after == 2) & (state_before != 2))):
        out.setdefault(int(lab), set()).add(int(w))
    return out


def stats(tok, labels, weights, state):
    n_labels = weights.shape[0]
    member = (state != 0).astype(np.uint8)
    _, _, hits, after = reward(tok, labels, weights, member)
    labels = np.asarray(labels)
    return {lab: {'captions': int((labels == lab).sum()), 'with_word': int((hits[labels == lab] > 0).sum()),
                  'hits': int(hits[labels == lab].sum()), 'distinct': int((after[lab] == 2).sum())}
            for lab in range(n_labels)}


def powers(base, n):
    """[base ** 0 .. base ** (n - 1)] formed by repeated multiplication in Python, as the decay forms them."""
    out, x = [], 1.0
    for _ in range(n):
        out.append(x)
        x *= base
    return out


def accumulate_case(seed=0, n=4096):
    """The accumulate case of the GPU test: base standard-normal float32 [n], weights 0.9 ** k, k in [0, 12), flag 0.05 ->
    (base, k, weights by k)."""
    rng = np.random.default_rng(seed)
    base = rng.standard_normal(n).astype(np.float32)
    k = rng.integers(0, 12, size=n)
    return base, k, np.asarray(powers(0.9, 12), dtype=np.float64)
