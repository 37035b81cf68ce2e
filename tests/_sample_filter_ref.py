"""fp64 numpy reference of the filtered sampler (temperature / top-k / top-p), the semantics of
include/insenticap_hip.h: isc_rollout_finalize_filtered.  Test code only.

Per row: tokens ranked by raw logit x (largest first, ties to the smaller id); mass w_i = exp((x_i - max x) / T);
top-k keeps the first k ranks (0 or >= V: off); top-p, on the survivors with summed mass W_k, keeps rank j iff the summed
mass of the ranks < j is < top_p * W_k (rank 0 always; >= 1: off); the draw is the first kept id, in VOCABULARY order,
whose cumulative kept mass exceeds u * (kept mass)."""
import numpy as np

EPS_MASS = 2e-6          # the project's bar on a normalised fp32 cumulative mass (tests/test_gpu_sampling.py)


def ranking(x):
    """Token ids by rank.  x: [V] or [B,V]."""
    x = np.asarray(x, dtype=np.float64)
    return np.argsort(-x, axis=-1, kind='stable')       # stable: ties keep the smaller id in front


def masses(x, tau):
    x = np.asarray(x, dtype=np.float64)
    return np.exp((x - x.max()) / float(tau))


def kept_count(x, tau, top_k, top_p, order=None):
    """Length of the kept rank prefix of one row."""
    x = np.asarray(x, dtype=np.float64)
    V = x.shape[0]
    order = ranking(x) if order is None else order
    ws = masses(x, tau)[order]
    n_k = V if (top_k == 0 or top_k >= V) else int(top_k)
    if top_p >= 1.0:
        return n_k
    ws = ws[:n_k]
    excl = np.cumsum(ws) - ws
    return max(1, int((excl < top_p * ws.sum()).sum()))


def kept_set(x, tau, top_k, top_p, order=None):
    order = ranking(x) if order is None else order
    return order[:kept_count(x, tau, top_k, top_p, order)]


def interval(x, tau, kept_ids, tok):
    """(lo, hi, log(w_tok / W_K)) of `tok`'s slot of the normalised CDF over the kept set in vocabulary order, or None when
    `tok` is not kept."""
    x = np.asarray(x, dtype=np.float64)
    mask = np.zeros(x.shape[0], dtype=bool)
    mask[kept_ids] = True
    if not mask[tok]:
        return None
    w = np.where(mask, masses(x, tau), 0.0)
    W = w.sum()
    hi = w[:tok + 1].sum() / W
    return hi - w[tok] / W, hi, float(np.log(w[tok] / W))


def draw(x, u, tau=1.0, top_k=0, top_p=1.0, order=None):
    """The reference's token for uniform u."""
    x = np.asarray(x, dtype=np.float64)
    mask = np.zeros(x.shape[0], dtype=bool)
    mask[kept_set(x, tau, top_k, top_p, order)] = True
    cdf = np.cumsum(np.where(mask, masses(x, tau), 0.0))
    hit = np.nonzero(cdf > float(u) * cdf[-1])[0]
    return int(hit[0]) if hit.size else int(np.nonzero(mask)[0][-1])


class RowCheck:
    """What the fp64 reference says about one row and one parameter set: the kept prefix, the prefixes for top_p -+ 2e-6
    (strict row: all three equal), and the verdict on a device token."""

    def __init__(self, x, u, tau, top_k, top_p, order=None):
        self.x, self.u, self.tau = np.asarray(x, dtype=np.float64), float(u), float(tau)
        self.order = ranking(self.x) if order is None else order
        self.n = kept_count(self.x, tau, top_k, top_p, self.order)
        if top_p >= 1.0:
            self.n_lo = self.n_hi = self.n                           # no mass boundary
        else:
            self.n_lo = kept_count(self.x, tau, top_k, top_p - EPS_MASS, self.order)
            self.n_hi = kept_count(self.x, tau, top_k, min(top_p + EPS_MASS, 1.0), self.order)
        self.strict = self.n_lo == self.n_hi
        self.top_k, self.top_p = top_k, top_p

    def ref_token(self):
        return draw(self.x, self.u, self.tau, self.top_k, self.top_p, self.order)

    def near_boundary(self):
        """u within 2e-6 of a boundary of the reference token's CDF slot."""
        lo, hi, _ = interval(self.x, self.tau, self.order[:self.n], self.ref_token())
        return min(abs(self.u - lo), abs(self.u - hi)) <= EPS_MASS

    def _ok(self, n, tok):
        iv = interval(self.x, self.tau, self.order[:n], tok)
        return iv is not None and iv[0] - EPS_MASS <= self.u <= iv[1] + EPS_MASS

    def token_ok(self, tok):
        """Strict row: tok in K and u inside its CDF slot over K widened by 2e-6.  Relaxed row: the same for SOME prefix
        between the two neighbours."""
        tok = int(tok)
        if self.strict:
            return self._ok(self.n, tok)
        return any(self._ok(n, tok) for n in range(self.n_lo, self.n_hi + 1))

    def sampling_logprob(self, tok):
        iv = interval(self.x, self.tau, self.order[:self.n], int(tok))
        return None if iv is None else iv[2]
