"""fp64 reference of the roll-out's token constraints (include/insenticap_hip.h: isc_decode_constraints), the beam
search's rules (captioner.py:394-399) carried to the roll-out.  Test code only.

At step t a live row may not choose: <PAD>, <SOS>, <UNK> under `suppress_special` (only when pad_id != eos_id); the token
fed into the step under `decoding_constraint` (seq[b, t-1]; <SOS> at t = 0); <EOS> while t < min_len.  Greedy = arg-max
over the allowed ids, ties to the smaller id.  Sampled = the filtered sampler of tests/_sample_filter_ref.py on the
REDUCED row (the allowed ids in vocabulary order), tokens mapped back."""
import numpy as np
import torch

import _sample_filter_ref as ref
from insenticap_model_amd import synth
from oracle import captioner_oracle as O

T = 12
KEYS = ('fc_feats', 'att_feats', 'cpt_words', 'senti_words', 'senti_labels')


def setup(V, dtype=torch.float64):
    """The inputs of the beam-1 identity: <UNK> and <EOS> made likely, so that the plain greedy roll-out emits <UNK>,
    stutters and ends early."""
    st = synth.TINY_SETTINGS
    w = synth.make_weights(V, st, seed=5)
    i2w = synth.make_idx2word(V)
    w['classifier.bias'] = w['classifier.bias'].copy()
    w['classifier.bias'][i2w.index('<UNK>')] += 4
    w['classifier.bias'][i2w.index('<EOS>')] += 3
    d = synth.make_inputs(8, V, st, regions=6, seq_len=T, seed=15)
    ins = [torch.from_numpy(np.asarray(d[k])) for k in KEYS]
    ins = [x.to(dtype) if x.is_floating_point() else x for x in ins]
    return st, w, i2w, O.to_params(w, dtype=dtype), O.Ids(i2w, synth.SENTIMENT_CATEGORIES), ins


def allowed(V, oid, prev, t, suppress_special=False, decoding_constraint=0, min_len=0):
    """Boolean [V]: the ids a live row may choose at step t, `prev` being the token fed into the step."""
    ok = np.ones(V, dtype=bool)
    if suppress_special and oid.pad != oid.eos:
        ok[[oid.pad, oid.sos, oid.unk]] = False
    if decoding_constraint:
        ok[int(prev)] = False
    if t < min_len:
        ok[oid.eos] = False
    return ok


def allowed_from_ids(V, banned):
    ok = np.ones(V, dtype=bool)
    ok[[int(i) for i in banned if i >= 0]] = False
    return ok


def greedy(x, ok):
    """(arg-max over the allowed ids - the smaller id on ties -, fp64 margin to the second-best allowed id)."""
    x = np.asarray(x, dtype=np.float64)
    ids = np.nonzero(ok)[0]
    order = ref.ranking(x[ids])
    return int(ids[order[0]]), float(x[ids[order[0]]] - x[ids[order[1]]])


class RowCheck:
    """_sample_filter_ref.RowCheck over the reduced row; tokens in, tokens out are vocabulary ids."""

    def __init__(self, x, ok, u, tau=1.0, top_k=0, top_p=1.0):
        self.ids = np.nonzero(ok)[0]
        self.pos = -np.ones(len(ok), dtype=np.int64)
        self.pos[self.ids] = np.arange(len(self.ids))
        k = top_k if 0 < top_k < len(ok) else 0       # (top-k ranks the allowed tokens; k >= V: off, as on the device)
        self.rc = ref.RowCheck(np.asarray(x, dtype=np.float64)[self.ids], u, tau, k, top_p)
        self.strict, self.n_lo, self.n_hi = self.rc.strict, self.rc.n_lo, self.rc.n_hi

    def token_ok(self, tok):
        return self.pos[int(tok)] >= 0 and self.rc.token_ok(self.pos[int(tok)])

    def ref_token(self):
        return int(self.ids[self.rc.ref_token()])

    def sampling_logprob(self, tok):
        return None if self.pos[int(tok)] < 0 else self.rc.sampling_logprob(self.pos[int(tok)])


def rollout(prm, oid, inputs, T, sample_max=1, suppress_special=False, decoding_constraint=0, min_len=0,
            uniforms=None, tau=1.0, top_k=0, top_p=1.0, replay=None):
    """The oracle's roll-out loop (oracle.captioner_oracle.prologue / step) under the constraints.  sample_max=1: greedy;
    0: the reference draw for `uniforms` [B,T] - or, with `replay` [B,T], those raw tokens are fed instead and only the
    rows are recorded.  Returns dict(seq, raw, logprobs, masks, margins [B,T] (greedy: best minus second-best allowed,
    inf where the row is finished), rows = per executed step the [B,V] fp64 log-prob rows, fed = per step the fed
    tokens, live = per step the unfinished flags)."""
    fc = inputs[0]
    B = fc.shape[0]
    with torch.no_grad():
        P = O.prologue(prm, oid, 'rl', *inputs, None, 0.5)
        state = O.init_state(prm, B)
        it = torch.full((B,), oid.sos, dtype=torch.long)
        unf = np.ones(B, dtype=bool)
        seq, raw = np.zeros((B, T), dtype=np.int64), np.zeros((B, T), dtype=np.int64)
        lps, masks = np.zeros((B, T)), np.zeros((B, T))
        margins = np.full((B, T), np.inf)
        rows, fed, live = [], [], []
        for t in range(T):
            logp, state, _ = O.step(prm, it, state, P.fc_e, P.att_e, P.p_att, P.words_e, P.p_words, P.label_e, None, 0.5)
            x = logp.double().numpy()
            V = x.shape[1]
            rows.append(x)
            fed.append(it.numpy().copy())
            live.append(unf.copy())
            for b in range(B):
                ok = allowed(V, oid, int(it[b]), t, suppress_special, decoding_constraint, min_len)
                if replay is not None:
                    raw[b, t] = int(replay[b, t])
                elif sample_max:
                    raw[b, t], m = greedy(x[b], ok)
                    if unf[b]:
                        margins[b, t] = m
                else:
                    raw[b, t] = RowCheck(x[b], ok, float(uniforms[b, t]), tau, top_k, top_p).ref_token()
            lps[:, t] = x[np.arange(B), raw[:, t]]
            masks[:, t] = unf
            seq[:, t] = raw[:, t] * unf
            it = torch.from_numpy(seq[:, t].copy())
            unf = unf & (seq[:, t] != oid.eos)
            if not unf.any():
                break
    return dict(seq=seq, raw=raw, logprobs=lps, masks=masks, margins=margins, rows=rows, fed=fed, live=live)
