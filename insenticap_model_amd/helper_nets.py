"""The two frozen helper networks of the RL step, restated as plain PyTorch-ROCm modules, and the concept detector of the
pre-stage (ConceptDetector below: its eval forward runs on the library's kernels by default, isc_concept_fwd).

They are harness dependencies of the hot path, not part of it:
`Detector` only ever runs them in eval mode without gradients (decoder.py:31-32,83,133-136 and
self_critical/utils.py:120-151), their dense conv / LSTM work goes to MIOpen / rocBLAS through
stock torch ops, and only their *outputs* (sentiment labels, per-token reward weights) enter the
hand-written kernels.  Parameter names and shapes equal the reference's, so its checkpoints load
(train_rl.py:42-53,88-97).  The sentence classifier has an opt-in native forward on the library's own kernels
(`enable_native`, include/insenticap_hip.h: isc_sent_cls_fwd), the image detector one on the library's implicit-GEMM
convolution (isc_senti_det_fwd); both off by default.

* SentimentDetector            /root/reference/models/sentiment_detector.py:5-64
* SentenceSentimentClassifier  /root/reference/models/sent_senti_cls.py:6-72
* ConceptDetector, MultiLabelClsLoss  /root/reference/models/concept_detector.py:5-58
"""
import torch
import torch.nn as nn


class SentimentDetector(nn.Module):
    """Image-level sentiment from the [B,h,w,F] feature grid: two 3x3 convs (F -> F/2 -> F/4, no
    non-linearity in between), dropout, ReLU, a 1x1 conv to one map per sentiment, global average
    pooling and `sentiment_fcs_num` small linear layers."""
    native = False          # (class default: an instance unpickled from before the switch existed reads it)
    _native_pack = None

    def __init__(self, sentiment_categories, settings):
        super().__init__()
        self.sentiment_categories = sentiment_categories
        self.neu_idx = sentiment_categories.index('neutral')
        ch = settings['fc_feat_dim']
        self.convs = nn.Sequential()
        for i in range(settings['sentiment_convs_num']):
            self.convs.add_module('conv_%d' % i, nn.Conv2d(ch, ch // 2, 3, padding=1))
            ch //= 2
        self.convs.add_module('dropout', nn.Dropout(settings['dropout_p']))
        self.convs.add_module('relu', nn.ReLU())
        k = len(sentiment_categories)
        self.senti_conv = nn.Conv2d(ch, k, 1)
        self.global_pool = nn.AdaptiveAvgPool2d(1)
        self.output = nn.Sequential(*[nn.Linear(k, k) for _ in range(settings['sentiment_fcs_num'])])
        # Opt-in: the eval-mode forward on the library's own kernels (isc_senti_det_fwd: the 3x3 convolutions as implicit
        # GEMMs on the split-f16 engine over the channels-last grid as it is stored - fp32 or float16 - and one tail
        # kernel per image) instead of stock torch ops (permute, vendor-library fp32 convolutions, a dozen small
        # launches).  enable_native() / `native = True`.
        self.native = False
        self._native_pack = None        # (key, packed conv weights): rebuilt when a parameter's (data_ptr, _version) moves

    def enable_native(self, on=True):
        self.native = bool(on)
        return self

    def native_params(self):
        """The parameters in state_dict order: (weight, bias) of every 3x3 conv, of senti_conv and of every FC layer."""
        mods = [m for m in self.convs if isinstance(m, nn.Conv2d)] + [self.senti_conv] + list(self.output)
        return [t for m in mods for t in (m.weight, m.bias)]

    def native_active(self, features):
        """Whether forward(features) takes the native path now: the flag is on, eval mode (no dropout), the tensors live
        on the ROCm device, nothing asks for a gradient of a parameter, and the split-f16 engine is in use (mode 0 /
        `ops.exact_fp32_engine()` - the engine that serves features beyond |x| < 65504 - runs the torch code, as do
        train mode, CPU tensors and the detector's own training)."""
        if not self.native or self.training or not features.is_cuda:
            return False
        params = self.native_params()
        if params[0].device != features.device or features.dtype not in (torch.float32, torch.float16):
            return False
        if torch.is_grad_enabled() and (features.requires_grad or any(p.requires_grad for p in params)):
            return False
        from . import ops
        return ops.h3_mode() != 0

    def forward_native(self, features, threshold=0, ksplit=0):
        """The native forward in full: -> (logits [B,k], sentiment map [B,h,w], labels [B] int64 - neu_idx where the
        largest probability is under `threshold` -, largest probabilities [B]).  features [B,h,w,F] fp32 or float16."""
        from . import ops
        params = [p.detach() for p in self.native_params()]
        key = tuple((q.data_ptr(), q._version) for q in params)
        if self._native_pack is None or self._native_pack[0] != key:
            n_convs = sum(1 for m in self.convs if isinstance(m, nn.Conv2d))
            self._native_pack = (key, ops.senti_det_pack(params[0:2 * n_convs:2]))
        with torch.no_grad():
            return ops.senti_det_fwd(params, features.contiguous(), threshold, self.neu_idx,
                                     packed=self._native_pack[1], ksplit=ksplit)

    def forward(self, features):
        if self.native_active(features):
            return self.forward_native(features)[:2]
        if features.dtype != self.senti_conv.weight.dtype:
            features = features.to(self.senti_conv.weight.dtype)
        x = self.convs(features.permute(0, 3, 1, 2))
        maps = self.senti_conv(x)                                   # [B,k,h,w]
        logits = self.output(maps.mean(dim=(2, 3)))                 # GAP + FCs
        B, k, h, w = maps.shape
        weighted = torch.bmm(logits.softmax(dim=-1).unsqueeze(1), maps.reshape(B, k, h * w))
        return logits, weighted.reshape(B, h, w)

    @torch.no_grad()
    def sample_device(self, features, senti_threshold=0):
        """`sample` without the category names: (labels [B] int64, sentiment map, max-probabilities), all on the device -
        nothing is read back, so the caller can queue its next step (the beam search takes the labels as a tensor) before
        the host looks at them (`names`)."""
        self.eval()
        if self.native_active(features):
            _, maps, labels, scores = self.forward_native(features, senti_threshold)
            return labels, maps, scores
        logits, maps = self.forward(features)
        scores, labels = logits.softmax(dim=-1).max(dim=-1)
        labels = torch.where(scores < senti_threshold, torch.full_like(labels, self.neu_idx), labels)
        return labels, maps, scores

    def names(self, labels):
        return [self.sentiment_categories[i] for i in labels.tolist()]          # (one read-back, not one per label)

    @torch.no_grad()
    def sample(self, features, senti_threshold=0):
        """-> (labels [B] int64, sentiment map [B,h,w], category names, max-probabilities [B]);
        a maximum probability below the threshold falls back to `neutral`."""
        labels, maps, scores = self.sample_device(features, senti_threshold)
        return labels, maps, self.names(labels), scores

    def get_optim_criterion(self, lr, weight_decay=0, fused=False):
        """`fused=True`: optim.FusedClampAdam (clamp + Adam in one launch) for train.senti_det_train_step; the default is
        the reference's torch.optim.Adam."""
        if fused:
            from .optim import FusedClampAdam
            return FusedClampAdam(self.parameters(), lr=lr, weight_decay=weight_decay), nn.CrossEntropyLoss()
        return torch.optim.Adam(self.parameters(), lr=lr, weight_decay=weight_decay), nn.CrossEntropyLoss()


class SentenceSentimentClassifier(nn.Module):
    """Sentence-level sentiment: word embedding -> one-layer LSTM -> squeeze-excite style token
    weights (mean over channels of a sigmoid MLP of every hidden state) -> weighted sum -> MLP."""
    native = False          # (class default: an instance unpickled from before the switch existed reads it)

    def __init__(self, idx2word, sentiment_categories, settings):
        super().__init__()
        self.sentiment_categories = sentiment_categories
        self.pad_id = idx2word.index('<PAD>')
        self.vocab_size = len(idx2word)
        W, H = settings['word_emb_dim'], settings['rnn_hid_dim']
        self.word_embed = nn.Sequential(nn.Embedding(self.vocab_size, W, padding_idx=self.pad_id), nn.ReLU(),
                                        nn.Dropout(settings['dropout_p']))
        self.rnn = nn.LSTM(W, H, bidirectional=False)
        self.drop = nn.Dropout(settings['dropout_p'])
        self.excitation = nn.Sequential(nn.Linear(H, H), nn.ReLU(), nn.Linear(H, H), nn.Sigmoid())
        self.squeeze = nn.AdaptiveAvgPool1d(1)
        self.sent_senti_cls = nn.Sequential(nn.Linear(H, H), nn.ReLU(), nn.Dropout(settings['dropout_p']),
                                            nn.Linear(H, len(sentiment_categories)))
        # Opt-in: the eval-mode forward on the library's own kernels (isc_sent_cls_fwd: embed gather, ONE input GEMM over
        # all steps, the fused LSTM cell per step, pooling and head kernels - L + 7 launches, capturable) instead of stock
        # torch ops (an nn.LSTM of the vendor library plus a dozen small launches).  enable_native() / `native = True`.
        self.native = False

    def enable_native(self, on=True):
        self.native = bool(on)
        return self

    def native_params(self):
        """The thirteen tensors of the state_dict in ops.SENT_CLS_PARAMS order."""
        ex, cls = self.excitation, self.sent_senti_cls
        return (self.word_embed[0].weight, self.rnn.weight_ih_l0, self.rnn.weight_hh_l0, self.rnn.bias_ih_l0,
                self.rnn.bias_hh_l0, ex[0].weight, ex[0].bias, ex[2].weight, ex[2].bias, cls[0].weight, cls[0].bias,
                cls[3].weight, cls[3].bias)

    def native_active(self, seqs):
        """Whether forward(seqs, ...) takes the native path now: the flag is on, the module is in eval mode (no dropout),
        the tensors live on the ROCm device and nothing asks for a gradient of a parameter (train mode, CPU tensors and
        autograd through forward() run the torch code below; the classifier's training on the library's kernels is a
        separate entry point, train.sent_cls_train_step)."""
        if not self.native or self.training or not seqs.is_cuda:
            return False
        params = self.native_params()
        if params[0].device != seqs.device:
            return False
        return not (torch.is_grad_enabled() and any(p.requires_grad for p in params))

    def forward_native(self, seqs, lengths, labels=None, pad_to=None):
        """The native forward in full: -> (logits [B,k], weights [B,T_out], pred [B] int32, reward [B,T_out] or None) with
        T_out = pad_to or L, L = max(lengths) for host lengths and seqs.shape[1] for a device tensor [B]; weights and
        reward (= weights where pred == labels, else 0) are exactly 0 at and beyond a row's length.  Every entry of
        seqs[:, :L] must be a valid id (entries behind a row's length are read, never summed)."""
        from . import ops
        if torch.is_tensor(lengths) and lengths.device == seqs.device:
            L, lens = seqs.shape[1], lengths.to(torch.int32)
        else:
            lengths = [int(x) for x in lengths]
            L = max(lengths)
            lens = torch.tensor(lengths, dtype=torch.int32).pin_memory().to(seqs.device, non_blocking=True)
        if labels is not None:
            labels = labels.to(device=seqs.device, dtype=torch.int64).contiguous()
        with torch.no_grad():
            return ops.sent_cls_fwd([p.detach() for p in self.native_params()], seqs[:, :L], lens.contiguous(), labels,
                                    pad_to=pad_to)

    def forward(self, seqs, lengths):
        """seqs [B,L] int64, lengths: B ints (>= 1), or a device tensor [B]. Returns (logits [B,k], token weights
        [B,max(lengths)] - [B,L] for device lengths).
        Positions at or beyond a row's length contribute nothing (the reference packs the sequences;
        here the padded LSTM outputs are masked instead - the recurrence is causal, so valid positions
        are unaffected by what follows them)."""
        if self.native_active(seqs):
            return self.forward_native(seqs, lengths)[:2]
        if torch.is_tensor(lengths) and lengths.device == seqs.device and seqs.is_cuda:
            # lengths that live on the device: no host read - the LSTM runs over all L columns (it is causal and the
            # positions at or beyond a row's length are masked below, so the valid positions are what the packed form
            # computes; the token weights come back [B,L] with zeros behind each row's length)
            Lmax, lens = seqs.shape[1], lengths.to(torch.int64)
        else:
            lengths = [int(x) for x in lengths]
            Lmax = max(lengths)
            if seqs.is_cuda:    # (through pinned memory: a pageable copy would hold the host until the stream reaches it)
                lens = torch.tensor(lengths, dtype=torch.int64).pin_memory().to(seqs.device, non_blocking=True)
            else:
                lens = torch.as_tensor(lengths, device=seqs.device)
        x = self.word_embed(seqs[:, :Lmax])                                   # [B,Lmax,W]
        out, _ = self.rnn(x.transpose(0, 1))                                  # time-major LSTM
        out = out.transpose(0, 1)                                             # [B,Lmax,H]
        valid = (torch.arange(Lmax, device=seqs.device).unsqueeze(0) < lens.unsqueeze(1)).to(out.dtype)
        out = self.drop(out * valid.unsqueeze(-1))
        weights = (self.excitation(out) * valid.unsqueeze(-1)).mean(dim=-1)  # [B,Lmax]
        feats = torch.bmm(weights.unsqueeze(1), out).squeeze(1)               # [B,H]
        return self.sent_senti_cls(feats), weights

    @torch.no_grad()
    def sample(self, seqs, lengths):
        self.eval()
        pred, att_weights = self.forward(seqs, lengths)
        result = [int(p.argmax(-1)) for p in pred]
        return result, [self.sentiment_categories[r] for r in result], att_weights

    def get_optim_and_crit(self, lr, weight_decay=0, fused=False):
        """`fused=True`: optim.FusedClampAdam (clamp + Adam in one launch) for train.sent_cls_train_step; the default is
        the reference's torch.optim.Adam."""
        if fused:
            from .optim import FusedClampAdam
            return FusedClampAdam(self.parameters(), lr=lr, weight_decay=weight_decay), nn.CrossEntropyLoss()
        return torch.optim.Adam(self.parameters(), lr=lr, weight_decay=weight_decay), nn.CrossEntropyLoss()


class MultiLabelClsLoss(nn.Module):
    """The concept detector's criterion (what concept_detector.py:44-58 computes): binary cross-entropy on PROBABILITIES
    p [B, C] against 0/1 targets, as the sum of two separately averaged halves - the set targets' -log p and the unset
    ones' -log(1 - p), each averaged over the concepts and then over the rows (in that order, so the fp32 bits are the
    reference's).  Plain torch, for drop-in callers, the CPU path and the native path's comparison; the native training
    step (train.concept_train_step) computes the same loss from the logits in the stable softplus form
    (isc_concept_loss), which stays finite where the log of a saturated sigmoid does not."""

    def forward(self, probs, target):
        t = target.to(probs.dtype)
        row_mean = lambda x: x.mean(dim=-1).mean(dim=-1)
        return -row_mean(t * probs.log()) + -row_mean((1 - t) * (1 - probs).log())


class ConceptDetector(nn.Module):
    """The concept detector (concept_detector.py:5-41): fc features -> Linear + ReLU -> Linear + ReLU -> Dropout ->
    Linear -> Sigmoid over the concept vocabulary.  `output` keeps the reference's indices (Linear at 0, 2, 5; Dropout
    at 4), so its state_dict loads by name.

    Native path (isc_concept_fwd: three isc_linear_fwd launches and the head kernel) - ON by default whenever eligible,
    see native_active.  `enable_native(False)` gives the stock torch ops, which remain the CPU path and the probe's
    comparison.

    Top-`num` order of the native path: larger logit first, lower index on equal logits, NaN last; the torch path sorts
    the probabilities (stable, descending), which agrees wherever the probabilities are distinct."""
    native = True

    def __init__(self, idx2concept, settings):
        super().__init__()
        self.idx2concept = idx2concept
        F, H = settings['fc_feat_dim'], settings['concept_mid_him']
        self.output = nn.Sequential(nn.Linear(F, H), nn.ReLU(), nn.Linear(H, H), nn.ReLU(),
                                    nn.Dropout(settings['dropout_p']), nn.Linear(H, len(idx2concept)), nn.Sigmoid())
        self.native = True
        self._concept_word = None           # [C] int64 vocabulary ids (set_vocabulary), on the host
        self._concept_word_dev = {}         # device -> the same table there

    # ---- tables
    def set_vocabulary(self, word2idx):
        """Builds the concept -> vocabulary id table (`words` of sample_device, the captioner's cpts_tensor).  A concept
        that the vocabulary lacks raises KeyError, as train_rl.py:122 does."""
        self._concept_word = torch.tensor([word2idx[c] for c in self.idx2concept], dtype=torch.int64)
        self._concept_word_dev = {}
        return self

    def concept_word(self, device):
        """The table on `device`, or None before set_vocabulary."""
        if self._concept_word is None:
            return None
        device = torch.device(device)
        t = self._concept_word_dev.get(device)
        if t is None:
            t = self._concept_word_dev[device] = self._concept_word.to(device)
        return t

    # ---- native switch
    def enable_native(self, on=True):
        self.native = bool(on)
        return self

    def native_params(self):
        o = self.output
        return [o[0].weight, o[0].bias, o[2].weight, o[2].bias, o[5].weight, o[5].bias]

    def native_active(self, features):
        """Whether forward / sample / sample_device take the native path now: the flag is on, eval mode (no dropout), the
        tensors live on the ROCm device, the features are a [B, F] fp32 or float16 matrix, nothing asks for a gradient,
        and isc_linear_fwd can take the three layers - it contracts in 32-deep chunks, so fc_feat_dim % 32 == 0 and
        concept_mid_him % 32 == 0 (the number of concepts may be anything; feature rows that are not 16-byte aligned
        or whose row stride is not a multiple of 4 elements are copied first).  Both GEMM engines serve it (split-f16
        and, under ops.set_h3_mode(0), exact fp32).  Everything else - train mode, CPU tensors, the detector's own
        autograd training, other widths - runs the torch ops."""
        if not self.native or self.training or not torch.is_tensor(features) or not features.is_cuda:
            return False
        params = self.native_params()
        if params[0].device != features.device or features.dim() != 2 or \
                features.dtype not in (torch.float32, torch.float16) or params[0].dtype != torch.float32:
            return False
        if torch.is_grad_enabled() and (features.requires_grad or any(p.requires_grad for p in params)):
            return False
        from . import ops
        return ops.concept_shape_ok(params[0].shape[1], params[0].shape[0])

    def _native(self, features, num, want_probs, want_topk=True):
        from . import ops
        if features.stride(1) != 1 or features.stride(0) % 4 or features.data_ptr() % 16:
            features = features.contiguous()
        with torch.no_grad():
            return ops.concept_fwd([p.detach() for p in self.native_params()], features, num,
                                   concept_word=self.concept_word(features.device), want_probs=want_probs,
                                   want_topk=want_topk)

    # ---- the reference's surface
    def forward(self, features):
        """features [B, F] -> probabilities [B, C]."""
        if self.native_active(features):
            return self._native(features, 1, True, want_topk=False)['probs']
        if features.dtype != self.output[0].weight.dtype:
            features = features.to(self.output[0].weight.dtype)
        return self.output(features)

    def _sample_torch(self, features, num):
        from . import ops
        C_ = len(self.idx2concept)
        num = ops._check_num(num, C_)
        if features.dtype != self.output[0].weight.dtype:
            features = features.to(self.output[0].weight.dtype)
        out = self.output(features)
        scores, idx = out.sort(dim=-1, descending=True, stable=True)
        return out, idx[:, :num].contiguous(), scores[:, :num].contiguous()

    @torch.no_grad()
    def sample_device(self, features, num):
        """-> (idx [B, num] int64, scores [B, num], words [B, num] int64 vocabulary ids - None before set_vocabulary), all
        on the features' device; nothing is read back.  num outside [1, min(16, C)] raises ValueError."""
        self.eval()
        if self.native_active(features):
            r = self._native(features, num, False)
            return r['idx'], r['scores'], r.get('words')
        _, idx, scores = self._sample_torch(features, num)
        table = self.concept_word(features.device)
        return idx, scores, table[idx] if table is not None else None

    @torch.no_grad()
    def sample(self, features, num):
        """-> (probabilities [B, C], concept names per row (best first), scores [B, num]): the reference's triple
        (concept_detector.py:24-37), with ONE read-back for the names instead of one `.item()` per element."""
        self.eval()
        if self.native_active(features):
            r = self._native(features, num, True)
            out, idx, scores = r['probs'], r['idx'], r['scores']
        else:
            out, idx, scores = self._sample_torch(features, num)
        return out, [[self.idx2concept[i] for i in row] for row in idx.tolist()], scores

    def get_optim_criterion(self, lr, weight_decay=0):
        from .optim import FusedClampAdam
        return FusedClampAdam(self.parameters(), lr=lr, weight_decay=weight_decay), MultiLabelClsLoss()
