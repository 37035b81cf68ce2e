"""Thin torch-tensor -> C-ABI adapters. PyTorch is plumbing here (device memory + streams);
all arithmetic happens in libinsenticap_hip.so."""
import ctypes as C
import gc
import threading
import time

import torch

from . import _lib
from ._lib import LinearProblem, LstmProblem, RolloutStep, ScanProblem, check


def stream():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


class KernelTimer:
    """Optional per-launch timing with HIP events recorded on the stream the kernels run on
    (torch's current stream). bench.py arms it for one decode step per timed roll-out; when
    `armed` is False the wrappers below add no work."""

    def __init__(self):
        self.armed = False
        self.arm_step = None   # decode step whose kernels get timed (-1 = prologue, None = off)
        self.phase = 'step'    # 'prologue' kernels run once per roll-out, 'step' kernels T times
        self.records = []   # (name, start_event, end_event, flops, bytes)

    def begin(self):
        if not self.armed:
            return None
        e = torch.cuda.Event(enable_timing=True)
        e.record()
        self._h3_before = _lib.load().isc_h3_launches()
        return e

    def end(self, e0, name, flops=0.0, nbytes=0.0):
        if e0 is None:
            return
        e1 = torch.cuda.Event(enable_timing=True)
        e1.record()
        h3 = _lib.load().isc_h3_launches() != self._h3_before     # the op went out on the split-f16 GEMM path
        self.records.append((name, e0, e1, flops, nbytes, self.phase, h3))

    def summary(self):
        """name -> dict(n, avg_ms, flops, bytes); call after a device synchronize."""
        out = {}
        for name, e0, e1, fl, nb, ph, h3 in self.records:
            d = out.setdefault(name, dict(n=0, total_ms=0.0, flops=fl, bytes=nb, phase=ph, h3=h3))
            d['n'] += 1
            d['total_ms'] += e0.elapsed_time(e1)
        for d in out.values():
            d['avg_ms'] = d['total_ms'] / d['n']
        return out


TIMER = KernelTimer()


def planes_ptrs(planes):
    """(hi, lo) pointers of a split-f16 plane buffer: a [2, rows, K] f16 tensor used as ONE buffer in which the two
    planes are interleaved per 32-wide k-block (include/insenticap_hip.h, isc_seg.A_hi): lo = hi + 32 halfs."""
    return planes.data_ptr(), planes.data_ptr() + 64


def _seg_k(segs):
    return sum(sg[0].shape[1] for sg in segs)


_SPLITK_WS = {}
_WS_SIZES = {}


def splitk_ws_floats():
    """Size of a per-(device, stream) split-K workspace, asked of the library (isc_splitk_workspace_bytes): the
    deepest K split of a [4096 x 512] output - the widest few-tile launch of the step at the headline batch - =
    128 MB; also holds the f16 weight planes of a split-f16 launch issued outside a weights scope."""
    if 'ws' not in _WS_SIZES:
        _WS_SIZES['ws'] = int(_lib.load().isc_splitk_workspace_bytes(4096, 512)) // 4
    return _WS_SIZES['ws']


def h3w_bytes():
    """Size of a weights-scope plane buffer (isc_h3_weights_workspace_bytes): hi + lo planes of up to 24 Mi weight
    values (the reference architecture at V = 10k has 22 063 379, of which ~16 M are GEMM operands) in the forward
    layout AND transposed for the backward = 192 MB."""
    if 'h3w' not in _WS_SIZES:
        _WS_SIZES['h3w'] = int(_lib.load().isc_h3_weights_workspace_bytes(24 * 1024 * 1024, 1))
    return _WS_SIZES['h3w']


def graphs_allowed_here():
    """Graph serving that is ON BY DEFAULT (beam search, small greedy roll-outs) applies on the main host thread only:
    a capture begins with a device-wide synchronisation and an allocator sweep, and two threads capturing at once is
    not something this package has exercised.  Worker threads run the same calls eagerly (same results)."""
    return threading.current_thread() is threading.main_thread()


def graph_capture(graph, **kw):
    """torch.cuda.graph(graph, **kw) for this package's captures, safe next to a torch.distributed process group
    (`settle=False`: skip the wait described below - for the second and later captures of one owner in a row).
    The backend's watchdog thread polls the completion event of every collective still on its list (hipEventQuery,
    every ~100 ms) and retires finished work only at such a pass.  On ROCm a poll of a collective issued shortly before a
    capture opened, landing INSIDE the capture window, fails with hipErrorCapturedEvent - in the watchdog thread, which
    aborts the process (RCCL, one rank: by chance at the full model size where a capture takes ~100 ms, for certain
    with a 0.4 s window - tests/_rccl_child.py keeps that case).  So, with a group alive: everything queued is finished
    and one watchdog pass is let go by before the capture opens (its list is then empty for the whole window - nothing
    this package captures issues a collective), and the capture runs in 'thread_local' error mode (calls of other
    host threads are not policed; autograd's backward thread launches into the capture in any mode).  Captures are
    once per geometry: the 0.25 s do not recur."""
    try:
        import torch.distributed as dist
        grouped = dist.is_available() and dist.is_initialized()
    except Exception:                   # a torch build without distributed
        grouped = False
    # 'thread_local' always: another host thread serving its own captioner on its own stream (include/insenticap_hip.h
    # allows that) may allocate or synchronise while this one captures; 'global' would fail ITS calls
    kw.setdefault('capture_error_mode', 'thread_local')
    settle = kw.pop('settle', True)     # False: a capture right behind another one of the same owner (nothing was issued between)
    if grouped and settle:
        # ... and no collective may still be on the watchdog's list when the capture opens: it retires finished work
        # at its next pass (every 100 ms), so finish everything and let one pass go by.  Captures are once per geometry.
        torch.cuda.synchronize()
        time.sleep(0.25)
    return _Capture(torch.cuda.graph(graph, **kw))


class _Capture:
    """torch.cuda.graph(...) with Python's automatic garbage collection held off while the capture is open.  torch
    collects once when a capture begins; a generational collection that fires DURING it can still run the destructor of
    cyclic garbage from earlier work - an older captured graph, a stream's buffers - and destroying a HIP graph (or
    freeing through the runtime) on a thread that is capturing aborts the process (seen as 'Fatal Python error: Aborted
    ... Garbage-collecting' inside a roll-out capture).  The cycle collector is switched back on after capture_end."""

    def __init__(self, inner):
        self.inner, self.was = inner, False

    def __enter__(self):
        out = self.inner.__enter__()
        self.was = gc.isenabled()
        gc.disable()
        return out

    def __exit__(self, *exc):
        try:
            return self.inner.__exit__(*exc)
        finally:
            if self.was:
                gc.enable()


def graph_node_counts(graph):
    """{'kernel', 'memcpy', 'memset', 'other'} node counts of a torch.cuda.CUDAGraph created with keep_graph=True
    (measurement / tests: the launches one replay issues).  HIP runtime calls only - nothing of this package's library."""
    hip = C.CDLL('libamdhip64.so')          # the runtime torch has already loaded
    raw = C.c_void_p(graph.raw_cuda_graph())
    n = C.c_size_t(0)
    if hip.hipGraphGetNodes(raw, None, C.byref(n)) != 0:
        raise RuntimeError('hipGraphGetNodes failed')
    nodes = (C.c_void_p * max(n.value, 1))()
    if hip.hipGraphGetNodes(raw, nodes, C.byref(n)) != 0:
        raise RuntimeError('hipGraphGetNodes failed')
    out = {'kernel': 0, 'memcpy': 0, 'memset': 0, 'other': 0}
    names = {0: 'kernel', 1: 'memcpy', 2: 'memset'}          # hipGraphNodeTypeKernel / Memcpy / Memset
    for i in range(n.value):
        ty = C.c_int(-1)
        if hip.hipGraphNodeGetType(C.c_void_p(nodes[i]), C.byref(ty)) != 0:
            raise RuntimeError('hipGraphNodeGetType failed')
        out[names.get(ty.value, 'other')] += 1
    return out


def graph_kernel_nodes(graph):
    """Launch-issuing nodes (kernels, copies, fills) of a kept graph - what a kernel trace counts per replay."""
    c = graph_node_counts(graph)
    return c['kernel'] + c['memcpy'] + c['memset']


_CAPTURE = threading.local()      # per host thread: the (workspace, weight-plane buffer) pair of a HIP-graph capture


class capture_buffers:
    """`with ops.capture_buffers(ws, wp):` - while THIS thread captures a HIP graph, split-K launches use `ws` and
    weights scopes put their planes into `wp` (the graph's owner keeps both alive for the replays) instead of the
    per-stream buffers.  Thread-local: another thread entering a scope on its own stream meanwhile is unaffected."""

    def __init__(self, ws, wp):
        self.pair = (ws, wp)

    def __enter__(self):
        self.prev = getattr(_CAPTURE, 'pair', None)
        _CAPTURE.pair = self.pair
        return self

    def __exit__(self, *exc):
        _CAPTURE.pair = self.prev
        return False


def _capture_pair():
    return getattr(_CAPTURE, 'pair', None) or (None, None)


def splitk_ws(device=None):
    """Split-K workspace of the CURRENT stream on `device` (allocated once per (device, stream)): kernels on one
    stream use it one after another; two streams never share one - their split-K launches may overlap."""
    cap_ws = _capture_pair()[0]
    if cap_ws is not None:
        return cap_ws
    device = torch.device(device if device is not None else torch.cuda.current_device())
    index = device.index if device.index is not None else torch.cuda.current_device()
    key = (index, torch.cuda.current_stream(index).cuda_stream)
    ws = _SPLITK_WS.get(key)
    if ws is None:
        ws = _SPLITK_WS[key] = torch.empty(splitk_ws_floats(), dtype=torch.float32, device=device)
    return ws


def _attach_ws(problem, like_ptr_device):
    if not problem.splitk_ws:
        ws = splitk_ws(like_ptr_device)
        problem.splitk_ws, problem.splitk_ws_floats = ws.data_ptr(), ws.numel()


def ptr(t):
    return None if t is None else t.data_ptr()


def upload(values, dtype, device):
    """Small host list -> device tensor through pinned memory, asynchronously.  A pageable
    `torch.tensor(values, device=...)` is a stream-ordered blocking copy: the host would stall behind every
    kernel already queued (1.2 ms per criterion call in the XE training step).  A tensor that already lives on the
    device passes through (static inputs of a captured training iteration: no host copy may sit inside a graph)."""
    if isinstance(values, torch.Tensor):
        if values.is_cuda:
            return values if values.dtype == dtype else values.to(dtype)
        return values.to(dtype).pin_memory().to(device, non_blocking=True)
    return torch.tensor(values, dtype=dtype).pin_memory().to(device, non_blocking=True)


def to_device(x, device):
    """A batch tensor on `device` without stalling the host: a tensor in pageable host memory goes through pinned memory
    and a non-blocking copy (`x.to(device)` from pageable memory is stream-ordered AND blocks the host - it waits for
    everything queued, i.e. for the previous iteration); device tensors and data.RowGather pass through / expand."""
    if not torch.is_tensor(x):
        return x.to(device)                  # (data.RowGather: expanded on the device)
    if x.is_cuda or torch.device(device).type != 'cuda':
        return x.to(device)
    if x.is_pinned():
        return x.to(device, non_blocking=True)
    if x.numel() * x.element_size() > (1 << 20):
        # whole feature batches from pageable memory (151 MB for 512 images): page-locking a fresh buffer per batch costs
        # more than the runtime's own staged copy - data.DevicePrefetcher (kept pinned buffers) or data.DeviceFeatureStore
        # are the ways to take these off the host's critical path
        return x.to(device)
    return x.pin_memory().to(device, non_blocking=True)


def require_device(*tensors):
    for t in tensors:
        if t is not None and not t.is_cuda:
            raise _lib.HipLibraryError(
                'insenticap_model_amd runs on a ROCm device only (got a CPU tensor); there is no CPU path')


def _fill_segs(dst, segs):
    if not 1 <= len(segs) <= _lib.ISC_MAX_SEG:
        raise ValueError('1..4 K-segments supported')
    for i, sg in enumerate(segs):
        A, W = sg[0], sg[1]
        assert A.dim() == 2 and W.dim() == 2 and A.stride(1) == 1 and W.stride(1) == 1
        assert A.shape[1] == W.shape[1], (A.shape, W.shape)
        assert A.dtype in (torch.float32, torch.float16) and W.dtype == torch.float32
        s = dst[i]
        s.A, s.W = A.data_ptr(), W.data_ptr()
        s.lda, s.ldw, s.K = A.stride(0), W.stride(0), A.shape[1]
        s.a_f16 = int(A.dtype == torch.float16)      # float16 rows (isc_seg.a_f16): linear_problem / linear_fwd only
        planes = sg[2] if len(sg) > 2 else None      # optional [2, M, K] f16 planes of A (isc_seg.A_hi / A_lo)
        if planes is not None:
            assert planes.dtype == torch.float16 and planes.is_contiguous() and planes.shape == (2,) + tuple(A.shape)
            s.A_hi, s.A_lo = planes_ptrs(planes)
        else:
            s.A_hi = s.A_lo = None


def set_tile_override(tile):
    """Force the GEMM tile shape (0..3, see include/insenticap_hip.h) or -1 for the cost model; returns the previous value."""
    return _lib.load().isc_set_tile_override(int(tile))


def set_h3_mode(mode):
    """Split-f16 GEMM path: 0 = off, 1 = auto (default), 2 = large kernels whenever shapes allow, 3 / 4 = skinny kernel
    with 32 x 32 / 64 x 64 tiles whenever shapes allow (include/insenticap_hip.h); returns the previous mode."""
    return _lib.load().isc_set_h3_mode(int(mode))


class OutOfDomain(Exception):
    """Raised inside the product when a roll-out met non-finite values with the split-f16 engine on - at a point where
    nothing has been updated yet; the owner of the iteration redoes it on the exact-fp32 engine (Detector.forward)."""


_EXACT = {'depth': 0, 'prev': 1, 'lock': threading.Lock()}


class exact_fp32_engine:
    """`with ops.exact_fp32_engine():` - every GEMM launched meanwhile runs on the exact-fp32 MFMA tiles
    (isc_set_h3_mode(0); operand domain = fp32's), the previous mode is restored when the outermost block ends.  The mode
    is a process-wide tuning word: launches of other host threads inside the window also take the exact tiles (same
    results up to fp32 summation order).  Used by the product to SERVE inputs beyond the split-f16 domain |x| < 65504
    instead of rejecting them (Captioner / Detector: numerics_checks)."""

    def __enter__(self):
        with _EXACT['lock']:
            if _EXACT['depth'] == 0:
                _EXACT['prev'] = set_h3_mode(0)
            _EXACT['depth'] += 1
        return self

    def __exit__(self, *exc):
        with _EXACT['lock']:
            _EXACT['depth'] -= 1
            if _EXACT['depth'] == 0:
                set_h3_mode(_EXACT['prev'])
        return False


def h3_mode():
    """The current split-f16 mode (isc_set_h3_mode) without changing it."""
    return _lib.load().isc_set_h3_mode(-1)


def set_gemv_rows(rows):
    """Few-row launches (M <= rows <= 8) as fused matrix-vector kernels; 0 = off.  Returns the previous value."""
    return _lib.load().isc_set_gemv_rows(int(rows))


_H3W_BUF = {}


class h3_weights_scope:
    """`with ops.h3_weights_scope(device):` - the weights passed to the forward GEMMs do not change inside the block
    (include/insenticap_hip.h: isc_h3_weights_begin), so their f16 planes are built once per block, not per launch.
    The scope belongs to the CURRENT stream (library side: one slot per stream; here: one plane buffer and one
    nesting depth per (device, stream)), so two host threads running two captioners on two streams are independent.
    Nested scopes on the same stream are ignored (the outer one stays in force).
    `key` (hashable, optional): identifies the weight VALUES (Captioner passes the parameters' storage pointers and
    version counters).  A keyed scope is suspended, not closed, on exit; the next keyed scope on the stream with an
    equal key resumes it with its planes intact - consecutive eval-mode calls then split the weights once."""
    _depth = {}
    _suspended = {}          # (device, stream) -> key of the suspended scope
    _cold_begins = {}        # (device, stream) -> scopes begun afresh there (planes rebuilt, entries laid out anew)
    _lock = threading.Lock()

    @classmethod
    def cold_begins(cls, keys):
        """How often a scope on these (device index, stream handle) pairs started afresh (HIP graphs captured there hold
        plane addresses of the layout that was current at capture)."""
        with cls._lock:
            return sum(cls._cold_begins.get(k, 0) for k in keys)

    @classmethod
    def rekey_epoch(cls, keys, epoch_before):
        """Suspended scopes on these streams whose key carried `epoch_before`: move them to the current WEIGHT_EPOCH
        (their planes were refreshed by launches the host did not see: a replayed training graph)."""
        with cls._lock:
            for k in keys:
                wk = cls._suspended.get(k)
                if isinstance(wk, tuple) and wk and wk[-1] == epoch_before:
                    cls._suspended[k] = wk[:-1] + (WEIGHT_EPOCH,)

    @classmethod
    def forget(cls, pred):
        """Drops the suspended scopes whose key satisfies `pred` (a Captioner being freed: its planes must never be
        resumed); the next scope on such a stream begins afresh."""
        with cls._lock:
            for k in [k for k, wk in cls._suspended.items() if pred(wk)]:
                del cls._suspended[k]

    def __init__(self, device, key=None):
        self.device = torch.device(device)
        self.wkey = key

    def __enter__(self):
        cls = h3_weights_scope
        index = self.device.index if self.device.index is not None else torch.cuda.current_device()
        self.key = key = (index, torch.cuda.current_stream(index).cuda_stream)     # one buffer per stream, as splitk_ws
        self.opened = False
        with cls._lock:
            depth = cls._depth[key] = cls._depth.get(key, 0) + 1
        try:                      # anything that raises below must give the depth back: __exit__ will not run, and a
            buf = was = None      # depth stuck at >= 1 would turn every later scope on this stream into a no-op
            cap_wp = _capture_pair()[1]
            if depth == 1 and cap_wp is not None:         # a HIP graph is being captured: the graph owns the plane
                buf = cap_wp                              # buffer, and replays must re-split (weights may change
                self.wkey = None                          # in place between replays): never keyed, never resumed
            elif depth == 1:
                with cls._lock:
                    buf = _H3W_BUF.get(key)
                    was = cls._suspended.pop(key, None)
                if buf is None:
                    buf = torch.empty(h3w_bytes(), dtype=torch.uint8, device=self.device)
                    with cls._lock:
                        _H3W_BUF[key] = buf
            if buf is not None:
                lib = _lib.load()
                if self.wkey is not None and was == self.wkey and \
                        lib.isc_h3_weights_resume(buf.data_ptr(), C.c_void_p(key[1])) == 0:
                    self.opened = True
                else:
                    rc = lib.isc_h3_weights_begin(buf.data_ptr(), buf.numel(), C.c_void_p(key[1]))
                    with cls._lock:
                        cls._cold_begins[key] = cls._cold_begins.get(key, 0) + 1
                    if rc != -4:                          # ISC_E_WORKSPACE: all scope slots taken - run without one
                        _lib.check(rc, 'isc_h3_weights_begin')
                        self.opened = True
        except BaseException:
            with cls._lock:
                cls._depth[key] -= 1
            raise
        return self

    def __exit__(self, *exc):
        cls = h3_weights_scope
        with cls._lock:
            cls._depth[self.key] -= 1
            if self.opened and self.wkey is not None and exc[0] is None:
                cls._suspended[self.key] = self.wkey
        if self.opened:
            if self.wkey is not None and exc[0] is None:
                _lib.load().isc_h3_weights_suspend(C.c_void_p(self.key[1]))
            else:
                _lib.load().isc_h3_weights_end(C.c_void_p(self.key[1]))
        return False


def linear_problem(segs, out, bias0=None, bias1=None, bias2=None, relu=False, keep_mask=None, mask_scale=1.0,
                   out_pre=None, accumulate=False):
    """out[M,N] = act(sum_s A_s W_s^T + bias0 + bias1) [* keep_mask * mask_scale]."""
    p = LinearProblem()
    _fill_segs(p.seg, segs)
    p.f16_segs = [(i, sg[0]) for i, sg in enumerate(segs) if sg[0].dtype == torch.float16]
    p.nseg = len(segs)
    p.M, p.N = out.shape
    assert segs[0][0].shape[0] == p.M and segs[0][1].shape[0] == p.N
    assert out.stride(1) == 1
    p.relu = int(relu)
    p.bias0, p.bias1, p.bias2 = ptr(bias0), ptr(bias1), ptr(bias2)
    p.keep_mask = ptr(keep_mask)
    p.mask_scale = mask_scale
    p.ldc = out.stride(0)
    p.C = out.data_ptr()
    p.C_pre = ptr(out_pre)
    p.accumulate = int(accumulate)
    if out_pre is not None:
        assert out_pre.stride(0) == out.stride(0)
    return p


def f16_to_f32(x, out=None):
    """fp32 copy of a float16 matrix [rows, cols] (unit column stride) by the library's kernel (isc_f16_to_f32)."""
    assert x.dtype == torch.float16 and x.dim() == 2 and x.stride(1) == 1
    if out is None:
        out = torch.empty(x.shape, dtype=torch.float32, device=x.device)
    if x.numel():
        check(_lib.load().isc_f16_to_f32(x.data_ptr(), x.stride(0), out.data_ptr(), out.stride(0), x.shape[0],
                                         x.shape[1], stream()), 'isc_f16_to_f32')
    return out


def f16_convert_launches():
    return _lib.load().isc_f16_convert_launches()


def h3_f16a_launches():
    return _lib.load().isc_h3_f16a_launches()


def f32_launches(kind):
    """Launches of the exact-fp32 GEMM kernels so far (isc_f32_launches): kind 0 / 1 / 2 = the register-staged 128 / 64 /
    32-row tile, 3 = XL, 4 = LD, 5 = MD, 6 = a split-K reduce; -1 for any other kind."""
    return _lib.load().isc_f32_launches(int(kind))


H3_KINDS = 17


def h3_kernel_launches(kind):
    """Launches of the split-f16 GEMM kernels so far, by instantiation (isc_h3_kernel_launches): 3 g + f = the large
    tile of 128 / 256 / 64 rows (g = 0 / 1 / 2) on planes / fp32 rows / f16 rows (f = 0 / 1 / 2); 9 / 10 / 11 = the skinny
    kernel 32 x 32 on four waves / on eight / 64 x 64; 12 / 13 = its vocabulary form on four / eight waves; 14 / 15 =
    gemm_h3v_kernel on planes / fp32 rows; 16 = an operand-split launch; -1 for any other kind."""
    return _lib.load().isc_h3_kernel_launches(int(kind))


def linear_fwd(problems):
    lib = _lib.load()
    _attach_ws(problems[0], torch.cuda.current_device())
    arr = (LinearProblem * len(problems))(*problems)
    if any(getattr(q, 'f16_segs', None) for q in problems) and \
            not lib.isc_linear_f16_native(arr, len(problems), stream()):
        # float16 activations on a launch the large split-f16 kernels will not take (few rows, exact engine, a K or a
        # stride they cannot stage ...): an fp32 copy for this launch - explicit, counted (isc_f16_convert_launches)
        for q in problems:
            for i, A in getattr(q, 'f16_segs', None) or ():
                A32 = f16_to_f32(A)
                q.keep = getattr(q, 'keep', []) + [A32]          # (lives as long as the problem)
                q.seg[i].A, q.seg[i].lda, q.seg[i].a_f16 = A32.data_ptr(), A32.stride(0), 0
            q.f16_segs = []
        arr = (LinearProblem * len(problems))(*problems)
    e0 = TIMER.begin()
    check(lib.isc_linear_fwd(arr, len(problems), stream()), 'isc_linear_fwd')
    if e0 is not None:
        fl = sum(2.0 * q.M * q.N * sum(q.seg[i].K for i in range(q.nseg)) for q in problems)
        TIMER.end(e0, 'linear[' + '+'.join('%dx%dx%d' % (q.M, q.N, sum(q.seg[i].K for i in range(q.nseg)))
                                          for q in problems) + ']', fl)


def lstm_fwd(segs, b_ih, b_hh, c_prev, h_out, c_out, gates_out=None, h_keep_mask=None,
             mask_scale=1.0, hdrop_out=None, pre=None, tab=None, tab_ids=None, h_planes=None, pre_div=1, ws=None):
    """h_planes: optional [2, M, H] f16 tensor receiving the split-f16 planes of h_out (for consumers' segments).
    pre_div > 1: `pre` is [M / pre_div, 4H], one row per image, and row m adds pre[m // pre_div].
    ws: optional fp32 tensor used as the launch's split-K workspace instead of the stream's (as a pre-set
    `splitk_ws` on a linear problem)."""
    lib = _lib.load()
    p = LstmProblem()
    _fill_segs(p.seg, segs)
    p.nseg = len(segs)
    p.M, p.H = c_prev.shape
    assert c_prev.is_contiguous() and h_out.is_contiguous() and c_out.is_contiguous()
    p.b_ih, p.b_hh = ptr(b_ih), ptr(b_hh)
    if pre is not None:
        pre_div = max(int(pre_div), 1)
        assert pre.is_contiguous() and p.M % pre_div == 0 and pre.shape == (p.M // pre_div, 4 * p.H)
        p.pre, p.pre_div = pre.data_ptr(), pre_div
    if tab is not None:
        assert tab.is_contiguous() and tab.shape[1] == 4 * p.H and tab_ids.dtype == torch.int64
        p.tab, p.tab_ids, p.tab_ids_stride = tab.data_ptr(), tab_ids.data_ptr(), tab_ids.stride(0)
    p.c_prev, p.h_out, p.c_out = c_prev.data_ptr(), h_out.data_ptr(), c_out.data_ptr()
    p.gates_out = ptr(gates_out)
    p.h_keep_mask = ptr(h_keep_mask)
    p.mask_scale = mask_scale
    p.hdrop_out = ptr(hdrop_out)
    if h_planes is not None:
        assert h_planes.dtype == torch.float16 and h_planes.is_contiguous() and h_planes.shape == (2, p.M, p.H)
        p.h_hi, p.h_lo = planes_ptrs(h_planes)
    if ws is not None:
        assert ws.dtype == torch.float32 and ws.is_contiguous()
        p.splitk_ws, p.splitk_ws_floats = ws.data_ptr(), ws.numel()
    _attach_ws(p, c_prev.device)
    e0 = TIMER.begin()
    check(lib.isc_lstm_fwd(C.byref(p), stream()), 'isc_lstm_fwd')
    if e0 is not None:
        k = _seg_k(segs)
        TIMER.end(e0, 'lstm[%dx%dx%d]' % (p.M, 4 * p.H, k), 2.0 * p.M * 4 * p.H * k)


def step_fwd(plan):
    """One decode step from a prepared isc_step_plan (all kernels enqueued by the library)."""
    check(_lib.load().isc_step_fwd(C.byref(plan), stream()), 'isc_step_fwd')


class stream_gate:
    """`with ops.stream_gate(ptr):` - the forward launches enqueued on the current stream inside the block return at once
    when the device int32 at address `ptr` reads 0 at run time (isc_set_stream_gate: a batched beam search's step t under
    live[t]).  ptr None / 0: no gate, the block is plain."""

    def __init__(self, ptr):
        self.ptr = int(ptr) if ptr else 0
        self.st = None

    def __enter__(self):
        if self.ptr:
            self.st = stream()
            check(_lib.load().isc_set_stream_gate(C.c_void_p(self.ptr), self.st), 'isc_set_stream_gate')
        return self

    def __exit__(self, et, ev, tb):
        if self.st is not None:
            _lib.load().isc_set_stream_gate(None, self.st)
            self.st = None
        return False


def rows_stats_tile(V):
    """Column-tile width of the few-row classifier's statistics (isc_rows_stats_tile)."""
    return _lib.load().isc_rows_stats_tile(int(V))


def set_rows_scan_max(rows):
    """Largest inference step whose gated scan runs on the one-workgroup-per-row kernel (isc_set_rows_scan_max; 0 = off,
    negative = query).  Returns the previous value."""
    return _lib.load().isc_set_rows_scan_max(int(rows))


def copy_multi(dsts, srcs):
    """dsts[i].copy_(srcs[i]) for up to 8 pairs of contiguous same-shape, same-dtype device tensors in ONE launch
    (isc_copy_multi); longer lists go out in groups of 8."""
    pairs = [(d, s) for d, s in zip(dsts, srcs) if d is not None and d.numel()]
    for d, s in pairs:
        if d.dtype != s.dtype or d.shape != s.shape or not (d.is_contiguous() and s.is_contiguous() and d.is_cuda and s.is_cuda):
            raise ValueError('copy_multi: contiguous device tensors of equal shape and dtype expected')
    lib = _lib.load()
    for i in range(0, len(pairs), 8):
        grp = pairs[i:i + 8]
        n = len(grp)
        D = (C.c_void_p * n)(*[d.data_ptr() for d, _ in grp])
        S = (C.c_void_p * n)(*[s.data_ptr() for _, s in grp])
        Bn = (C.c_int64 * n)(*[d.numel() * d.element_size() for d, _ in grp])
        check(lib.isc_copy_multi(D, S, Bn, n, stream()), 'isc_copy_multi')


def stage_inputs(dsts, srcs):
    """A call's inputs -> the static buffers of a captured graph (None entries skipped): one launch when every pair
    is contiguous and of one dtype, torch's per-dtype copies otherwise."""
    pairs = [(d, s) for d, s in zip(dsts, srcs) if d is not None]
    if all(d.dtype == s.dtype and d.shape == s.shape and s.is_cuda and s.is_contiguous() and d.is_contiguous()
           for d, s in pairs):
        copy_multi([d for d, _ in pairs], [s for _, s in pairs])
        return
    by_dtype = {}
    for d, s in pairs:
        by_dtype.setdefault(d.dtype, ([], []))
        by_dtype[d.dtype][0].append(d)
        by_dtype[d.dtype][1].append(s)
    for ds, ss in by_dtype.values():
        torch._foreach_copy_(ds, ss, non_blocking=True)


def set_h3v(on):
    """Classifier launches of the skinny split-f16 path on gemm_h3v_kernel (isc_set_h3v; 0 = the ring-staged form it
    replaced).  Returns the previous value."""
    return _lib.load().isc_set_h3v(int(on))


def set_h3_vocab_tile(rows):
    """Tile geometry of the classifier launches of the large split-f16 kernels (isc_set_h3_vocab_tile): 0 = auto (128
    rows), 128 / 256 = that many rows per tile at any tile count.  Returns the previous value."""
    rows = int(rows)
    if rows not in (0, 128, 256):
        raise ValueError('set_h3_vocab_tile: 0 (auto), 128 or 256, got %r' % rows)
    return _lib.load().isc_set_h3_vocab_tile(rows)


def rows_step_supported(plan):
    return bool(_lib.load().isc_rows_step_supported(C.byref(plan)))


def rows_shape_supported(rows, H, E, A, W, V, R=1, Mw=1, has_tab=True):
    """isc_rows_step_supported's answer from the widths and counts alone (isc_rows_shape_supported; nothing is issued)."""
    return bool(_lib.load().isc_rows_shape_supported(int(rows), int(H), int(E), int(A), int(W), int(V), int(R), int(Mw),
                                                     int(bool(has_tab))))


def rows_vocab_supported(M, V, K):
    """Whether the few-row classifier takes M rows of width K over V columns (isc_rows_vocab_supported)."""
    return bool(_lib.load().isc_rows_vocab_supported(int(M), int(V), int(K)))


ROWS_ROUTE_KERNELS = ('lstm', 'linear', 'scan', 'vocab')


def rows_routes(n=0):
    """(launches of rows kernels recorded so far, the last min(n, 16) of them, oldest first) - isc_rows_routes; a
    record is (kernel name, MR, UPW | NP | single, NT, BAN, S, J, K-slices)."""
    n = max(0, min(int(n), 16))
    buf = (C.c_int32 * (8 * max(n, 1)))()
    total = _lib.load().isc_rows_routes(buf, n)
    have = min(n, total)
    return total, [(ROWS_ROUTE_KERNELS[buf[8 * i]],) + tuple(buf[8 * i + 1:8 * i + 8]) for i in range(have)]


def set_rows_nt(mode):
    """Cache policy of the rows kernels' weight streams (isc_set_rows_nt: 0 / 1 / 2).  Returns the previous mode."""
    return _lib.load().isc_set_rows_nt(int(mode))


def rows_step_fwd(plan, ext, ban=None):
    """One decode step on <= 8 rows from a prepared isc_step_plan + isc_rows_ext (csrc/rows.hip: five launches); `ban`
    (an isc_rows_ban): the rows' ban lists in the tile candidates (isc_rows_step_banned_fwd)."""
    if ban is not None:
        return check(_lib.load().isc_rows_step_banned_fwd(C.byref(plan), C.byref(ext), C.byref(ban), stream()),
                     'isc_rows_step_banned_fwd')
    check(_lib.load().isc_rows_step_fwd(C.byref(plan), C.byref(ext), stream()), 'isc_rows_step_fwd')


def rows_vocab_fwd(h, W, bias, part_max, part_sum, part_idx, ext, logits=None, ban=None):
    lib = _lib.load()
    M, K = h.shape
    V = W.shape[0]
    assert h.stride(1) == 1 and W.stride(1) == 1
    args = (h.data_ptr(), h.stride(0), W.data_ptr(), W.stride(0), bias.data_ptr(), M, V, K, part_max.data_ptr(),
            part_sum.data_ptr(), part_idx.data_ptr(), ptr(logits), logits.stride(0) if logits is not None else 0, C.byref(ext))
    if ban is not None:
        return check(lib.isc_rows_vocab_banned_fwd(*args, C.byref(ban), stream()), 'isc_rows_vocab_banned_fwd')
    check(lib.isc_rows_vocab_fwd(*args, stream()), 'isc_rows_vocab_fwd')


def beam_select(args):
    """Top-k + candidate merge of one beam step in one launch (isc_beam_select)."""
    check(_lib.load().isc_beam_select(C.byref(args), stream()), 'isc_beam_select')


def beam_select_groups(args, groups, diversity):
    """isc_beam_select under the diverse search's rule (isc_beam_select_groups; see beam_merge_groups)."""
    check(_lib.load().isc_beam_select_groups(C.byref(args), groups, diversity, stream()), 'isc_beam_select_groups')


def step_bwd(plan):
    check(_lib.load().isc_step_bwd(C.byref(plan), stream()), 'isc_step_bwd')


def vocab_fwd(h, W, bias, part_max, part_sum, part_idx, logits=None, h_planes=None, ws=None):
    """ws: optional fp32 tensor used as the launch's split-K workspace instead of the stream's."""
    lib = _lib.load()
    hi = lo = None
    if h_planes is not None:
        assert h_planes.dtype == torch.float16 and h_planes.is_contiguous() and h_planes.shape == (2,) + tuple(h.shape)
        hi, lo = planes_ptrs(h_planes)
    M, K = h.shape
    V = W.shape[0]
    assert h.stride(1) == 1 and W.stride(1) == 1
    ld = logits.stride(0) if logits is not None else 0
    e0 = TIMER.begin()
    if ws is None:
        ws = splitk_ws(h.device)
    else:
        assert ws.dtype == torch.float32 and ws.is_contiguous()
    check(lib.isc_vocab_fwd(h.data_ptr(), h.stride(0), W.data_ptr(), W.stride(0), bias.data_ptr(), M, V, K,
                            ptr(logits), ld, part_max.data_ptr(), part_sum.data_ptr(),
                            part_idx.data_ptr(), hi, lo, ws.data_ptr(), ws.numel(), stream()), 'isc_vocab_fwd')
    TIMER.end(e0, 'vocab[%dx%dx%d]' % (M, V, K), 2.0 * M * V * K)


def logsoftmax_apply(logits, part_max, part_sum, lse_out=None):
    lib = _lib.load()
    M, V = logits.shape
    assert logits.stride(1) == 1
    check(lib.isc_logsoftmax_apply(logits.data_ptr(), logits.stride(0), M, V, part_max.data_ptr(),
                                   part_sum.data_ptr(), ptr(lse_out), stream()), 'isc_logsoftmax_apply')


def logsoftmax_apply_steps(logits_btv, part_max_tbn, part_sum_tbn, src_tbv=None, step_rows=0):
    """log-softmax over all steps of a [B,T,V] logits tensor from the per-step tile statistics [T,B,n_tile]: in place,
    or from raw logits stacked per step `src_tbv` [T,B,V] (one classifier launch over all steps).
    step_rows > 0 (merged unroll): the statistics / src are [T, :B] row slices of stacks with `step_rows` rows per step
    (views whose first element is this branch's first row)."""
    B, T, V = logits_btv.shape
    assert logits_btv.stride(2) == 1
    if step_rows:
        n_tile = part_max_tbn.shape[2]
        assert step_rows >= B and part_max_tbn.shape[:2] == (T, B) and part_sum_tbn.shape == part_max_tbn.shape
        for x, w in ((part_max_tbn, n_tile), (part_sum_tbn, n_tile)) + (((src_tbv, V),) if src_tbv is not None else ()):
            assert x.stride(2) == 1 and x.stride(1) == w and x.stride(0) == step_rows * w, (x.shape, x.stride())
    else:
        assert part_max_tbn.is_contiguous() and part_sum_tbn.is_contiguous()
        assert part_max_tbn.shape[:2] == (T, B) and part_sum_tbn.shape == part_max_tbn.shape
        assert src_tbv is None or (src_tbv.is_contiguous() and src_tbv.shape == (T, B, V))
    check(_lib.load().isc_logsoftmax_apply_steps(logits_btv.data_ptr(), logits_btv.stride(0), logits_btv.stride(1), B, T,
                                                 V, part_max_tbn.data_ptr(), part_sum_tbn.data_ptr(), ptr(src_tbv),
                                                 int(step_rows), stream()),
          'isc_logsoftmax_apply_steps')


def _planes_ptrs(planes, like):
    if planes is None:
        return None, None
    assert planes.dtype == torch.float16 and planes.is_contiguous() and planes.shape == (2,) + tuple(like.shape)
    return planes_ptrs(planes)


def scan_problem(P, V, q, w, w_bias, out, alpha_out=None, q2=None, out_planes=None, row_ids=None, row_div=1):
    """P [B,R,A], V [B,R,D] contiguous; q/q2 [B,A]; w [A] (or [1,A]); out [B,D];
    alpha_out: [B,R] view with unit inner stride (row stride arbitrary).
    row_ids (gather mode): int64 [B,R]; P / V are then tables [n,A] / [n,D] and region r of row b is their row
    row_ids[b,r].
    row_div > 1 (isc_scan_problem.row_div): P, V, q2 and row_ids hold one entry per image, [B / row_div, ...], and row b
    of q / out / alpha_out reads entry b // row_div."""
    s = ScanProblem()
    assert P.is_contiguous() and V.is_contiguous() and q.is_contiguous() and out.is_contiguous()
    s.P, s.V, s.q, s.q2, s.w = P.data_ptr(), V.data_ptr(), q.data_ptr(), ptr(q2), w.data_ptr()
    s.w_bias = ptr(w_bias)
    if row_ids is not None:
        assert row_ids.dtype == torch.int64 and row_ids.dim() == 2 and row_ids.stride(1) == 1 and P.dim() == 2
        s.row_ids, s.row_ids_ld = row_ids.data_ptr(), row_ids.stride(0)
        s.R, s.A, s.D = row_ids.shape[1], P.shape[1], V.shape[1]
    else:
        s.R, s.A, s.D = P.shape[1], P.shape[2], V.shape[2]
    s.out = out.data_ptr()
    s.out_hi, s.out_lo = _planes_ptrs(out_planes, out)
    if alpha_out is not None:
        assert alpha_out.stride(1) == 1
        s.alpha_out, s.alpha_ld = alpha_out.data_ptr(), alpha_out.stride(0)
    row_div = max(int(row_div), 1)
    if row_div > 1:
        per_image = (row_ids if row_ids is not None else P).shape[0]
        assert q.shape[0] == per_image * row_div and (q2 is None or q2.shape[0] == per_image)
        s.row_div = row_div
    return s


def attn_scan_fwd(problems, B):
    lib = _lib.load()
    arr = (ScanProblem * len(problems))(*problems)
    e0 = TIMER.begin()
    check(lib.isc_attn_scan_fwd(arr, len(problems), B, stream()), 'isc_attn_scan_fwd')
    if e0 is not None:
        # algorithmic bytes: P and V streamed once per row (B*2*R*E*4 for the content scan)
        # (a grouped problem streams them once per image)
        nb = sum(4.0 * B / max(q.row_div, 1) * q.R * (q.A + q.D) for q in problems)
        TIMER.end(e0, 'attn_scan[' + '+'.join('%dx%dx%d' % (B, q.R, q.A) for q in problems) + ']', 0.0, nb)


def attn_scan_gate_fwd(scans, G, zh, b_gc, b_gs, w_gate, b_gate, f, beta_out=None, f_planes=None):
    """isc_attn_scan_gate_fwd: content + sentiment scan, gate sum and gate mix of one decode step in one launch.
    scans: [content, sentiment] isc_scan_problem (ops.scan_problem; their `out` is ignored); G: the two projected
    feature tensors / tables (ops-level contract: same row layout as the scan's V); zh [B,A]; f [B,D]."""
    a = _lib.ScanGateArgs()
    for i in range(2):
        C.memmove(C.byref(a.scan[i]), C.byref(scans[i]), C.sizeof(ScanProblem))
        a.scan[i].out = None
        a.scan[i].out_hi = a.scan[i].out_lo = None
        assert G[i].is_contiguous() and G[i].dtype == torch.float32
        a.G[i] = G[i].data_ptr()
    B = zh.shape[0]
    assert zh.is_contiguous() and f.is_contiguous()
    a.zh, a.b_gc, a.b_gs, a.w_gate, a.b_gate = zh.data_ptr(), b_gc.data_ptr(), b_gs.data_ptr(), w_gate.data_ptr(), ptr(b_gate)
    a.f = f.data_ptr()
    a.f_hi, a.f_lo = _planes_ptrs(f_planes, f)
    if beta_out is not None:
        a.beta, a.beta_ld = beta_out.data_ptr(), beta_out.stride(0)
    e0 = TIMER.begin()
    check(_lib.load().isc_attn_scan_gate_fwd(C.byref(a), B, stream()), 'isc_attn_scan_gate_fwd')
    if e0 is not None:
        nb = sum(4.0 * B * q.R * (2 * q.A + q.D) for q in scans)
        TIMER.end(e0, 'attn_scan_gate[' + '+'.join('%dx%dx%d' % (B, q.R, q.A) for q in scans) + ']', 0.0, nb)


def gate_mix_fwd(z, w, w_bias, v, s, out, beta_out=None, out_planes=None):
    lib = _lib.load()
    B, A = z.shape
    D = v.shape[1]
    assert z.is_contiguous() and v.is_contiguous() and s.is_contiguous() and out.is_contiguous()
    bl = beta_out.stride(0) if beta_out is not None else 0
    e0 = TIMER.begin()
    check(lib.isc_gate_mix_fwd(z.data_ptr(), w.data_ptr(), ptr(w_bias), v.data_ptr(), s.data_ptr(), B, A, D,
                               out.data_ptr(), ptr(beta_out), bl, *_planes_ptrs(out_planes, out), stream()),
          'isc_gate_mix_fwd')
    TIMER.end(e0, 'gate_mix[%dx%d]' % (B, A), 0.0, 4.0 * B * (A + 3 * D))


def embed_relu_fwd(emb, ids, out, add=None):
    lib = _lib.load()
    V, W = emb.shape
    assert ids.dtype == torch.int64 and ids.dim() == 1 and out.is_contiguous()
    check(lib.isc_embed_relu_fwd(emb.data_ptr(), V, W, ids.data_ptr(), ids.stride(0), ptr(add),
                                 ids.shape[0], out.data_ptr(), stream()), 'isc_embed_relu_fwd')


def embed_relu_mean_fwd(emb, ids, out):
    lib = _lib.load()
    V, W = emb.shape
    assert ids.dtype == torch.int64 and ids.is_contiguous()
    B, Cn = ids.shape
    check(lib.isc_embed_relu_mean_fwd(emb.data_ptr(), V, W, ids.data_ptr(), Cn, B, out.data_ptr(),
                                      stream()), 'isc_embed_relu_mean_fwd')


def embed_senti_words_fwd(emb, ids, pad_id, out, keep_mask=None, mask_scale=1.0):
    lib = _lib.load()
    V, W = emb.shape
    assert ids.dtype == torch.int64 and ids.is_contiguous()
    B, n = ids.shape
    check(lib.isc_embed_senti_words_fwd(emb.data_ptr(), V, W, ids.data_ptr(), n, pad_id, B,
                                        ptr(keep_mask), mask_scale, out.data_ptr(), stream()),
          'isc_embed_senti_words_fwd')


def rollout_finalize(step):
    lib = _lib.load()
    e0 = TIMER.begin()
    check(lib.isc_rollout_finalize(C.byref(step), stream()), 'isc_rollout_finalize')
    TIMER.end(e0, 'rollout_finalize[%d]' % step.B, 0.0, 4.0 * step.B * (3 * step.n_tile + 2 * step.W))


def check_sample_filter(temperature, top_k, top_p):
    """The domain of the sampling controls (isc_sample_filter): ValueError before anything touches the device."""
    import math
    t, p = float(temperature), float(top_p)
    if not (math.isfinite(t) and t > 0.0):
        raise ValueError('temperature must be finite and > 0, got %r' % (temperature,))
    if int(top_k) != top_k or top_k < 0:
        raise ValueError('top_k must be an integer >= 0 (0: off), got %r' % (top_k,))
    if not p > 0.0:
        raise ValueError('top_p must be > 0 (>= 1: off), got %r' % (top_p,))
    return t, int(top_k), p


def rollout_finalize_filtered(step, temperature=1.0, top_k=0, top_p=1.0, sampling_logprobs=None):
    """isc_rollout_finalize_filtered: the sampled roll-out's finalize with temperature / top-k / top-p (one launch)."""
    f = _lib.SampleFilter()
    f.temperature, f.top_k, f.top_p = check_sample_filter(temperature, top_k, top_p)
    f.sampling_logprobs = ptr(sampling_logprobs)
    lib = _lib.load()
    e0 = TIMER.begin()
    check(lib.isc_rollout_finalize_filtered(C.byref(step), C.byref(f), stream()), 'isc_rollout_finalize_filtered')
    TIMER.end(e0, 'rollout_finalize_filtered[%d]' % step.B, 0.0, 4.0 * step.B * (step.V + 2 * step.n_tile + 2 * step.W))


def check_decode_constraints(suppress_special, decoding_constraint, min_len, max_seq_len):
    """The domain of the roll-out's token constraints: ValueError before anything touches the device.  Returns them as
    (bool, bool, int)."""
    if not isinstance(suppress_special, (bool, int)) or suppress_special not in (0, 1):
        raise ValueError('suppress_special must be a bool, got %r' % (suppress_special,))
    if not isinstance(decoding_constraint, (bool, int)) or decoding_constraint not in (0, 1):
        raise ValueError('decoding_constraint must be 0 or 1, got %r' % (decoding_constraint,))
    if isinstance(min_len, bool) or not hasattr(min_len, '__index__') or not 0 <= int(min_len) <= int(max_seq_len):
        raise ValueError('min_len must be an integer in [0, max_seq_len = %r], got %r' % (max_seq_len, min_len))
    return bool(suppress_special), bool(decoding_constraint), int(min_len)


def decode_constraints(ban_ids=(), no_repeat=False, first_id=0, min_len=0):
    """An isc_decode_constraints struct."""
    ban_ids = [int(i) for i in ban_ids]
    if len(ban_ids) > 8:
        raise ValueError('at most 8 banned ids, got %d' % len(ban_ids))
    c = _lib.DecodeConstraints()
    for k, i in enumerate(ban_ids):
        c.ban_ids[k] = i
    c.n_ban, c.no_repeat, c.first_id, c.min_len = len(ban_ids), int(bool(no_repeat)), int(first_id), int(min_len)
    return c


def rollout_finalize_constrained(step, cons, filt=None, sampling_logprobs=None):
    """isc_rollout_finalize_constrained: the roll-out's finalize under the token constraints `cons` (decode_constraints).
    filt None: the plain finalize's choice (arg-max, or step.sample_u) over the allowed ids; (temperature, top_k, top_p):
    the filtered one's.  One launch."""
    f = None
    if filt is not None:
        f = _lib.SampleFilter()
        f.temperature, f.top_k, f.top_p = check_sample_filter(*filt)
        f.sampling_logprobs = ptr(sampling_logprobs)
    lib = _lib.load()
    e0 = TIMER.begin()
    check(lib.isc_rollout_finalize_constrained(C.byref(step), None if f is None else C.byref(f), C.byref(cons), stream()),
          'isc_rollout_finalize_constrained')
    TIMER.end(e0, 'rollout_finalize_constrained[%d]' % step.B, 0.0,
              4.0 * step.B * ((step.V if f is not None else 0) + 3 * step.n_tile + 2 * step.W))


def rollout_finalize_saved(step, cons, filt, sampling_logprobs, saved):
    """isc_rollout_finalize_saved: the filtered finalize (under `cons` when given) that also keeps what the backward of
    the sampling log-probabilities reads - saved: a mapping with 'kstar', 'gmax', 'logz' [B,T] and 'ban' ([B,T,10] or
    None).  One launch."""
    f, sv = _lib.SampleFilter(), _lib.FilterSaved()
    f.temperature, f.top_k, f.top_p = check_sample_filter(*filt)
    f.sampling_logprobs = ptr(sampling_logprobs)
    sv.kstar, sv.gmax, sv.logz, sv.ban = (ptr(saved.get(k)) for k in ('kstar', 'gmax', 'logz', 'ban'))
    e0 = TIMER.begin()
    check(_lib.load().isc_rollout_finalize_saved(C.byref(step), C.byref(f), None if cons is None else C.byref(cons),
                                                 C.byref(sv), stream()), 'isc_rollout_finalize_saved')
    TIMER.end(e0, 'rollout_finalize_saved[%d]' % step.B, 0.0, 4.0 * step.B * (step.V + 2 * step.n_tile + 2 * step.W))


def rollout_finalize_step(step, cons=None, filt=None, sampling_logprobs=None, saved=None):
    """One decode step's finalize in whichever of the three forms above it takes.  cons: decode_constraints or None;
    filt: the sampling controls (a mapping with 'temperature', 'top_k', 'top_p' and 'filtered' = any of them is on) or
    None.  Under constraints the sampled distribution is the restricted one, so a wanted `sampling_logprobs` sends the
    controls along even when they are the defaults.  saved (the differentiable roll-out): rollout_finalize_saved."""
    filtered = filt is not None and filt['filtered']
    controls = None if filt is None else (filt['temperature'], filt['top_k'], filt['top_p'])
    if saved is not None:
        rollout_finalize_saved(step, cons, controls, sampling_logprobs, saved)
    elif cons is not None:
        rollout_finalize_constrained(step, cons, controls if filtered or sampling_logprobs is not None else None,
                                     sampling_logprobs)
    elif filtered:
        rollout_finalize_filtered(step, *controls, sampling_logprobs)
    else:
        rollout_finalize(step)


def sched_sample(logp, part_max, part_sum, part_idx, u_select, u_draw, ss_prob, base_ids, out_ids, raw=False):
    """out_ids[b] = u_select[b] < ss_prob ? draw from exp(logp[b]) : base_ids[b]  (base_ids may be a strided column).
    raw: `logp` holds the row's raw logits (isc_sched_sample_raw)."""
    lib = _lib.load()
    M, V = logp.shape
    assert logp.stride(1) == 1 and out_ids.is_contiguous() and base_ids.dtype == torch.int64
    fn = lib.isc_sched_sample_raw if raw else lib.isc_sched_sample
    check(fn(logp.data_ptr(), logp.stride(0), M, V, part_max.data_ptr(), part_sum.data_ptr(),
             part_idx.data_ptr(), u_select.data_ptr(), u_draw.data_ptr(), float(ss_prob),
             base_ids.data_ptr(), base_ids.stride(0), out_ids.data_ptr(), stream()), 'isc_sched_sample')


def beam_topk(logits, part_max, part_sum, last_word, beam, pad_id, sos_id, unk_id, mask_special,
              decoding_constraint, top_val, top_idx):
    lib = _lib.load()
    rows, V = logits.shape
    n_tile = part_max.shape[1]
    check(lib.isc_beam_topk(logits.data_ptr(), logits.stride(0), part_max.data_ptr(), part_sum.data_ptr(),
                            n_tile, rows, V, beam, last_word.data_ptr(), pad_id, sos_id, unk_id,
                            int(mask_special), int(decoding_constraint), top_val.data_ptr(),
                            top_idx.data_ptr(), stream()), 'isc_beam_topk')


def beam_topk_banned(logits, part_max, part_sum, last_word, beam, pad_id, sos_id, unk_id, mask_special,
                     decoding_constraint, ban_ids, ban_cnt, top_val, top_idx):
    """beam_topk with the rows' ban lists (isc_beam_topk_banned): ban_ids int64 [rows, ld], ban_cnt int32 [rows]."""
    lib = _lib.load()
    rows, V = logits.shape
    n_tile = part_max.shape[1]
    assert ban_ids.dtype == torch.int64 and ban_cnt.dtype == torch.int32 and ban_ids.stride(1) == 1
    check(lib.isc_beam_topk_banned(logits.data_ptr(), logits.stride(0), part_max.data_ptr(), part_sum.data_ptr(),
                                   n_tile, rows, V, beam, last_word.data_ptr(), pad_id, sos_id, unk_id,
                                   int(mask_special), int(decoding_constraint), ban_ids.data_ptr(), ban_cnt.data_ptr(),
                                   ban_ids.stride(0), top_val.data_ptr(), top_idx.data_ptr(), stream()),
          'isc_beam_topk_banned')


def beam_ngram_ban(args):
    """The ban lists of a beam step from its candidate tables (isc_beam_ngram_ban)."""
    check(_lib.load().isc_beam_ngram_ban(C.byref(args), stream()), 'isc_beam_ngram_ban')


def check_beam_controls(no_repeat_ngram, min_len, max_seq_len, vocab_size, beam, device_merge):
    """The beam search's keywords `no_repeat_ngram` / `min_len`, checked before anything touches the device.  Returns
    them as plain ints; (0, 0) is the search without controls and asks nothing of the other arguments.  With a control on:
    vocab_size > max_seq_len + 4 + beam, the device-side merge (beam <= 8), and max_seq_len <= 256 (isc_beam_ngram_ban's
    bound, which the general merge alone does not have) - ValueError otherwise.  A `beam` that is no integer is left to the
    caller's own check."""
    def integer(name, v, lo, hi):
        if isinstance(v, bool) or not hasattr(v, '__index__') or not lo <= int(v) <= hi:
            raise ValueError('%s must be an integer in [%d, %d], got %r' % (name, lo, hi, v))
        return int(v)
    n = integer('no_repeat_ngram', no_repeat_ngram, 0, 4)
    m = integer('min_len', min_len, 0, int(max_seq_len))
    if n == 0 and m == 0:
        return 0, 0
    beam = int(beam) if hasattr(beam, '__index__') and not isinstance(beam, bool) else 1
    if vocab_size <= int(max_seq_len) + 4 + int(beam):
        raise ValueError('no_repeat_ngram / min_len can ban up to max_seq_len + 4 words of a step: a vocabulary of %d words '
                         'leaves fewer than beam_size = %d candidates at max_seq_len = %d'
                         % (vocab_size, beam, max_seq_len))
    if not device_merge or int(beam) > 8:
        raise ValueError('no_repeat_ngram / min_len are not built for the host merge (beam_device_merge = False or '
                         'beam_size > 8): the ban lists are formed on the device, behind the device-side merge')
    if int(max_seq_len) > 256:
        raise ValueError('no_repeat_ngram / min_len are not built for max_seq_len = %d > 256 (the ban-list kernel tests a '
                         'candidate in chunks of 64 positions up to 256)' % max_seq_len)
    return n, m


def beam_merge(args):
    """One candidate-merge step of a batched beam search on the device (isc_beam_merge)."""
    check(_lib.load().isc_beam_merge(C.byref(args), stream()), 'isc_beam_merge')


def beam_merge_groups(args, groups, diversity):
    """isc_beam_merge under the diverse search's rule: `groups` groups, Hamming penalty `diversity` per token already
    chosen at this step by a group in front (isc_beam_merge_groups)."""
    check(_lib.load().isc_beam_merge_groups(C.byref(args), groups, diversity, stream()), 'isc_beam_merge_groups')


def check_beam_groups(beam_groups, diversity, beam, device_merge):
    """The beam search's keywords `beam_groups` / `diversity`, checked before anything touches the device.  Returns
    (G, lambda) as a plain int and float.  G = 1 is the plain search for any lambda and asks nothing of the other
    arguments; G > 1 must divide `beam` and needs the device-side merge (beam <= 8) - ValueError otherwise.  A `beam` that
    is no integer is left to the caller's own check."""
    if isinstance(beam_groups, bool) or not hasattr(beam_groups, '__index__') or int(beam_groups) < 1:
        raise ValueError('beam_groups must be an integer >= 1, got %r' % (beam_groups,))
    G = int(beam_groups)
    if isinstance(diversity, bool) or not isinstance(diversity, (int, float)) or not 0.0 <= float(diversity) < float('inf'):
        raise ValueError('diversity must be a finite number >= 0, got %r' % (diversity,))
    lam = float(diversity)
    beam = int(beam) if hasattr(beam, '__index__') and not isinstance(beam, bool) else G
    if beam % G:
        raise ValueError('beam_groups = %d does not divide beam_size = %d' % (G, beam))
    if G > 1 and (not device_merge or beam > 8):
        raise ValueError('beam_groups > 1 is not built for the host merge (beam_device_merge = False or beam_size > 8): '
                         'the groups are ranked on the device, inside the device-side merge')
    return G, lam


def beam_gather(state_next, state_cur, gather, out):
    """[2,2,rows,H] recurrent states: out = [next ; current][gather] row by row (isc_beam_gather)."""
    rows, H = state_cur.shape[-2], state_cur.shape[-1]
    planes = state_cur.numel() // (rows * H)
    assert state_next.is_contiguous() and state_cur.is_contiguous() and out.is_contiguous()
    check(_lib.load().isc_beam_gather(state_next.data_ptr(), state_cur.data_ptr(), gather.data_ptr(), out.data_ptr(),
                                      planes, rows, H, stream()), 'isc_beam_gather')


def xe_loss_fwd(logp, target, lengths_i32, out2):
    lib = _lib.load()
    B, T, V = logp.shape
    assert logp.is_contiguous() and target.is_contiguous()
    check(lib.isc_xe_loss_fwd(logp.data_ptr(), target.data_ptr(), lengths_i32.data_ptr(), B, T, V,
                              out2.data_ptr(), stream()), 'isc_xe_loss_fwd')


SENT_CLS_PARAMS = ('emb', 'w_ih', 'w_hh', 'b_ih', 'b_hh', 'ex0_w', 'ex0_b', 'ex2_w', 'ex2_b', 'cls0_w', 'cls0_b', 'cls3_w',
                   'cls3_b')
_SENT_CLS_WS = {}           # (device index, stream, B, L, W, H) -> workspace of isc_sent_cls_fwd


def sent_cls_workspace_bytes(B, L, W, H):
    return int(_lib.load().isc_sent_cls_workspace_bytes(B, L, W, H))


def sent_cls_launches():
    return _lib.load().isc_sent_cls_launches()


def sent_cls_fwd(params, tokens, lens_i32, labels=None, pad_to=None, want_feats=False, workspace=None, out=None):
    """The frozen sentence-sentiment classifier's forward (isc_sent_cls_fwd): `params` = the thirteen tensors of the
    module's state_dict in SENT_CLS_PARAMS order, tokens [B,L] int64 (unit column stride; every entry a valid id),
    lens_i32 [B] int32 on the device (each in [1, L]), labels [B] int64 or None.  pad_to >= L: columns of the weights /
    reward rows (zeros behind L).  -> (logits [B,k], weights [B,T_out], pred [B] int32, reward [B,T_out] or None[, feats
    [B,H]]).  The workspace is kept per (device, stream, B, L, W, H) - two streams may run the classifier side by side -
    except inside a graph capture, where the caller hands `workspace` (and `out` = (logits, weights, pred, reward)) or
    a fresh one is drawn from the capture's pool.  A shape the library does not take raises (ISC_E_SHAPE); nothing is
    launched or written then."""
    lib = _lib.load()
    assert len(params) == len(SENT_CLS_PARAMS)
    require_device(tokens, lens_i32, labels, *params)
    assert tokens.dtype == torch.int64 and tokens.dim() == 2 and tokens.stride(1) == 1
    assert lens_i32.dtype == torch.int32 and lens_i32.is_contiguous() and lens_i32.shape == (tokens.shape[0],)
    for t in params:
        assert t.dtype == torch.float32 and t.is_contiguous(), 'classifier parameters: contiguous fp32'
    B, L = tokens.shape
    V, W = params[0].shape
    H = params[2].shape[1]
    k = params[11].shape[0]
    T_out = L if pad_to is None else int(pad_to)
    dev = tokens.device
    if labels is not None:
        assert labels.dtype == torch.int64 and labels.is_contiguous() and labels.shape == (B,)
    need = sent_cls_workspace_bytes(B, L, W, H)         # (0: a shape the library refuses - it says so below)
    if workspace is None:
        if torch.cuda.is_current_stream_capturing():
            workspace = torch.empty(max(need, 16), dtype=torch.uint8, device=dev)
        else:
            key = (dev.index, torch.cuda.current_stream(dev).cuda_stream, B, L, W, H)
            workspace = _SENT_CLS_WS.get(key)
            if workspace is None:
                workspace = _SENT_CLS_WS[key] = torch.empty(max(need, 16), dtype=torch.uint8, device=dev)
    if out is None:
        out = (torch.empty(B, k, dtype=torch.float32, device=dev), torch.empty(B, T_out, dtype=torch.float32, device=dev),
               torch.empty(B, dtype=torch.int32, device=dev),
               torch.empty(B, T_out, dtype=torch.float32, device=dev) if labels is not None else None)
    logits, weights, pred, reward = out
    assert logits.shape == (B, k) and weights.shape == (B, T_out) and pred.shape == (B,) and pred.dtype == torch.int32
    assert logits.is_contiguous() and weights.is_contiguous() and (reward is None or
                                                                   (reward.is_contiguous() and reward.shape == (B, T_out)))
    feats = torch.empty(B, H, dtype=torch.float32, device=dev) if want_feats else None
    p = _lib.SentClsProblem()
    p.B, p.L, p.W, p.H, p.V, p.k, p.T_out = B, L, W, H, V, k, T_out
    p.tokens, p.tokens_ld, p.lens = tokens.data_ptr(), tokens.stride(0), lens_i32.data_ptr()
    for name, t in zip(SENT_CLS_PARAMS, params):
        setattr(p, name, t.data_ptr())
    p.labels = ptr(labels)
    p.workspace, p.workspace_bytes = workspace.data_ptr(), workspace.numel()
    p.logits, p.weights, p.pred, p.reward, p.feats = (logits.data_ptr(), weights.data_ptr(), pred.data_ptr(), ptr(reward),
                                                      ptr(feats))
    check(lib.isc_sent_cls_fwd(C.byref(p), stream()), 'isc_sent_cls_fwd')
    return (logits, weights, pred, reward) + ((feats,) if want_feats else ())


# ---- the classifier's training (isc_sent_cls_train_fwd / isc_sent_cls_bwd and their two kernels on their own)
SENT_CLS_GRADS = tuple('d_' + n for n in SENT_CLS_PARAMS)


def sent_cls_bwd_launches():
    return _lib.load().isc_sent_cls_bwd_launches()


def sent_cls_train_shape_ok(W, H):
    """The shapes the training entry points take: the native forward's (W % 32 == H % 32 == 0, hence H % 4) and
    W <= 1024 (the embedding gradient's row width)."""
    return W >= 32 and H >= 32 and W % 32 == 0 and H % 32 == 0 and W <= 1024


def sent_cls_head_loss(hid, cls3_w, cls3_b, labels, g=1.0):
    """isc_sent_cls_head_loss on its own: hid [B,H] (the head's hidden layer), labels [B] int64 in [0, k) -> dict of
    logits [B,k], pred [B] int32, loss_rows [B], dz [B,8] (= g (softmax - onehot) / B, columns k..7 zero), dhid [B,H],
    dw3 [k,H], db3 [k], loss [1], wrong [1] int32."""
    require_device(hid, cls3_w, cls3_b, labels)
    assert hid.dtype == torch.float32 and hid.is_contiguous() and cls3_w.is_contiguous() and cls3_b.is_contiguous()
    assert labels.dtype == torch.int64 and labels.is_contiguous()
    B, H = hid.shape
    k = cls3_w.shape[0]
    dev = hid.device
    new = lambda *s, dt=torch.float32: torch.empty(*s, dtype=dt, device=dev)
    o = dict(logits=new(B, k), pred=new(B, dt=torch.int32), loss_rows=new(B), dz=new(B, 8), dhid=new(B, H),
             dw3=new(k, H), db3=new(k), loss=new(1), wrong=new(1, dt=torch.int32))
    check(_lib.load().isc_sent_cls_head_loss(hid.data_ptr(), cls3_w.data_ptr(), cls3_b.data_ptr(), labels.data_ptr(), B, H,
                                             k, float(g), *[o[n].data_ptr() for n in
                                                            ('logits', 'pred', 'loss_rows', 'dz', 'dhid', 'dw3', 'db3',
                                                             'loss', 'wrong')], stream()), 'isc_sent_cls_head_loss')
    return o


def sent_cls_pool_bwd(dfeats, e2, o, weights, lens_i32, de2=None, d_o=None, want_dw=True):
    """isc_sent_cls_pool_bwd on its own: dfeats [B,H], e2 and o [L,B,H] (time-major), weights [B,>=L], lens [B] int32 ->
    (de2 [L,B,H], d_o [L,B,H], dw [B,L] or None); the two outputs may be handed in (they are overwritten in full)."""
    require_device(dfeats, e2, o, weights, lens_i32)
    L, B, H = e2.shape
    assert dfeats.shape == (B, H) and o.shape == (L, B, H) and weights.shape[0] == B and weights.stride(1) == 1
    assert dfeats.is_contiguous() and e2.is_contiguous() and o.is_contiguous()
    assert lens_i32.dtype == torch.int32 and lens_i32.is_contiguous() and lens_i32.shape == (B,)
    de2 = torch.empty_like(e2) if de2 is None else de2
    d_o = torch.empty_like(o) if d_o is None else d_o
    assert de2.is_contiguous() and d_o.is_contiguous() and de2.shape == e2.shape and d_o.shape == o.shape
    dw = torch.empty(B, L, dtype=torch.float32, device=e2.device) if want_dw else None
    check(_lib.load().isc_sent_cls_pool_bwd(dfeats.data_ptr(), e2.data_ptr(), o.data_ptr(), weights.data_ptr(),
                                            weights.stride(0), lens_i32.data_ptr(), B, L, H, de2.data_ptr(), d_o.data_ptr(),
                                            ptr(dw), stream()), 'isc_sent_cls_pool_bwd')
    return de2, d_o, dw


def sent_cls_train_fwd(params, tokens, lens_i32, labels, grad_scale=1.0, keep_masks=None, mask_scale=1.0, pad_id=-1):
    """isc_sent_cls_train_fwd: the saved-activation forward and the loss.  params / tokens / lens_i32 as sent_cls_fwd,
    labels [B] int64; keep_masks = None or (emb_keep [L*B,W], out_keep [L*B,H], hid_keep [B,H]) uint8 over the time-major
    rows t*B+b (any of them None).  -> a state dict: logits, weights [B,L], pred, loss [1], wrong [1] int32, the scaled
    d_cls3_w / d_cls3_b, and what sent_cls_bwd needs (the filled problem struct and the tensors it points at)."""
    lib = _lib.load()
    assert len(params) == len(SENT_CLS_PARAMS)
    require_device(tokens, lens_i32, labels, *params)
    assert tokens.dtype == torch.int64 and tokens.dim() == 2 and tokens.stride(1) == 1
    B, L = tokens.shape
    assert lens_i32.dtype == torch.int32 and lens_i32.is_contiguous() and lens_i32.shape == (B,)
    assert labels.dtype == torch.int64 and labels.is_contiguous() and labels.shape == (B,)
    for t in params:
        assert t.dtype == torch.float32 and t.is_contiguous(), 'classifier parameters: contiguous fp32'
    V, W = params[0].shape
    H = params[2].shape[1]
    k = params[11].shape[0]
    dev = tokens.device
    masks = tuple(keep_masks) if keep_masks is not None else (None, None, None)
    for m, shape in zip(masks, ((L * B, W), (L * B, H), (B, H))):
        assert m is None or (m.dtype == torch.uint8 and m.is_contiguous() and m.shape == shape and m.device == dev)
    new = lambda *s, dt=torch.float32: torch.empty(*s, dtype=dt, device=dev)
    st = dict(logits=new(B, k), weights=new(B, L), pred=new(B, dt=torch.int32), loss=new(1),
              wrong=new(1, dt=torch.int32), d_cls3_w=new(k, H), d_cls3_b=new(k),
              saved=new(max(int(lib.isc_sent_cls_train_saved_bytes(B, L, W, H)), 16), dt=torch.uint8),
              keep=(params, tokens, lens_i32, labels, masks))
    p = _lib.SentClsTrainProblem()
    p.B, p.L, p.W, p.H, p.V, p.k, p.T_out = B, L, W, H, V, k, L
    p.tokens, p.tokens_ld, p.lens, p.labels = tokens.data_ptr(), tokens.stride(0), lens_i32.data_ptr(), labels.data_ptr()
    for name, t in zip(SENT_CLS_PARAMS, params):
        setattr(p, name, t.data_ptr())
    p.emb_keep, p.out_keep, p.hid_keep = (ptr(m) for m in masks)
    p.mask_scale, p.grad_scale, p.pad_id = float(mask_scale), float(grad_scale), int(pad_id)
    p.saved, p.saved_bytes = st['saved'].data_ptr(), st['saved'].numel()
    for name in ('logits', 'weights', 'pred', 'loss', 'wrong', 'd_cls3_w', 'd_cls3_b'):
        setattr(p, name, st[name].data_ptr())
    check(lib.isc_sent_cls_train_fwd(C.byref(p), stream()), 'isc_sent_cls_train_fwd')
    st['problem'] = p
    return st


def sent_cls_bwd(state):
    """isc_sent_cls_bwd: the reverse sweep behind sent_cls_train_fwd's state -> the thirteen gradients in SENT_CLS_PARAMS
    order, each times the forward's grad_scale (d_cls3_w / d_cls3_b are the forward's)."""
    lib = _lib.load()
    p = state['problem']
    params = state['keep'][0]
    dev = params[0].device
    grads = [state[n] if n in state else torch.empty_like(t) for n, t in zip(SENT_CLS_GRADS, params)]
    ws = torch.empty(max(int(lib.isc_sent_cls_bwd_workspace_bytes(p.B, p.L, p.W, p.H, p.V)), 16), dtype=torch.uint8,
                     device=dev)
    sk = splitk_ws(dev)
    p.workspace, p.workspace_bytes = ws.data_ptr(), ws.numel()
    p.splitk_ws, p.splitk_ws_floats = sk.data_ptr(), sk.numel()
    for name, g in zip(SENT_CLS_GRADS, grads):
        setattr(p, name, g.data_ptr())
    check(lib.isc_sent_cls_bwd(C.byref(p), stream()), 'isc_sent_cls_bwd')
    return grads


_SENTI_DET_WS = {}          # (device index, stream, B, h, w, C, n_convs, ksplit) -> workspace of isc_senti_det_fwd


def senti_det_launches(kind=None):
    """Launches of the image-sentiment detector's kernels so far: a dict over _lib.SENTI_DET_KINDS ('direct', 'split',
    'reduce', 'tail', 'pack', 'f16' = conv launches that read float16 rows natively), or one kind's count."""
    lib = _lib.load()
    if kind is not None:
        return lib.isc_senti_det_launches(_lib.SENTI_DET_KINDS.index(kind))
    return {name: lib.isc_senti_det_launches(i) for i, name in enumerate(_lib.SENTI_DET_KINDS)}


def _senti_det_split_params(params):
    """params: the module's tensors in state_dict order - (weight, bias) of every 3x3 conv, of the 1x1 senti_conv and of
    every FC layer -> (conv weights, conv biases, senti_w, senti_b, fc weights, fc biases)."""
    params = list(params)
    assert len(params) >= 4 and len(params) % 2 == 0, 'weight / bias pairs: convs, senti_conv, fcs'
    n_convs = 0
    while 2 * n_convs < len(params) and params[2 * n_convs].dim() == 4 and tuple(params[2 * n_convs].shape[2:]) == (3, 3):
        n_convs += 1
    assert n_convs >= 1 and len(params) >= 2 * n_convs + 2
    conv_w, conv_b = params[0:2 * n_convs:2], params[1:2 * n_convs:2]
    senti_w, senti_b = params[2 * n_convs], params[2 * n_convs + 1]
    fc_w, fc_b = params[2 * n_convs + 2::2], params[2 * n_convs + 3::2]
    return conv_w, conv_b, senti_w, senti_b, fc_w, fc_b


def senti_det_pack(conv_weights):
    """The detector's conv weights ([Cout, Cin, 3, 3] fp32, layer after layer) as the split-f16 planes isc_senti_det_fwd
    reads (isc_senti_det_pack: tap-major K = 9 Cin, one launch per layer) -> a uint8 tensor.  The weights are frozen: pack
    once per weight version."""
    lib = _lib.load()
    conv_weights = list(conv_weights)
    require_device(*conv_weights)
    Cf, n = conv_weights[0].shape[1], len(conv_weights)
    for i, t in enumerate(conv_weights):
        assert t.dtype == torch.float32 and t.is_contiguous(), 'conv weights: contiguous fp32'
        if tuple(t.shape) != ((Cf >> i) // 2, Cf >> i, 3, 3):
            raise _lib.HipLibraryError('isc_senti_det_pack failed: ISC_E_SHAPE (conv %d is %s)' % (i, tuple(t.shape)))
    nbytes = int(lib.isc_senti_det_pack_bytes(Cf, n))
    packed = torch.empty(max(nbytes, 16), dtype=torch.uint8, device=conv_weights[0].device)
    ptrs = (C.c_void_p * n)(*[t.data_ptr() for t in conv_weights])
    check(lib.isc_senti_det_pack(ptrs, Cf, n, packed.data_ptr(), stream()), 'isc_senti_det_pack')
    return packed


def senti_det_fwd(params, feats, threshold, neu_idx, *, packed=None, ksplit=0, out=None, want_conv_out=False,
                  workspace=None):
    """The frozen image-sentiment detector's forward (isc_senti_det_fwd): `params` = the module's tensors in state_dict
    order ((weight, bias) of every 3x3 conv, of senti_conv and of every FC layer), feats [B,h,w,C] contiguous, fp32 or
    float16 (read natively).  packed: senti_det_pack(conv weights) - built here when None.  ksplit: 0 = the library
    chooses each conv layer's route, n >= 1 forces n workgroups per tile.  -> (logits [B,k], maps [B,h,w], labels [B]
    int64, scores [B][, conv_out [B*h*w, C >> n_convs]]).  `out` = (logits, maps, labels, scores) to write into.  The
    workspace is kept per (device, stream, geometry) except inside a graph capture (hand `workspace`, or a fresh one is
    drawn from the capture's pool).  A shape the library does not take raises (ISC_E_SHAPE); nothing is launched or
    written then."""
    lib = _lib.load()
    conv_w, conv_b, senti_w, senti_b, fc_w, fc_b = _senti_det_split_params(params)
    require_device(feats, *params)
    register_status_words(feats.device)                 # (a non-finite logit flags the numerics status)
    assert feats.dim() == 4 and feats.is_contiguous() and feats.dtype in (torch.float32, torch.float16)
    for t in list(params):
        assert t.dtype == torch.float32 and t.is_contiguous(), 'detector parameters: contiguous fp32'
    B, h, w, Cf = feats.shape
    n_convs, n_fcs, k = len(conv_w), len(fc_w), senti_w.shape[0]
    dev = feats.device
    if n_convs > _lib.SENTI_DET_MAX_CONVS or n_fcs > _lib.SENTI_DET_MAX_FCS or conv_w[0].shape[1] != Cf or \
            senti_w.numel() != k * (Cf >> n_convs):
        raise _lib.HipLibraryError('isc_senti_det_fwd failed: ISC_E_SHAPE (unsupported size)')
    CL = Cf >> n_convs
    if out is None:
        out = (torch.empty(B, k, dtype=torch.float32, device=dev), torch.empty(B, h, w, dtype=torch.float32, device=dev),
               torch.empty(B, dtype=torch.int64, device=dev), torch.empty(B, dtype=torch.float32, device=dev))
    logits, maps, labels, scores = out
    assert logits.shape == (B, k) and maps.shape == (B, h, w) and labels.shape == (B,) and scores.shape == (B,)
    assert labels.dtype == torch.int64 and all(t.is_contiguous() for t in out)
    need = int(lib.isc_senti_det_workspace_bytes(B, h, w, Cf, n_convs, int(ksplit)))   # (0: refused - said below)
    if need and packed is None:
        packed = senti_det_pack(conv_w)
    if workspace is None:
        if torch.cuda.is_current_stream_capturing():
            workspace = torch.empty(max(need, 16), dtype=torch.uint8, device=dev)
        else:
            key = (dev.index, torch.cuda.current_stream(dev).cuda_stream, B, h, w, Cf, n_convs, int(ksplit))
            workspace = _SENTI_DET_WS.get(key)
            if workspace is None:
                workspace = _SENTI_DET_WS[key] = torch.empty(max(need, 16), dtype=torch.uint8, device=dev)
    conv_out = torch.empty(B * h * w, CL, dtype=torch.float32, device=dev) if want_conv_out else None
    p = _lib.SentiDetProblem()
    p.feats, p.feats_f16 = feats.data_ptr(), int(feats.dtype == torch.float16)
    p.B, p.h, p.w, p.C, p.n_convs, p.n_fcs, p.k = B, h, w, Cf, n_convs, n_fcs, k
    p.neu_idx, p.ksplit, p.threshold = int(neu_idx), int(ksplit), float(threshold)
    p.packed = packed.data_ptr() if packed is not None else workspace.data_ptr()   # (refused shapes: never read)
    for i, t in enumerate(conv_b):
        p.conv_b[i] = t.data_ptr()
    p.senti_w, p.senti_b = senti_w.data_ptr(), senti_b.data_ptr()
    for i, (tw, tb) in enumerate(zip(fc_w, fc_b)):
        p.fc_w[i], p.fc_b[i] = tw.data_ptr(), tb.data_ptr()
    p.workspace, p.workspace_bytes = workspace.data_ptr(), workspace.numel()
    p.logits, p.maps, p.labels, p.scores = logits.data_ptr(), maps.data_ptr(), labels.data_ptr(), scores.data_ptr()
    p.conv_out = ptr(conv_out)
    check(lib.isc_senti_det_fwd(C.byref(p), stream()), 'isc_senti_det_fwd')
    return (logits, maps, labels, scores) + ((conv_out,) if want_conv_out else ())


# ---- the detector's training (isc_senti_det_train_fwd / isc_senti_det_bwd and two of its kernels on their own)
_SENTI_DET_TRAIN_WS = {}    # (device index, stream, B, h, w, C, n_convs, n_fcs) -> (saved, backward workspace)


def senti_det_bwd_launches(kind=None):
    """Launches of the detector's training calls so far: a dict over _lib.SENTI_DET_TRAIN_KINDS ('fwd', 'bwd', and of
    either 'reduce' = slab reduces behind split-route convolutions), or one kind's count."""
    lib = _lib.load()
    if kind is not None:
        return lib.isc_senti_det_bwd_launches(_lib.SENTI_DET_TRAIN_KINDS.index(kind))
    return {name: lib.isc_senti_det_bwd_launches(i) for i, name in enumerate(_lib.SENTI_DET_TRAIN_KINDS)}


def senti_det_train_buffers(dev, B, h, w, Cf, n_convs, n_fcs):
    """(saved, workspace) of one training iteration.  saved belongs to the iteration (the caching allocator hands it
    out without a device call); the backward's workspace is scratch, kept per (device, stream, geometry) as
    _SENTI_DET_WS is - except inside a graph capture (a fresh one from the capture's pool)."""
    lib = _lib.load()
    new = lambda n: torch.empty(max(int(n), 16), dtype=torch.uint8, device=dev)
    saved = new(lib.isc_senti_det_train_saved_bytes(B, h, w, Cf, n_convs, n_fcs))
    need = lib.isc_senti_det_bwd_workspace_bytes(B, h, w, Cf, n_convs)
    if torch.cuda.is_current_stream_capturing():
        return saved, new(need)
    key = (dev.index, torch.cuda.current_stream(dev).cuda_stream, B, h, w, Cf, n_convs, n_fcs)
    ws = _SENTI_DET_TRAIN_WS.get(key)
    if ws is None:
        ws = _SENTI_DET_TRAIN_WS[key] = new(need)
    return saved, ws


def senti_det_train_fwd(params, feats, labels, scale=1.0, keep=None, mask_scale=1.0, buffers=None):
    """isc_senti_det_train_fwd: the saved-activation forward and the loss.  params as senti_det_fwd, feats [B,h,w,C] fp32
    contiguous, labels [B] int64 on the device, keep = None or a uint8 keep-mask [B,h,w,C >> n_convs].  -> a state dict:
    logits [B,k], maps [B,h,w], loss [1] (= scale * mean cross-entropy) and what senti_det_bwd needs."""
    lib = _lib.load()
    conv_w, conv_b, senti_w, senti_b, fc_w, fc_b = _senti_det_split_params(params)
    require_device(feats, labels, *params)
    register_status_words(feats.device)
    assert feats.dim() == 4 and feats.is_contiguous() and feats.dtype == torch.float32
    for t in list(params):
        assert t.dtype == torch.float32 and t.is_contiguous(), 'detector parameters: contiguous fp32'
    B, h, w, Cf = feats.shape
    n_convs, n_fcs, k = len(conv_w), len(fc_w), senti_w.shape[0]
    dev = feats.device
    if n_convs > _lib.SENTI_DET_MAX_CONVS or n_fcs > _lib.SENTI_DET_MAX_FCS or conv_w[0].shape[1] != Cf or \
            senti_w.numel() != k * (Cf >> n_convs):
        raise _lib.HipLibraryError('isc_senti_det_train_fwd failed: ISC_E_SHAPE (unsupported size)')
    assert labels.dtype == torch.int64 and labels.is_contiguous() and labels.shape == (B,)
    CL = Cf >> n_convs
    assert keep is None or (keep.dtype == torch.uint8 and keep.is_contiguous() and keep.numel() == B * h * w * CL
                            and keep.device == dev)
    saved, workspace = buffers if buffers is not None else senti_det_train_buffers(dev, B, h, w, Cf, n_convs, n_fcs)
    new = lambda *s: torch.empty(*s, dtype=torch.float32, device=dev)
    st = dict(logits=new(B, k), maps=new(B, h, w), loss=new(1), saved=saved, workspace=workspace,
              keep=(list(params), feats, labels, keep))
    p = _lib.SentiDetTrainProblem()
    p.feats = feats.data_ptr()
    p.B, p.h, p.w, p.C, p.n_convs, p.n_fcs, p.k = B, h, w, Cf, n_convs, n_fcs, k
    p.mask_scale, p.scale = float(mask_scale), float(scale)
    for i, (tw, tb) in enumerate(zip(conv_w, conv_b)):
        p.conv_w[i], p.conv_b[i] = tw.data_ptr(), tb.data_ptr()
    p.senti_w, p.senti_b = senti_w.data_ptr(), senti_b.data_ptr()
    for i, (tw, tb) in enumerate(zip(fc_w, fc_b)):
        p.fc_w[i], p.fc_b[i] = tw.data_ptr(), tb.data_ptr()
    p.labels, p.keep = labels.data_ptr(), ptr(keep)
    p.saved, p.saved_bytes = saved.data_ptr(), saved.numel()
    p.logits, p.maps, p.loss = st['logits'].data_ptr(), st['maps'].data_ptr(), st['loss'].data_ptr()
    check(lib.isc_senti_det_train_fwd(C.byref(p), stream()), 'isc_senti_det_train_fwd')
    st['problem'] = p
    return st


def senti_det_bwd(state, want_dx=False):
    """isc_senti_det_bwd: the reverse sweep behind senti_det_train_fwd's state -> the gradients in the order of `params`
    [, dx [B*h*w, C/2]: the gradient of conv_0's output (tests; two convs or more)]."""
    lib = _lib.load()
    p = state['problem']
    params = state['keep'][0]
    grads = [torch.empty_like(t) for t in params]
    conv_w, conv_b, senti_w, senti_b, fc_w, fc_b = _senti_det_split_params(grads)
    for i, (tw, tb) in enumerate(zip(conv_w, conv_b)):
        p.d_conv_w[i], p.d_conv_b[i] = tw.data_ptr(), tb.data_ptr()
    p.d_senti_w, p.d_senti_b = senti_w.data_ptr(), senti_b.data_ptr()
    for i, (tw, tb) in enumerate(zip(fc_w, fc_b)):
        p.d_fc_w[i], p.d_fc_b[i] = tw.data_ptr(), tb.data_ptr()
    ws = state['workspace']
    p.workspace, p.workspace_bytes = ws.data_ptr(), ws.numel()
    dx = torch.empty(p.B * p.h * p.w, p.C // 2, dtype=torch.float32, device=ws.device) if want_dx else None
    p.dx_out = ptr(dx)
    check(lib.isc_senti_det_bwd(C.byref(p), stream()), 'isc_senti_det_bwd')
    return grads + ([dx] if want_dx else [])


def senti_det_bwd_tail(state):
    """What isc_senti_det_bwd's first two launches left in the workspace of `state` (after senti_det_bwd; tests): a dict
    of views - g [n_fcs,B,8], dpool [B,8], rsum [B,CL], dr [B,CL], eb [B], ratio [B]."""
    p = state['problem']
    off = (C.c_int64 * 6)()
    check(_lib.load().isc_senti_det_bwd_tail_offsets(p.B, p.h, p.w, p.C, p.n_convs, off), 'isc_senti_det_bwd_tail_offsets')
    ws = state['workspace'].view(torch.float32)
    CL = p.C >> p.n_convs
    shapes = dict(g=(p.n_fcs, p.B, 8), dpool=(p.B, 8), rsum=(p.B, CL), dr=(p.B, CL), eb=(p.B,), ratio=(p.B,))
    out = {}
    for o, (name, shape) in zip(off, shapes.items()):
        n = 1
        for d in shape:
            n *= d
        out[name] = ws[o:o + n].view(shape)
    return out


def senti_det_dw(dy, x, Cout, ratio=None, unscale=None):
    """isc_senti_det_dw on its own: dy [B*h*w, ld >= Cout], x [B,h,w,Cin] fp32 -> dw [Cout,Cin,3,3] =
    unscale * sum_m dy[m,co] ratio[b(m)] x[pixel(m) + tap, ci]; ratio [B] / unscale [1] device tensors or None (= 1)."""
    require_device(dy, x)
    assert dy.dtype == x.dtype == torch.float32 and dy.is_contiguous() and x.is_contiguous() and x.dim() == 4
    B, h, w, Cin = x.shape
    assert dy.shape[0] == B * h * w
    dw = torch.empty(Cout, Cin, 3, 3, dtype=torch.float32, device=x.device)
    check(_lib.load().isc_senti_det_dw(dy.data_ptr(), dy.shape[1], x.data_ptr(), B, h, w, Cin, Cout, ptr(ratio),
                                       ptr(unscale), dw.data_ptr(), stream()), 'isc_senti_det_dw')
    return dw


def senti_det_pack_flipped(w):
    """isc_senti_det_pack_flipped: w [Cout,Cin,3,3] -> the float16 planes [Cin, 2 * 9 * Cp] (Cp = Cout rounded up to 32)
    of W'[ci, (2-ky, 2-kx), co] = w[co, ci, ky, kx] in the plane layout of the convolution kernel."""
    require_device(w)
    assert w.dtype == torch.float32 and w.is_contiguous() and w.dim() == 4 and tuple(w.shape[2:]) == (3, 3)
    Cout, Cin = w.shape[:2]
    Cp = (Cout + 31) // 32 * 32
    planes = torch.empty(Cin, 2 * 9 * Cp, dtype=torch.float16, device=w.device)
    check(_lib.load().isc_senti_det_pack_flipped(w.data_ptr(), Cout, Cin, planes.data_ptr(), stream()),
          'isc_senti_det_pack_flipped')
    return planes


__all__ = [n for n in dir() if n.endswith('_fwd') or n.endswith('_problem')] + [
    'RolloutStep', 'rollout_finalize', 'rollout_finalize_filtered', 'beam_topk', 'logsoftmax_apply', 'require_device']


# ---------------------------------------------------------------------------- backward
NN, TN = 1, 2


def gemm_problem(segs, out, layout, accumulate=False, bias0=None):
    """layout NN: out[M,N] (+)= sum_s A_s[M,K] @ W_s[K,N];  TN: out[M,N] (+)= sum_s A_s[K,M]^T @ W_s[K,N].
    All operands are 2-D views with unit inner stride."""
    p = LinearProblem()
    if not 1 <= len(segs) <= _lib.ISC_MAX_SEG:
        raise ValueError('1..4 K-segments supported')
    p.nseg = len(segs)
    p.M, p.N = out.shape
    for i, (A, W) in enumerate(segs):
        assert A.dim() == 2 and W.dim() == 2 and A.stride(1) == 1 and W.stride(1) == 1
        assert A.dtype == torch.float32 and W.dtype == torch.float32
        s = p.seg[i]
        s.A, s.W, s.lda, s.ldw = A.data_ptr(), W.data_ptr(), A.stride(0), W.stride(0)
        if layout == NN:
            assert A.shape[0] == p.M and W.shape[1] == p.N and A.shape[1] >= W.shape[0], (A.shape, W.shape)
            s.K = W.shape[0]
        else:
            assert A.shape[1] == p.M and W.shape[1] == p.N and A.shape[0] == W.shape[0], (A.shape, W.shape)
            s.K = A.shape[0]
    assert out.stride(1) == 1
    p.ldc, p.C = out.stride(0), out.data_ptr()
    p.accumulate = int(accumulate)
    p.bias0 = ptr(bias0)
    return p


def gemm_bwd(problems, layout):
    lib = _lib.load()
    _attach_ws(problems[0], torch.cuda.current_device())
    arr = (LinearProblem * len(problems))(*problems)
    e0 = TIMER.begin()
    check(lib.isc_gemm_bwd(arr, len(problems), layout, stream()), 'isc_gemm_bwd')
    if e0 is not None:
        fl = sum(2.0 * q.M * q.N * sum(q.seg[i].K for i in range(q.nseg)) for q in problems)
        TIMER.end(e0, ('gemm_nn[' if layout == NN else 'gemm_tn[') +
                  '+'.join('%dx%dx%d' % (q.M, q.N, sum(q.seg[i].K for i in range(q.nseg))) for q in problems) + ']',
                  fl)


def logsoftmax_bwd(dlogp, logp, dlogits, M, V, remap_T=0):
    """dlogp/logp: M contiguous rows of V; dlogits [M, ld_out>=V] (padding zero-filled).
    remap_T>0: input rows are (b,t) b-major, output rows (t,b) t-major."""
    lib = _lib.load()
    assert dlogp.is_contiguous() and logp.is_contiguous() and dlogits.stride(1) == 1
    check(lib.isc_logsoftmax_bwd(dlogp.data_ptr(), logp.data_ptr(), V, M, V, dlogits.data_ptr(),
                                 dlogits.stride(0), remap_T, stream()), 'isc_logsoftmax_bwd')


def logsoftmax_bwd_sparse(dense, logp, sparse, dlogits, M, V, remap_T=0, scale=None, out_step_rows=0):
    """isc_logsoftmax_bwd_sparse: d logits from an optional dense d log-prob [M,V] plus up to two (ids [M] int64,
    coef [M] fp32) pairs - one column per row each - times the optional device scalar `scale`.
    out_step_rows > 0 (with remap_T): rows per step of the time-major output; `dlogits` starts at this branch's first row."""
    lib = _lib.load()
    assert logp.is_contiguous() and dlogits.stride(1) == 1 and (dense is None or dense.is_contiguous())
    n = len(sparse)
    ids = (C.c_void_p * max(n, 1))(*[i.data_ptr() for i, _ in sparse])
    cf = (C.c_void_p * max(n, 1))(*[c.data_ptr() for _, c in sparse])
    for i, c in sparse:
        assert i.dtype == torch.int64 and c.dtype == torch.float32 and i.is_contiguous() and c.is_contiguous()
        assert i.numel() == M and c.numel() == M
    check(lib.isc_logsoftmax_bwd_sparse(ptr(dense), logp.data_ptr(), V, M, V, ids, cf, n, ptr(scale),
                                        dlogits.data_ptr(), dlogits.stride(0), remap_T, int(out_step_rows), stream()),
          'isc_logsoftmax_bwd_sparse')


def gather_logp_raw(raw, ld_b, ld_t, B, T, V, part_max, part_sum, step_rows, ids, out, live=None):
    """out[b,t] = log p(ids[b,t]) from the RAW logits (row (b,t) at raw + b*ld_b + t*ld_t floats) and the step-stacked
    tile statistics (row t*step_rows + b) - isc_gather_logp_raw; `live` [T] optionally multiplies column t."""
    assert ids.dtype == torch.int64 and ids.is_contiguous() and ids.numel() == B * T and out.is_contiguous()
    assert out.numel() == B * T and out.dtype == torch.float32
    check(_lib.load().isc_gather_logp_raw(raw.data_ptr(), int(ld_b), int(ld_t), B, T, V, part_max.data_ptr(),
                                          part_sum.data_ptr(), int(step_rows), ids.data_ptr(), ptr(live), out.data_ptr(),
                                          stream()), 'isc_gather_logp_raw')


def xe_loss_tokens_fwd(tlp, lengths_i32, out2):
    B, T = tlp.shape
    assert tlp.is_contiguous() and tlp.dtype == torch.float32
    check(_lib.load().isc_xe_loss_tokens_fwd(tlp.data_ptr(), lengths_i32.data_ptr(), B, T, out2.data_ptr(), stream()),
          'isc_xe_loss_tokens_fwd')


def logsoftmax_bwd_raw(raw, ld_b, ld_t, B, T, V, part_max, part_sum, step_rows, sparse, dlogits, scale=None,
                       out_step_rows=0):
    """isc_logsoftmax_bwd_raw: d logits (time-major rows t*out_step_rows + b of `dlogits`) from (ids, coef) pairs in
    [B,T] order, the softmax term recomputed from the raw logits and their tile statistics."""
    n = len(sparse)
    assert 1 <= n <= 2 and dlogits.stride(1) == 1
    for i, c in sparse:
        assert i.dtype == torch.int64 and c.dtype == torch.float32 and i.is_contiguous() and c.is_contiguous()
        assert i.numel() == B * T and c.numel() == B * T
    ids = (C.c_void_p * n)(*[i.data_ptr() for i, _ in sparse])
    cf = (C.c_void_p * n)(*[c.data_ptr() for _, c in sparse])
    check(_lib.load().isc_logsoftmax_bwd_raw(raw.data_ptr(), int(ld_b), int(ld_t), B, T, V, part_max.data_ptr(),
                                             part_sum.data_ptr(), int(step_rows), ids, cf, n, ptr(scale), dlogits.data_ptr(),
                                             dlogits.stride(0), int(out_step_rows), stream()), 'isc_logsoftmax_bwd_raw')


def logsoftmax_bwd_raw_filtered(raw, ld_b, ld_t, B, T, V, part_max, part_sum, step_rows, sparse, flt, dlogits, scale=None,
                                out_step_rows=0):
    """isc_logsoftmax_bwd_raw_filtered: logsoftmax_bwd_raw's d logits (zero to two model pairs) plus, in the same pass,
    the gradient of the sampled distribution's log-probability.  flt: a mapping with 'tok' (int64 [B,T]), 'coef' (fp32
    [B,T]), 'inv_tau' and the forward's saved 'kstar' (int64), 'gmax', 'logz' (fp32) [B,T], 'ban' (int32 [B,T,10] or
    None)."""
    n = len(sparse)
    assert 0 <= n <= 2 and dlogits.stride(1) == 1
    for i, c in sparse:
        assert i.dtype == torch.int64 and c.dtype == torch.float32 and i.is_contiguous() and c.is_contiguous()
        assert i.numel() == B * T and c.numel() == B * T
    for k, dt in (('tok', torch.int64), ('kstar', torch.int64), ('coef', torch.float32), ('gmax', torch.float32),
                  ('logz', torch.float32)):
        assert flt[k].dtype == dt and flt[k].is_contiguous() and flt[k].numel() == B * T, k
    ban = flt.get('ban')
    assert ban is None or (ban.dtype == torch.int32 and ban.is_contiguous() and ban.numel() == B * T * 10)
    ids = (C.c_void_p * max(n, 1))(*[i.data_ptr() for i, _ in sparse])
    cf = (C.c_void_p * max(n, 1))(*[c.data_ptr() for _, c in sparse])
    check(_lib.load().isc_logsoftmax_bwd_raw_filtered(
        raw.data_ptr(), int(ld_b), int(ld_t), B, T, V, ptr(part_max), ptr(part_sum), int(step_rows), ids, cf, n,
        flt['tok'].data_ptr(), flt['coef'].data_ptr(), float(flt['inv_tau']), flt['kstar'].data_ptr(),
        flt['gmax'].data_ptr(), flt['logz'].data_ptr(), ptr(ban), ptr(scale), dlogits.data_ptr(), dlogits.stride(0),
        int(out_step_rows), stream()), 'isc_logsoftmax_bwd_raw_filtered')


def grad_scale(sources, out2, maxima=()):
    """isc_grad_scale: out[0:2] = {S, 1/S}, S the power of two that brings max |x| over `sources` into [2^-4, 2^-3);
    `out2` is a ZEROED float32[4] (its last two words are the reduction's state, left zeroed).  `maxima`: [1] tensors
    max |x| of further gradients, joined into one source.  Any number of sources: past the library's ISC_SCALE_SRC_MAX,
    the surplus is reduced to its maxima and joins them."""
    assert out2.numel() >= 4
    srcs = [x for x in sources if x is not None and x.numel() > 0]
    maxima = list(maxima)
    cap = _lib.ISC_SCALE_SRC_MAX
    if len(srcs) + (1 if maxima else 0) > cap:
        maxima += [x.abs().amax().reshape(1) for x in srcs[cap - 1:]]
        srcs = srcs[:cap - 1]
    if maxima:
        srcs.append(torch.cat(maxima))
    for x in srcs:
        assert x.dtype == torch.float32 and x.is_contiguous()
    n = len(srcs)
    pp = (C.c_void_p * max(n, 1))(*[x.data_ptr() for x in srcs])
    nn_ = (C.c_int64 * max(n, 1))(*[x.numel() for x in srcs])
    check(_lib.load().isc_grad_scale(pp, nn_, n, out2.data_ptr(), stream()), 'isc_grad_scale')


def xe_loss_bwd_sparse(lengths_i32, T, gout, sum_count, coef):
    B = lengths_i32.numel()
    check(_lib.load().isc_xe_loss_bwd_sparse(lengths_i32.data_ptr(), B, T, gout.data_ptr(), sum_count.data_ptr(),
                                             coef.data_ptr(), stream()), 'isc_xe_loss_bwd_sparse')


def reward_loss_fwd(seq_logprobs, seq_masks, reward, out2):
    B, T = seq_logprobs.shape
    check(_lib.load().isc_reward_loss_fwd(seq_logprobs.data_ptr(), seq_masks.data_ptr(), reward.data_ptr(), B, T,
                                          out2.data_ptr(), stream()), 'isc_reward_loss_fwd')


def reward_loss_bwd(seq_masks, reward, gout, sum_count, dlogp):
    B, T = seq_masks.shape
    check(_lib.load().isc_reward_loss_bwd(seq_masks.data_ptr(), reward.data_ptr(), B, T, gout.data_ptr(),
                                          sum_count.data_ptr(), dlogp.data_ptr(), stream()), 'isc_reward_loss_bwd')


def group_reward(scores, n, cls_reward, cls_flag, T, reward=None, stats4=None):
    """isc_group_reward: the reward of self-critical RL on n samples per image from the I*n float64 scores on the device
    (row i*n + j = sample j of image i) and the optional classifier reward [I*n, T] fp32.  Returns (reward [I*n, T] fp32,
    stats4 float64 = mean score, mean advantage, mean classifier reward, mean reward)."""
    require_device(scores, cls_reward)
    assert scores.dtype == torch.float64 and scores.dim() == 1 and scores.is_contiguous()
    rows, n, T = scores.numel(), int(n), int(T)
    assert n >= 1 and rows % n == 0
    if cls_reward is not None:
        assert cls_reward.dtype == torch.float32 and cls_reward.is_contiguous() and tuple(cls_reward.shape) == (rows, T)
    if reward is None:
        reward = torch.empty(rows, T, dtype=torch.float32, device=scores.device)
    if stats4 is None:
        stats4 = torch.empty(4, dtype=torch.float64, device=scores.device)
    assert reward.dtype == torch.float32 and reward.is_contiguous() and reward.numel() == rows * T
    assert stats4.dtype == torch.float64 and stats4.is_contiguous() and stats4.numel() == 4
    check(_lib.load().isc_group_reward(scores.data_ptr(), rows // n, n, ptr(cls_reward), float(cls_flag), T,
                                       reward.data_ptr(), stats4.data_ptr(), stream()), 'isc_group_reward')
    return reward, stats4


def cider_dev_score(hyps, row_div, table, img_cap_off, ord_off, ref_norms, ref_length, ref_keys, ref_vals, n, sigma,
                    ref_len, sos_id, eos_id, out=None):
    """isc_cider_dev_score: CIDEr-D of the raw roll-out rows `hyps` int64 [N, T] on the device, row r against the cooked
    references of image r // row_div -> float64 [N].  table int64 [capacity, 2] (the 16-byte slots), img_cap_off int32
    [I + 1], ord_off int32 [C, 5], ref_norms float64 [C, 4], ref_length float64 [C], ref_keys int64 [E] (the keys' bits),
    ref_vals float64 [E] - rewards.DeviceCiderD builds them.  T > 63 raises (ISC_E_SHAPE); nothing is written then."""
    require_device(hyps, table, img_cap_off, ord_off, ref_norms, ref_length, ref_keys, ref_vals, out)
    assert hyps.dtype == torch.int64 and hyps.dim() == 2 and hyps.is_contiguous()
    assert table.dtype == torch.int64 and table.dim() == 2 and table.shape[1] == 2 and table.is_contiguous()
    assert img_cap_off.dtype == torch.int32 and img_cap_off.dim() == 1 and img_cap_off.is_contiguous()
    C_ = ref_length.numel()
    assert ord_off.dtype == torch.int32 and tuple(ord_off.shape) == (C_, 5) and ord_off.is_contiguous()
    assert ref_norms.dtype == torch.float64 and tuple(ref_norms.shape) == (C_, 4) and ref_norms.is_contiguous()
    assert ref_length.dtype == torch.float64 and ref_length.is_contiguous()
    assert ref_keys.dtype == torch.int64 and ref_vals.dtype == torch.float64 and ref_keys.shape == ref_vals.shape
    assert ref_keys.dim() == 1 and ref_keys.is_contiguous() and ref_vals.is_contiguous()
    N, T = hyps.shape
    if out is None:
        out = torch.empty(N, dtype=torch.float64, device=hyps.device)
    assert out.dtype == torch.float64 and out.is_contiguous() and out.numel() == N
    check(_lib.load().isc_cider_dev_score(hyps.data_ptr(), N, T, int(row_div), table.data_ptr(), table.shape[0],
                                          img_cap_off.data_ptr(), img_cap_off.numel() - 1, ord_off.data_ptr(),
                                          ref_norms.data_ptr(), ref_length.data_ptr(), ref_keys.data_ptr(),
                                          ref_vals.data_ptr(), int(n), float(sigma), float(ref_len), int(sos_id),
                                          int(eos_id), out.data_ptr(), stream()), 'isc_cider_dev_score')
    return out


def bleu_dev_score(hyps, row_div, img_ent_off, ref_keys, ref_counts, img_cap_off, ref_lens, order, sos_id, eos_id,
                   out=None, stats=None):
    """isc_bleu_dev_score: BLEU of the raw roll-out rows `hyps` int64 [N, T] on the device, row r against the cooked
    references of image r // row_div -> float64 [N] = BLEU-`order` (order 1..4) or [N, 4] (order 0).  img_ent_off int32
    [I, 5], ref_keys int64 [E] (the keys' bits), ref_counts int32 [E], img_cap_off int32 [I + 1], ref_lens int32 [C] -
    rewards.DeviceBleu builds them.  `stats`: int32 [N, 10] to fill, or None.  T > 63 raises (ISC_E_SHAPE); nothing is
    written then."""
    require_device(hyps, img_ent_off, ref_keys, ref_counts, img_cap_off, ref_lens, out, stats)
    assert hyps.dtype == torch.int64 and hyps.dim() == 2 and hyps.is_contiguous()
    n_img = img_cap_off.numel() - 1
    assert img_cap_off.dtype == torch.int32 and img_cap_off.dim() == 1 and img_cap_off.is_contiguous()
    assert img_ent_off.dtype == torch.int32 and tuple(img_ent_off.shape) == (n_img, 5) and img_ent_off.is_contiguous()
    assert ref_keys.dtype == torch.int64 and ref_counts.dtype == torch.int32 and ref_keys.shape == ref_counts.shape
    assert ref_keys.dim() == 1 and ref_keys.is_contiguous() and ref_counts.is_contiguous()
    assert ref_lens.dtype == torch.int32 and ref_lens.dim() == 1 and ref_lens.is_contiguous()
    N, T = hyps.shape
    order = int(order)
    cols = 4 if order == 0 else 1
    if out is None:
        out = torch.empty((N, 4) if order == 0 else (N,), dtype=torch.float64, device=hyps.device)
    assert out.dtype == torch.float64 and out.is_contiguous() and out.numel() == N * cols
    if stats is not None:
        assert stats.dtype == torch.int32 and stats.is_contiguous() and stats.numel() == N * 10
    check(_lib.load().isc_bleu_dev_score(hyps.data_ptr(), N, T, int(row_div), img_ent_off.data_ptr(), ref_keys.data_ptr(),
                                         ref_counts.data_ptr(), img_cap_off.data_ptr(), ref_lens.data_ptr(), n_img, order,
                                         int(sos_id), int(eos_id), out.data_ptr(), ptr(stats), stream()),
          'isc_bleu_dev_score')
    return out


def lm_dev_score(hyps, labels, slots, lm_off, lm_capacity, lm_order, vocab_size, eos_mode, unk_as_word, sos_id, eos_id,
                 out=None, n_scored=None, n_oov=None, tok_logp=None):
    """isc_lm_dev_score: the back-off language-model score of the raw rows `hyps` int64 [N, T] on the device, row r by
    model labels[r] (labels None: model 0) -> (score float64 [N], n_scored int32 [N], n_oov int32 [N]).  slots int64
    [S, 2] (the 16-byte slots), lm_off / lm_capacity int64 [n_lm], lm_order int32 [n_lm] - rewards.DeviceNgramLMSet builds
    them.  `tok_logp`: float64 [N, T + 2] to fill, or None.  T > 62 raises (ISC_E_SHAPE); nothing is written then."""
    require_device(hyps, labels, slots, lm_off, lm_capacity, lm_order, out, n_scored, n_oov, tok_logp)
    assert hyps.dtype == torch.int64 and hyps.dim() == 2 and hyps.is_contiguous()
    assert slots.dtype == torch.int64 and slots.dim() == 2 and slots.shape[1] == 2 and slots.is_contiguous()
    n_lm = lm_off.numel()
    assert lm_off.dtype == torch.int64 and lm_capacity.dtype == torch.int64 and lm_order.dtype == torch.int32
    assert n_lm >= 1 and lm_capacity.numel() == n_lm and lm_order.numel() == n_lm
    assert lm_off.is_contiguous() and lm_capacity.is_contiguous() and lm_order.is_contiguous()
    N, T = hyps.shape
    if labels is not None:
        assert labels.dtype == torch.int64 and labels.is_contiguous() and labels.numel() == N
    if out is None:
        out = torch.empty(N, dtype=torch.float64, device=hyps.device)
    if n_scored is None:
        n_scored = torch.empty(N, dtype=torch.int32, device=hyps.device)
    if n_oov is None:
        n_oov = torch.empty(N, dtype=torch.int32, device=hyps.device)
    assert out.dtype == torch.float64 and out.is_contiguous() and out.numel() == N
    for x in (n_scored, n_oov):
        assert x.dtype == torch.int32 and x.is_contiguous() and x.numel() == N
    if tok_logp is not None:
        assert tok_logp.dtype == torch.float64 and tok_logp.is_contiguous() and tok_logp.numel() == N * (T + 2)
    check(_lib.load().isc_lm_dev_score(hyps.data_ptr(), N, T, ptr(labels), n_lm, slots.data_ptr(), lm_off.data_ptr(),
                                       lm_capacity.data_ptr(), lm_order.data_ptr(), int(vocab_size), int(eos_mode),
                                       int(bool(unk_as_word)), int(sos_id), int(eos_id), out.data_ptr(),
                                       n_scored.data_ptr(), n_oov.data_ptr(), ptr(tok_logp), stream()),
          'isc_lm_dev_score')
    return out, n_scored, n_oov


def sw_reward(tok, labels, weights, state, flag=0.0, reward_io=None, accumulate=False, reward64=None, row_hits=None,
              mark=True):
    """isc_sw_reward: the sentiment-word reward of the rows `tok` int64 [N, T] on the device, row r under the lexicon of
    labels[r]: weights float64 [n_labels, V], state uint8 [n_labels, V] (rewards.SentimentWordWeights holds them).
    `reward_io` float32 [N, T]: written ((float)w) or, `accumulate`, added to (+ (float)flag * (float)w); `reward64`
    float64 [N, T] and `row_hits` int32 [N]: filled where given.  `mark`: the words that were paid get state 2.  Nothing is
    allocated and nothing is returned: every output is the caller's."""
    require_device(tok, labels, weights, state, reward_io, reward64, row_hits)
    assert tok.dtype == torch.int64 and tok.dim() == 2 and tok.is_contiguous()
    N, T = tok.shape
    assert labels.dtype == torch.int64 and labels.is_contiguous() and labels.numel() == N
    assert weights.dtype == torch.float64 and weights.dim() == 2 and weights.is_contiguous()
    assert state.dtype == torch.uint8 and state.shape == weights.shape and state.is_contiguous()
    n_labels, V = weights.shape
    if reward_io is not None:
        assert reward_io.dtype == torch.float32 and reward_io.is_contiguous() and tuple(reward_io.shape) == (N, T)
    if reward64 is not None:
        assert reward64.dtype == torch.float64 and reward64.is_contiguous() and tuple(reward64.shape) == (N, T)
    if row_hits is not None:
        assert row_hits.dtype == torch.int32 and row_hits.is_contiguous() and row_hits.numel() == N
    check(_lib.load().isc_sw_reward(tok.data_ptr(), N, T, labels.data_ptr(), n_labels, V, weights.data_ptr(),
                                    state.data_ptr(), float(flag), ptr(reward_io), int(bool(accumulate)), ptr(reward64),
                                    ptr(row_hits), int(bool(mark)), stream()), 'isc_sw_reward')


def sw_decay(weights, state, factor):
    """isc_sw_decay: weights *= factor (float64) where state == 2, and those states back to 1, in place."""
    require_device(weights, state)
    assert weights.dtype == torch.float64 and weights.is_contiguous()
    assert state.dtype == torch.uint8 and state.shape == weights.shape and state.is_contiguous()
    check(_lib.load().isc_sw_decay(weights.data_ptr(), state.data_ptr(), weights.numel(), float(factor), stream()),
          'isc_sw_decay')


def lstm_bwd(dh, dh2, dc_next, gates, c_prev, c, dgates, dc_prev, dgates_sum=None):
    lib = _lib.load()
    M, H = c.shape
    for x in (dh, dh2, dc_next, gates, c_prev, c, dgates, dc_prev, dgates_sum):
        assert x is None or x.is_contiguous()
    check(lib.isc_lstm_bwd(dh.data_ptr(), ptr(dh2), ptr(dc_next), gates.data_ptr(), c_prev.data_ptr(),
                           c.data_ptr(), M, H, dgates.data_ptr(), dc_prev.data_ptr(), ptr(dgates_sum),
                           stream()), 'isc_lstm_bwd')


def scan_bwd_problem(P, V, q, w, alpha, dout, dP, dV, dq, dw_rows, accumulate, q2=None, de_out=None, row_div=1):
    """row_div > 1 (isc_scan_bwd_problem.row_div): P, V and q2 hold one entry per image, [rows / row_div, ...], and row b
    reads entry b // row_div; dP and dV must be None (attn_dp_from_de / attn_dv_from_alpha with group= form them)."""
    s = _lib.ScanBwdProblem()
    s.row_div = int(row_div) if int(row_div) > 1 else 0
    for x in (P, V, q, dout, dP, dV, dq, dw_rows):
        assert x is None or x.is_contiguous()          # (dV None: attn_dv_from_alpha forms it after the sweep)
    assert alpha.stride(1) == 1
    s.P, s.V, s.q, s.q2, s.w = P.data_ptr(), V.data_ptr(), q.data_ptr(), ptr(q2), w.data_ptr()
    s.alpha, s.alpha_ld, s.dout = alpha.data_ptr(), alpha.stride(0), dout.data_ptr()
    s.R, s.A, s.D = P.shape[1], P.shape[2], V.shape[2]
    s.accumulate = int(accumulate)
    s.dP, s.dV, s.dq, s.dw_rows = ptr(dP), ptr(dV), dq.data_ptr(), dw_rows.data_ptr()
    s.de_out = ptr(de_out)
    return s


def attn_dv_from_alpha(alpha, dout_all, dV, step_rows=0, group=1):
    """dV[b,r,:] = sum_t alpha[b,t,r] * dout_all[t,b,:] in the backward sweep's order (isc_attn_dv_from_alpha).
    alpha: [B,T,R] view with unit inner stride; dout_all [T,B,D] contiguous - or, step_rows > 0, the [:, :B] rows of a
    [T,step_rows,D] stack (merged unroll); dV [B,R,D] contiguous.
    group = n > 1 (isc_attn_dv_from_alpha_group): dV is [B / n, R, D], one entry per image, summed over the image's rows
    i*n + j as well - j ascending outermost, t = T-1 down inside."""
    B, T, R = alpha.shape
    D = dV.shape[2]
    group = int(group)
    assert group >= 1 and dV.shape[0] * group == B and dV.shape[1] == R
    assert alpha.stride(2) == 1 and dV.is_contiguous() and dout_all.shape == (T, B, D)
    if step_rows:
        assert dout_all.stride(2) == 1 and dout_all.stride(1) == D and dout_all.stride(0) == step_rows * D
    else:
        assert dout_all.is_contiguous()
    e0 = TIMER.begin()
    check(_lib.load().isc_attn_dv_from_alpha_group(alpha.data_ptr(), alpha.stride(0), alpha.stride(1),
                                                   dout_all.data_ptr(), B, group, T, R, D, dV.data_ptr(),
                                                   int(step_rows), stream()), 'isc_attn_dv_from_alpha_group')
    if e0 is not None:          # what must move: alpha and dout once, dV once
        TIMER.end(e0, 'attn_dv_from_alpha[%dx%dx%dx%d/%d]' % (B, T, R, D, group), 0.0,
                  4.0 * (B * T * (R + D) + dV.numel()))


def attn_dp_from_de(P, q_all, w, de_all, dP, q2=None, group=1):
    """dP[b,r,:] = sum_t de_all[t,b,r] * w * (1 - tanh^2(P[b,r,:] + q_all[t,b,:] (+ q2[b,:]))) in the backward sweep's
    order (isc_attn_dp_from_de).  P, dP [B,R,A]; q_all [T,B,A]; de_all [T,B,R]; all contiguous.
    group = n > 1 (isc_attn_dp_from_de_group): P, dP and q2 hold one entry per image, [B / n, ...]; the sum also runs over
    the image's rows i*n + j - j ascending outermost, t = T-1 down inside."""
    I, R, A = P.shape
    T, B = q_all.shape[:2]
    group = int(group)
    for x in (P, q_all, de_all, dP, q2):
        assert x is None or x.is_contiguous()
    assert group >= 1 and I * group == B and (q2 is None or q2.shape == (I, A))
    assert q_all.shape == (T, B, A) and de_all.shape == (T, B, R) and dP.shape == P.shape
    e0 = TIMER.begin()
    check(_lib.load().isc_attn_dp_from_de_group(P.data_ptr(), q_all.data_ptr(), ptr(q2), w.data_ptr(),
                                                de_all.data_ptr(), B, group, T, R, A, dP.data_ptr(), stream()),
          'isc_attn_dp_from_de_group')
    if e0 is not None:          # what must move: P, q and de once, dP once
        TIMER.end(e0, 'attn_dp_from_de[%dx%dx%dx%d/%d]' % (B, T, R, A, group), 0.0,
                  4.0 * (2 * P.numel() + B * T * (R + A)))


def attn_scan_bwd(problems, B):
    lib = _lib.load()
    arr = (_lib.ScanBwdProblem * len(problems))(*problems)
    e0 = TIMER.begin()
    check(lib.isc_attn_scan_bwd(arr, len(problems), B, stream()), 'isc_attn_scan_bwd')
    if e0 is not None:
        nb = sum(4.0 * B / max(q.row_div, 1) * q.R * 3 * (q.A + q.D) for q in problems)   # read P,V; read-modify-write dP,dV
        TIMER.end(e0, 'attn_scan_bwd[' + '+'.join('%dx%dx%d' % (B, q.R, q.A) for q in problems) + ']', 0.0, nb)


def gate_mix_bwd(z, w, v, s, beta, dfeat, dv, ds, dz, dw_rows, db_rows, accumulate):
    lib = _lib.load()
    B, A = z.shape
    D = v.shape[1]
    check(lib.isc_gate_mix_bwd(z.data_ptr(), w.data_ptr(), v.data_ptr(), s.data_ptr(), beta.data_ptr(),
                               beta.stride(0), dfeat.data_ptr(), B, A, D, dv.data_ptr(), ds.data_ptr(),
                               dz.data_ptr(), dw_rows.data_ptr(), db_rows.data_ptr(), int(accumulate),
                               stream()), 'isc_gate_mix_bwd')


def embed_relu_bwd(emb, ids, dout, demb, n_rows, rows_per_grad=1, scale=1.0, ids_stride=1, pad_first=0,
                   pad_id=0, keep_mask=None, mask_scale=1.0, skip_id=-1):
    lib = _lib.load()
    V, W = emb.shape
    assert dout.is_contiguous() and demb.is_contiguous() and ids.dtype == torch.int64
    ws = splitk_ws(emb.device)          # position index of the ids (the stream's workspace: launches are ordered)
    check(lib.isc_embed_relu_bwd_ws(emb.data_ptr(), V, W, ids.data_ptr(), ids_stride, n_rows, rows_per_grad,
                                    pad_first, pad_id, dout.data_ptr(), scale, ptr(keep_mask), mask_scale,
                                    demb.data_ptr(), skip_id, ws.data_ptr(), ws.numel() * 4, stream()),
          'isc_embed_relu_bwd_ws')


def colsum(x, out, accumulate=False):
    lib = _lib.load()
    M, N = x.shape
    assert x.stride(1) == 1 and out.is_contiguous() and out.numel() >= N
    ws = splitk_ws(x.device)
    check(lib.isc_colsum(x.data_ptr(), x.stride(0), M, N, out.data_ptr(), int(accumulate), ws.data_ptr(),
                         ws.numel(), stream()), 'isc_colsum')


def colsum_multi(jobs):
    """jobs: list of (x [M,N], [out tensors, 1..3], accumulate) - every column sum in at most two launches per 24 jobs
    (isc_colsum_multi).  The caller keeps every x alive and untouched until this returns."""
    lib = _lib.load()
    if not jobs:
        return
    ws = splitk_ws(jobs[0][0].device)
    for lo in range(0, len(jobs), _lib.ISC_COLSUM_MAX_JOBS):
        part = jobs[lo:lo + _lib.ISC_COLSUM_MAX_JOBS]
        arr = (_lib.ColsumJob * len(part))()
        for q, (x, outs, acc) in zip(arr, part):
            M, N = x.shape
            assert x.stride(1) == 1 and x.dtype == torch.float32 and 1 <= len(outs) <= _lib.ISC_COLSUM_MAX_OUT
            q.x, q.ld, q.M, q.N, q.n_out, q.accumulate = x.data_ptr(), x.stride(0), M, N, len(outs), int(acc)
            for i, o in enumerate(outs):
                assert o.is_contiguous() and o.numel() >= N and o.dtype == torch.float32
                q.out[i] = o.data_ptr()
        check(lib.isc_colsum_multi(arr, len(part), ws.data_ptr(), ws.numel(), stream()), 'isc_colsum_multi')


def relu_mask_bwd(dy, y, dz, keep_mask=None, scale=1.0):
    """dz = dy * (y > 0) [* mask * scale]; y=None skips the ReLU test (pure dropout backward)."""
    lib = _lib.load()
    assert dy.is_contiguous() and dz.is_contiguous() and (y is None or y.is_contiguous())
    check(lib.isc_relu_mask_bwd(dy.data_ptr(), ptr(y), ptr(keep_mask), scale, dy.numel(), dz.data_ptr(),
                                stream()), 'isc_relu_mask_bwd')


def xe_loss_bwd(target, lengths_i32, gout, sum_count, dlogp):
    lib = _lib.load()
    B, T, V = dlogp.shape
    check(lib.isc_xe_loss_bwd(target.data_ptr(), lengths_i32.data_ptr(), B, T, V, gout.data_ptr(),
                              sum_count.data_ptr(), dlogp.data_ptr(), stream()), 'isc_xe_loss_bwd')


WEIGHT_EPOCH = 0   # bumped by every in-place parameter update done behind torch's back (version counters)


STATUS_NONFINITE_STATS, STATUS_NONFINITE_LINEAR = 1, 2


_STATUS_WORDS = {}          # device index -> pinned int32[2] the kernels flag into (isc_set_status_words)


def register_status_words(device=None):
    """Once per device: hand the library two pinned host words for its numerics flags.  Cheap to call again."""
    index = torch.device(device).index if device is not None else None
    if index is None:
        index = torch.cuda.current_device()
    w = _STATUS_WORDS.get(index)
    if w is None:
        w = torch.zeros(2, dtype=torch.int32).pin_memory()
        with torch.cuda.device(index):
            check(_lib.load().isc_set_status_words(w.data_ptr()), 'isc_set_status_words')
        _STATUS_WORDS[index] = w
    return w


def device_status(reset=True, device=None):
    """Numerics bits flagged by the work the host has ALREADY waited for (no device call, no synchronisation)."""
    w = register_status_words(device)
    bits = (STATUS_NONFINITE_STATS if int(w[0]) else 0) | (STATUS_NONFINITE_LINEAR if int(w[1]) else 0)
    if reset and bits:
        w.zero_()
    return bits


def check_numerics(where=''):
    """Raises HipLibraryError if a decode step or a split-f16 launch over caller data went non-finite since the last
    check (and clears the flags).  Reads two host words: it sees what the host has waited for - call it after a
    synchronisation or a host read of the results (the product does: beam search, the RL step)."""
    st = device_status(reset=True)
    if st:
        what = []
        if st & STATUS_NONFINITE_LINEAR:
            what.append('a linear layer over caller-supplied features produced non-finite values')
        if st & STATUS_NONFINITE_STATS:
            what.append('a decode step saw non-finite logits')
        raise _lib.HipLibraryError(
            '%s%s: an input left the split-f16 domain |x| < 65504 (or was NaN / inf). Results since the last check '
            'are invalid; scale the features, or run the exact-fp32 engine with ops.set_h3_mode(0).'
            % (where + ': ' if where else '', '; '.join(what)))


_OWNED_STREAMS = set()      # (device index, stream handle) of the streams this package's objects hold for themselves


def private_stream(device):
    """A torch.cuda.Stream that no other owner inside this package holds (and that is not the caller's current stream).
    torch hands out the 32 pool streams of a device round robin, so the 33rd Stream() IS the first again - and
    everything kept per stream here (split-K workspace, weight planes, weights-scope slot) would be shared with it.
    Owners: train_graph.XETrainGraph (two), a captioner's roll-out and beam-search streams, the eager training step's side stream."""
    device = torch.device(device)
    idx = device.index if device.index is not None else torch.cuda.current_device()
    cur = torch.cuda.current_stream(idx).cuda_stream
    for attempt in range(2):
        for _ in range(48):
            st = torch.cuda.Stream(device=idx)
            key = (idx, st.cuda_stream)
            if key not in _OWNED_STREAMS and st.cuda_stream != cur:
                _OWNED_STREAMS.add(key)
                return st
        # every pool stream is held: owners that are garbage but sit in reference cycles (training-graph objects, captioners
        # with captured graphs) give theirs back in their finalizers - collect once and look again
        if attempt == 0 and not torch.cuda.is_current_stream_capturing():
            gc.collect()
    raise RuntimeError('no free stream left in the pool of device %d (%d held by this package)' % (idx, len(_OWNED_STREAMS)))


def release_stream_state(index, handle):
    """Forget everything kept per (device index, stream handle): split-K workspace, weight-plane buffer, the suspended
    weights scope and the library's scope slot.  For owners of private streams that go away (train_graph)."""
    key = (index, handle)
    cls = h3_weights_scope
    with cls._lock:
        if cls._depth.get(key, 0) != 0:
            return False
        cls._suspended.pop(key, None)
        cls._cold_begins.pop(key, None)
        _H3W_BUF.pop(key, None)
    _SPLITK_WS.pop(key, None)
    _OWNED_STREAMS.discard(key)
    _lib.load().isc_h3_weights_end(C.c_void_p(handle))
    return True


_REFRESH = threading.local()


class refresh_only:
    """`with ops.refresh_only(stream_handles):` - refresh_weight_planes() on this thread touches only the suspended
    scopes of these streams (a training iteration being captured into a HIP graph must not pull a stream that is not
    part of the capture into it; the other streams' scopes go stale with the epoch and rebuild on their next use)."""

    def __init__(self, handles):
        self.only = frozenset(handles)

    def __enter__(self):
        self.prev = getattr(_REFRESH, 'only', None)
        _REFRESH.only = self.only
        return self

    def __exit__(self, *exc):
        _REFRESH.only = self.prev
        return False


def refresh_weight_planes(epoch_before):
    """After an in-place weight update enqueued on the current stream (the fused optimiser; WEIGHT_EPOCH was
    `epoch_before` when it started): re-split the weights behind every suspended weights scope of this device whose key
    was valid until then, in place and in few batched launches (isc_h3_weights_refresh), and re-key it to the new epoch -
    the next forward / backward sweeps then RESUME their scope instead of rebuilding it with one split launch per weight
    operand (39 per XE iteration at B = 128).  A scope on another stream (the seq2seq unroll's side stream) is refreshed
    on ITS stream, after that stream has been made to wait for this one.  Returns the number of scopes refreshed."""
    cls = h3_weights_scope
    cur = torch.cuda.current_stream()
    index = cur.device.index
    only = getattr(_REFRESH, 'only', None)
    with cls._lock:
        items = [(k, wk) for k, wk in cls._suspended.items()
                 if k[0] == index and isinstance(wk, tuple) and wk and wk[-1] == epoch_before
                 and cls._depth.get(k, 0) == 0 and (only is None or k[1] in only)]
    lib = _lib.load()
    done = 0
    for key, wk in items:
        handle = key[1]
        other = torch.cuda.ExternalStream(handle, device=index) if handle != cur.cuda_stream else None
        if other is not None:
            other.wait_stream(cur)
        rc = lib.isc_h3_weights_refresh(C.c_void_p(handle))
        if other is not None and torch.cuda.is_current_stream_capturing():
            cur.wait_stream(other)             # a capture must end with every forked stream joined
        with cls._lock:
            if cls._suspended.get(key) == wk:
                if rc == 0:
                    cls._suspended[key] = wk[:-1] + (WEIGHT_EPOCH,)
                    done += 1
                else:
                    del cls._suspended[key]
    return done


def adam_hyper(lr, beta1, beta2, step):
    """{lr, 1 - beta1^step, sqrt(1 - beta2^step)} as isc_clamp_adam derives them (double arithmetic, then float)."""
    return [float(lr), 1.0 - beta1 ** float(step), (1.0 - beta2 ** float(step)) ** 0.5]


def clamp_adam(params, grads, exp_avg, exp_avg_sq, lr, beta1, beta2, eps, weight_decay, clip, step, hyper=None):
    """hyper: optional device float tensor {lr, bc1, bc2_sqrt} read by the kernel instead of lr / step (a launch that
    is captured into a HIP graph; adam_hyper() gives the values to store there before each replay)."""
    global WEIGHT_EPOCH
    WEIGHT_EPOCH += 1
    lib = _lib.load()
    n = len(params)
    mk = lambda ts: (C.c_void_p * n)(*[t.data_ptr() for t in ts])
    for t in list(params) + list(grads) + list(exp_avg) + list(exp_avg_sq):
        assert t.is_contiguous() and t.dtype == torch.float32 and t.is_cuda
    numel = (C.c_int64 * n)(*[t.numel() for t in params])
    if hyper is not None:
        assert hyper.is_cuda and hyper.dtype == torch.float32 and hyper.numel() == 3 and hyper.is_contiguous()
        check(lib.isc_clamp_adam_hyper(mk(params), mk(grads), mk(exp_avg), mk(exp_avg_sq), numel, n, hyper.data_ptr(),
                                       beta1, beta2, eps, weight_decay, clip, stream()), 'isc_clamp_adam_hyper')
        return
    check(lib.isc_clamp_adam(mk(params), mk(grads), mk(exp_avg), mk(exp_avg_sq), numel, n, lr, beta1, beta2,
                             eps, weight_decay, clip, step, stream()), 'isc_clamp_adam')


# ---------------------------------------------------------------------------- concept detector (csrc/concept.hip)
CONCEPT_MAX_NUM = _lib.CONCEPT_MAX_NUM
SENTI_WORDS_CAP = _lib.SENTI_WORDS_CAP
SENTI_WORDS_MAX_OUT = _lib.SENTI_WORDS_MAX_OUT
_CONCEPT_WS = {}            # (device index, stream) -> workspace of isc_concept_fwd, grown when a call needs more


def _check_num(num, C_):
    """The head's shape limits as a ValueError (the library answers ISC_E_SHAPE and launches nothing)."""
    if isinstance(num, bool) or not hasattr(num, '__index__') or not 1 <= int(num) <= min(CONCEPT_MAX_NUM, C_):
        raise ValueError('num must be an integer in [1, min(%d, C = %d)], got %r' % (CONCEPT_MAX_NUM, C_, num))
    return int(num)


def _targets(targets, B, C_):
    assert targets.dtype in (torch.uint8, torch.int64), 'targets: uint8 or int64'
    assert targets.is_contiguous() and tuple(targets.shape) == (B, C_)
    return targets.data_ptr(), int(targets.dtype == torch.int64)


def concept_head(logits, num, concept_word=None, targets=None, want=('probs', 'idx', 'scores', 'words', 'hits')):
    """isc_concept_head on logits [B, C] fp32 (unit column stride, any row stride): -> dict with the outputs named in
    `want` - probs [B, C], idx [B, num] int64, scores [B, num], words [B, num] int64 (needs `concept_word` [C] int64),
    hits / n_true [B] int32 (need `targets` [B, C] uint8 or int64).  Larger logit first, lower index on ties, NaN last.
    num outside [1, min(16, C)] raises ValueError."""
    require_device(logits, concept_word, targets)
    assert logits.dtype == torch.float32 and logits.dim() == 2 and logits.stride(1) == 1
    B, C_ = logits.shape
    num = _check_num(num, C_)
    dev = logits.device
    out = {}
    if 'probs' in want:
        out['probs'] = torch.empty(B, C_, dtype=torch.float32, device=dev)
    if 'idx' in want:
        out['idx'] = torch.empty(B, num, dtype=torch.int64, device=dev)
    if 'scores' in want:
        out['scores'] = torch.empty(B, num, dtype=torch.float32, device=dev)
    if 'words' in want and concept_word is not None:
        assert concept_word.dtype == torch.int64 and concept_word.is_contiguous() and concept_word.numel() == C_
        out['words'] = torch.empty(B, num, dtype=torch.int64, device=dev)
    tp, t64 = (None, 0)
    if 'hits' in want and targets is not None:
        tp, t64 = _targets(targets, B, C_)
        out['hits'] = torch.empty(B, dtype=torch.int32, device=dev)
        out['n_true'] = torch.empty(B, dtype=torch.int32, device=dev)
    check(_lib.load().isc_concept_head(logits.data_ptr(), logits.stride(0), B, C_, num, ptr(out.get('probs')),
                                       ptr(out.get('idx')), ptr(out.get('scores')), ptr(concept_word),
                                       ptr(out.get('words')), tp, t64, ptr(out.get('hits')), ptr(out.get('n_true')),
                                       stream()), 'isc_concept_head')
    return out


def concept_loss(logits, targets, g=1.0, want_dz=False):
    """isc_concept_loss: MultiLabelClsLoss from the logits [B, C] (stable softplus form) -> (out3 = {term of the set
    targets, term of the unset ones, loss} fp32 on the device, dz [B, C] = (sigmoid(z) - t) g / (B C) or None)."""
    require_device(logits, targets)
    assert logits.dtype == torch.float32 and logits.dim() == 2 and logits.stride(1) == 1
    B, C_ = logits.shape
    tp, t64 = _targets(targets, B, C_)
    dev = logits.device
    ws = torch.empty(2 * B, dtype=torch.float64, device=dev)
    out3 = torch.empty(3, dtype=torch.float32, device=dev)
    dz = torch.empty(B, C_, dtype=torch.float32, device=dev) if want_dz else None
    check(_lib.load().isc_concept_loss(logits.data_ptr(), logits.stride(0), B, C_, tp, t64, float(g), ws.data_ptr(),
                                       ws.numel() * 8, out3.data_ptr(), ptr(dz), stream()), 'isc_concept_loss')
    return out3, dz


def senti_words_pack_check(off, num):
    """The longest list of a CSR offset array (host ints, [C + 1]); ValueError when `num` concepts of that length
    exceed the kernel's cap of SENTI_WORDS_CAP candidates per image (never a silent cut)."""
    n = len(off) - 1
    arr = (C.c_int32 * (n + 1))(*[int(x) for x in off])
    longest = C.c_int(0)
    rc = _lib.load().isc_senti_words_pack_check(arr, n, int(num), C.byref(longest))
    if rc != 0:
        raise ValueError('sentiment-word table: %d concepts x the longest list (%d entries) exceed the device cap of %d '
                         'candidates per image' % (num, longest.value, SENTI_WORDS_CAP))
    return longest.value


def senti_words_from_concepts(idx, off, word, score, max_list, n_out, pad_id, out=None):
    """isc_senti_words_from_concepts: idx [B, num] int64 concept indices, CSR table off int32 [C + 1] / word int64 [nnz] /
    score float64 [nnz] on the device -> int64 [B, n_out] vocabulary ids of the image's sentiment words, padded."""
    require_device(idx, off, word, score, out)
    assert idx.dtype == torch.int64 and idx.dim() == 2 and idx.stride(1) == 1
    assert off.dtype == torch.int32 and off.is_contiguous() and word.dtype == torch.int64 and word.is_contiguous()
    assert score.dtype == torch.float64 and score.is_contiguous() and word.numel() == score.numel()
    B, num = idx.shape
    if not 1 <= int(n_out) <= SENTI_WORDS_MAX_OUT:
        raise ValueError('n_out must be in [1, %d], got %r' % (SENTI_WORDS_MAX_OUT, n_out))
    if not 1 <= num <= CONCEPT_MAX_NUM or num * int(max_list) > SENTI_WORDS_CAP:
        raise ValueError('%d concepts x lists of up to %d entries exceed the device cap of %d candidates per image'
                         % (num, max_list, SENTI_WORDS_CAP))
    if out is None:
        out = torch.empty(B, int(n_out), dtype=torch.int64, device=idx.device)
    assert out.dtype == torch.int64 and out.is_contiguous() and tuple(out.shape) == (B, int(n_out))
    check(_lib.load().isc_senti_words_from_concepts(idx.data_ptr(), idx.stride(0), B, num, off.numel() - 1,
                                                    off.data_ptr(), ptr(word) if word.numel() else None,
                                                    ptr(score) if score.numel() else None, int(max_list), int(n_out),
                                                    int(pad_id), out.data_ptr(), stream()),
          'isc_senti_words_from_concepts')
    return out


def concept_launches():
    return _lib.load().isc_concept_launches()


def concept_shape_ok(F, H):
    """What isc_linear_fwd asks of the concept MLP's contraction lengths: multiples of 32 (its 32-deep chunks)."""
    return F >= 32 and H >= 32 and F % 32 == 0 and H % 32 == 0


def concept_fwd(params, feats, num, concept_word=None, want_probs=True, want_logits=False, want_topk=True):
    """isc_concept_fwd: the concept detector's eval forward.  params = (W0 [H,F], b0, W2 [H,H], b2, W5 [C,H], b5)
    contiguous fp32; feats [B, F] fp32 or float16 (unit column stride).  -> dict(idx, scores[, probs][, words][, logits]);
    want_topk=False: probabilities / logits only (the head then selects nothing)."""
    lib = _lib.load()
    require_device(feats, concept_word, *params)
    for t in params:
        assert t.dtype == torch.float32 and t.is_contiguous(), 'concept detector parameters: contiguous fp32'
    assert feats.dim() == 2 and feats.stride(1) == 1 and feats.dtype in (torch.float32, torch.float16)
    B, F = feats.shape
    H, C_ = params[0].shape[0], params[4].shape[0]
    assert params[0].shape == (H, F) and params[2].shape == (H, H) and params[4].shape == (C_, H)
    num = _check_num(num, C_)
    dev = feats.device
    need = max(int(lib.isc_concept_workspace_bytes(B, F, H, C_)), 16)
    if torch.cuda.is_current_stream_capturing():
        workspace = torch.empty(need, dtype=torch.uint8, device=dev)
    else:                       # one per (device, stream): calls on a stream run one after another
        key = (dev.index, torch.cuda.current_stream(dev).cuda_stream)
        workspace = _CONCEPT_WS.get(key)
        if workspace is None or workspace.numel() < need:
            workspace = _CONCEPT_WS[key] = torch.empty(need, dtype=torch.uint8, device=dev)
    out = {}
    if want_topk:
        out['idx'] = torch.empty(B, num, dtype=torch.int64, device=dev)
        out['scores'] = torch.empty(B, num, dtype=torch.float32, device=dev)
    if want_probs:
        out['probs'] = torch.empty(B, C_, dtype=torch.float32, device=dev)
    if want_logits:
        out['logits'] = torch.empty(B, C_, dtype=torch.float32, device=dev)
    if concept_word is not None and want_topk:
        assert concept_word.dtype == torch.int64 and concept_word.is_contiguous() and concept_word.numel() == C_
        out['words'] = torch.empty(B, num, dtype=torch.int64, device=dev)
    sk = splitk_ws(dev)
    p = _lib.ConceptProblem()
    p.feats, p.feats_ld, p.feats_f16 = feats.data_ptr(), feats.stride(0), int(feats.dtype == torch.float16)
    p.B, p.F, p.H, p.C, p.num = B, F, H, C_, num
    p.w0, p.b0, p.w2, p.b2, p.w5, p.b5 = [t.data_ptr() for t in params]
    p.concept_word = ptr(concept_word)
    p.workspace, p.workspace_bytes = workspace.data_ptr(), workspace.numel()
    p.splitk_ws, p.splitk_ws_floats = sk.data_ptr(), sk.numel()
    p.logits, p.probs, p.idx, p.scores, p.words = (ptr(out.get('logits')), ptr(out.get('probs')), ptr(out.get('idx')),
                                                   ptr(out.get('scores')), ptr(out.get('words')))
    check(lib.isc_concept_fwd(C.byref(p), stream()), 'isc_concept_fwd')
    return out


# ---- the image encoder (csrc/encoder.hip): isc_encoder_* and its parts on their own
_ENCODER_WS = {}            # (device index, stream) -> workspace of isc_encoder_fwd, grown when a call needs more


def _grown_workspace(cache, key, need, device):
    """ONE uint8 workspace per key, replaced by a larger one when a call needs more (the old one is dropped): the cache
    holds the largest need seen, whatever the number of distinct geometries - image sizes are unbounded."""
    ws = cache.get(key)
    if ws is None or ws.numel() < need:
        cache.pop(key, None)                # (freed before the larger one is drawn)
        ws = None
        ws = cache[key] = torch.empty(max(need, 16), dtype=torch.uint8, device=device)
    return ws


def encoder_launches(kind=None):
    """Launches of the encoder's kernels so far: a dict over _lib.ENCODER_KINDS ('stem', 'pool', 'direct', 'split',
    'reduce', 'tail', 'pack'; 'r1' / 'r3' = convolution launches of the 1x1 / 3x3 form, either route), or one kind's."""
    lib = _lib.load()
    if kind is not None:
        return lib.isc_encoder_launches(_lib.ENCODER_KINDS.index(kind))
    return {name: lib.isc_encoder_launches(i) for i, name in enumerate(_lib.ENCODER_KINDS)}


def _f32c(*tensors):
    for t in tensors:
        assert t is None or (t.dtype == torch.float32 and t.is_contiguous()), 'contiguous fp32'


def _layers4(layers):
    layers = tuple(int(n) for n in layers)
    assert len(layers) == 4, 'four layer block counts'
    return layers, (C.c_int * 4)(*layers)


def encoder_pack(convs, layers, width):
    """convs: [(weight, bn.weight, bn.bias, bn.running_mean, bn.running_var)] in the library's order (the stem, then per
    block conv1, conv2, conv3 and the first block's downsample) -> the packed uint8 buffer isc_encoder_fwd reads (batch
    norms folded in double, weights split into f16 planes).  Pack once per weight version."""
    lib = _lib.load()
    layers, l4 = _layers4(layers)
    convs = [tuple(c) for c in convs]
    for c in convs:
        require_device(*c)
        _f32c(*c)
    nbytes = int(lib.isc_encoder_pack_bytes(l4, int(width)))
    if not nbytes or len(convs) != lib.isc_encoder_num_convs(l4, int(width)):
        raise _lib.HipLibraryError('isc_encoder_pack failed: ISC_E_SHAPE (layers %s, width %s, %d convolutions)'
                                   % (layers, width, len(convs)))
    packed = torch.empty(nbytes, dtype=torch.uint8, device=convs[0][0].device)
    arr = (_lib.EncoderConvParams * len(convs))()
    for a, c in zip(arr, convs):
        a.w, a.gamma, a.beta, a.mean, a.var = [t.data_ptr() for t in c]
    check(lib.isc_encoder_pack(arr, len(convs), l4, int(width), packed.data_ptr(), stream()), 'isc_encoder_pack')
    return packed


def encoder_final_grid(H, W):
    """(h, w) of the layer-4 grid of an H x W image; raises for an image the encoder refuses."""
    h, w = C.c_int(), C.c_int()
    check(_lib.load().isc_encoder_final_grid(int(H), int(W), C.byref(h), C.byref(w)), 'isc_encoder_final_grid')
    return h.value, w.value


def encoder_fwd(packed, image, layers, width, att_size=14, *, ksplit=0, want_f16=False, workspace=None):
    """isc_encoder_fwd: image [B, H, W, 3] contiguous, uint8 (normalised as the stem loads it) or fp32 (already
    normalised) -> (fc [B, C], att [B, a, a, C]) fp32 [, fc, att float16].  One workspace is kept per (device, stream)
    and grown when a call needs more, except inside a graph capture (hand `workspace`, or a fresh one is drawn from the capture's pool).  A shape
    the library does not take raises (ISC_E_SHAPE); nothing is launched or written then."""
    lib = _lib.load()
    require_device(packed, image)
    assert image.dim() == 4 and image.shape[3] == 3 and image.is_contiguous() and \
        image.dtype in (torch.uint8, torch.float32), 'image: contiguous [B, H, W, 3] uint8 or fp32'
    layers, l4 = _layers4(layers)
    B, H, W = (int(n) for n in image.shape[:3])
    dev, a, width = image.device, int(att_size), int(width)
    need = int(lib.isc_encoder_workspace_bytes_ksplit(B, H, W, l4, width, int(ksplit)))       # (0: refused - said below)
    Cf = 32 * width
    if workspace is None:
        if torch.cuda.is_current_stream_capturing():
            workspace = torch.empty(max(need, 16), dtype=torch.uint8, device=dev)
        else:
            workspace = _grown_workspace(_ENCODER_WS, (dev.index, torch.cuda.current_stream(dev).cuda_stream), need, dev)
    a_ok = max(min(a, 64), 1)
    fc = torch.empty(B, Cf, dtype=torch.float32, device=dev)
    att = torch.empty(B, a_ok, a_ok, Cf, dtype=torch.float32, device=dev)
    fc16 = torch.empty(B, Cf, dtype=torch.float16, device=dev) if want_f16 else None
    att16 = torch.empty(B, a_ok, a_ok, Cf, dtype=torch.float16, device=dev) if want_f16 else None
    p = _lib.EncoderProblem()
    p.image, p.image_u8, p.B, p.H, p.W = image.data_ptr(), int(image.dtype == torch.uint8), B, H, W
    for i, n in enumerate(layers):
        p.layers[i] = n
    p.width, p.att_size, p.ksplit = width, a, int(ksplit)
    p.packed, p.packed_bytes = packed.data_ptr(), packed.numel()
    p.workspace, p.workspace_bytes = workspace.data_ptr(), workspace.numel() if need else 0     # (refused: never read)
    p.fc, p.att, p.fc_f16, p.att_f16 = fc.data_ptr(), att.data_ptr(), ptr(fc16), ptr(att16)
    check(lib.isc_encoder_fwd(C.byref(p), stream()), 'isc_encoder_fwd')
    return (fc, att) + ((fc16, att16) if want_f16 else ())


def conv_pack(w, bn=None):
    """isc_conv_pack: w [N, Cin, R, R] (R 1 or 3) -> (planes uint8, bias [N] or None); bn = (weight, bias, running_mean,
    running_var) folds the batch norm, None packs w as it is."""
    require_device(w)
    _f32c(w, *(bn or ()))
    N, Cin, R = w.shape[0], w.shape[1], w.shape[2]
    planes = torch.empty(max(4 * N * R * R * Cin, 16), dtype=torch.uint8, device=w.device)
    bias = torch.empty(N, dtype=torch.float32, device=w.device) if bn is not None else None
    g = [t.data_ptr() for t in bn] if bn is not None else [None] * 4
    check(_lib.load().isc_conv_pack(w.data_ptr(), *g, N, Cin, R, planes.data_ptr(), ptr(bias), stream()), 'isc_conv_pack')
    return planes, bias


def conv_fwd(x, planes, bias, N, R, stride=1, residual=None, relu=False, ksplit=0, out=None, workspace=None):
    """isc_conv_fwd: x [B, h, w, Cin] fp32 channels-last -> out [B, ho, wo, N] = (relu)(conv + bias (+ residual))."""
    lib = _lib.load()
    require_device(x, planes, bias, residual)
    _f32c(x, bias, residual)
    B, h, w, Cin = (int(n) for n in x.shape)
    ho, wo = ((h - 1) // 2 + 1, (w - 1) // 2 + 1) if stride == 2 else (h, w)
    if out is None:
        out = torch.empty(B, ho, wo, N, dtype=torch.float32, device=x.device)
    need = int(lib.isc_conv_workspace_bytes(B, h, w, Cin, int(N), int(R), int(stride), int(ksplit)))
    if workspace is None:
        workspace = torch.empty(max(need, 16), dtype=torch.uint8, device=x.device)
    p = _lib.ConvProblem()
    p.x, p.B, p.h, p.w, p.Cin, p.N, p.R, p.stride = x.data_ptr(), B, h, w, Cin, int(N), int(R), int(stride)
    p.relu, p.ksplit = int(bool(relu)), int(ksplit)
    p.planes, p.bias, p.residual = planes.data_ptr(), bias.data_ptr(), ptr(residual)
    p.workspace, p.workspace_bytes, p.out = workspace.data_ptr(), workspace.numel(), out.data_ptr()
    check(lib.isc_conv_fwd(C.byref(p), stream()), 'isc_conv_fwd')
    return out


def encoder_stem_pack(w, bn=None):
    """isc_encoder_stem_pack: w [C0, 3, 7, 7] -> (wk [147, C0], bias [C0] or None)."""
    require_device(w)
    _f32c(w, *(bn or ()))
    C0 = w.shape[0]
    wk = torch.empty(147, C0, dtype=torch.float32, device=w.device)
    bias = torch.empty(C0, dtype=torch.float32, device=w.device) if bn is not None else None
    g = [t.data_ptr() for t in bn] if bn is not None else [None] * 4
    check(_lib.load().isc_encoder_stem_pack(w.data_ptr(), *g, C0, wk.data_ptr(), ptr(bias), stream()),
          'isc_encoder_stem_pack')
    return wk, bias


def encoder_stem(image, wk, bias, out=None):
    """isc_encoder_stem: image [B, H, W, 3] uint8 or fp32 -> relu(conv7x7/2 + bias) [B, Ho, Wo, C0]."""
    require_device(image, wk, bias)
    _f32c(wk, bias)
    assert image.is_contiguous() and image.dtype in (torch.uint8, torch.float32)
    B, H, W = (int(n) for n in image.shape[:3])
    C0 = wk.shape[1]
    if out is None:
        out = torch.empty(B, (H - 1) // 2 + 1, (W - 1) // 2 + 1, C0, dtype=torch.float32, device=image.device)
    check(_lib.load().isc_encoder_stem(image.data_ptr(), int(image.dtype == torch.uint8), B, H, W, C0, wk.data_ptr(),
                                       bias.data_ptr(), out.data_ptr(), stream()), 'isc_encoder_stem')
    return out


def encoder_maxpool(x, out=None):
    """isc_encoder_maxpool: x [B, h, w, C] -> [B, ho, wo, C], 3x3 / 2, pad 0, ceil mode."""
    require_device(x)
    _f32c(x)
    B, h, w, Cc = (int(n) for n in x.shape)
    if out is None:
        out = torch.empty(B, max((h - 2) // 2 + 1, 1), max((w - 2) // 2 + 1, 1), Cc, dtype=torch.float32, device=x.device)
    check(_lib.load().isc_encoder_maxpool(x.data_ptr(), B, h, w, Cc, out.data_ptr(), stream()), 'isc_encoder_maxpool')
    return out


def encoder_tail(x, att_size, want_f16=False):
    """isc_encoder_tail: x [B, h, w, C] -> (fc [B, C], att [B, a, a, C]) [, float16 copies]."""
    require_device(x)
    _f32c(x)
    B, h, w, Cc = (int(n) for n in x.shape)
    a = int(att_size)
    fc = torch.empty(B, Cc, dtype=torch.float32, device=x.device)
    att = torch.empty(B, a, a, Cc, dtype=torch.float32, device=x.device)
    fc16 = torch.empty(B, Cc, dtype=torch.float16, device=x.device) if want_f16 else None
    att16 = torch.empty(B, a, a, Cc, dtype=torch.float16, device=x.device) if want_f16 else None
    check(_lib.load().isc_encoder_tail(x.data_ptr(), B, h, w, Cc, a, fc.data_ptr(), att.data_ptr(), ptr(fc16), ptr(att16),
                                       stream()), 'isc_encoder_tail')
    return (fc, att) + ((fc16, att16) if want_f16 else ())
