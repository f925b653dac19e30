"""Host-side mirror of the reference merger interfaces, bound to libmergenet_hip.so over ctypes.

Same names, argument meaning and error behaviour as the reference for this path:

* :func:`run_segmentation` -- the Cython binding ``utils/csegment/c_segment.pyx:30-86``
  (typed-buffer checks, clip to ``[eps32, 1-eps32]``, int32 offset array, output allocation,
  ``-1``-terminated class table read over ``range(H*W-1)``), calling the ABI-compatible
  ``c_run_segmentation`` (``utils/csegment/segment.cc:742-754``) of the HIP library.
* :class:`SegmenterOptions`, :class:`ObjectSegmenter` -- ``utils/segmenter.py:21-24,225-483``
  (Python-variant semantics: ``n1*n2`` denominator, bias inside, merge on ``>=``, ``prune``).
* :class:`Merger` -- device-resident API for PyTorch-ROCm callers (tensors in, tensors out,
  current HIP stream); PyTorch is only used for memory and streams.

There is NO CPU fallback: if the HIP library is missing or no GPU is visible the calls raise.
"""

from __future__ import annotations

import ctypes
import os
import threading
from collections import namedtuple
from typing import List, Optional, Sequence, Tuple

import numpy as np

from . import rle as rle_mod
from .abi import *  # noqa: F401,F403 -- the MN_* constants, MnOptions, MnStats, _f32p, _i32p, SIGNATURES, EXPORTS

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("MN_LIB") or os.path.join(_HERE, "libmergenet_hip.so")   # MN_LIB: a variant build (tuning only)

SegmenterOptions = namedtuple("SegmenterOptions",
                              ["same_different_bias", "object_merge_factor", "merge_logprob_bias"])


_lib_handle = None


def load_library() -> ctypes.CDLL:
    """Load libmergenet_hip.so (built in-tree by ``__graft_entry__.build``); fail loudly."""
    global _lib_handle
    if _lib_handle is not None:
        return _lib_handle
    if not os.path.exists(LIB_PATH):
        raise RuntimeError("HIP extension missing: %s (run __graft_entry__.build() / make -C "
                           "mergenet_amd/csrc); there is no CPU fallback" % LIB_PATH)
    # One HIP runtime per process: PyTorch-ROCm ships its own libamdhip64.so.7.  If our library
    # were loaded first it would pull /opt/rocm's copy and torch would later see no device (or
    # vice versa), so when torch is installed its runtime is loaded first and we bind to it.
    try:
        import torch  # noqa: F401
    except ImportError:
        pass
    lib = ctypes.CDLL(LIB_PATH)
    for name, (restype, argtypes) in SIGNATURES.items():
        fn = getattr(lib, name, None)      # a variant build (MN_LIB) may lack a symbol: _typed / _entry say so at the call
        if fn is not None:
            fn.restype, fn.argtypes = restype, argtypes
    _lib_handle = lib
    return lib


class MergeNetError(RuntimeError):
    def __init__(self, status: int):
        lib = load_library()
        super().__init__("mergenet_hip status %d: %s" % (status, lib.mn_status_string(status).decode()))
        self.status = status


def _ok(rc: int) -> None:
    if rc != 0:
        raise MergeNetError(rc)


def _stream(dev) -> ctypes.c_void_p:
    """The current torch stream of `dev`, as the entry points take it."""
    import torch
    return ctypes.c_void_p(torch.cuda.current_stream(dev).cuda_stream)


def _dev_tensor(t, what: str, dtype=None, shape=None, dim=None, at_least=None, numel=None, device=None,
                contiguous=True):
    """`t`, if it is a tensor on the GPU that meets every condition given: `dtype` (one, or a tuple of accepted
    ones), `shape`, `dim`, `at_least` (a minimum numel), `numel` (an exact one), `device` (a torch.device, or a
    device index) and, unless `contiguous` is False, contiguity.  ValueError(what) otherwise."""
    if not (t.is_cuda and (not contiguous or t.is_contiguous())
            and (dtype is None or (t.dtype in dtype if isinstance(dtype, tuple) else t.dtype == dtype))
            and (dim is None or t.dim() == dim)
            and (shape is None or tuple(t.shape) == tuple(shape))
            and (at_least is None or t.numel() >= at_least)
            and (numel is None or t.numel() == numel)
            and (device is None or (t.device.index if isinstance(device, int) else t.device) == device)):
        raise ValueError(what)
    return t


def _check_match_inputs(table, pred_classes, truth_classes, scores, crowd, device=None):
    """What Merger.match_instances and DatasetEval.add take (the latter on its own `device`); returns (K, G)."""
    import torch
    _dev_tensor(table, "table: the contiguous int32 [K+1, G+1] tensor of overlap_table()%s"
                % (", on the evaluator's GPU" if device is not None else ""), torch.int32, dim=2, at_least=1, device=device)
    K, G = int(table.shape[0]) - 1, int(table.shape[1]) - 1
    if pred_classes is None or truth_classes is None:
        raise ValueError("pred_classes and truth_classes are needed")
    for x, name, dtype, n in ((pred_classes, "pred_classes", torch.int32, K),
                              (truth_classes, "truth_classes", torch.int32, G), (scores, "scores", torch.float32, K),
                              (crowd, "crowd", (torch.uint8, torch.bool), G)):
        if x is not None:
            _dev_tensor(x, "%s: a contiguous %s tensor of at least %d entries on the table's GPU" % (name, dtype, n),
                        dtype, at_least=n, device=table.device)
    return K, G


def default_options(**overrides) -> MnOptions:
    o = MnOptions()
    load_library().mn_default_options(ctypes.byref(o))
    for k, v in overrides.items():
        setattr(o, k, v)
    return o


def _class_list(table: np.ndarray) -> List[int]:
    out = []
    for i in range(table.shape[0] - 1):       # c_segment.pyx:80-84
        if table[i] == -1:
            break
        out.append(int(table[i]))
    return out


def _check_buffer(name: str, a) -> np.ndarray:
    """The typed-buffer contract of c_segment.pyx:30-31 (float32, ndim 3, C-contiguous)."""
    if a is None:
        raise TypeError("Argument '%s' must not be None" % name)
    if not isinstance(a, np.ndarray):
        raise TypeError("Argument '%s' has incorrect type (expected numpy.ndarray, got %s)"
                        % (name, type(a).__name__))
    if a.dtype != np.float32:
        raise ValueError("Buffer dtype mismatch, expected 'float' but got '%s'" % a.dtype)
    if a.ndim != 3:
        raise ValueError("Buffer has wrong number of dimensions (expected 3, got %d)" % a.ndim)
    if not a.flags["C_CONTIGUOUS"]:
        raise ValueError("ndarray is not C-contiguous")
    return a


def run_segmentation(class_pred, adj_pred, num_classes: int, offset_list,
                     same_different_bias: float, object_merge_factor: float,
                     merge_logprob_bias: float):
    """Drop-in for ``csegment.c_segment.run_segmentation`` (c_segment.pyx:30-86).

    Returns ``(mask int32[H, W], object_class list)``; label 0 = every class-0 object.
    """
    class_pred = _check_buffer("class_pred", class_pred)
    adj_pred = _check_buffer("adj_pred", adj_pred)
    if offset_list is None or not isinstance(offset_list, list):
        raise TypeError("Argument 'offset_list' has incorrect type (expected list)")
    epsilon = np.finfo(np.float32).eps
    class_pred = np.ascontiguousarray(class_pred.clip(epsilon, 1.0 - epsilon), dtype=np.float32)
    adj_pred = np.ascontiguousarray(adj_pred.clip(epsilon, 1.0 - epsilon), dtype=np.float32)
    offset_array = np.ascontiguousarray(np.array(offset_list).astype(np.int32))
    class_dim = class_pred.shape[0]
    offset_dim = adj_pred.shape[0]
    img_height, img_width = adj_pred.shape[1], adj_pred.shape[2]
    mask_pred = np.zeros((img_height, img_width)).astype(np.int32)
    object_class_pred = np.zeros((1, img_height * img_width)).astype(np.int32)
    lib = load_library()
    lib.c_run_segmentation(class_pred.ctypes.data_as(_f32p), class_dim,
                           adj_pred.ctypes.data_as(_f32p), offset_dim, img_width, img_height,
                           int(num_classes), offset_array.ctypes.data_as(_i32p),
                           mask_pred.ctypes.data_as(_i32p), object_class_pred.ctypes.data_as(_i32p),
                           float(same_different_bias), float(object_merge_factor),
                           float(merge_logprob_bias))
    _ok(lib.mn_last_status())            # the reference would exit(1) or crash
    return mask_pred, _class_list(object_class_pred[0])


class HostContext:
    """Owns an mn_context for host-pointer calls (numpy in, numpy out)."""

    def __init__(self, H: int, W: int, C: int, O: int, device: int = 0):
        self.lib = load_library()
        self.handle = self.lib.mn_create(device, H, W, C, O)
        if not self.handle:
            raise MergeNetError(self.lib.mn_last_status())
        self.shape = (H, W, C, O)

    def close(self):
        if self.handle:
            self.lib.mn_destroy(self.handle)
            self.handle = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def workspace_bytes(self) -> int:
        return int(self.lib.mn_workspace_bytes(self.handle))

    def segment(self, class_probs: np.ndarray, same_probs: np.ndarray, offsets,
                opts: Optional[MnOptions] = None, want_partition: bool = True):
        cp = np.ascontiguousarray(class_probs, dtype=np.float32)
        sp = np.ascontiguousarray(same_probs, dtype=np.float32)
        C, H, W = cp.shape
        O = sp.shape[0]
        off = np.ascontiguousarray(np.asarray(offsets, dtype=np.int32).reshape(-1, 2))
        if off.shape[0] != O or sp.shape[1:] != (H, W):
            raise AssertionError("shape mismatch between class, sameness maps and offsets")
        opts = opts if opts is not None else default_options()
        mask = np.zeros((H, W), np.int32)
        table = np.zeros(H * W, np.int32)
        part = np.zeros((H, W), np.int32) if want_partition else None
        stats = MnStats()
        rc = self.lib.mn_segment_host(self.handle, cp.ctypes.data_as(_f32p), C,
                                      sp.ctypes.data_as(_f32p), O, W, H, C,
                                      off.ctypes.data_as(_i32p), mask.ctypes.data_as(_i32p),
                                      table.ctypes.data_as(_i32p),
                                      part.ctypes.data_as(_i32p) if part is not None else None,
                                      ctypes.byref(opts), ctypes.byref(stats))
        _ok(rc)
        return mask, _class_list(table), part, stats.as_dict()


_host_contexts = {}
_host_contexts_lock = threading.Lock()


def _cached_host_context(H: int, W: int, C: int, O: int) -> "HostContext":
    """The HostContext of this shape AND this thread, created on first use (at most two shapes per thread are
    kept).  A context serves one call at a time (mn_context: one thread at a time), so threads do not share
    one; the cache itself is guarded by a lock, and a context is only evicted by the thread that owns it."""
    tid = threading.get_ident()
    key = (tid, H, W, C, O)
    with _host_contexts_lock:
        ctx = _host_contexts.get(key)
        if ctx is None or not ctx.handle:
            mine = [k for k in _host_contexts if k[0] == tid]
            while len(mine) >= 2:
                _host_contexts.pop(mine.pop(0)).close()
            ctx = _host_contexts[key] = HostContext(H, W, C, O)
        return ctx


def close_cached_contexts() -> None:
    """Free the contexts ObjectSegmenter keeps between calls (call it when no run_segmentation is in flight)."""
    with _host_contexts_lock:
        while _host_contexts:
            _host_contexts.popitem()[1].close()


class ObjectSegmenter:
    """``utils/segmenter.py:225-483`` look-alike running on the GPU (Python-variant semantics).

    ``ObjectSegmenter(class_probs, sameness_probs, num_classes, offsets, opts).run_segmentation()``
    returns ``(mask int64[H, W], object_class list)`` after ``prune(200)``.  Shape mismatches
    raise ``AssertionError`` as the reference's asserts do (segmenter.py:245-250); a prune with
    no class-0 object raises ``NameError`` as the reference does (segmenter.py:356,365).
    """

    def __init__(self, nnet_class_probs, nnet_sameness_probs, num_classes, offsets, opts=None):
        self.opts = opts if opts is not None else self.default_options()
        epsilon = np.finfo(np.float32).eps
        self.class_probs = np.asarray(nnet_class_probs).clip(epsilon, 1.0 - epsilon)
        self.sameness_probs = np.asarray(nnet_sameness_probs).clip(epsilon, 1.0 - epsilon)
        self.num_classes = num_classes
        self.offsets = offsets
        class_dim, self.img_height, self.img_width = self.class_probs.shape
        offset_dim, img_height, img_width = self.sameness_probs.shape
        assert class_dim == self.num_classes
        assert offset_dim == len(self.offsets)
        assert self.img_height == img_height
        assert self.img_width == img_width
        self.stats = None

    def default_options(self):
        return SegmenterOptions(same_different_bias=0.0, object_merge_factor=1.0,
                                merge_logprob_bias=0.0)

    def run_segmentation(self, prune_threshold: float = 200.0, mode: int = MN_MODE_AUTO):
        # (one context per shape is kept between calls -- creating one allocates the whole workspace,
        #  hundreds of MB at full size, for a merge that takes a fraction of a millisecond)
        ctx = _cached_host_context(self.img_height, self.img_width, self.num_classes, len(self.offsets))
        o = default_options(same_different_bias=float(self.opts.same_different_bias),
                            object_merge_factor=float(self.opts.object_merge_factor),
                            merge_logprob_bias=float(self.opts.merge_logprob_bias),
                            variant=MN_VARIANT_PYSEGMENTER, mode=mode,
                            prune_threshold=float(prune_threshold))
        try:
            mask, classes, _, self.stats = ctx.segment(self.class_probs, self.sameness_probs,
                                                       self.offsets, o, want_partition=False)
        except MergeNetError as e:
            if e.status == MN_ERR_NO_BACKGROUND:
                raise NameError("name 'background_obj' is not defined") from None
            raise
        return mask.astype(np.int64), classes


class Merger:
    """Device-resident merger for PyTorch-ROCm callers: tensors in, tensors out, no host copies.

    ``class_probs`` [C,H,W] and ``same_probs`` [O,H,W] are float32 CUDA(HIP) tensors, e.g. the
    sigmoid outputs of the network (``utils/inference_utils.py:44,96``); ``clip_inputs=1`` fuses
    the binding's clip (c_segment.pyx:53-55) into the loads.

    Both may also be ``float16`` or ``bfloat16`` (the same dtype for the two), as a network under autocast
    writes them: the kernels read them in that width -- no float32 copy is made -- and the result is what
    the float32 call gives on ``maps.float()`` with ``clip_inputs=1`` (16-bit maps are always clipped on load).

    ``logits=True`` on the methods that take maps says that both tensors hold the network's logits, not
    probabilities: the kernels take ``1 / (1 + expf(-x))`` in float32 where they load an element, so no
    ``torch.sigmoid`` pass runs before the merge and a 16-bit logit keeps its own probability up to a logit of
    about 17.  The result is what the float32 call gives on ``prepare(x, H, W, apply_sigmoid=True, clip=False)``
    with ``clip_inputs=1`` (logits are always clipped on load).
    """

    DTYPE_NAMES = "float32, float16 or bfloat16"
    MAPS_WANTED = "expected contiguous %s [K,H,W] tensors on the Merger's GPU" % DTYPE_NAMES
    MASK_WANTED = "expected a contiguous int32 [H,W] tensor on the GPU"

    def __init__(self, H: int, W: int, C: int, O: int, device: Optional[int] = None):
        import torch
        if not torch.cuda.is_available():
            raise RuntimeError("mergenet_amd.Merger needs a HIP device; there is no CPU fallback")
        self.torch = torch
        self.device = torch.cuda.current_device() if device is None else int(device)
        self.lib = load_library()
        self.handle = self.lib.mn_create(self.device, H, W, C, O)
        if not self.handle:
            raise MergeNetError(self.lib.mn_last_status())
        self.H, self.W, self.C, self.O = H, W, C, O
        self._dtype_codes = {torch.float32: MN_DTYPE_F32, torch.float16: MN_DTYPE_F16, torch.bfloat16: MN_DTYPE_BF16}

    def close(self):
        if getattr(self, "handle", None):
            self.lib.mn_destroy(self.handle)
            self.handle = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def workspace_bytes(self) -> int:
        return int(self.lib.mn_workspace_bytes(self.handle))

    def _dtype(self, t) -> int:
        """enum mn_dtype of a map tensor; ValueError for anything but the three accepted dtypes."""
        code = self._dtype_codes.get(t.dtype)
        if code is None:
            raise ValueError("expected %s tensors, got %s" % (self.DTYPE_NAMES, t.dtype))
        return code

    def _out_dtype(self, out_dtype) -> int:
        code = self._dtype_codes.get(out_dtype)
        if code is None:
            raise ValueError("out_dtype: %s, got %s" % (self.DTYPE_NAMES, out_dtype))
        return code

    def _typed(self, name: str, dtype: int, logits: bool = False):
        """The entry point that takes `dtype` and the arguments that carry it: (function, (dtype,)) of the *_t
        form, or -- float32 probability maps on a variant build without the typed forms (MN_LIB) -- (float
        function, ()).  `logits` travels as MN_MAPS_LOGITS in that dtype."""
        fn = getattr(self.lib, name + "_t", None)
        if fn is not None:
            return fn, (dtype | (MN_MAPS_LOGITS if logits else 0),)
        if dtype != MN_DTYPE_F32 or logits:
            raise RuntimeError("%s has no %s_t: 16-bit maps and logits need the current library" % (LIB_PATH, name))
        return getattr(self.lib, name), ()

    def _check(self, class_probs, same_probs, offsets):
        for t in (class_probs, same_probs):
            _dev_tensor(t, self.MAPS_WANTED, dim=3, device=self.device)
            self._dtype(t)
            if t.dtype != class_probs.dtype:
                raise ValueError("class and sameness maps must share one dtype (%s), got %s and %s"
                                 % (self.DTYPE_NAMES, class_probs.dtype, same_probs.dtype))
        C, H, W = class_probs.shape
        O = same_probs.shape[0]
        if same_probs.shape[1:] != (H, W) or len(offsets) != O:
            raise AssertionError("shape mismatch between class, sameness maps and offsets")
        off = np.ascontiguousarray(np.asarray(offsets, dtype=np.int32).reshape(-1, 2))
        return C, H, W, O, off

    def segment(self, class_probs, same_probs, offsets, opts: Optional[MnOptions] = None,
                want_partition: bool = False, logits: bool = False):
        """Returns (mask int32[H,W] tensor, object_class int32[H*W] tensor, partition|None, stats)."""
        torch = self.torch
        C, H, W, O, off = self._check(class_probs, same_probs, offsets)
        opts = opts if opts is not None else default_options()
        dev = class_probs.device
        mask = torch.empty((H, W), dtype=torch.int32, device=dev)
        table = torch.empty((H * W,), dtype=torch.int32, device=dev)
        part = torch.empty((H, W), dtype=torch.int32, device=dev) if want_partition else None
        stats = MnStats()
        stream = _stream(dev)
        fn, dt = self._typed("mn_segment_device", self._dtype(class_probs), logits)
        rc = fn(self.handle, class_probs.data_ptr(), C, same_probs.data_ptr(), O, *dt, W, H, C,
                off.ctypes.data_as(_i32p), mask.data_ptr(), table.data_ptr(),
                part.data_ptr() if part is not None else None,
                ctypes.byref(opts), stream, ctypes.byref(stats))
        _ok(rc)
        return mask, table, part, stats.as_dict()

    def segment_async(self, class_probs, same_probs, offsets, opts: Optional[MnOptions] = None,
                      want_partition: bool = False, out=None, logits: bool = False) -> "PendingSegment":
        """Queue one image (``mn_segment_launch``) and return at once; ``.result()`` of the returned
        object waits and gives what :meth:`segment` gives.  The Merger is busy until then -- use
        two of them alternately on one stream to keep the GPU busy across images: the launch of
        image i+1 then precedes the read-back of image i, and kernels of different images still
        do not overlap (their timings stay clean).

        ``out=(mask, table)`` (int32 [H,W] and [H*W] tensors of the caller) receives the result instead
        of fresh tensors.  A serving loop that feeds the same input and output buffers every time can
        add ``MN_DEBUG_REPLAY | MN_DEBUG_LEAN_EVENTS`` to ``opts.debug_flags``: from the third such call
        on, the library replays two recorded hipGraphs instead of issuing ~17 launches."""
        torch = self.torch
        C, H, W, O, off = self._check(class_probs, same_probs, offsets)
        opts = opts if opts is not None else default_options()
        dev = class_probs.device
        if out is not None:
            what = "out=(mask int32 [H,W], table int32 [H*W]) on the GPU"
            mask = _dev_tensor(out[0], what, torch.int32, numel=H * W)
            table = _dev_tensor(out[1], what, torch.int32, at_least=H * W, contiguous=False)
        else:
            mask = torch.empty((H, W), dtype=torch.int32, device=dev)
            table = torch.empty((H * W,), dtype=torch.int32, device=dev)
        part = torch.empty((H, W), dtype=torch.int32, device=dev) if want_partition else None
        stream = _stream(dev)
        fn, dt = self._typed("mn_segment_launch", self._dtype(class_probs), logits)
        rc = fn(self.handle, class_probs.data_ptr(), C, same_probs.data_ptr(), O, *dt, W, H, C,
                off.ctypes.data_as(_i32p), mask.data_ptr(), table.data_ptr(),
                part.data_ptr() if part is not None else None,
                ctypes.byref(opts), stream)
        _ok(rc)
        return PendingSegment(self, mask, table, part, (class_probs, same_probs, opts))

    def score(self, class_probs, same_probs, offsets, opts: Optional[MnOptions] = None,
              want_arrays: bool = False, logits: bool = False):
        """Phase A only.  Returns (ms_class_pass, ms_edge_pass[, cls uint8[H,W], best int64[H,W]])."""
        torch = self.torch
        C, H, W, O, off = self._check(class_probs, same_probs, offsets)
        opts = opts if opts is not None else default_options()
        dev = class_probs.device
        cls = torch.empty((H, W), dtype=torch.uint8, device=dev) if want_arrays else None
        best = torch.empty((H, W), dtype=torch.int64, device=dev) if want_arrays else None
        a, b = ctypes.c_float(0), ctypes.c_float(0)
        stream = _stream(dev)
        fn, dt = self._typed("mn_score_device", self._dtype(class_probs), logits)
        rc = fn(self.handle, class_probs.data_ptr(), C, same_probs.data_ptr(),
                O, *dt, W, H, C, off.ctypes.data_as(_i32p), ctypes.byref(opts), stream,
                cls.data_ptr() if cls is not None else None,
                best.data_ptr() if best is not None else None,
                ctypes.byref(a), ctypes.byref(b))
        _ok(rc)
        if want_arrays:
            return a.value, b.value, cls, best
        return a.value, b.value


    def sweep(self, class_probs, same_probs, offsets, opts: Optional[MnOptions] = None, logits: bool = False):
        """The affinity-scoring sweep of the default path alone (mn_cc_sign).  Returns a dict: bits uint32[H,W]
        (as int32 tensor), neg float32[O,H,W] (NaN = not listed), cls uint8[H,W] | None, gsum int32[C,H*W/4] |
        None, logsum float, pixels_per_lane, fused_class, margin_edges."""
        torch = self.torch
        C, H, W, O, off = self._check(class_probs, same_probs, offsets)
        opts = opts if opts is not None else default_options()
        dev = class_probs.device
        bits = torch.empty((H, W), dtype=torch.int32, device=dev)
        neg = torch.empty((O, H, W), dtype=torch.float32, device=dev)
        cls = torch.zeros((H, W), dtype=torch.uint8, device=dev)
        gsum = torch.zeros((C, (H * W + 3) // 4), dtype=torch.int32, device=dev)
        logsum = ctypes.c_double(0.0)
        info = (ctypes.c_int * 3)()
        stream = _stream(dev)
        fn, dt = self._typed("mn_sweep_device", self._dtype(class_probs), logits)
        rc = fn(self.handle, class_probs.data_ptr(), C, same_probs.data_ptr(), O, *dt, W, H, C,
                off.ctypes.data_as(_i32p), ctypes.byref(opts), stream,
                bits.data_ptr(), neg.data_ptr(), cls.data_ptr(), gsum.data_ptr(),
                ctypes.byref(logsum), info)
        _ok(rc)
        fused = bool(info[1])
        return dict(bits=bits, neg=neg, cls=cls if fused else None, gsum=gsum if fused else None,
                    logsum=logsum.value, pixels_per_lane=int(info[0]), fused_class=fused, margin_edges=int(info[2]))

    def sweep_time(self, inputs: Sequence, offsets, opts: Optional[MnOptions] = None, reps: int = 400,
                   logits: bool = False) -> float:
        """Tuning aid (``mn_sweep_time_device``): microseconds per launch of the sweep alone, back to back over
        the (class_probs, same_probs) pairs of ``inputs`` in rotation."""
        for a, b in inputs:
            C, H, W, O, off = self._check(a, b, offsets)
            if a.dtype != inputs[0][0].dtype or a.shape != inputs[0][0].shape:
                raise ValueError("the input sets of a sweep timing share one dtype and shape")
        opts = opts if opts is not None else default_options()
        n = len(inputs)
        vp = ctypes.c_void_p * n
        out = ctypes.c_float(0)
        stream = _stream(inputs[0][0].device)
        fn, dt = self._typed("mn_sweep_time_device", self._dtype(inputs[0][0]), logits)
        rc = fn(self.handle, vp(*[a.data_ptr() for a, _ in inputs]),
                vp(*[b.data_ptr() for _, b in inputs]), *dt, n, C, O, W, H, C,
                off.ctypes.data_as(_i32p), ctypes.byref(opts), stream,
                int(reps), ctypes.byref(out))
        _ok(rc)
        return out.value

    def exact_phase_a(self, class_probs, same_probs, offsets, opts: Optional[MnOptions] = None,
                      logits: bool = False):
        """Phase A of the exact engine: (cls uint8[H,W], oml float32[O,H,W], prio float32[O,H,W]) in the
        layout of the oracle's phase-A export (NaN where an edge leaves the image)."""
        torch = self.torch
        C, H, W, O, off = self._check(class_probs, same_probs, offsets)
        opts = opts if opts is not None else default_options()
        dev = class_probs.device
        cls = torch.empty((H, W), dtype=torch.uint8, device=dev)
        oml = torch.empty((O, H, W), dtype=torch.float32, device=dev)
        prio = torch.empty((O, H, W), dtype=torch.float32, device=dev)
        stream = _stream(dev)
        fn, dt = self._typed("mn_exact_phase_a_device", self._dtype(class_probs), logits)
        rc = fn(self.handle, class_probs.data_ptr(), C, same_probs.data_ptr(),
                O, *dt, W, H, C, off.ctypes.data_as(_i32p), ctypes.byref(opts),
                stream, cls.data_ptr(), oml.data_ptr(),
                prio.data_ptr())
        _ok(rc)
        return cls, oml, prio

    def prepare(self, maps, out_height: int, out_width: int, apply_sigmoid: bool = False,
                clip: bool = True, out_dtype=None):
        """Network output -> merger input on the device: optional sigmoid, bilinear resize with
        cv2.resize coordinates (egs/cityscape/local/segment.py:115-123) and clip, one pass.
        maps: float32, float16 or bfloat16 [K, Hin, Win] tensor on this GPU.  Returns [K, out_height, out_width]
        in float32, or in ``out_dtype`` (torch.float16 / torch.bfloat16): the float32 value the kernel computed,
        rounded to nearest even."""
        torch = self.torch
        _dev_tensor(maps, self.MAPS_WANTED, dim=3)
        in_code = self._dtype(maps)
        out_dtype = torch.float32 if out_dtype is None else out_dtype
        out_code = self._out_dtype(out_dtype)
        K, Hin, Win = maps.shape
        out = torch.empty((K, out_height, out_width), dtype=out_dtype, device=maps.device)
        stream = _stream(maps.device)
        if in_code == MN_DTYPE_F32 and out_code == MN_DTYPE_F32 and not hasattr(self.lib, "mn_prepare_device_t"):
            rc = self.lib.mn_prepare_device(self.handle, maps.data_ptr(), K, Hin, Win, out.data_ptr(),
                                            out_height, out_width, int(apply_sigmoid), int(clip),
                                            stream)      # (a variant build without the typed forms)
        else:
            rc = self.lib.mn_prepare_device_t(self.handle, maps.data_ptr(), in_code, K, Hin, Win, out.data_ptr(),
                                              out_code, out_height, out_width, int(apply_sigmoid), int(clip), stream)
        _ok(rc)
        return out

    def upsample_mask(self, mask, out_height: int, out_width: int):
        """Instance mask int32 [H,W] on this GPU -> int32 [out_height, out_width], growing or shrinking: what
        ``cv2.resize(mask, (out_width, out_height), interpolation=cv2.INTER_NEAREST)`` gives (segment.py:146-149).
        The source index of each axis is cv2's, formed in double: ``min(floor(dst * (1. / (dst_size / src_size))),
        src_size - 1)`` -- not the float32 index of ``torch.nn.functional.interpolate(mode="nearest")``, which takes
        the neighbouring source row or column at many size pairs (8 -> 82 at index 41, 1000 -> 1040 at 30 indices),
        and not the rational floor either (8 -> 98 at index 49).  ``resize.upsample_mask`` is the numpy statement,
        written from OpenCV's published source."""
        torch = self.torch
        H, W = self._check_mask(mask)
        out = torch.empty((out_height, out_width), dtype=torch.int32, device=mask.device)
        stream = _stream(mask.device)
        rc = self.lib.mn_upsample_mask_device(self.handle, mask.data_ptr(), H, W, out.data_ptr(), out_height, out_width,
                                              stream)
        _ok(rc)
        return out

    def encode_rle(self, mask, num_instances: int, drop_zero_area: bool = False):
        """COCO run-length encoding of every instance of an int32 [H,W] mask on this GPU.

        Equivalent of ``[maskUtils.encode(np.asfortranarray(mask == i)) for i in 1..K]``
        (egs/cityscape/local/segment.py:165-186) from ONE device pass over the mask (the run
        boundaries of all instances at once) and one native host pass that groups them and writes
        pycocotools' compressed counts strings.  Returns a list of ``{"size": [H, W], "counts": bytes,
        "area": pixels, "label": k}``, one per instance in label order; ``drop_zero_area`` leaves out
        instances without pixels (e.g. lost in the nearest-neighbour resize), as
        ``egs/cityscape/local/evaluate.py:52-54`` does before COCOeval.  A label outside ``1..num_instances`` in
        the mask -- a negative ignore label, a label above the count -- is ignored: it gets no entry and counts as
        zeros in the strings of the others, as ``mask == i`` does.  A mask with more label changes than the
        Merger's buffer holds (at first ``max(1024, H * W / 16)``) is counted, the buffer grown, and encoded again.
        """
        torch = self.torch
        H, W = self._check_mask(mask)
        cap = getattr(self, "_rle_cap", max(1024, H * W // 16))
        while True:
            if getattr(self, "_rle_pts", None) is None or self._rle_pts.shape[1] != cap:
                self._rle_pts = torch.empty((3, cap), dtype=torch.int32, device=mask.device)
                self._rle_host = torch.empty((3, cap), dtype=torch.int32).pin_memory()
                self._rle_cap = cap
            n = ctypes.c_int(0)
            stream = _stream(mask.device)
            rc = self.lib.mn_rle_points_device(self.handle, mask.data_ptr(), H, W, self._rle_pts.data_ptr(),
                                               cap, ctypes.byref(n), stream)
            if rc == -4 and n.value > cap:
                cap = n.value
                continue
            _ok(rc)
            break
        nn = n.value
        for r in range(3):                                    # only the used part of each row travels
            self._rle_host[r, :nn].copy_(self._rle_pts[r, :nn], non_blocking=True)
        torch.cuda.current_stream(mask.device).synchronize()
        K = int(num_instances)
        offsets = (ctypes.c_longlong * (K + 1))()
        areas = (ctypes.c_int * max(1, K))()
        out_cap = 8 * nn + 16 * K + 64                        # a count takes at most 7 bytes
        out = ctypes.create_string_buffer(out_cap)
        need = self.lib.mn_rle_encode_host(ctypes.cast(self._rle_host.data_ptr(), _i32p), cap, nn, H, W, K,
                                           ctypes.cast(out, ctypes.c_void_p), out_cap, offsets, areas)
        if need < 0 or need > out_cap:
            raise MergeNetError(int(need) if need < 0 else -20)
        raw = out.raw
        res = []
        for k in range(1, K + 1):
            if drop_zero_area and areas[k - 1] == 0:
                continue
            res.append({"size": [H, W], "counts": raw[offsets[k - 1]:offsets[k]], "area": int(areas[k - 1]),
                        "label": k})
        return res


    def decode_rle(self, rles, height: int, width: int, values=None, return_area: bool = False):
        """The int32 [H,W] label mask of a list of COCO run-length encodings, built on this GPU: what
        ``anns_to_mask`` (utils/dataset.py:486-506) builds on the host -- annotations painted in list order, the
        first to cover a pixel keeps it -- and what :meth:`overlap_table`, :meth:`map_scores` and
        :meth:`sameness_targets` take as the ground truth; ``rle.label_mask`` is the numpy statement.

        ``rles``: a sequence whose items are dicts ``{"size": [H, W], "counts": ...}`` (what :meth:`encode_rle` and
        :meth:`coco_results` write), bare compressed counts strings (``bytes`` or ``str``) or lists of integer
        counts.  Annotation ``i`` paints ``values[i]`` (``i + 1`` without ``values``; class ids give
        ``anns_to_mask_class``, dataset.py:511-522); the value 0 paints nothing.  Polygon annotations are not taken:
        convert them to RLE once on the host, as the reference's ``ann_to_rle`` does (dataset.py:525-542).
        With ``return_area`` also int32 [A] on the GPU: the sum of each annotation's odd-indexed counts
        (``maskUtils.area``), hidden or not.

        The strings are unpacked natively (``mn_rle_counts_host``); counts, starts and values travel with one small
        copy each on the current stream, the scratch stays on the Merger, nothing is synchronised.  ValueError,
        before anything is launched: an item whose ``size`` is not ``[height, width]``, counts that are negative or
        do not sum to ``height * width``, a malformed string, a negative value, ``len(values) != len(rles)``, more
        than 65535 annotations."""
        torch = self.torch
        fn = self._entry("mn_rle_decode_device")
        parse = self._entry("mn_rle_counts_host")
        H, W = int(height), int(width)
        if H <= 0 or W <= 0 or H * W >= 2 ** 31:
            raise ValueError("height and width must be positive, height * width below 2^31")
        rles = list(rles)
        A = len(rles)
        vals = rle_mod.checked_values(values, A)
        items = [rle_mod.item_counts(item, H, W, parse=lambda b: b) for item in rles]
        room = 0
        for i, it in enumerate(items):
            if not isinstance(it, bytes):
                it = items[i] = np.asarray(it, dtype=np.int64).reshape(-1)
                if it.size and (it.min() < 0 or it.max() > 2 ** 31 - 1):
                    raise ValueError("annotation %d: counts must lie in 0 .. 2^31 - 1" % i)
            room += len(it)                                   # (a count takes at least one byte of a string)
        if room >= 2 ** 31:
            raise ValueError("too many counts")
        counts = np.empty(max(1, room), np.uint32)
        starts = np.zeros(A + 1, np.int32)
        total = ctypes.c_longlong(0)
        at = 0
        for i, it in enumerate(items):
            if isinstance(it, bytes):
                n = parse(it, len(it), counts[at:].ctypes.data, room - at, ctypes.byref(total))
                if n < 0:
                    raise ValueError("annotation %d: a malformed counts string (%s)" %
                                     (i, "a count beyond 31 bits" if n == -4 else
                                      "it ends inside a group or holds a negative count"))
                n, sum_i = int(n), int(total.value)
            else:
                n = int(it.size)
                counts[at:at + n] = it
                sum_i = int(it.sum())
            if sum_i != H * W:
                raise ValueError("annotation %d: counts sum to %d, not %d" % (i, sum_i, H * W))
            at += n
            starts[i + 1] = at
        dev = torch.device("cuda", self.device)
        with torch.cuda.device(dev):
            stream = _stream(dev)
            d_counts = torch.from_numpy(counts[:max(1, at)].view(np.int32)).to(dev, non_blocking=True)
            d_starts = torch.from_numpy(starts).to(dev, non_blocking=True)
            d_values = torch.from_numpy(vals).to(dev, non_blocking=True) if vals is not None and A else None
            if getattr(self, "_rld_ends", None) is None or self._rld_ends.numel() < at:
                self._rld_ends = torch.empty((max(1024, at),), dtype=torch.int32, device=dev)
            if getattr(self, "_rld_rec", None) is None or self._rld_rec.shape[0] < A:
                self._rld_rec = torch.empty((max(64, A), 4), dtype=torch.int32, device=dev)
            mask = torch.empty((H, W), dtype=torch.int32, device=dev)
            area = torch.empty((A,), dtype=torch.int32, device=dev) if return_area else None
            rc = fn(self.handle, d_counts.data_ptr(), d_starts.data_ptr(), A, at,
                    d_values.data_ptr() if d_values is not None else None, H, W, self._rld_ends.data_ptr(),
                    self._rld_rec.data_ptr(), mask.data_ptr(), area.data_ptr() if area is not None and A else None,
                    stream)
        _ok(rc)
        return (mask, area) if return_area else mask

    def sameness_targets(self, mask, offsets):
        """Instance mask int32 [H,W] -> float32 [O,H,W] sameness targets (utils/dataset.py:259-277)."""
        torch = self.torch
        H, W = self._check_mask(mask)
        off = np.ascontiguousarray(np.asarray(offsets, dtype=np.int32).reshape(-1, 2))
        out = torch.empty((off.shape[0], H, W), dtype=torch.float32, device=mask.device)
        stream = _stream(mask.device)
        rc = self.lib.mn_sameness_targets_device(self.handle, mask.data_ptr(), H, W,
                                                 off.ctypes.data_as(_i32p), off.shape[0],
                                                 out.data_ptr(), stream)
        _ok(rc)
        return out

    def instance_scores(self, num_instances: int, device=None):
        """lp[cls] - lp[0] of each instance of the last segmentation on this Merger (float32 [K];
        ``labels.instance_scores`` is the float64 statement).  The scores of that segmentation, or MergeNetError
        (``MN_ERR_ARGUMENT``, nothing launched): before the first segmentation, between ``segment_async`` and its
        ``result()``, after a segmentation that failed half-way, and after ``score``, ``sweep``, ``sweep_time`` or
        ``exact_phase_a``, which overwrite what the call reads.  Every other call may come in between.  The class
        maps of that segmentation must still be alive and unchanged (single-pixel instances read them)."""
        torch = self.torch
        dev = torch.device("cuda", self.device) if device is None else device
        out = torch.zeros((max(1, num_instances),), dtype=torch.float32, device=dev)
        stream = _stream(dev)
        rc = self.lib.mn_instance_scores_device(self.handle, out.data_ptr(), stream)
        _ok(rc)
        return out[:num_instances]

    def _check_mask(self, mask):
        _dev_tensor(mask, self.MASK_WANTED, self.torch.int32, dim=2)
        return int(mask.shape[0]), int(mask.shape[1])

    def _entry(self, name: str):
        fn = getattr(self.lib, name, None)
        if fn is None:
            raise RuntimeError("%s has no %s: the instance table and the filter need the current library" % (LIB_PATH, name))
        return fn

    def instance_table(self, mask, num_instances: int):
        """int32 [K,5] tensor on the mask's device: row k-1 = {area, x_min, y_min, x_max, y_max} of label k, maxima
        inclusive, {0, W, H, -1, -1} for a label without pixels (``labels.instance_table`` is the numpy statement).
        One pass over the mask on the current stream; nothing is synchronised or copied.  Any image size."""
        torch = self.torch
        fn = self._entry("mn_instance_table_device")
        H, W = self._check_mask(mask)
        K = int(num_instances)
        if K < 0:
            raise ValueError("num_instances must not be negative")
        table = torch.empty((K, 5), dtype=torch.int32, device=mask.device)
        stream = _stream(mask.device)
        rc = fn(self.handle, mask.data_ptr(), H, W, K, table.data_ptr(), stream)
        _ok(rc)
        return table

    def filter_instances(self, mask, class_table, num_instances: int, min_area: int = 1, scores=None,
                         min_score: Optional[float] = None, inplace: bool = False, table=None,
                         return_remap: bool = False):
        """Drop the instances with fewer than ``min_area`` pixels (and, with ``scores`` and ``min_score``, those
        that score less) and renumber the survivors 1..K' in ascending old label -- the zero-area drop of
        ``egs/cityscape/local/evaluate.py:52-54`` with a threshold, on the device, leaving mask, class table,
        scores and instance table in agreement.  ``class_table``: int32, at least K entries (what ``segment``
        returns); ``scores``: float32 [K] or None -- without ``min_score`` they are carried along, except that a NaN
        score fails every comparison and is dropped whenever scores are given; ``table``: what :meth:`instance_table` gave for this mask
        (computed here when None); ``inplace`` rewrites ``mask`` itself.  Returns ``(mask, class_table int32 [K]
        with -1 from K' on, scores [K'] or None, table [K',5], K')`` (and the int32 [K+1] old -> new ``remap`` with
        ``return_remap``).  Reading K' is the one synchronisation; ``labels.filter_instances`` is the numpy statement."""
        torch = self.torch
        fn = self._entry("mn_filter_instances_device")
        H, W = self._check_mask(mask)
        K = int(num_instances)
        if K < 0:
            raise ValueError("num_instances must not be negative")
        dev = mask.device
        what = "%s: a contiguous %s tensor of at least num_instances entries on the mask's GPU"
        _dev_tensor(class_table, what % ("class_table", "int32"), torch.int32, at_least=K, device=dev)
        if scores is not None:
            _dev_tensor(scores, what % ("scores", "float32"), torch.float32, at_least=K, device=dev)
        if table is None:
            table = self.instance_table(mask, K)
        else:
            _dev_tensor(table, "table: the contiguous int32 [num_instances,5] tensor of instance_table()",
                        torch.int32, shape=(K, 5), device=dev)
        out_mask = mask if inplace else torch.empty_like(mask)
        remap = torch.empty((K + 1,), dtype=torch.int32, device=dev)
        table_out = torch.empty((K, 5), dtype=torch.int32, device=dev)
        classes_out = torch.empty((K,), dtype=torch.int32, device=dev)
        scores_out = torch.empty((K,), dtype=torch.float32, device=dev) if scores is not None else None
        count = torch.empty((1,), dtype=torch.int32, device=dev)
        stream = _stream(dev)
        threshold = float("-inf") if min_score is None else float(min_score)
        rc = fn(
            self.handle, mask.data_ptr(), H, W, K, table.data_ptr(), class_table.data_ptr(),
            scores.data_ptr() if scores is not None else None, int(min_area), threshold, out_mask.data_ptr(),
            remap.data_ptr(), table_out.data_ptr(), classes_out.data_ptr(),
            scores_out.data_ptr() if scores_out is not None else None, count.data_ptr(), stream)
        _ok(rc)
        new_k = int(count.item())                             # the one synchronisation
        res = (out_mask, classes_out, scores_out[:new_k] if scores_out is not None else None, table_out[:new_k], new_k)
        return res + (remap,) if return_remap else res

    def coco_results(self, mask, class_table, num_instances: int, image_id, cat_ids, scores=None, min_area: int = 1):
        """The detection results of one image, as ``convert_to_coco_result`` forms them
        (egs/cityscape/local/segment.py:165-186), with the ``area`` and ``bbox`` that ``COCO.loadRes`` would add:
        a list of ``{"image_id", "category_id": cat_ids[class], "score" (1 without ``scores``, segment.py:181),
        "segmentation": {"size": [H, W], "counts": bytes}, "bbox": [x_min, y_min, width, height] as floats (the
        documented COCO [x, y, w, h]), "area"}``, in label order after :meth:`filter_instances` (``min_area``)."""
        fmask, classes, fscores, table, new_k = self.filter_instances(mask, class_table, num_instances,
                                                                      min_area=min_area, scores=scores)
        rles = self.encode_rle(fmask, new_k)
        classes = classes[:new_k].cpu().numpy()
        table = table.cpu().numpy()
        fscores = fscores.cpu().numpy() if fscores is not None else None
        res = []
        for k in range(new_k):
            area, x0, y0, x1, y1 = (int(v) for v in table[k])
            res.append({"image_id": image_id, "category_id": cat_ids[int(classes[k])],
                        "score": float(fscores[k]) if fscores is not None else 1,
                        "segmentation": {"size": rles[k]["size"], "counts": rles[k]["counts"]},
                        "bbox": [float(x0), float(y0), float(x1 - x0 + 1), float(y1 - y0 + 1)], "area": area})
        return res

    def overlap_table(self, pred, truth, num_pred: int, num_truth: int):
        """int32 [K+1, G+1] tensor on the masks' device: entry [p][g] = number of pixels with prediction label p and
        truth label g; a label outside its range counts as 0 (``labels.overlap_table`` is the numpy statement).  Row
        sums are the prediction areas, column sums the truth areas.  ``truth`` is the label mask of the ground truth
        (utils/dataset.py:486-506, what :meth:`sameness_targets` takes).  One pass over both masks on the current
        stream; nothing is synchronised or copied.  Any image size."""
        torch = self.torch
        fn = self._entry("mn_overlap_table_device")
        H, W = self._check_mask(pred)
        _dev_tensor(truth, "truth: a contiguous int32 mask of the prediction's shape on the prediction's GPU",
                    torch.int32, shape=(H, W), device=pred.device)
        K, G = int(num_pred), int(num_truth)
        if K < 0 or G < 0:
            raise ValueError("num_pred and num_truth must not be negative")
        if (K + 1) * (G + 1) > 2 ** 28:
            raise ValueError("(num_pred + 1) * (num_truth + 1) must not exceed 2^28")
        table = torch.empty((K + 1, G + 1), dtype=torch.int32, device=pred.device)
        stream = _stream(pred.device)
        rc = fn(self.handle, pred.data_ptr(), truth.data_ptr(), H, W, K, G, table.data_ptr(), stream)
        _ok(rc)
        return table

    def match_instances(self, table, pred_classes, truth_classes, scores=None, crowd=None, thresholds=None,
                        area_range=(0.0, 1e10), return_iou: bool = False):
        """COCO's per-image evaluation from the overlap table (egs/cityscape/local/evaluate.py:67-73:
        ``COCOeval.evaluateImg`` with maxDets >= K), for every IoU threshold at once.  ``table``: what
        :meth:`overlap_table` gave, int32 [K+1, G+1]; ``pred_classes`` / ``truth_classes``: int32, at least K / G
        entries; ``scores``: float32 [K] or None (label order); ``crowd``: uint8 or bool [G] or None;
        ``thresholds``: None for COCO's ten (``np.linspace(0.5, 0.95, 10)``) or up to 16 values; ``area_range``: truth
        instances outside it are ignored, as are unmatched detections outside it.  K, G <= 4096.
        Returns a dict of tensors on the table's device: ``pred_match`` int32 [T,K] (the truth label, 0 = none),
        ``truth_match`` int32 [T,G] (the prediction label, 0 = none), ``pred_ignore`` bool [T,K], ``truth_ignore``
        bool [G], and ``iou`` float64 [K,G] with ``return_iou``; entry k-1 belongs to label k.
        ``labels.match_instances`` is the numpy statement and gives the definitions.  Nothing is synchronised."""
        torch = self.torch
        fn = self._entry("mn_match_overlaps_device")
        K, G = _check_match_inputs(table, pred_classes, truth_classes, scores, crowd)
        dev = table.device
        th = np.ascontiguousarray(np.linspace(0.5, 0.95, 10) if thresholds is None else
                                  np.asarray(thresholds, np.float64).reshape(-1))
        T = int(th.size)
        if not 1 <= T <= 16:
            raise ValueError("thresholds: 1 to 16 values")
        pred_match = torch.empty((T, K), dtype=torch.int32, device=dev)
        truth_match = torch.empty((T, G), dtype=torch.int32, device=dev)
        pred_ignore = torch.empty((T, K), dtype=torch.uint8, device=dev)
        truth_ignore = torch.empty((G,), dtype=torch.uint8, device=dev)
        iou = torch.empty((K, G), dtype=torch.float64, device=dev) if return_iou else None
        stream = _stream(dev)
        rc = fn(self.handle, table.data_ptr(), K, G, pred_classes.data_ptr(),
                scores.data_ptr() if scores is not None else None, truth_classes.data_ptr(),
                crowd.data_ptr() if crowd is not None else None, th.ctypes.data_as(ctypes.POINTER(ctypes.c_double)), T,
                float(area_range[0]), float(area_range[1]), iou.data_ptr() if iou is not None else None,
                pred_match.data_ptr(), truth_match.data_ptr(), pred_ignore.data_ptr(), truth_ignore.data_ptr(), stream)
        _ok(rc)
        res = {"pred_match": pred_match, "truth_match": truth_match, "pred_ignore": pred_ignore.view(torch.bool),
               "truth_ignore": truth_ignore.view(torch.bool)}
        if return_iou:
            res["iou"] = iou
        return res

    def dataset_eval(self, num_classes: int, thresholds=None, rec_thresholds=None, area_ranges=None,
                     max_dets=(1, 10, 100), capacity: int = 16384):
        """A :class:`DatasetEval` on this Merger: the evaluation log of a validation pass on the device and, from
        it, COCOeval's accumulate and summarize (egs/cityscape/local/evaluate.py:67-73).  ``num_classes`` C: the
        class axis of the results is class 0..C-1; ``thresholds``: None for COCO's ten or 1..16 IoU thresholds;
        ``rec_thresholds``: None for ``np.linspace(0, 1, 101)`` or float64 values, passed to the device as they are;
        ``area_ranges``: None for COCO's four (all, small, medium, large) or 1..4 ``(lo, hi)`` pairs; ``max_dets``:
        1..4 ascending positive values; ``capacity``: records the log holds at first (it grows by doubling)."""
        return DatasetEval(self, num_classes, thresholds, rec_thresholds, area_ranges, max_dets, capacity)

    def _check_truth(self, truth, truth_classes, H, W, dev) -> int:
        """The ground truth of :meth:`map_scores` and :meth:`mask_bce`: the label mask and the classes of its labels.
        Returns G, the number of truth labels."""
        torch = self.torch
        _dev_tensor(truth, "truth: a contiguous int32 mask of the maps' height and width on the maps' GPU",
                    torch.int32, shape=(H, W), device=dev)
        if truth_classes is None:
            return 0
        _dev_tensor(truth_classes, "truth_classes: a contiguous int32 [G] tensor on the maps' GPU, or None",
                    torch.int32, dim=1, device=dev)
        return int(truth_classes.numel())

    def map_scores(self, class_probs, same_probs, offsets, truth, truth_classes, logits: bool = False, into=None):
        """The network's maps themselves against the ground truth: what ``runningScore.update`` and
        ``offsetIoU.update`` (utils/score.py:20-32,77-86) accumulate per image, in one pass over the maps on the
        device -- no host copy of a plane, no target planes.  ``class_probs`` [C,H,W] and ``same_probs`` [O,H,W] as
        for :meth:`segment` (float32, float16 or bfloat16; ``logits=True`` for logits); ``truth``: the int32 [H,W]
        label mask of the ground truth (what :meth:`sameness_targets` and :meth:`overlap_table` take);
        ``truth_classes``: int32, entry g-1 the class of truth label g, or None for no instances -- its length is the
        number of truth labels.  Returns ``{"confusion": int64 [C,C], "sums": float64 [3,O]}`` on the maps' device:
        ``confusion[t][q]`` counts the pixels of truth class t predicted q (pixels whose truth class is outside
        0..C-1 are left out), ``sums[0]`` / ``sums[1]`` are the sums of ``1 - p`` over the pixels whose neighbour at
        the offset carries another truth label / over all pixels, ``sums[2]`` the number of the former
        (``labels.map_scores`` is the numpy statement and gives the definitions; ``labels.class_scores`` and
        ``labels.offset_iou`` turn the totals into the reference's summaries).  ``into``: a previous result of the
        same shapes, to which this image is added -- the running totals of a validation loop.  The sums of a call are
        bit-identical from run to run.  Any image size; nothing is synchronised or copied.  The calls of one Merger
        share a buffer of partial sums: keep them on ONE stream (a second stream needs a Merger of its own).  NaN in a
        map is undefined, as everywhere."""
        torch = self.torch
        fn = self._entry("mn_map_scores_device")
        C, H, W, O, off = self._check(class_probs, same_probs, offsets)
        dev = class_probs.device
        G = self._check_truth(truth, truth_classes, H, W, dev)
        if into is None:
            confusion = torch.empty((C, C), dtype=torch.int64, device=dev)
            sums = torch.empty((3, O), dtype=torch.float64, device=dev)
        else:
            confusion, sums = into["confusion"], into["sums"]
            what = "into: a previous result of map_scores for %d classes and %d offsets on the maps' GPU" % (C, O)
            _dev_tensor(confusion, what, torch.int64, shape=(C, C), device=dev)
            _dev_tensor(sums, what, torch.float64, shape=(3, O), device=dev)
        stream = _stream(dev)
        rc = fn(self.handle, class_probs.data_ptr(), C, same_probs.data_ptr(), O,
                self._dtype(class_probs) | (MN_MAPS_LOGITS if logits else 0), W, H, C, off.ctypes.data_as(_i32p),
                truth.data_ptr(), G, truth_classes.data_ptr() if G else None, confusion.data_ptr(), sums.data_ptr(),
                1 if into is not None else 0, stream)
        _ok(rc)
        return {"confusion": confusion, "sums": sums}

    def mask_bce(self, class_logits, same_logits, offsets, truth, truth_classes, scale_class: float = 1.0,
                 scale_same: float = 1.0, grad: bool = True, into=None, out=None):
        """The training criterion of the reference from the label mask: ``torch.nn.BCEWithLogitsLoss`` of the class
        planes and of the offset planes (egs/cityscape/local/train.py:183-195) as sums, and its gradient, in one pass
        on the device -- each logit is read once, each gradient element written once, no target plane exists.
        ``class_logits`` [C,H,W] and ``same_logits`` [O,H,W]: contiguous float32, float16 or bfloat16 LOGITS (views
        of one prediction tensor are fine); either may be None or have no planes (offset-only or class-only
        training), not both.  ``truth``, ``truth_classes``: as for :meth:`map_scores`; a pixel whose truth class is
        outside 0..C-1 is an ignore class: no class term, class gradient 0, offset planes as usual.  Returns
        ``{"sums": float64 [2+O], "grad_class": [C,H,W] or None, "grad_same": [O,H,W] or None}`` on the maps' device:
        ``sums[0]`` the sum of the class terms, ``sums[1+k]`` the sum of the terms of offset k, ``sums[1+O]`` the
        number of kept pixels (``labels.mask_bce`` is the numpy statement and gives the definitions).  The gradients
        are ``(sigmoid(x) - y) * scale_class`` / ``* scale_same`` in the maps' dtype; ``grad=False``: the sums alone
        (the validation loss), bit-equal to those of a call with gradients.  ``out=(grad_class, grad_same)``: the
        caller's buffers of the maps' shapes and dtype, which may be views (and None for a part that has no planes).
        ``into``: a previous result (or its ``sums`` tensor), to which this image's sums are added with one IEEE
        addition each.  A float16 gradient scaled by 1 / (number of elements) underflows: pass larger scales (loss
        scaling) or use bfloat16.  The sums of a call are bit-identical from run to run and do not depend on where the
        tensors lie in memory.  Any image size; nothing is synchronised or copied.  The calls of one Merger share a
        buffer of partial sums with :meth:`map_scores`: keep them on ONE stream."""
        torch = self.torch
        fn = self._entry("mn_mask_bce_device")
        maps = [None if t is None or t.shape[0] == 0 else t for t in (class_logits, same_logits)]
        first = next((t for t in maps if t is not None), None)
        if first is None:
            raise MergeNetError(MN_ERR_ARGUMENT)                 # (what the entry point answers to C == 0 and O == 0)
        for t in maps:
            if t is None:
                continue
            _dev_tensor(t, self.MAPS_WANTED, dim=3, device=self.device)
            if t.dtype != first.dtype:
                raise ValueError("class and offset logits must share one dtype (%s)" % self.DTYPE_NAMES)
            if t.shape[1:] != first.shape[1:]:
                raise ValueError("class and offset logits differ in height or width")
        code = self._dtype(first)
        dev = first.device
        H, W = int(first.shape[1]), int(first.shape[2])
        C = 0 if maps[0] is None else int(maps[0].shape[0])
        O = 0 if maps[1] is None else int(maps[1].shape[0])
        off = np.ascontiguousarray(np.asarray(offsets if O else [], dtype=np.int32).reshape(-1, 2))
        if off.shape[0] != O:
            raise ValueError("%d offsets for %d offset planes" % (off.shape[0], O))
        G = self._check_truth(truth, truth_classes, H, W, dev)
        if into is None:
            sums = torch.empty((2 + O,), dtype=torch.float64, device=dev)
        else:
            sums = into["sums"] if isinstance(into, dict) else into
            _dev_tensor(sums, "into: a previous result of mask_bce for %d offsets on the maps' GPU" % O,
                        torch.float64, shape=(2 + O,), device=dev)
        grads = [None, None]
        if out is not None:
            if not grad or len(out) != 2:
                raise ValueError("out: (grad_class, grad_same), with grad=True")
            what = "out: contiguous buffers of the maps' shapes and dtype on the maps' GPU"
            for i, (g, t) in enumerate(zip(out, maps)):
                if t is None:
                    continue
                if g is None:
                    raise ValueError(what)
                grads[i] = _dev_tensor(g, what, t.dtype, shape=t.shape, device=dev)
        elif grad:
            grads = [None if t is None else torch.empty_like(t) for t in maps]
        stream = _stream(dev)
        rc = fn(self.handle, maps[0].data_ptr() if C else None, maps[1].data_ptr() if O else None, code, W, H, C, O,
                off.ctypes.data_as(_i32p) if O else None, truth.data_ptr(), G,
                truth_classes.data_ptr() if G else None, grads[0].data_ptr() if grads[0] is not None else None,
                grads[1].data_ptr() if grads[1] is not None else None, float(scale_class), float(scale_same),
                sums.data_ptr(), 1 if into is not None else 0, stream)
        _ok(rc)
        return {"sums": sums, "grad_class": grads[0], "grad_same": grads[1]}

    def _check_planes(self, logits, part, offsets, truth, truth_classes):
        """One part of the network's output for :meth:`plane_sums` and :meth:`plane_grad`: returns (part code, dtype
        code, P, H, W, the offsets as an int32 array or None, G)."""
        code_of = {"class": MN_PART_CLASS, "offset": MN_PART_OFFSET, MN_PART_CLASS: MN_PART_CLASS,
                   MN_PART_OFFSET: MN_PART_OFFSET}
        if part not in code_of:
            raise ValueError("part: 'class' or 'offset'")
        part = code_of[part]
        _dev_tensor(logits, self.MAPS_WANTED, dim=3, device=self.device)
        code = self._dtype(logits)
        P, H, W = (int(v) for v in logits.shape)
        off = None
        if part == MN_PART_OFFSET:
            off = np.ascontiguousarray(np.asarray(offsets, dtype=np.int32).reshape(-1, 2))
            if off.shape[0] != P:
                raise ValueError("%d offsets for %d offset planes" % (off.shape[0], P))
        G = self._check_truth(truth, truth_classes if part == MN_PART_CLASS else None, H, W, logits.device)
        return part, code, P, H, W, off, G

    def plane_sums(self, logits, part, offsets, truth, truth_classes, complement: bool = False, terms: bool = False,
                   into=None, out=None):
        """Step 1 of the criteria whose gradient needs totals over a plane (the reference's ``SoftDiceLoss`` and
        ``MultiBCEWithLogitsLoss``, utils/loss.py:38-76), from the label mask: the sums of one image.  ``logits``
        [P,H,W]: contiguous float32, float16 or bfloat16 LOGITS of ONE part of the output (a view of the prediction
        is fine); ``part``: ``'class'`` -- targets and ignore class of :meth:`mask_bce`'s class planes -- or
        ``'offset'`` with ``offsets`` (P pairs); ``truth``, ``truth_classes``: as for :meth:`mask_bce`
        (``truth_classes`` is not used by the offset part).  Returns float64 [5*P + 1] on the maps' device: per plane
        ``Q = sum q``, ``I = sum of q where z``, ``Z = number of z``, ``L1`` / ``L0 = sum of the BCE term where the
        target is 1 / 0`` (computed only with ``terms``, else 0), then the number of pixels that took part; ``q =
        sigmoid(x)``, ``z = y``, or with ``complement`` ``q = sigmoid(-x)``, ``z = !y`` (``labels.plane_sums`` is the
        numpy statement).  ``into``: a previous result, to which this image's sums are added with one IEEE addition
        each; ``out``: a caller's buffer in which they are stored (a row of a batch's table).  The sums are
        bit-identical from run to run and do not depend on where the tensor lies.  Any image size; nothing is
        synchronised or copied.  Keep the calls of one Merger on ONE stream."""
        torch = self.torch
        fn = self._entry("mn_plane_sums_device")
        part, code, P, H, W, off, G = self._check_planes(logits, part, offsets, truth, truth_classes)
        if into is not None and out is not None:
            raise ValueError("into (add) or out (store), not both")
        sums = into if into is not None else out
        if sums is None:
            sums = torch.empty((5 * P + 1,), dtype=torch.float64, device=logits.device)
        else:
            _dev_tensor(sums, "into / out: a contiguous float64 [%d] tensor on the maps' GPU" % (5 * P + 1),
                        torch.float64, shape=(5 * P + 1,), device=logits.device)
        flags = (MN_PLANE_COMPLEMENT if complement else 0) | (MN_PLANE_TERMS if terms else 0)
        stream = _stream(logits.device)
        rc = fn(self.handle, logits.data_ptr(), code, W, H, part, P, off.ctypes.data_as(_i32p) if off is not None else None,
                truth.data_ptr(), G, truth_classes.data_ptr() if G else None, flags, sums.data_ptr(),
                1 if into is not None else 0, stream)
        _ok(rc)
        return sums

    def plane_coeffs(self, criterion, sums, pixels: float = 0.0, smooth: float = 1.0, scale: float = 1.0,
                     complement: bool = False, into=None, out=None):
        """Step 2: per plane the value of the criterion and the four float32 coefficients of :meth:`plane_grad`, from
        the ``sums`` of :meth:`plane_sums` (one image's, or a batch's added up), in one small launch in float64.
        ``criterion``: ``'dice'`` (``smooth`` > 0; ``complement`` as the sums were taken) or ``'mbce'`` (``pixels`` =
        H*W; sums taken with ``terms=True``).  Returns ``{"coeffs": float32 [4,P], "loss": float64 []}``: the loss is
        ``scale`` times the planes' values added in ascending order (``labels.plane_coeffs`` is the numpy statement
        and gives the formulas).  ``out``: a caller's [4,P] buffer for the coefficients; ``into``: a previous loss
        tensor (or result) to which this loss is ADDED with one IEEE addition."""
        torch = self.torch
        fn = self._entry("mn_plane_coeffs_device")
        crit = {"dice": MN_CRIT_DICE, "mbce": MN_CRIT_MBCE, MN_CRIT_DICE: MN_CRIT_DICE, MN_CRIT_MBCE: MN_CRIT_MBCE}.get(criterion)
        if crit is None:
            raise ValueError("criterion: 'dice' or 'mbce'")
        what = "sums: a result of plane_sums on the Merger's GPU"
        if _dev_tensor(sums, what, torch.float64, dim=1, at_least=6, device=self.device).numel() % 5 != 1:
            raise ValueError(what)
        P = sums.numel() // 5
        dev = sums.device
        coeffs = torch.empty((4, P), dtype=torch.float32, device=dev) if out is None else out
        _dev_tensor(coeffs, "out: a contiguous float32 [4,%d] tensor on the sums' GPU" % P, torch.float32, shape=(4, P),
                    device=dev)
        loss = into["loss"] if isinstance(into, dict) else into
        if loss is None:
            loss = torch.empty((), dtype=torch.float64, device=dev)
        else:
            _dev_tensor(loss, "into: a float64 scalar on the sums' GPU", torch.float64, numel=1, device=dev,
                        contiguous=False)
        stream = _stream(dev)
        rc = fn(self.handle, crit, MN_PLANE_COMPLEMENT if complement else 0, sums.data_ptr(), P, float(pixels),
                float(smooth), float(scale), coeffs.data_ptr(), loss.data_ptr(), 1 if into is not None else 0, stream)
        _ok(rc)
        return {"coeffs": coeffs, "loss": loss}

    def plane_grad(self, logits, part, offsets, truth, truth_classes, coeffs, factor=None, complement: bool = False,
                   out=None):
        """Step 3: the gradient of one image from its logits, the label mask and the coefficients of
        :meth:`plane_coeffs` (arguments as for :meth:`plane_sums`): ``factor * (q*(1-q)*(c0 where z else c1) +
        (s - y)*(c2 where y else c3))`` in float32, rounded into the maps' dtype; 0 at an ignored pixel
        (``labels.plane_grad`` is the numpy statement).  ``factor``: None for 1, or a float32 scalar tensor on the
        device that the kernel reads -- the incoming gradient of a backward pass: no synchronisation and no multiply
        pass.  ``out``: a caller's buffer of the maps' shape and dtype (may be a view; must not overlap the maps).
        Each logit is read once, each gradient element written once."""
        torch = self.torch
        fn = self._entry("mn_plane_grad_device")
        part, code, P, H, W, off, G = self._check_planes(logits, part, offsets, truth, truth_classes)
        dev = logits.device
        _dev_tensor(coeffs, "coeffs: a contiguous float32 [4,%d] tensor on the maps' GPU" % P, torch.float32, shape=(4, P),
                    device=dev)
        if factor is not None:
            _dev_tensor(factor, "factor: a float32 scalar tensor on the maps' GPU, or None", torch.float32, numel=1,
                        device=dev, contiguous=False)
        grad = torch.empty_like(logits) if out is None else out
        _dev_tensor(grad, "out: a contiguous buffer of the maps' shape and dtype on the maps' GPU", logits.dtype,
                    shape=logits.shape, device=dev)
        stream = _stream(dev)
        rc = fn(self.handle, logits.data_ptr(), code, W, H, part, P, off.ctypes.data_as(_i32p) if off is not None else None,
                truth.data_ptr(), G, truth_classes.data_ptr() if G else None, MN_PLANE_COMPLEMENT if complement else 0,
                coeffs.data_ptr(), factor.data_ptr() if factor is not None else None, grad.data_ptr(), stream)
        _ok(rc)
        return grad

    def mask_ce(self, logits, part, offsets, truth, truth_classes, scale: float = 1.0, grad: bool = True, into=None,
                out=None):
        """The reference's ``CrossEntropyLossOneHot`` (utils/loss.py:24-35: ``F.cross_entropy(input,
        target.max(1)[1])``, ``--loss ce`` of the recipes) on ONE part of the output, from the label mask: the sum of
        the pixels' terms and the gradient in one pass on the device -- no target plane and no argmax plane exists,
        each gradient element is written once.  ``logits`` [P,H,W]: contiguous float32, float16 or bfloat16 LOGITS (a
        view of the prediction is fine); ``part``: ``'class'`` or ``'offset'`` with ``offsets`` (P pairs); ``truth``,
        ``truth_classes``: as for :meth:`mask_bce` (``truth_classes`` is not used by the offset part).  Target plane of
        a pixel: its truth class (class part), or the first offset plane whose target is 1, plane 0 if none is (offset
        part) -- what ``max(1)[1]`` elects on the one-hot planes.  A pixel whose truth class is outside 0..P-1 is an
        ignore class: no term, gradient 0, not counted (the reference has none: it would elect class 0 there).
        Returns ``{"sums": float64 [2], "grad": [P,H,W] or None}`` on the maps' device: ``sums[0]`` the sum of
        ``logsumexp(x) - x_target`` over the kept pixels, ``sums[1]`` their number (``labels.mask_ce`` is the numpy
        statement and gives the definitions).  The gradient is ``(softmax(x) - onehot(target)) * scale`` in the maps'
        dtype; ``grad=False``: the sums alone (the validation loss), bit-equal to those of a call with a gradient.
        ``out``: the caller's buffer of the maps' shape and dtype, which may be a view.  ``into``: a previous result
        (or its ``sums`` tensor), to which this image's sums are added with one IEEE addition each.  A float16
        gradient scaled by 1 / (number of pixels) underflows: pass a larger scale (loss scaling) or use bfloat16.
        The sums of a call are bit-identical from run to run and do not depend on where the tensors lie in memory.
        Up to 20 planes every logit is read once; above that the planes are read three times (twice without a
        gradient), the repeats through the cache.  Any image size; nothing is synchronised or copied.  The calls of
        one Merger share a buffer of partial sums with :meth:`map_scores`: keep them on ONE stream."""
        torch = self.torch
        fn = self._entry("mn_mask_ce_device")
        part, code, P, H, W, off, G = self._check_planes(logits, part, offsets, truth, truth_classes)
        dev = logits.device
        if into is None:
            sums = torch.empty((2,), dtype=torch.float64, device=dev)
        else:
            sums = into["sums"] if isinstance(into, dict) else into
            _dev_tensor(sums, "into: a previous result of mask_ce on the maps' GPU", torch.float64, shape=(2,),
                        device=dev)
        g = None
        if out is not None:
            if not grad:
                raise ValueError("out: the gradient's buffer, with grad=True")
            g = _dev_tensor(out, "out: a contiguous buffer of the maps' shape and dtype on the maps' GPU", logits.dtype,
                            shape=logits.shape, device=dev)
        elif grad:
            g = torch.empty_like(logits)
        stream = _stream(dev)
        rc = fn(self.handle, logits.data_ptr(), code, W, H, part, P,
                off.ctypes.data_as(_i32p) if off is not None else None, truth.data_ptr(), G,
                truth_classes.data_ptr() if G else None, g.data_ptr() if g is not None else None, float(scale),
                sums.data_ptr(), 1 if into is not None else 0, stream)
        _ok(rc)
        return {"sums": sums, "grad": g}

    def tile_class_maps(self, tiles, flip_tiles, row_starts, col_starts, height: int, width: int, num_classes: int,
                        out_dtype=None, clip: bool = False):
        """The image's class planes from the LOGITS of a semantic network run on overlapping tiles: what the
        reference's ``tile_predict`` (models/pspnet_caffe.py:492-560) assembles in numpy on the host, in one kernel.
        ``tiles`` [T,Cn,th,tw] (float32, float16 or bfloat16, contiguous, on the GPU): tile t = i * len(col_starts) + j
        has its top-left pixel at (row_starts[i], col_starts[j]); ``flip_tiles``: the same shape and dtype or None,
        the network's output on the horizontally flipped slice as it came out.  ``row_starts`` / ``col_starts``:
        sequences of at most 32 ints (``tiles.tile_starts`` gives the reference's); duplicates are legal.  Per tile
        pixel the softmax over the Cn classes, the two passes averaged, plane 0 = the maximum over the first
        Cn - C + 1 classes, planes 1..C-1 = the rest; per image pixel the sum over the covering tiles, divided by
        their number, renormalised over the C planes, then the merger's clip if ``clip`` -- float32 throughout
        (``tiles.tile_class_maps_reference`` is the numpy statement).  Returns [C,height,width] on the tiles' device in
        ``out_dtype`` (None: the tiles' dtype; a 16-bit output is the float32 value rounded to nearest even).  Runs
        on the current stream; nothing is synchronised or copied.  Any image size; Cn <= 64.  A tile that leaves the
        image or a pixel that no tile covers raises MergeNetError before anything is launched."""
        torch = self.torch
        fn = self._entry("mn_tile_class_maps_device")
        _dev_tensor(tiles, "tiles: a contiguous %s [T,Cn,th,tw] tensor on the Merger's GPU" % self.DTYPE_NAMES, dim=4,
                    device=self.device)
        code = self._dtype(tiles)
        if flip_tiles is not None:
            _dev_tensor(flip_tiles, "flip_tiles: a contiguous tensor of the shape, dtype and device of tiles, or None",
                        tiles.dtype, shape=tiles.shape, device=tiles.device)
        out_dtype = tiles.dtype if out_dtype is None else out_dtype
        out_code = self._out_dtype(out_dtype)
        rows = np.ascontiguousarray(np.asarray(list(row_starts), dtype=np.int32).reshape(-1))
        cols = np.ascontiguousarray(np.asarray(list(col_starts), dtype=np.int32).reshape(-1))
        T, Cn, th, tw = (int(v) for v in tiles.shape)
        if T != len(rows) * len(cols):
            raise ValueError("%d tiles for %d x %d starts" % (T, len(rows), len(cols)))
        H, W, C = int(height), int(width), int(num_classes)
        if H <= 0 or W <= 0 or C <= 0:
            raise MergeNetError(-1)
        out = torch.empty((C, H, W), dtype=out_dtype, device=tiles.device)
        stream = _stream(tiles.device)
        rc = fn(self.handle, tiles.data_ptr(), flip_tiles.data_ptr() if flip_tiles is not None else None, code,
                Cn, th, tw, rows.ctypes.data_as(_i32p), len(rows), cols.ctypes.data_as(_i32p), len(cols),
                H, W, C, out.data_ptr(), out_code, int(bool(clip)), stream)
        _ok(rc)
        return out


class DatasetEval:
    """The evaluation of a whole validation pass on the device (``Merger.dataset_eval``):

        ev = merger.dataset_eval(num_classes=9)
        for image in validation_set:
            ...
            table = merger.overlap_table(mask, truth, K, G)
            ev.add(table, classes, truth_classes, scores, crowd)      # enqueues only
        numbers = ev.summarize()                                      # {"AP": ..., "AP50": ..., ...}

    ``add`` appends one record per detection to a log on the device -- class, score, rank among the image's detections
    of its class, image ordinal, and a matched and an ignored bit per area range and IoU threshold -- and adds the
    image's non-ignored truth instances to ``npig``.  The host knows the number of records an image adds (K, from the
    table's shape), so it keeps the fill of the log itself: no counter lives on the device and nothing is ever read
    back.  ``accumulate`` is COCOeval.accumulate over the log; ``summarize`` makes the one host copy.
    ``labels.eval_records``, ``labels.coco_accumulate`` and ``labels.coco_summarize`` are the numpy statements and
    give the definitions; the device arrays equal them bit for bit.  (The contract is pinned to those statements and
    to hand-computed cases, not to pycocotools, which is not a dependency.)
    All calls of one evaluator, and the other matching calls of its Merger, belong on ONE stream."""

    def __init__(self, merger, num_classes: int, thresholds=None, rec_thresholds=None, area_ranges=None,
                 max_dets=(1, 10, 100), capacity: int = 16384):
        from . import labels
        torch = merger.torch
        self._append = merger._entry("mn_eval_append_device")
        self._keys = merger._entry("mn_eval_keys_device")
        self._accumulate = merger._entry("mn_eval_accumulate_device")
        self.merger, self.torch = merger, torch
        self.num_classes = int(num_classes)
        if self.num_classes < 1:
            raise ValueError("num_classes >= 1")
        th, ar, md = labels._eval_params(thresholds, area_ranges, max_dets)
        self.thresholds = np.ascontiguousarray(th, np.float64)
        self.area_ranges = np.ascontiguousarray(ar, np.float64)
        self.max_dets = tuple(md)
        self._max_dets_c = (ctypes.c_int * len(md))(*md)
        rec = labels.COCO_REC_THRESHOLDS if rec_thresholds is None else np.asarray(rec_thresholds, np.float64)
        self.rec_thresholds = np.ascontiguousarray(rec.reshape(-1), np.float64)
        if int(capacity) < 1:
            raise ValueError("capacity >= 1")
        self.device = torch.device("cuda", merger.device)
        self._rec_dev = torch.from_numpy(self.rec_thresholds.copy()).to(self.device)
        self._capacity0 = int(capacity)
        self.reset()

    def reset(self) -> None:
        """Empty the log and zero ``npig`` (on the current stream); the capacity goes back to the initial one."""
        torch = self.torch
        self._log = torch.empty((self._capacity0, MN_EVAL_RECORD_BYTES // 4), dtype=torch.int32, device=self.device)
        self._npig = torch.zeros((self.num_classes, len(self.area_ranges)), dtype=torch.int64, device=self.device)
        self.num_records = 0
        self.num_images = 0

    @property
    def capacity(self) -> int:
        return int(self._log.shape[0])

    def add(self, table, pred_classes, truth_classes, scores=None, crowd=None) -> None:
        """One image: the arguments of :meth:`Merger.match_instances`.  Enqueues on the current stream; nothing is
        synchronised.  K, G <= 4096."""
        torch = self.torch
        K, G = _check_match_inputs(table, pred_classes, truth_classes, scores, crowd, device=self.device)
        if K > MN_MATCH_MAX_INSTANCES or G > MN_MATCH_MAX_INSTANCES:
            raise ValueError("at most %d prediction and truth instances per image" % MN_MATCH_MAX_INSTANCES)
        if self.num_records + K > 2 ** 31 - 1:
            raise ValueError("the log holds at most 2^31 - 1 records")
        if self.num_records + K > self.capacity:                 # grow by doubling: a copy on the stream, no read-back
            grown = torch.empty((max(2 * self.capacity, self.num_records + K), self._log.shape[1]),
                                dtype=torch.int32, device=self.device)
            grown[:self.num_records].copy_(self._log[:self.num_records])
            self._log = grown
        _f64p = ctypes.POINTER(ctypes.c_double)
        stream = _stream(self.device)
        rc = self._append(self.merger.handle, table.data_ptr(), K, G, pred_classes.data_ptr(),
                          scores.data_ptr() if scores is not None else None, truth_classes.data_ptr(),
                          crowd.data_ptr() if crowd is not None else None, self.thresholds.ctypes.data_as(_f64p),
                          len(self.thresholds), self.area_ranges.ctypes.data_as(_f64p), len(self.area_ranges),
                          self.max_dets[-1], self.num_classes, self.num_images,
                          self._log.data_ptr() + self.num_records * MN_EVAL_RECORD_BYTES, self._npig.data_ptr(), stream)
        _ok(rc)
        self.num_records += K
        self.num_images += 1

    def accumulate(self) -> dict:
        """``{"precision": float64 [T,R,C,A,M], "recall": float64 [T,C,A,M], "scores": float64 [T,R,C,A,M], "npig":
        int64 [C,A]}`` on the device, as ``labels.coco_accumulate`` defines them; -1 where a class has no non-ignored
        truth instance in an area range (everywhere for an evaluator without images).  A key per record, torch's
        stable sort of the keys, then one pass over the sorted log.  The log is left as it is: more images may follow."""
        torch = self.torch
        T, R, C = len(self.thresholds), len(self.rec_thresholds), self.num_classes
        A, M, N = len(self.area_ranges), len(self.max_dets), self.num_records
        stream = _stream(self.device)
        keys = index = None
        if N:
            raw = torch.empty((N,), dtype=torch.int64, device=self.device)
            rc = self._keys(self.merger.handle, self._log.data_ptr(), N, C, raw.data_ptr(), stream)
            _ok(rc)
            keys, index = torch.sort(raw, stable=True)
        precision = torch.empty((T, R, C, A, M), dtype=torch.float64, device=self.device)
        recall = torch.empty((T, C, A, M), dtype=torch.float64, device=self.device)
        scores = torch.empty((T, R, C, A, M), dtype=torch.float64, device=self.device)
        rc = self._accumulate(self.merger.handle, self._log.data_ptr() if N else None, N,
                              keys.data_ptr() if N else None, index.data_ptr() if N else None, self._npig.data_ptr(),
                              C, T, self._rec_dev.data_ptr() if R else None, R, A, self._max_dets_c, M,
                              precision.data_ptr(), recall.data_ptr(), scores.data_ptr(), stream)
        _ok(rc)
        return {"precision": precision, "recall": recall, "scores": scores, "npig": self._npig.clone()}

    def summarize(self, result=None, classes=None) -> dict:
        """The twelve numbers of COCOeval.summarize (``labels.coco_summarize``; keys ``labels.eval_summary_names``) over
        ``classes`` (default 1..C-1).  ``result``: what :meth:`accumulate` gave, or None to run it.  Copies the
        arrays to the host: the one synchronisation of the evaluation."""
        from . import labels
        result = self.accumulate() if result is None else result
        host = {k: result[k].cpu().numpy() for k in ("precision", "recall")}
        return labels.coco_summarize(host, self.thresholds, self.max_dets, classes)

    def records(self) -> dict:
        """The log on the host, for inspection and tests (synchronises): what ``labels.eval_records`` returns for each
        image, concatenated in ``add`` order -- ``classes``, ``scores``, ``rank``, ``image`` [N], ``matched`` and
        ``ignored`` bool [A,T,N]."""
        T, A, N = len(self.thresholds), len(self.area_ranges), self.num_records
        raw = self._log[:N].cpu().numpy()
        bits = np.arange(A * T, dtype=np.uint64)
        words = raw[:, 4:8].copy().view(np.uint64).reshape(N, 2)

        def planes(col):
            return ((words[:, col][None, :] >> bits[:, None]) & np.uint64(1)).astype(bool).reshape(A, T, N)

        return {"classes": raw[:, 0].copy(), "scores": raw[:, 1].copy().view(np.float32), "rank": raw[:, 2].copy(),
                "image": raw[:, 3].copy(), "matched": planes(0), "ignored": planes(1)}


class PendingSegment:
    """An image queued by :meth:`Merger.segment_async`; ``result()`` finishes it (once)."""

    def __init__(self, merger, mask, table, part, keepalive):
        self._merger, self._out, self._keepalive = merger, (mask, table, part), keepalive
        self._done = None

    def result(self):
        if self._done is None:
            stats = MnStats()
            rc = self._merger.lib.mn_segment_finish(self._merger.handle, ctypes.byref(stats))
            self._keepalive = None
            _ok(rc)
            self._done = self._out + (stats.as_dict(),)
        return self._done


class ExactBatch:
    """``count`` images of one shape through the exact engine in ONE launch of its loop
    (``mn_segment_exact_batch``): the engine is one wavefront per image, so images in flight are its
    throughput.  One context (workspace) per image; ``segment`` takes lists of [C,H,W] / [O,H,W] tensors
    (at most ``count``) and returns a list of what :meth:`Merger.segment` returns.

    ``require_proof = 1`` is applied per image as a single call applies it: results that are ``proof 3`` are redone
    together in the reference's order among equals.  Where that cannot be done (the Python variant) the call raises
    ``MergeNetError`` with status ``MN_ERR_UNPROVEN`` whose ``results`` attribute is the list ``segment`` would have
    returned: every image's output is valid, and ``stats["status"] == MN_ERR_UNPROVEN`` marks the unproven ones."""

    def __init__(self, H: int, W: int, C: int, O: int, count: int, device: Optional[int] = None):
        if count < 1:
            raise ValueError("count >= 1")
        self.mergers = [Merger(H, W, C, O, device=device) for _ in range(count)]
        self.lib = self.mergers[0].lib
        self.torch = self.mergers[0].torch

    def segment(self, class_probs: Sequence, same_probs: Sequence, offsets, opts: Optional[MnOptions] = None,
                want_partition: bool = False, logits: bool = False):
        torch = self.torch
        n = len(class_probs)
        if n < 1 or n > len(self.mergers) or len(same_probs) != n:
            raise ValueError("between 1 and %d images" % len(self.mergers))
        shape = None
        for cp, sp in zip(class_probs, same_probs):
            C, H, W, O, off = self.mergers[0]._check(cp, sp, offsets)
            if shape is not None and shape != (C, H, W, O, cp.dtype):
                raise ValueError("the images of a batch have one shape and one dtype")
            shape = (C, H, W, O, cp.dtype)
        opts = opts if opts is not None else default_options()
        dev = class_probs[0].device
        masks = [torch.empty((H, W), dtype=torch.int32, device=dev) for _ in range(n)]
        tables = [torch.empty((H * W,), dtype=torch.int32, device=dev) for _ in range(n)]
        parts = [torch.empty((H, W), dtype=torch.int32, device=dev) for _ in range(n)] if want_partition else None
        vp = ctypes.c_void_p * n
        stats = (MnStats * n)()
        stream = _stream(dev)
        fn, dt = self.mergers[0]._typed("mn_segment_exact_batch", self.mergers[0]._dtype(class_probs[0]), logits)
        rc = fn(
            vp(*[m.handle for m in self.mergers[:n]]), n, vp(*[t.data_ptr() for t in class_probs]), C,
            vp(*[t.data_ptr() for t in same_probs]), O, *dt, W, H, C, off.ctypes.data_as(_i32p),
            vp(*[t.data_ptr() for t in masks]), vp(*[t.data_ptr() for t in tables]),
            vp(*[t.data_ptr() for t in parts]) if parts is not None else None,
            ctypes.byref(opts), stream, stats)
        results = [(masks[i], tables[i], parts[i] if parts is not None else None, stats[i].as_dict())
                   for i in range(n)]
        if rc == MN_ERR_UNPROVEN:
            err = MergeNetError(rc)
            err.results = results
            raise err
        _ok(rc)
        return results

    def close(self):
        for m in self.mergers:
            m.close()
        self.mergers = []


class MergerPool:
    """Several images in flight on one GPU: ``depth`` contexts, each with its own HIP stream and
    its own host thread.

    One merge has a host round trip (record count and statistics) and mostly latency-bound
    kernels, so a single context leaves the GPU idle part of the time; four images in flight
    nearly double the images per second on an MI355X.  ``submit`` returns a
    ``concurrent.futures.Future`` whose result is what ``Merger.segment`` returns; inputs may
    still be in flight on the submitting thread's current stream (the worker waits for them), and
    the outputs are safe to use on that stream.

        pool = MergerPool(H, W, C, O, depth=4)
        futures = [pool.submit(cp, sp, offsets, opts) for cp, sp in images]
        for f in futures:
            mask, class_table, _, stats = f.result()
        pool.close()
    """

    def __init__(self, H: int, W: int, C: int, O: int, depth: int = 4, device: Optional[int] = None):
        import queue
        import threading
        import torch
        if depth < 1:
            raise ValueError("depth >= 1")
        self.torch = torch
        self.device = torch.cuda.current_device() if device is None else int(device)
        self.mergers = [Merger(H, W, C, O, device=self.device) for _ in range(depth)]
        self.jobs = queue.Queue()
        self.threads = [threading.Thread(target=self._work, args=(m,), daemon=True) for m in self.mergers]
        for t in self.threads:
            t.start()

    def _work(self, merger):
        torch = self.torch
        dev = torch.device("cuda", self.device)
        torch.cuda.set_device(dev)
        stream = torch.cuda.Stream(dev)
        while True:
            job = self.jobs.get()
            if job is None:
                return
            fut, ready, home, args, kwargs = job
            if not fut.set_running_or_notify_cancel():
                continue
            try:
                with torch.cuda.stream(stream):
                    stream.wait_event(ready)             # the producer of the inputs
                    out = merger.segment(*args, **kwargs)   # returns after its stream has drained
                    for t in out[:3]:
                        if t is not None:
                            t.record_stream(home)        # allocator: also in use on the caller's stream
                fut.set_result(out)
            except BaseException as e:                   # noqa: BLE001 -- handed to the caller
                fut.set_exception(e)

    def submit(self, class_probs, same_probs, offsets, opts: Optional[MnOptions] = None,
               want_partition: bool = False, logits: bool = False):
        from concurrent.futures import Future
        torch = self.torch
        if not self.threads:
            raise RuntimeError("MergerPool is closed")
        home = torch.cuda.current_stream(torch.device("cuda", self.device))
        ready = torch.cuda.Event()
        ready.record(home)
        fut = Future()
        self.jobs.put((fut, ready, home, (class_probs, same_probs, offsets),
                       {"opts": opts, "want_partition": want_partition, "logits": logits}))
        return fut

    def map(self, images, offsets, opts: Optional[MnOptions] = None, logits: bool = False):
        """Results for an iterable of (class_probs, same_probs), in order, all images in flight."""
        futures = [self.submit(cp, sp, offsets, opts, logits=logits) for cp, sp in images]
        return [f.result() for f in futures]

    def close(self):
        for _ in self.threads:
            self.jobs.put(None)
        for t in self.threads:
            t.join()
        self.threads = []
        for m in self.mergers:
            m.close()
        self.mergers = []

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def pack_wire(mask, class_table, num_instances: int, wire, max_instances: int,
              total_logprob: float = float("nan")) -> None:
    """Device tensors: int32 mask [H,W] + class table -> int16 wire buffer of the mask exchange
    (``mn_pack_wire_device``; layout in ``mergenet_amd/distributed.py``).  Runs on the current
    torch stream of the mask's device."""
    import torch
    lib = load_library()
    n = mask.numel()
    if (mask.dtype != torch.int32 or class_table.dtype != torch.int32 or wire.dtype != torch.int16
            or not mask.is_contiguous() or wire.numel() < n + 1 + max_instances + 4
            or class_table.numel() < num_instances):
        raise AssertionError("pack_wire: int32 mask/table, int16 wire of n + 1 + max_instances + 4")
    stream = _stream(mask.device)
    rc = lib.mn_pack_wire_device(mask.data_ptr(), class_table.data_ptr(), int(num_instances),
                                 float(total_logprob), n, int(max_instances), wire.data_ptr(), stream)
    _ok(rc)



def runs_wire_words(capacity: int, max_instances: int) -> int:
    """int32 words of the run-length wire buffer (``mn_runs_wire_words``)."""
    return 4 + capacity + (capacity + 1) // 2 + (max_instances + 3) // 4


def pack_runs(merger, mask, class_table, num_instances: int, wire, capacity: int, max_instances: int,
              total_logprob: float = float("nan")) -> None:
    """Device tensors: int32 mask [H,W] + class table -> int32 run-length wire buffer
    (``mn_pack_runs_device``: row-major label change points; layout in include/mergenet_hip.h).
    Runs on the current torch stream; no host synchronisation."""
    import torch
    n = mask.numel()
    if (mask.dtype != torch.int32 or class_table.dtype != torch.int32 or wire.dtype != torch.int32
            or not mask.is_contiguous() or wire.numel() < runs_wire_words(capacity, max_instances)
            or class_table.numel() < num_instances):
        raise AssertionError("pack_runs: int32 mask/table, int32 wire of runs_wire_words(capacity, max_instances)")
    stream = _stream(mask.device)
    rc = merger.lib.mn_pack_runs_device(merger.handle, mask.data_ptr(), class_table.data_ptr(),
                                        int(num_instances), float(total_logprob), n, int(capacity),
                                        int(max_instances), wire.data_ptr(), stream)
    _ok(rc)


def unpack_runs_batch(wires, height: int, width: int, capacity: int, max_instances: int):
    """`count` run-length wires (device, int32 [count, words], rows may be strided) -> (masks int32 [count,H,W],
    class tables int32 [count, max_instances]) in ONE launch."""
    import torch
    lib = load_library()
    count = int(wires.shape[0])
    masks = torch.empty((count, height, width), dtype=torch.int32, device=wires.device)
    tables = torch.empty((count, max_instances), dtype=torch.int32, device=wires.device)
    stream = _stream(wires.device)
    rc = lib.mn_unpack_runs_batch_device(wires.data_ptr(), int(wires.stride(0)), count, height * width,
                                         int(capacity), int(max_instances), masks.data_ptr(), tables.data_ptr(), stream)
    _ok(rc)
    return masks, tables


def unpack_runs(wire, height: int, width: int, capacity: int, max_instances: int):
    """Run-length wire buffer (device, int32) -> (mask int32 [H,W], class table int32 [max_instances])."""
    import torch
    lib = load_library()
    mask = torch.empty((height, width), dtype=torch.int32, device=wire.device)
    table = torch.empty((max_instances,), dtype=torch.int32, device=wire.device)
    stream = _stream(wire.device)
    rc = lib.mn_unpack_runs_device(wire.data_ptr(), height * width, int(capacity), int(max_instances),
                                   mask.data_ptr(), table.data_ptr(), stream)
    _ok(rc)
    return mask, table
