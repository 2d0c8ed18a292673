"""Functional layer over the C ABI: buffer ownership (torch allocates, the library only borrows),
stream selection, and the autograd.Function that replaces the reference's ~45-op autograd graph
(DG-SCT/AVE/nets/net_trans.py:552-674) by one forward and one backward library call."""
from __future__ import annotations

import contextlib
import dataclasses
import os
import threading
import warnings
from typing import Dict, List, Optional, Tuple

import torch

from . import _lib
from ._lib import AdapterDesc, Lib, P_COUNT, P_INDEX, PARAM_NAMES


@dataclasses.dataclass(frozen=True)
class AdapterSpec:
    """Static description of one adapter (everything in dgsct_adapter_desc except BT/dtype/training)."""
    N: int
    C: int
    No: int
    Co: int
    tk: int = 32
    r: int = 8
    g: int = 2
    use_bn: bool = True
    use_gate: bool = True
    ln_before: bool = True
    ln_post: bool = True
    gate_before_ln_post: bool = False
    remap: str = "conv"          # "conv" | "bicubic"
    alpha: float = 0.3
    beta: float = 0.05
    gamma: float = 0.0
    temporal: bool = False
    T: int = 10
    eps: float = 1e-5
    bn_momentum: float = 0.1
    fp8: bool = False            # bf16 + fp8 (e4m3) MFMA operands for fc / fc_affine_video_1 / fc_affine_video_2 (BASELINE configs[4])

    def desc(self, BT: int, dtype: torch.dtype, training: bool) -> AdapterDesc:
        key = (self, BT, dtype, bool(training))
        d = _DESC_CACHE.get(key)
        if d is not None:
            return d
        d = _DESC_CACHE[key] = self._make_desc(BT, dtype, training)
        return d

    def _make_desc(self, BT: int, dtype: torch.dtype, training: bool) -> AdapterDesc:
        d = AdapterDesc()
        d.BT, d.T, d.N, d.C, d.No, d.Co, d.tk, d.r, d.g = BT, self.T, self.N, self.C, self.No, self.Co, self.tk, self.r, self.g
        d.dtype = (_lib.BF16_FP8 if self.fp8 else _lib.BF16) if dtype == torch.bfloat16 else _lib.F32
        d.remap = _lib.REMAP_CONV if self.remap == "conv" else _lib.REMAP_FIXED
        d.use_bn, d.use_gate, d.ln_before, d.ln_post = int(self.use_bn), int(self.use_gate), int(self.ln_before), int(self.ln_post)
        d.gate_before_ln_post, d.temporal, d.training = int(self.gate_before_ln_post), int(self.temporal), int(training)
        d.alpha, d.beta, d.gamma, d.eps, d.bn_momentum = self.alpha, self.beta, self.gamma, self.eps, self.bn_momentum
        return d


_DESC_CACHE: Dict[Tuple, AdapterDesc] = {}
_SIZE_CACHE: Dict[Tuple, object] = {}


def _sizes(lib: Lib, d: AdapterDesc):
    """dgsct_query results are pure functions of the descriptor and of the layout switch the library reads from the environment
    at every call (test hook: DGSCT_WIDE_ATTN): ask once per (library, descriptor, switch)."""
    key = (id(lib), id(d), os.environ.get("DGSCT_WIDE_ATTN"))
    s = _SIZE_CACHE.get(key)
    if s is None:
        s = _SIZE_CACHE[key] = lib.query(d)
    return s


# ---------------------------------------------------------------------------------------------
# scratch: one growing buffer per (device, stream); calls on a stream serialise, so sharing is safe.
_WS: Dict[Tuple, torch.Tensor] = {}
_WS_LOCK = threading.Lock()


def _stream_of(t: torch.Tensor) -> int:
    return torch.cuda.current_stream(t.device).cuda_stream if t.is_cuda else 0


_AUX: Dict[Tuple, "torch.cuda.Stream"] = {}
USE_AUX_STREAM = os.environ.get("DGSCT_NO_AUX", "0") != "1"


COMPUTE_PRIORITY_CLASS = int(os.environ.get("DGSCT_COMPUTE_PRIORITY", "-1"))      # second adapter stream (AdapterStack)
# aux streams carry work nothing waits for until the end of the call (weight gradients, dX): LOW priority, so the
# dispatcher prefers the kernels of the dependency chain whenever both are runnable (76.8 vs 77.8 ms per step), and a
# third queue pool, so main (normal) / second adapter stream (high) / aux (low) can never share a hardware queue
AUX_PRIORITY_CLASS = int(os.environ.get("DGSCT_AUX_PRIORITY", "1"))


def priority_stream(lib: Lib, device: torch.device, priority_class: int) -> "torch.cuda.Stream":
    """A torch handle on a library-created HIP stream of the given priority class (-1 high / 0 / +1 low).  Streams of
    different classes never share a hardware queue (include/dgsct.h, dgsct_stream_create), whatever else (RCCL, torch's
    stream pool) has created streams before."""
    with torch.cuda.device(device):
        raw = lib.stream_create(priority_class)
    return torch.cuda.ExternalStream(raw, device=device)


_SIDE: Dict[int, "torch.cuda.Stream"] = {}


def side_stream(lib: Lib, device: torch.device) -> "torch.cuda.Stream":
    """THE second adapter stream of a device (AdapterStack runs the audio adapter of a pair on it).  One per device for the
    whole process, like the aux streams below: every extra stream an instance created would land on some hardware queue
    of its pool, and two busy streams on one queue serialise (measured: a second AdapterStack with its own streams ran
    its step in 124 ms instead of 73)."""
    with _WS_LOCK:
        s = _SIDE.get(device.index)
        if s is None:
            s = _SIDE[device.index] = priority_stream(lib, device, COMPUTE_PRIORITY_CLASS)
    return s


def _aux_stream(lib: Lib, t: torch.Tensor, stream: int) -> Optional[int]:
    """one low-priority side stream per (device, caller stream): weight gradients overlap the data-gradient chain on it"""
    if not (USE_AUX_STREAM and t.is_cuda):
        return None
    key = (t.device.index, stream)
    with _WS_LOCK:
        s = _AUX.get(key)
        if s is None:
            s = _AUX[key] = priority_stream(lib, t.device, AUX_PRIORITY_CLASS)
    return s.cuda_stream


def _workspace(device: torch.device, stream: int, nbytes: int, slot: int = 0) -> torch.Tensor:
    key = (device.type, device.index, stream, slot)
    with _WS_LOCK:
        buf = _WS.get(key)
        if buf is None or buf.numel() < nbytes:
            buf = torch.empty(int(nbytes * 1.0) + 256, dtype=torch.uint8, device=device)
            _WS[key] = buf
    return buf


def release_workspaces():
    drain_aux()
    with _WS_LOCK:
        _WS.clear()


# ---- deferred join of the weight-gradient (aux) stream (round 5) -------------------------------------------------------------
# dgsct_adapter_backward_ex(DGSCT_BWD_NO_JOIN) returns with its weight gradients still running on the aux stream: the chain of the
# NEXT backward call on the same stream starts at once instead of waiting for them (0.9 ms of the 50 ms AVE step, most of it the
# remap weight gradient of stage 0).  What that leaves to the caller is done here:
#   * two workspaces per stream, used alternately: call k + 1 never overwrites what call k's aux kernels still read;
#   * an event recorded on the aux stream behind call k is waited for by the main stream at the END of call k + 1 (it has long
#     completed by then); only then are call k's buffers (saved activations, inputs, its workspace) let go;
#   * the gradients of the LAST calls are ordered by drain_aux(): queued as an autograd end-of-backward callback (the stream that
#     called backward() waits for every pending aux event), and called by the data-parallel reducer before it launches a collective.
# Only the flat-parameter path defers (autograd adopts the gradient buffer without reading it); DGSCT_DEFER_AUX=0 switches it off.
DEFER_AUX_JOIN = os.environ.get("DGSCT_DEFER_AUX", "1") != "0"
_PENDING: Dict[Tuple, Tuple] = {}          # (device index, stream) -> (event on aux, tensors kept alive)
_SLOT: Dict[Tuple, int] = {}


def drain_aux(device: Optional[torch.device] = None):
    """Order the CURRENT stream -- and each stream whose backward calls deferred their join -- after every weight-gradient stream that
    still has work in flight.  Cheap when nothing is pending."""
    if not _PENDING:
        return
    want = None if device is None else (device.index if device.index is not None else torch.cuda.current_device())
    with _WS_LOCK:
        items = [(k, v) for k, v in _PENDING.items() if want is None or k[0] == want]
        for k, _ in items:
            del _PENDING[k]
    for (dev, stream), (ev, keep) in items:
        torch.cuda.current_stream(dev).wait_event(ev)
        prod = torch.cuda.ExternalStream(stream, device=torch.device("cuda", dev)) if stream else torch.cuda.default_stream(dev)
        prod.wait_event(ev)
        del keep


def _wait_pending(dev: torch.device, stream: int):
    """A call that does NOT defer (forward, joined backward) is about to reuse workspace slot 0 of this stream: if the previous
    backward on the stream deferred its join, its weight-gradient kernels on the aux stream may still be reading that workspace
    (stream_fork only orders aux behind main, never the reverse).  Order the current stream behind that call's aux event first, and
    let its buffers go.  A dictionary lookup when nothing is pending."""
    if not _PENDING:
        return
    key = (dev.index, stream)
    with _WS_LOCK:
        prev = _PENDING.pop(key, None)
    if prev is not None:
        torch.cuda.current_stream(dev).wait_event(prev[0])
        del prev


def _queue_drain():
    """drain_aux() when the autograd engine has run the last node of this backward pass.  Queued by EVERY deferring call: backward nodes
    run on the engine's per-device worker threads and the callbacks on whichever thread finishes the graph task, so a once-per-pass
    flag cannot live in thread-local storage; a drain that finds nothing pending costs a dictionary lookup.  The engine runs final
    callbacks on the stream that was current around the user's backward() call, which is the stream that reads the gradients next."""
    try:
        torch.autograd.Variable._execution_engine.queue_callback(drain_aux)
    except RuntimeError:                   # not inside a backward pass (raw calls from tests / tools): the caller drains
        pass


def _dev_guard(t: torch.Tensor):
    """The library launches on the CURRENT HIP device (kernel launches, occupancy queries, event creation): make it the
    device that owns the tensors and streams of this call (a module on cuda:1 called while cuda:0 is current)."""
    return torch.cuda.device(t.device) if t.is_cuda else contextlib.nullcontext()


def _ptrs(params: List[Optional[torch.Tensor]]):
    return Lib.ptr_table([p.data_ptr() if p is not None else None for p in params])


def check_param(name: str, p: Optional[torch.Tensor], device) -> Optional[torch.Tensor]:
    if p is None:
        return None
    if p.dtype != torch.float32 or not p.is_contiguous() or p.device != device:
        raise RuntimeError(f"dg-sct_amd: parameter {name} must be a contiguous fp32 tensor on {device}")
    return p


def prepare(lib: Lib, spec: AdapterSpec, params: List[Optional[torch.Tensor]], dtype: torch.dtype, device) -> torch.Tensor:
    """fp32 master parameters -> MFMA-operand copies + derived bias vectors (dgsct_prepare)."""
    d = spec.desc(spec.T, dtype, False)
    sz = _sizes(lib, d)
    prep = torch.empty(max(int(sz.prep_bytes), 256), dtype=torch.uint8, device=device)
    if os.environ.get("DGSCT_POISON", "0") == "1":
        prep.fill_(0xFF)
    some = next(p for p in params if p is not None)
    with _dev_guard(some):
        lib.prepare(d, _ptrs(params), prep.data_ptr(), _stream_of(some))
    return prep


_POISON = os.environ.get("DGSCT_POISON", "0") == "1"      # test hook: fill every buffer handed to the library with NaN


def _poison(*tensors):
    """DGSCT_POISON=1: every output / scratch / saved buffer starts as NaN bit patterns, so a kernel that reads memory it
    (or an earlier kernel of the call) did not write shows up as NaN in the results instead of depending on what the
    caching allocator happened to hand out."""
    for t in tensors:
        if t is not None:
            t.view(torch.uint8).fill_(0xFF)


def _mark_stream_use(*tensors):
    """Tell torch's caching allocator that these tensors are read on the CURRENT stream.  With AdapterStack's two adapter
    streams an input map (or an incoming gradient) is usually allocated on the other stream; without this, the block can be
    handed out again on its home stream while kernels enqueued here are still reading it."""
    for t in tensors:
        if t is not None and t.is_cuda:
            t.record_stream(torch.cuda.current_stream(t.device))


def raw_forward(lib: Lib, spec: AdapterSpec, params, prep, X: torch.Tensor, Y: torch.Tensor, training: bool,
                residual: Optional[torch.Tensor] = None):
    """X [BT,N,C], Y [BT,No,Co] contiguous, same dtype (fp32|bf16).  Returns (out, map, tmap, saved, desc).
    residual [BT,N,C] (may be X itself): out = residual + adapter(X, Y), the add fused into the last kernel."""
    BT = X.shape[0]
    if X.shape != (BT, spec.N, spec.C) or Y.shape != (BT, spec.No, spec.Co):
        raise RuntimeError(f"dg-sct_amd: expected X [BT,{spec.N},{spec.C}] and Y [BT,{spec.No},{spec.Co}], got "
                           f"{tuple(X.shape)} and {tuple(Y.shape)}")
    if X.dtype != Y.dtype or X.dtype not in (torch.float32, torch.bfloat16):
        raise RuntimeError("dg-sct_amd: X and Y must both be float32 or both bfloat16")
    if residual is not None and (residual.shape != X.shape or residual.dtype != X.dtype or not residual.is_contiguous()):
        raise RuntimeError("dg-sct_amd: residual must be a contiguous tensor of X's shape and dtype")
    _mark_stream_use(X, Y, residual, prep)
    d = spec.desc(BT, X.dtype, training)
    sz = _sizes(lib, d)
    dev = X.device
    out = torch.empty_like(X)
    amap = torch.empty(BT, spec.N, dtype=torch.float32, device=dev)
    tmap = torch.empty(BT, dtype=torch.float32, device=dev) if spec.temporal else None
    saved = torch.empty(int(sz.saved_bytes), dtype=torch.uint8, device=dev)
    stream = _stream_of(X)
    _wait_pending(dev, stream)                 # slot 0 may still be read by a deferred backward's weight gradients
    ws = _workspace(dev, stream, int(sz.ws_fwd_bytes))
    if _POISON:
        _poison(out, amap, tmap, saved, ws)
    with _dev_guard(X):
        lib.forward(d, _ptrs(params), prep.data_ptr(), X.data_ptr(), Y.data_ptr(), out.data_ptr(), amap.data_ptr(),
                    tmap.data_ptr() if tmap is not None else None, saved.data_ptr(), ws.data_ptr(), stream,
                    residual.data_ptr() if residual is not None else None, _aux_stream(lib, X, stream))
    return out, amap, tmap, saved, d


def raw_backward(lib: Lib, spec: AdapterSpec, d: AdapterDesc, params, prep, X, Y, saved, dOut, dMap, dTmap, flat_out=False,
                 skip_into_dx=False, defer_join=False, hold_dy=False, dx_event=None, slot_base=0):
    """defer_join: the call returns without joining its weight-gradient stream (see DEFER_AUX_JOIN above); `grads` is complete only
    after drain_aux() -- dX / dY are ordered on the current stream as always.
    hold_dy: everything but the product that writes dY (pair backward below): returns (dX, ws, grads) -- `ws` is what
    raw_backward_dy() needs; dx_event (raw hipEvent_t) is recorded on the call's stream once dX is complete."""
    _mark_stream_use(X, Y, saved, dOut, dMap, dTmap, prep)
    sz = _sizes(lib, d)
    dev = X.device
    dX = torch.empty_like(X)
    dY = None if hold_dy else torch.empty_like(Y)
    grads = torch.empty(int(sz.grad_floats), dtype=torch.float32, device=dev)
    stream = _stream_of(X)
    aux = _aux_stream(lib, X, stream)
    defer = bool(defer_join and DEFER_AUX_JOIN and aux is not None)
    key = (dev.index, stream)
    slot = 0
    if defer:
        slot = _SLOT[key] = 1 - _SLOT.get(key, 1)
    else:
        _wait_pending(dev, stream)             # a joined call takes slot 0 whatever the deferred call before it used
        _SLOT.pop(key, None)                   # (the next deferring call starts at slot 0 again: nothing is pending then)
    ws = _workspace(dev, stream, int(sz.ws_bwd_bytes), slot_base + slot)
    if _POISON:
        _poison(dX, dY, grads, ws)
    with _dev_guard(X):
        if hold_dy:
            lib.backward_hold_dy(d, _ptrs(params), prep.data_ptr(), X.data_ptr(), Y.data_ptr(), saved.data_ptr(), dOut.data_ptr(),
                                 dMap.data_ptr() if dMap is not None else None, dTmap.data_ptr() if dTmap is not None else None,
                                 dX.data_ptr(), grads.data_ptr(), ws.data_ptr(), stream, aux, skip_into_dx, defer, dx_event)
        else:
            lib.backward(d, _ptrs(params), prep.data_ptr(), X.data_ptr(), Y.data_ptr(), saved.data_ptr(), dOut.data_ptr(),
                         dMap.data_ptr() if dMap is not None else None, dTmap.data_ptr() if dTmap is not None else None,
                         dX.data_ptr(), dY.data_ptr(), grads.data_ptr(), ws.data_ptr(), stream, aux, skip_into_dx, defer)
        if defer:
            ev = torch.cuda.Event()
            ev.record(_AUX[key])                                       # behind everything this call put on its aux stream
            with _WS_LOCK:
                prev = _PENDING.get(key)
                # (NOT `grads`: autograd adopts the flat gradient only while nothing else references it -- a second reference makes
                #  AccumulateGrad CLONE it on the calling stream, i.e. read it before the aux stream has finished writing)
                _PENDING[key] = (ev, (saved, X, Y, dOut, dMap, dTmap, prep, ws))
            if prev is not None:
                torch.cuda.current_stream(dev).wait_event(prev[0])     # the call before this one: long done; its buffers go now
                del prev
            _queue_drain()
    if hold_dy:
        return dX, ws, grads
    if flat_out:
        return dX, dY, grads
    lay = grad_layout(lib, d)
    per_param: List[Optional[torch.Tensor]] = [grads[off:off + n] if off >= 0 else None for off, n in lay]
    return dX, dY, per_param


def raw_backward_dy(lib: Lib, d: AdapterDesc, params, prep, ws, Y, residual=None, wait_event=None):
    """The product raw_backward(hold_dy=True) held back, on the current stream: dY = residual + d adapter / dY, issued behind
    `wait_event` (raw hipEvent_t).  `ws` is the workspace that call returned; Y only gives the shape / dtype / device."""
    _mark_stream_use(residual, prep)
    dY = torch.empty_like(Y)
    if _POISON:
        _poison(dY)
    with _dev_guard(Y):
        lib.backward_only_dy(d, _ptrs(params), prep.data_ptr(), dY.data_ptr(), ws.data_ptr(), _stream_of(Y),
                             residual.data_ptr() if residual is not None else None, wait_event)
    return dY


def grad_layout(lib: Lib, d: AdapterDesc):
    """[(float offset, numel)] per C-ABI parameter slot (offset -1: no gradient); the layout of the flat gradient buffer,
    which is also the layout of a flattened parameter (VisualAdapter.flatten_parameters)."""
    sz = _sizes(lib, d)
    lay = _GRAD_LAYOUT.get(id(sz))
    if lay is None:
        lay = _GRAD_LAYOUT[id(sz)] = [(int(sz.grad_offset[i]), int(sz.grad_numel[i])) for i in range(P_COUNT)]
    return lay


_GRAD_LAYOUT: Dict[int, list] = {}


class _AdapterFn(torch.autograd.Function):
    """forward(X, Y, *params) -> (out, map[, tmap]); one library call each way."""

    @staticmethod
    def forward(ctx, lib, spec, training, prep, skip, res, X, Y, *params):
        plist = list(params)
        out, amap, tmap, saved, d = raw_forward(lib, spec, plist, prep, X, Y, training, X if skip else res)
        ctx.lib, ctx.spec, ctx.desc, ctx.prep = lib, spec, d, prep
        ctx.skip, ctx.has_res = bool(skip), res is not None
        ctx.saved_buf = saved
        ctx.save_for_backward(X, Y, *[p for p in plist if p is not None])
        ctx.present = [p is not None for p in plist]
        ctx.shapes = [tuple(p.shape) if p is not None else None for p in plist]
        ctx.set_materialize_grads(False)      # unused outputs (map of all but the last layer, tmap) arrive as None, not zeros
        if tmap is None:
            tmap = torch.empty(0, device=X.device)
        return out, amap, tmap

    @staticmethod
    def backward(ctx, dOut, dMap, dTmap):
        if ctx.saved_buf is None:
            raise RuntimeError("dg-sct_amd: backward through an adapter call twice is not supported "
                               "(the saved-activation buffer is consumed in place)")
        tensors = ctx.saved_tensors
        X, Y = tensors[0], tensors[1]
        it = iter(tensors[2:])
        plist = [next(it) if pres else None for pres in ctx.present]
        spec = ctx.spec
        if dOut is None:
            dOut = torch.zeros_like(X)
        dOut = dOut.contiguous()
        if dOut.dtype != X.dtype:
            dOut = dOut.to(X.dtype)
        dMap = dMap.contiguous().float() if dMap is not None else None
        dTm = dTmap.contiguous().float() if (spec.temporal and dTmap is not None and dTmap.numel()) else None
        dX, dY, grads = raw_backward(ctx.lib, spec, ctx.desc, plist, ctx.prep, X, Y, ctx.saved_buf, dOut, dMap, dTm,
                                     skip_into_dx=ctx.skip)
        ctx.saved_buf = None
        pg = []
        for i, g in enumerate(grads):
            if not ctx.present[i]:
                pg.append(None)
            elif g is None:
                pg.append(None)
            else:
                pg.append(g.view(ctx.shapes[i]))
        return (None, None, None, None, None, dOut if ctx.has_res else None, dX, dY, *pg)


class _AdapterFlatFn(torch.autograd.Function):
    """Same call, but every trainable tensor of the adapter lives in ONE flat fp32 parameter laid out like the
    library's gradient buffer: the backward returns that buffer as the parameter's gradient -- one tensor that owns its
    storage, so autograd adopts it without copying (1 AccumulateGrad instead of ~30 clones), the optimizer steps 48
    tensors instead of ~1900, and data-parallel all-reduce runs on it in place."""

    @staticmethod
    def forward(ctx, lib, spec, training, prep, plist, skip, res, X, Y, flat):
        out, amap, tmap, saved, d = raw_forward(lib, spec, plist, prep, X, Y, training, X if skip else res)
        ctx.lib, ctx.spec, ctx.desc, ctx.prep, ctx.plist = lib, spec, d, prep, plist
        ctx.skip, ctx.has_res = bool(skip), res is not None
        ctx.saved_buf = saved
        ctx.flat = flat
        _count_use(flat)
        ctx.save_for_backward(X, Y)
        ctx.set_materialize_grads(False)
        if tmap is None:
            tmap = torch.empty(0, device=X.device)
        return out, amap, tmap

    @staticmethod
    def backward(ctx, dOut, dMap, dTmap):
        if ctx.saved_buf is None:
            raise RuntimeError("dg-sct_amd: backward through an adapter call twice is not supported "
                               "(the saved-activation buffer is consumed in place)")
        X, Y = ctx.saved_tensors
        # The join of the weight-gradient stream is deferred only when autograd will ADOPT the returned buffer untouched: the
        # parameter has no gradient yet (else AccumulateGrad adds the new one into it on this stream, right now) and no tensor
        # hook wants to see it.  Gradient accumulation over several backward passes therefore joins from the second pass on.
        flat = ctx.flat
        can_defer = _may_adopt(flat)
        _use_done(flat)
        # (a DataParallel replica's flat tensor is NOT a leaf: its gradient is consumed by the broadcast's backward at once)
        ctx.flat = None
        spec = ctx.spec
        if dOut is None:
            dOut = torch.zeros_like(X)
        dOut = dOut.contiguous()
        if dOut.dtype != X.dtype:
            dOut = dOut.to(X.dtype)
        dMap = dMap.contiguous().float() if dMap is not None else None
        dTm = dTmap.contiguous().float() if (spec.temporal and dTmap is not None and dTmap.numel()) else None
        dX, dY, gflat = raw_backward(ctx.lib, spec, ctx.desc, ctx.plist, ctx.prep, X, Y, ctx.saved_buf, dOut, dMap, dTm,
                                     flat_out=True, skip_into_dx=ctx.skip, defer_join=can_defer)
        ctx.saved_buf = None
        return None, None, None, None, None, None, dOut if ctx.has_res else None, dX, dY, gflat


def _may_adopt(flat) -> bool:
    """True when autograd will ADOPT the gradient buffer returned for this flat parameter without reading it on the calling stream --
    the condition for leaving the weight-gradient (aux) stream un-joined.  It reads the buffer (clone / add / hook) when: the
    parameter already has a gradient (accumulation), a tensor hook or a post-accumulate-grad hook other than this package's reducer
    wants to see it (torch DDP's reducer hooks read .grad mid-backward; dp.GradAllReducer drains the aux streams first and marks its
    hooks), grad mode is on (create_graph=True: AccumulateGrad clones), or the same parameter is used by more than one call of the
    graph (the engine's input buffer SUMS the two buffers before accumulation: `_dgsct_uses`, counted in forward)."""
    if not (isinstance(flat, torch.Tensor) and flat.is_leaf and flat.grad is None):
        return False
    if getattr(flat, "_backward_hooks", None) or torch.is_grad_enabled():
        return False
    post = getattr(flat, "_post_accumulate_grad_hooks", None)
    if post and any(not getattr(h, "_dgsct_drains_aux", False) for h in post.values()):
        return False
    return getattr(flat, "_dgsct_uses", 1) <= 1


def _count_use(flat):
    """forward side of `_may_adopt`: how many calls of the graph being built read this flat parameter.  The count stands until the
    LAST of those calls has run its backward (every one of them must join); a forward whose graph is dropped without a backward
    leaves the count high, which only costs the deferral (safe side)."""
    if isinstance(flat, torch.Tensor) and flat.requires_grad and torch.is_grad_enabled():
        flat._dgsct_uses = getattr(flat, "_dgsct_uses", 0) + 1
        flat._dgsct_left = getattr(flat, "_dgsct_left", 0) + 1


def _use_done(flat):
    if isinstance(flat, torch.Tensor) and getattr(flat, "_dgsct_left", 0) > 0:
        flat._dgsct_left -= 1
        if flat._dgsct_left == 0:
            flat._dgsct_uses = 0


PAIR_BACKWARD = os.environ.get("DGSCT_NO_PAIR", "0") != "1"
_PAIR_EVENTS: Dict[int, list] = {}
_PAIR_RING = 16


def _pair_events(dev: torch.device):
    """two recorded-once events of a small per-device ring (a torch event has no handle before its first record); the library
    re-records them in the middle of the two calls of a pair"""
    ring = _PAIR_EVENTS.get(dev.index)
    if ring is None:
        ring = _PAIR_EVENTS[dev.index] = [[], 0]
        cur = torch.cuda.current_stream(dev)
        for _ in range(_PAIR_RING):
            e = torch.cuda.Event()
            e.record(cur)
            ring[0].append(e)
    i = ring[1]
    ring[1] = (i + 2) % _PAIR_RING
    return ring[0][i], ring[0][i + 1]


def _cotangent(dOut, X):
    if dOut is None:
        return torch.zeros_like(X)
    dOut = dOut.contiguous()
    return dOut if dOut.dtype == X.dtype else dOut.to(X.dtype)


class _PairFlatFn(torch.autograd.Function):
    """The audio and the visual adapter of one position (net_trans.py:891-906) as ONE autograd node:
        f_a' = f_a + audio_adapter(f_a, f_v),   f_v' = f_v + vis_adapter(f_v, f_a)
    so that  d f_a = dX(audio) + dY(visual)  and  d f_v = dX(visual) + dY(audio)  are formed by the products that write dY (their
    epilogues read the other call's dX: include/dgsct.h, dgsct_adapter_backward_ex2) instead of by autograd's accumulation -- one
    pass over [BT][N][C] per adapter call less, on the critical path between two positions.  `side`: the second adapter stream
    (None: both calls on the current stream, in order -- the host-emulated library of the CPU tests)."""

    @staticmethod
    def forward(ctx, lib, side, call_a, call_v, f_a, f_v, flat_a, flat_v):
        # call_x = (spec, training, prep, plist) of VisualAdapter._token_call
        def one(call, X, Y):
            spec, training, prep, plist = call
            out, amap, _, saved, d = raw_forward(lib, spec, plist, prep, X, Y, training, X)
            return out, amap, saved, d
        if side is not None:
            main = torch.cuda.current_stream(f_a.device)
            side.wait_stream(main)
            with torch.cuda.stream(side):
                oa, ma, sa, da = one(call_a, f_a, f_v)
            ov, mv, sv, dv = one(call_v, f_v, f_a)
            main.wait_stream(side)
            oa.record_stream(main)
            ma.record_stream(main)
        else:
            oa, ma, sa, da = one(call_a, f_a, f_v)
            ov, mv, sv, dv = one(call_v, f_v, f_a)
        ctx.lib, ctx.side = lib, side
        ctx.calls = (call_a, call_v)
        ctx.descs = (da, dv)
        ctx.saved_bufs = (sa, sv)
        ctx.flats = (flat_a, flat_v)
        _count_use(flat_a)
        _count_use(flat_v)
        ctx.save_for_backward(f_a, f_v)
        ctx.set_materialize_grads(False)
        return oa, ma, ov, mv

    @staticmethod
    def backward(ctx, dOa, dMa, dOv, dMv):
        if ctx.saved_bufs is None:
            raise RuntimeError("dg-sct_amd: backward through an adapter call twice is not supported "
                               "(the saved-activation buffer is consumed in place)")
        f_a, f_v = ctx.saved_tensors
        lib, side = ctx.lib, ctx.side
        (spec_a, _, prep_a, pl_a), (spec_v, _, prep_v, pl_v) = ctx.calls
        d_a, d_v = ctx.descs
        s_a, s_v = ctx.saved_bufs
        defer = [_may_adopt(fl) for fl in ctx.flats]                    # (as in _AdapterFlatFn.backward)
        for fl in ctx.flats:
            _use_done(fl)
        ctx.flats = ctx.saved_bufs = None
        dOa, dOv = _cotangent(dOa, f_a), _cotangent(dOv, f_v)
        dMa = dMa.contiguous().float() if dMa is not None else None
        dMv = dMv.contiguous().float() if dMv is not None else None

        def main_part(spec, d, pl, prep, X, Y, saved, dO, dM, can_defer, ev, slot_base=0):
            return raw_backward(lib, spec, d, pl, prep, X, Y, saved, dO, dM, None, flat_out=True, skip_into_dx=True,
                                defer_join=can_defer, hold_dy=True, dx_event=ev, slot_base=slot_base)

        if side is not None:
            dev = f_a.device
            ev_a, ev_v = _pair_events(dev)
            main = torch.cuda.current_stream(dev)
            side.wait_stream(main)
            with torch.cuda.stream(side):
                dXa, ws_a, g_a = main_part(spec_a, d_a, pl_a, prep_a, f_a, f_v, s_a, dOa, dMa, defer[0], ev_a.cuda_event)
            dXv, ws_v, g_v = main_part(spec_v, d_v, pl_v, prep_v, f_v, f_a, s_v, dOv, dMv, defer[1], ev_v.cuda_event)
            with torch.cuda.stream(side):                               # d f_v = dX(visual) + dY(audio call)
                df_v = raw_backward_dy(lib, d_a, pl_a, prep_a, ws_a, f_v, dXv, ev_v.cuda_event)
            df_a = raw_backward_dy(lib, d_v, pl_v, prep_v, ws_v, f_a, dXa, ev_a.cuda_event)     # d f_a = dX(audio) + dY(visual call)
            main.wait_stream(side)
            df_v.record_stream(main)
        else:
            dXa, ws_a, g_a = main_part(spec_a, d_a, pl_a, prep_a, f_a, f_v, s_a, dOa, dMa, defer[0], None)
            # (one stream = one workspace per slot: the second call must not overwrite what the first one's dY product still reads)
            dXv, ws_v, g_v = main_part(spec_v, d_v, pl_v, prep_v, f_v, f_a, s_v, dOv, dMv, defer[1], None, slot_base=2)
            df_v = raw_backward_dy(lib, d_a, pl_a, prep_a, ws_a, f_v, dXv)
            df_a = raw_backward_dy(lib, d_v, pl_v, prep_v, ws_v, f_a, dXa)
        return None, None, None, None, df_a, df_v, g_a, g_v


def pair_apply(lib: Lib, side, call_a, call_v, f_a: torch.Tensor, f_v: torch.Tensor, flat_a: torch.Tensor, flat_v: torch.Tensor):
    """(f_a + audio_adapter(f_a, f_v), map_a, f_v + vis_adapter(f_v, f_a), map_v); token-major contiguous maps of the adapters'
    compute dtype, both adapters with flat parameters and without a temporal gate (AdapterStack checks)."""
    return _PairFlatFn.apply(lib, side, call_a, call_v, f_a, f_v, flat_a, flat_v)


def adapter_apply(lib: Lib, spec: AdapterSpec, training: bool, prep: torch.Tensor, X: torch.Tensor, Y: torch.Tensor,
                  params: List[Optional[torch.Tensor]], flat: Optional[torch.Tensor] = None,
                  residual: Optional[torch.Tensor] = None, skip: bool = False):
    """residual: out = residual + adapter(X, Y) (any tensor of X's shape; its gradient is dOut).
    skip: out = X + adapter(X, Y) with the matching `dX += dOut` fused into backward."""
    if skip and residual is not None:
        raise RuntimeError("dg-sct_amd: pass either residual= or skip=True, not both")
    if flat is not None:
        out, amap, tmap = _AdapterFlatFn.apply(lib, spec, training, prep, params, skip, residual, X, Y, flat)
    else:
        out, amap, tmap = _AdapterFn.apply(lib, spec, training, prep, skip, residual, X, Y, *params)
    return out, amap, (tmap if spec.temporal else None)


# ---- spatial-map pooling of the task heads ------------------------------------------------------
class _MapPoolFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, lib, f, amap):
        BT, N, C_ = f.shape
        pooled = torch.empty(BT, C_, dtype=torch.float32, device=f.device)
        with _dev_guard(f):
            lib.map_pool_forward(0 if f.dtype == torch.float32 else 1, BT, N, C_, f.data_ptr(), amap.data_ptr(),
                                 pooled.data_ptr(), _stream_of(f))
        ctx.lib = lib
        ctx.save_for_backward(f, amap)
        return pooled

    @staticmethod
    def backward(ctx, dpooled):
        f, amap = ctx.saved_tensors
        BT, N, C_ = f.shape
        dpooled = dpooled.contiguous().float()
        _mark_stream_use(f, amap, dpooled)
        df = torch.empty_like(f) if ctx.needs_input_grad[1] else None
        dmap = torch.empty_like(amap) if ctx.needs_input_grad[2] else None
        with _dev_guard(f):
            ctx.lib.map_pool_backward(0 if f.dtype == torch.float32 else 1, BT, N, C_, f.data_ptr(), amap.data_ptr(),
                                      dpooled.data_ptr(), df.data_ptr() if df is not None else None,
                                      dmap.data_ptr() if dmap is not None else None, _stream_of(f))
        return None, df, dmap


def map_pool(f: torch.Tensor, spatial_att_maps: torch.Tensor, lib: Optional[Lib] = None) -> torch.Tensor:
    """Drop-in for `torch.bmm(spatial_att_maps, f)` at the end of the reference's layer loop
    (DG-SCT/AVE/nets/net_trans.py:922-924): f [BT,N,C] (fp32 | bf16), spatial_att_maps [BT,1,N] (the second output of the
    last p2 adapter) -> [BT,1,C] in f's dtype.  One HIP reduction forward, two kernels backward (dgsct_map_pool_*)."""
    if not f.is_cuda and lib is None:                     # (CPU tensors with lib=: the host emulation of the tests, nothing else)
        raise RuntimeError("dg-sct_amd: map_pool needs CUDA/HIP tensors (no CPU fallback)")
    BT, N, C_ = f.shape
    if spatial_att_maps.shape not in ((BT, 1, N), (BT, N)):
        raise RuntimeError(f"dg-sct_amd: spatial_att_maps must be [BT,1,N] = [{BT},1,{N}], got {tuple(spatial_att_maps.shape)}")
    if f.dtype not in (torch.float32, torch.bfloat16):
        raise RuntimeError("dg-sct_amd: map_pool supports float32 and bfloat16 maps")
    from ._lib import default_lib
    pooled = _MapPoolFn.apply(lib or default_lib(), f.contiguous(), spatial_att_maps.reshape(BT, N).contiguous().float())
    return pooled.to(f.dtype).unsqueeze(1)


# ---- fused window attention of the frozen backbone blocks -------------------------------------------------------
class _WindowAttnFn(torch.autograd.Function):
    """softmax(scale q k^T + bm) v per (frame, window, head) on the qkv projection of the UN-partitioned map; window partition and cyclic
    shift are address arithmetic inside the kernel (csrc/wattn.hip).  When autograd asks for the gradient of bm or scale (trainable blocks)
    the backward is the table variant (dgsct_window_attn_backward_tables: the same dqkv, plus dbm / dscale); otherwise the frozen one."""

    @staticmethod
    def forward(ctx, lib, qkv, bm, scale, H, W, ws, shift, heads, cosine=False):
        B, L, C3 = qkv.shape
        hd = C3 // (3 * heads)
        nW = (H // ws) * (W // ws)
        geom = (B, H, W, ws, shift, heads, hd, int(bm.shape[0]))
        out = torch.empty(B, L, heads * hd, dtype=qkv.dtype, device=qkv.device)
        lse = torch.empty(B, nW, heads, ws * ws, dtype=torch.float32, device=qkv.device)
        _mark_stream_use(qkv, bm, scale)
        with _dev_guard(qkv):
            lib.window_attn_forward(geom, qkv.data_ptr(), bm.data_ptr(), scale.data_ptr(), out.data_ptr(), lse.data_ptr(), _stream_of(qkv),
                                    1 if cosine else 0)
        ctx.lib, ctx.geom, ctx.flags = lib, geom, 1 if cosine else 0
        ctx.save_for_backward(qkv, bm, scale, out, lse)
        return out

    @staticmethod
    def backward(ctx, dout):
        qkv, bm, scale, out, lse = ctx.saved_tensors
        dout = dout.contiguous()
        if dout.dtype != qkv.dtype:
            dout = dout.to(qkv.dtype)
        dqkv = torch.empty_like(qkv)
        want_bm, want_scale = ctx.needs_input_grad[2], ctx.needs_input_grad[3]
        if (want_bm or want_scale) and not ctx.lib.has_window_attn_tables:
            _warn_no_tables(ctx.lib)
            want_bm = want_scale = False
        _mark_stream_use(qkv, bm, scale, out, lse, dout)
        dbm = dscale = None
        with _dev_guard(qkv):
            if want_bm or want_scale:
                dbm = torch.empty_like(bm) if want_bm else None                      # (zeroed by the call)
                dscale = torch.empty_like(scale) if want_scale else None
                ctx.lib.window_attn_backward_tables(ctx.geom, qkv.data_ptr(), bm.data_ptr(), scale.data_ptr(), out.data_ptr(),
                                                    lse.data_ptr(), dout.data_ptr(), dqkv.data_ptr(),
                                                    dbm.data_ptr() if dbm is not None else None,
                                                    dscale.data_ptr() if dscale is not None else None, _stream_of(qkv), ctx.flags)
            else:
                ctx.lib.window_attn_backward(ctx.geom, qkv.data_ptr(), bm.data_ptr(), scale.data_ptr(), out.data_ptr(), lse.data_ptr(),
                                             dout.data_ptr(), dqkv.data_ptr(), _stream_of(qkv), ctx.flags)
        return None, dqkv, dbm, dscale, None, None, None, None, None, None


_WARNED_NO_TABLES = set()


def _warn_no_tables(lib):
    """a library without dgsct_window_attn_backward_tables (the host emulation): the tables get no gradient, as before it existed"""
    if lib.path not in _WARNED_NO_TABLES:
        _WARNED_NO_TABLES.add(lib.path)
        warnings.warn(f"dg-sct_amd: {lib.path} has no dgsct_window_attn_backward_tables: the window-attention bias / scale tables get no "
                      f"gradient through it", RuntimeWarning, stacklevel=3)


def window_attention_supported(qkv: torch.Tensor, ws: int, heads: int) -> bool:
    """what csrc/wattn.hip takes: bf16 (the host emulation of the CPU tests: bf16 too), head width 8 / 16 / 24 / 32, windows of <= 144 tokens"""
    if qkv.dtype != torch.bfloat16 or qkv.dim() != 3 or qkv.shape[-1] % (3 * heads):
        return False
    hd = qkv.shape[-1] // (3 * heads)
    return hd in (8, 16, 24, 32) and ws * ws <= 144 and (ws * ws) % 4 == 0


def window_attention(qkv: torch.Tensor, bm: torch.Tensor, scale: torch.Tensor, H: int, W: int, ws: int, shift: int, heads: int,
                     lib: Optional[Lib] = None, cosine: bool = False) -> torch.Tensor:
    """qkv [B, H*W, 3*heads*hd] bf16 (token-major map, NOT partitioned / rolled), bm [1 | nW, heads, n, n] fp32, scale [heads] fp32
    -> O [B, H*W, heads*hd] at the map positions (what window_reverse + roll-back of the reference block produce).
    cosine: q and k are L2-normalised per head inside the kernel (Swin-V2), qkv is the raw projection."""
    if not window_attention_supported(qkv, ws, heads):
        raise RuntimeError("dg-sct_amd: window_attention takes bf16 qkv with head width 8/16/24/32 and windows of <= 144 tokens")
    nW = (H // ws) * (W // ws) if ws > 0 else 0
    if qkv.shape[1] != H * W:
        raise RuntimeError(f"dg-sct_amd: window_attention: qkv holds {qkv.shape[1]} tokens per frame, the map {H} x {W} = {H * W}")
    if (bm.dtype != torch.float32 or scale.dtype != torch.float32 or bm.dim() != 4 or bm.shape[1:] != (heads, ws * ws, ws * ws)
            or bm.shape[0] not in (1, nW) or tuple(scale.shape) != (heads,)):
        raise RuntimeError(f"dg-sct_amd: window_attention: bm must be fp32 [1 | {nW}, {heads}, {ws * ws}, {ws * ws}] and scale fp32 [{heads}] "
                           f"(got {tuple(bm.shape)} {bm.dtype}, {tuple(scale.shape)} {scale.dtype})")
    from ._lib import default_lib
    return _WindowAttnFn.apply(lib or default_lib(), qkv.contiguous(), bm.contiguous(), scale.contiguous(), H, W, ws, shift, heads, cosine)


# ---- LayerNorm (+ residual) of the frozen backbone blocks ----------------------------------------------------
_LN_SCRATCH: Dict[Tuple, torch.Tensor] = {}


class _LayerNormFn(torch.autograd.Function):
    """out = LN(x; w, b) (+ residual) on the adapter tail's row kernels (dgsct_layer_norm_*): one pass forward (row statistics kept), one
    pass backward; w / b fp32.  Gradients for w / b only when they ask for one (the blocks are frozen: main_trans.py:211-256)."""

    @staticmethod
    def forward(ctx, lib, x, w, b, eps, residual):
        C_ = x.shape[-1]
        rows = x.numel() // C_
        out = torch.empty_like(x)
        mu = torch.empty(rows, dtype=torch.float32, device=x.device)
        rstd = torch.empty(rows, dtype=torch.float32, device=x.device)
        _mark_stream_use(x, w, b, residual)
        with _dev_guard(x):
            lib.layer_norm_forward(0 if x.dtype == torch.float32 else 1, rows, C_, x.data_ptr(), w.data_ptr(), b.data_ptr(), float(eps),
                                   residual.data_ptr() if residual is not None else None, out.data_ptr(), mu.data_ptr(), rstd.data_ptr(),
                                   _stream_of(x))
        ctx.lib, ctx.eps, ctx.has_res = lib, float(eps), residual is not None
        ctx.save_for_backward(x, w, b, mu, rstd)
        return out

    @staticmethod
    def backward(ctx, dout):
        x, w, b, mu, rstd = ctx.saved_tensors
        C_ = x.shape[-1]
        rows = x.numel() // C_
        dout = dout.contiguous()
        if dout.dtype != x.dtype:
            dout = dout.to(x.dtype)
        dx = torch.empty_like(x)
        dwb = torch.zeros(2, C_, dtype=torch.float32, device=x.device)
        key = (id(ctx.lib), x.device, _stream_of(x), C_)
        scr = _LN_SCRATCH.get(key)
        if scr is None:
            scr = _LN_SCRATCH[key] = torch.empty(int(ctx.lib.c.dgsct_layer_norm_scratch_floats(C_)), dtype=torch.float32, device=x.device)
        _mark_stream_use(x, w, b, mu, rstd, dout)
        with _dev_guard(x):
            ctx.lib.layer_norm_backward(0 if x.dtype == torch.float32 else 1, rows, C_, dout.data_ptr(), x.data_ptr(), w.data_ptr(),
                                        b.data_ptr(), mu.data_ptr(), rstd.data_ptr(), ctx.eps, dx.data_ptr(), dwb[0].data_ptr(),
                                        dwb[1].data_ptr(), scr.data_ptr(), _stream_of(x))
        return (None, dx, dwb[0] if ctx.needs_input_grad[2] else None, dwb[1] if ctx.needs_input_grad[3] else None, None,
                dout if ctx.has_res else None)


def layer_norm_supported(x: torch.Tensor) -> bool:
    C_ = x.shape[-1]
    return x.dtype in (torch.float32, torch.bfloat16) and C_ <= 1536 and C_ % (8 if x.dtype == torch.bfloat16 else 4) == 0 and x.numel() > 0


def layer_norm(x: torch.Tensor, weight: torch.Tensor, bias: torch.Tensor, eps: float = 1e-5, residual: Optional[torch.Tensor] = None,
               lib: Optional[Lib] = None) -> torch.Tensor:
    """`F.layer_norm(x, (C,), weight, bias, eps)` (+ residual) over the last axis of x [..., C] (fp32 | bf16); weight / bias fp32 [C]."""
    if not layer_norm_supported(x):
        raise RuntimeError("dg-sct_amd: layer_norm takes fp32 / bf16 rows of <= 1536 channels (a multiple of 4; bf16: 8)")
    if weight.dtype != torch.float32 or bias.dtype != torch.float32:
        raise RuntimeError("dg-sct_amd: layer_norm: weight / bias must be fp32")
    from ._lib import default_lib
    if residual is not None:
        residual = residual.contiguous()
        if residual.shape != x.shape or residual.dtype != x.dtype:
            raise RuntimeError("dg-sct_amd: layer_norm: residual must match x")
    return _LayerNormFn.apply(lib or default_lib(), x.contiguous(), weight.contiguous(), bias.contiguous(), eps, residual)


# ---- audio / image front ends: waveform -> log-mel -> patch tokens (csrc/frontend.hip) ---------------------------
N_FFT, HOP, N_MELS, MAX_FRAMES = 1024, 320, 64, 1024


def _no_grad_inputs(who: str, *tensors):
    """these calls are forward-only (inputs are data, parameters frozen; `patch_embed_train` is the one with parameter gradients):
    refuse to cut a graph silently"""
    for t in tensors:
        if t is not None and t.requires_grad:
            raise RuntimeError(f"dg-sct_amd: {who} is forward-only: an input requires grad (detach it; the front end's parameters are frozen)")


def _dev_f32(who: str, name: str, t: torch.Tensor, shape, device) -> torch.Tensor:
    if not isinstance(t, torch.Tensor) or t.dtype != torch.float32 or tuple(t.shape) != tuple(shape) or t.device != device or not t.is_contiguous():
        got = f"{tuple(t.shape)} {t.dtype} on {t.device}" if isinstance(t, torch.Tensor) else type(t).__name__
        raise RuntimeError(f"dg-sct_amd: {who}: {name} must be a contiguous fp32 tensor {tuple(shape)} on {device} (got {got})")
    return t


def mel_ranges(melW: torch.Tensor) -> torch.Tensor:
    """int32 [n_mels, 2]: for every column of melW [bins, n_mels] the half-open row range outside of which it is zero (an all-zero
    column: [0, 0)).  Summing a column's product over its range equals the dense product.  Setup-time helper (reads melW back)."""
    nz = (melW.detach() != 0).cpu()
    rows = torch.arange(nz.shape[0]).unsqueeze(1)
    lo = torch.where(nz, rows, nz.shape[0]).amin(0)
    hi = torch.where(nz, rows + 1, 0).amax(0)
    lo = torch.minimum(lo, hi)
    return torch.stack([lo, hi], 1).to(torch.int32).contiguous().to(melW.device)


def logmel_frames(L: int) -> int:
    return L // HOP + 1


def logmel(waveform: torch.Tensor, melW: torch.Tensor, want_stats: bool = False, lib: Optional[Lib] = None,
           ranges: Optional[torch.Tensor] = None):
    """waveform [B, L] fp32 -> log-mel [B, T, 64] fp32, T = L // 320 + 1 (reflect-padded 1024-point Hann STFT, power, melW [513, 64],
    10 log10(max(., 1e-10))) in one launch; the power spectrogram is never stored.  want_stats: also returns (mean [64], biased variance
    [64]) of the log-mel over all B T frames per mel bin (one more tiny launch).  ranges: `mel_ranges(melW)` computed once by the caller
    (None: derived here, which reads melW back to the host)."""
    who = "logmel"
    if not isinstance(waveform, torch.Tensor) or not waveform.is_cuda:
        raise RuntimeError("dg-sct_amd: logmel needs CUDA/HIP tensors (no CPU fallback; HTSATFrontEnd(fused=False) is the ATen formulation)")
    if waveform.dim() != 2 or waveform.dtype != torch.float32 or not waveform.is_contiguous():
        raise RuntimeError(f"dg-sct_amd: logmel: waveform must be a contiguous fp32 [B, L] tensor (got {tuple(waveform.shape)} {waveform.dtype})")
    B, L = waveform.shape
    if B < 1 or L <= N_FFT // 2:
        raise RuntimeError(f"dg-sct_amd: logmel: need B >= 1 and L > {N_FFT // 2} samples (reflect padding), got [{B}, {L}]")
    T = logmel_frames(L)
    if T > MAX_FRAMES:
        raise RuntimeError(f"dg-sct_amd: logmel: {L} samples give {T} frames, more than the {MAX_FRAMES} the HTS-AT image holds")
    dev = waveform.device
    _dev_f32(who, "melW", melW, (N_FFT // 2 + 1, N_MELS), dev)
    _no_grad_inputs(who, waveform, melW)
    if ranges is None:
        ranges = mel_ranges(melW)
    if ranges.dtype != torch.int32 or tuple(ranges.shape) != (N_MELS, 2) or ranges.device != dev or not ranges.is_contiguous():
        raise RuntimeError(f"dg-sct_amd: logmel: ranges must be a contiguous int32 [{N_MELS}, 2] tensor on {dev}")
    lib = lib or _lib.default_lib()
    out = torch.empty(B, T, N_MELS, dtype=torch.float32, device=dev)
    stats = scratch = None
    if want_stats:
        stats = torch.empty(2, N_MELS, dtype=torch.float32, device=dev)
        scratch = torch.empty(lib.logmel_scratch_floats(B, L), dtype=torch.float32, device=dev)
    _mark_stream_use(waveform, melW, ranges)
    with _dev_guard(waveform):
        lib.logmel_forward(B, L, waveform.data_ptr(), melW.data_ptr(), ranges.data_ptr(), out.data_ptr(),
                           stats.data_ptr() if want_stats else None, scratch.data_ptr() if want_stats else None, _stream_of(waveform))
    return (out, stats[0], stats[1]) if want_stats else out


def check_stripes(stripes: torch.Tensor, B: int, T: int, who: str = "check_stripes") -> torch.Tensor:
    """a SpecAugment stripe table as the kernels take it: int32 [B, 4, 2] of half-open (begin, end), rows 0 and 1 inside the frame axis
    [0, T], rows 2 and 3 inside the mel axis [0, 64]; begin >= end is an empty stripe.  Returns it contiguous; raises otherwise.  The C calls
    do not read the table back (include/dgsct.h): this is where a stripe outside its axis is refused, on the host copy when there is one (a
    table that already lives on the device is read back once)."""
    if not isinstance(stripes, torch.Tensor) or stripes.dtype != torch.int32 or tuple(stripes.shape) != (B, 4, 2):
        got = f"{tuple(stripes.shape)} {stripes.dtype}" if isinstance(stripes, torch.Tensor) else type(stripes).__name__
        raise RuntimeError(f"dg-sct_amd: {who}: stripes must be an int32 tensor [{B}, 4, 2] of (begin, end) (got {got})")
    host = stripes.detach().cpu()
    for rows, width, axis in ((host[:, :2], T, "frame"), (host[:, 2:], N_MELS, "mel")):
        if int(rows.min()) < 0 or int(rows.max()) > width:
            raise RuntimeError(f"dg-sct_amd: {who}: a {axis} stripe lies outside [0, {width}] (stripes rows 0, 1: frames of the un-stretched "
                               f"log-mel; rows 2, 3: mel bins)")
    return stripes.contiguous()


def _aug_operands(who: str, stripes, mixup_lambda, B: int, T: int, dev):
    """(stripes int32 [B, 4, 2], lam fp32 [B]) on `dev`, either may be None; checked on the host before the upload"""
    if stripes is not None:
        stripes = check_stripes(stripes, B, T, who).to(dev)
    if mixup_lambda is not None:
        if not isinstance(mixup_lambda, torch.Tensor) or mixup_lambda.dtype != torch.float32 or tuple(mixup_lambda.shape) != (B,):
            got = f"{tuple(mixup_lambda.shape)} {mixup_lambda.dtype}" if isinstance(mixup_lambda, torch.Tensor) else type(mixup_lambda).__name__
            raise RuntimeError(f"dg-sct_amd: {who}: mixup_lambda must be an fp32 tensor [{B}], one lambda per sample (got {got})")
        if mixup_lambda.requires_grad:
            raise RuntimeError(f"dg-sct_amd: {who}: mixup_lambda is data and gets no gradient (detach it)")
        mixup_lambda = mixup_lambda.to(dev).contiguous()
    return stripes, mixup_lambda


def _need_aug(who: str, lib: Lib):
    if not lib.has_patch_embed_aug():
        raise RuntimeError(f"dg-sct_amd: {who}: {lib.path} does not export dgsct_patch_embed_forward_aug / dgsct_patch_embed_backward_params_aug "
                           f"(a library without the in-kernel augmentation; fused=False, the ATen formulation, augments without it)")


def patch_embed(x: torch.Tensor, weight: torch.Tensor, bias: torch.Tensor, ln_weight: torch.Tensor, ln_bias: torch.Tensor,
                eps: float = 1e-5, out_dtype: Optional[torch.dtype] = None, bn_scale: Optional[torch.Tensor] = None,
                bn_shift: Optional[torch.Tensor] = None, lib: Optional[Lib] = None, stripes: Optional[torch.Tensor] = None,
                mixup_lambda: Optional[torch.Tensor] = None) -> torch.Tensor:
    """4 x 4 / stride-4 patch convolution + bias + LayerNorm in one launch -> tokens [B, (H/4) (W/4), C] (fp32 | bf16).
    Image mode (bn_scale is None): x [B, in_chans, H, W] fp32 | bf16, in_chans 1 or 3.  Audio mode (bn_scale / bn_shift [64] given): x is the
    log-mel [B, T, 64] fp32; `x * bn_scale[f] + bn_shift[f]`, the bicubic stretch of the T frames to 1024 and the fold into the 256 x 256
    HTS-AT image are part of the kernel's loads.  weight [C, in_chans, 4, 4], bias / ln_weight / ln_bias [C] fp32; C % 32 == 0, C <= 192.
    Audio mode only: stripes (int32 [B, 4, 2], `check_stripes`) zeroes the `bn0` output inside two time and two mel stripes per sample and
    mixup_lambda (fp32 [B]) then mixes sample b with sample B-1-b, both before the stretch and both inside the same launch
    (dgsct_patch_embed_forward_aug); with both None the call is dgsct_patch_embed_forward as ever."""
    who = "patch_embed"
    if not isinstance(x, torch.Tensor) or not x.is_cuda:
        raise RuntimeError("dg-sct_amd: patch_embed needs CUDA/HIP tensors (no CPU fallback; PatchEmbed(fused=False) is the ATen formulation)")
    audio = bn_scale is not None or bn_shift is not None
    dev = x.device
    if not x.is_contiguous():
        raise RuntimeError("dg-sct_amd: patch_embed: x must be contiguous")
    if audio:
        if x.dim() != 3 or x.shape[-1] != N_MELS or x.dtype != torch.float32 or not 2 <= x.shape[1] <= MAX_FRAMES:
            raise RuntimeError(f"dg-sct_amd: patch_embed (audio): x must be an fp32 log-mel [B, T <= {MAX_FRAMES}, {N_MELS}] (got {tuple(x.shape)} {x.dtype})")
        B, T, in_chans, H, W = x.shape[0], x.shape[1], 1, 256, 256
        if bn_scale is None or bn_shift is None:
            raise RuntimeError("dg-sct_amd: patch_embed (audio): bn_scale and bn_shift go together")
        _dev_f32(who, "bn_scale", bn_scale, (N_MELS,), dev)
        _dev_f32(who, "bn_shift", bn_shift, (N_MELS,), dev)
        stripes, mixup_lambda = _aug_operands(who, stripes, mixup_lambda, B, T, dev)
    else:
        if stripes is not None or mixup_lambda is not None:
            raise RuntimeError("dg-sct_amd: patch_embed: stripes / mixup_lambda belong to audio mode (image-side augmentation is not built)")
        if x.dim() != 4 or x.dtype not in (torch.float32, torch.bfloat16) or x.shape[1] not in (1, 3) or x.shape[2] % 4 or x.shape[3] % 4 \
                or min(x.shape[2:]) < 4:
            raise RuntimeError(f"dg-sct_amd: patch_embed: x must be fp32 / bf16 [B, 1 | 3, H, W] with H, W multiples of 4 (got {tuple(x.shape)} {x.dtype})")
        B, in_chans, H, W = x.shape
        T = 0
    if B < 1:
        raise RuntimeError("dg-sct_amd: patch_embed: empty batch")
    C_ = weight.shape[0] if isinstance(weight, torch.Tensor) and weight.dim() == 4 else 0
    if C_ < 32 or C_ > 192 or C_ % 32:
        raise RuntimeError(f"dg-sct_amd: patch_embed: the embedding width must be a multiple of 32 up to 192 (weight {tuple(getattr(weight, 'shape', ()))})")
    _dev_f32(who, "weight", weight, (C_, in_chans, 4, 4), dev)
    for n, t in (("bias", bias), ("ln_weight", ln_weight), ("ln_bias", ln_bias)):
        _dev_f32(who, n, t, (C_,), dev)
    out_dtype = out_dtype or torch.float32
    if out_dtype not in (torch.float32, torch.bfloat16):
        raise RuntimeError("dg-sct_amd: patch_embed: out_dtype must be float32 or bfloat16")
    _no_grad_inputs(who, x, weight, bias, ln_weight, ln_bias, bn_scale, bn_shift)
    lib = lib or _lib.default_lib()
    aug = stripes is not None or mixup_lambda is not None
    if aug:
        _need_aug(who, lib)
    out = torch.empty(B, (H // 4) * (W // 4), C_, dtype=out_dtype, device=dev)
    code = lambda dt: _lib.F32 if dt == torch.float32 else _lib.BF16
    _mark_stream_use(x, weight, bias, ln_weight, ln_bias, bn_scale, bn_shift, stripes, mixup_lambda)
    if aug:
        ptr = lambda t: t.data_ptr() if t is not None else None
        with _dev_guard(x):
            lib.patch_embed_forward_aug(code(out_dtype), B, T, C_, x.data_ptr(), bn_scale.data_ptr(), bn_shift.data_ptr(), ptr(stripes),
                                        ptr(mixup_lambda), weight.data_ptr(), bias.data_ptr(), ln_weight.data_ptr(), ln_bias.data_ptr(),
                                        float(eps), out.data_ptr(), _stream_of(x))
        return out
    with _dev_guard(x):
        lib.patch_embed_forward(_lib.PATCH_AUDIO if audio else _lib.PATCH_IMAGE, code(x.dtype), code(out_dtype), B, in_chans, H, W, T, C_,
                                x.data_ptr(), bn_scale.data_ptr() if audio else None, bn_shift.data_ptr() if audio else None,
                                weight.data_ptr(), bias.data_ptr(), ln_weight.data_ptr(), ln_bias.data_ptr(), float(eps), out.data_ptr(),
                                _stream_of(x))
    return out


class _PatchEmbedTrainFn(torch.autograd.Function):
    """forward: `patch_embed` (the same launch as the frozen path); backward: dgsct_patch_embed_backward_params, which recomputes the
    convolution and the LayerNorm statistics from x -- nothing token-sized is saved"""

    @staticmethod
    def forward(ctx, lib, x, weight, bias, ln_weight, ln_bias, bn_weight, bn_bias, mean, var, eps, bn_eps, out_dtype, stripes=None, lam=None):
        audio = bn_weight is not None
        scale = shift = rstd = None
        if audio:
            rstd = torch.rsqrt(var + bn_eps)
            scale = bn_weight.detach() * rstd                          # (the arithmetic of HTSATFrontEnd._bn_affine: the tokens equal the frozen path's)
            shift = (bn_bias.detach() - mean * scale).contiguous()
            scale = scale.contiguous()
        w, b, lw, lb = weight.detach(), bias.detach(), ln_weight.detach(), ln_bias.detach()
        if audio:
            stripes, lam = _aug_operands("patch_embed_train", stripes, lam, x.shape[0], x.shape[1], x.device)    # (the two small tensors the backward needs again)
        out = patch_embed(x, w, b, lw, lb, eps, out_dtype, scale, shift, lib=lib, stripes=stripes, mixup_lambda=lam)
        ctx.lib, ctx.eps, ctx.audio = lib, float(eps), audio
        ctx.aug = (stripes is not None, lam is not None)
        ctx.save_for_backward(x, w, b, lw, lb, *((scale, shift, mean.contiguous(), rstd) if audio else ()), *(t for t in (stripes, lam) if t is not None))
        return out

    @staticmethod
    def backward(ctx, dout):
        x, w, b, lw, lb = ctx.saved_tensors[:5]
        scale, shift, mean, rstd = ctx.saved_tensors[5:9] if ctx.audio else (None,) * 4
        rest = list(ctx.saved_tensors[9:])
        stripes = rest.pop(0) if ctx.aug[0] else None
        lam = rest.pop(0) if ctx.aug[1] else None
        C_ = w.shape[0]
        if ctx.audio:
            B, T, in_chans, H, W = x.shape[0], x.shape[1], 1, 256, 256
        else:
            (B, in_chans, H, W), T = x.shape, 0
        if dout.dtype not in (torch.float32, torch.bfloat16):
            dout = dout.float()
        dout = dout.contiguous()
        f32 = dict(dtype=torch.float32, device=x.device)
        dw, db, dlw, dlb = torch.empty_like(w), torch.empty(C_, **f32), torch.empty(C_, **f32), torch.empty(C_, **f32)     # (written by the call)
        dbn = torch.empty(2, N_MELS, **f32) if ctx.audio else None
        mode = _lib.PATCH_AUDIO if ctx.audio else _lib.PATCH_IMAGE
        ws = torch.empty(ctx.lib.patch_embed_params_ws_floats(mode, B, in_chans, H, W, C_), **f32)
        code = lambda dt: _lib.F32 if dt == torch.float32 else _lib.BF16
        ptr = lambda t: t.data_ptr() if t is not None else None
        _mark_stream_use(x, w, b, lw, lb, scale, shift, mean, dout, stripes, lam)
        tail = (w.data_ptr(), b.data_ptr(), lw.data_ptr(), lb.data_ptr(), ctx.eps, dout.data_ptr(), dw.data_ptr(), db.data_ptr(), dlw.data_ptr(),
                dlb.data_ptr(), ptr(dbn), ws.data_ptr(), _stream_of(x))
        with _dev_guard(x):
            if stripes is not None or lam is not None:
                ctx.lib.patch_embed_backward_params_aug(code(dout.dtype), B, T, C_, x.data_ptr(), ptr(scale), ptr(shift), ptr(mean), ptr(stripes),
                                                        ptr(lam), *tail)
            else:
                ctx.lib.patch_embed_backward_params(mode, code(x.dtype), code(dout.dtype), B, in_chans, H, W, T, C_, x.data_ptr(), ptr(scale),
                                                    ptr(shift), ptr(mean), *tail)
        need = ctx.needs_input_grad
        # the pivot of the kernel's sums is the mean bn0 normalised with: d bn0.weight = rstd g1, d bn0.bias = g0
        dbw = dbn[0] * rstd if ctx.audio and need[6] else None
        dbb = dbn[1] if ctx.audio and need[7] else None
        return (None, None, dw if need[2] else None, db if need[3] else None, dlw if need[4] else None, dlb if need[5] else None, dbw, dbb,
                None, None, None, None, None, None, None)


def patch_embed_train(x: torch.Tensor, weight: torch.Tensor, bias: torch.Tensor, ln_weight: torch.Tensor, ln_bias: torch.Tensor,
                      eps: float = 1e-5, out_dtype: Optional[torch.dtype] = None, bn_weight: Optional[torch.Tensor] = None,
                      bn_bias: Optional[torch.Tensor] = None, mean: Optional[torch.Tensor] = None, var: Optional[torch.Tensor] = None,
                      bn_eps: float = 1e-5, lib: Optional[Lib] = None, stripes: Optional[torch.Tensor] = None,
                      mixup_lambda: Optional[torch.Tensor] = None) -> torch.Tensor:
    """`patch_embed` for a TRAINABLE front end: the same launch forward, and weight / bias / ln_weight / ln_bias (fp32) receive fp32
    gradients from dgsct_patch_embed_backward_params (dOut fp32 or bf16, every sum in fp32, no atomics: a repeated backward is bit-identical).
    Audio mode (bn_weight, bn_bias, mean, var [64] given; x the log-mel [B, T, 64]): `bn0` enters as its own tensors, scale = bn_weight
    rsqrt(var + bn_eps) and shift = bn_bias - mean scale are formed here, and bn_weight / bn_bias receive their gradients directly (mean and
    var -- running or batch statistics -- are functions of data and get none).  x may not require grad: no input gradient exists.
    stripes / mixup_lambda (audio mode, as in `patch_embed`): the forward and the backward take the *_aug exports and the recomputed convolution
    sees the augmented pixels; both are data and get no gradient.  Both None: exactly the calls above."""
    who = "patch_embed_train"
    audio = any(t is not None for t in (bn_weight, bn_bias, mean, var))
    if not isinstance(x, torch.Tensor) or not x.is_cuda:
        raise RuntimeError("dg-sct_amd: patch_embed_train needs CUDA/HIP tensors (no CPU fallback; fused=False is the ATen formulation)")
    if audio:
        for n, t in (("bn_weight", bn_weight), ("bn_bias", bn_bias), ("mean", mean), ("var", var)):
            if t is None:
                raise RuntimeError("dg-sct_amd: patch_embed_train (audio): bn_weight, bn_bias, mean and var go together")
            _dev_f32(who, n, t, (N_MELS,), x.device)
    if x.requires_grad or (audio and (mean.requires_grad or var.requires_grad)):
        raise RuntimeError(f"dg-sct_amd: {who} returns parameter gradients only: x (and bn0's mean / var) may not require grad (detach them)")
    lib = lib or _lib.default_lib()
    if not lib.has_patch_embed_params():
        raise RuntimeError(f"dg-sct_amd: {who}: {lib.path} does not export dgsct_patch_embed_backward_params (a library without the front "
                           f"end's parameter gradients; fused=False, the ATen formulation, trains without it)")
    if stripes is None and mixup_lambda is None:
        return _PatchEmbedTrainFn.apply(lib, x, weight, bias, ln_weight, ln_bias, bn_weight, bn_bias, mean, var, float(eps), float(bn_eps), out_dtype)
    if not audio:
        raise RuntimeError(f"dg-sct_amd: {who}: stripes / mixup_lambda belong to audio mode (image-side augmentation is not built)")
    _need_aug(who, lib)
    return _PatchEmbedTrainFn.apply(lib, x, weight, bias, ln_weight, ln_bias, bn_weight, bn_bias, mean, var, float(eps), float(bn_eps), out_dtype,
                                    stripes, mixup_lambda)


# ---- patch merging between two backbone stages (csrc/pmerge.hip) ------------------------------------------------
PMERGE_NORM_FIRST, PMERGE_NORM_LAST = _lib.PMERGE_NORM_FIRST, _lib.PMERGE_NORM_LAST


def patch_merge_supported(x: torch.Tensor, H: int, W: int, mode: int) -> bool:
    """what csrc/pmerge.hip takes: a bf16 GPU map [B, H*W, C], H and W even, C a multiple of 32 with 4C <= 1536 (NORM_FIRST) /
    2C <= 1536 (NORM_LAST)"""
    if not isinstance(x, torch.Tensor) or not x.is_cuda or x.dtype != torch.bfloat16 or x.dim() != 3 or x.shape[0] < 1:
        return False
    C_ = x.shape[-1]
    return (H >= 2 and W >= 2 and H % 2 == 0 and W % 2 == 0 and x.shape[1] == H * W and C_ >= 32 and C_ % 32 == 0
            and C_ <= (384 if mode == PMERGE_NORM_FIRST else 768))


class _PatchMergeFn(torch.autograd.Function):
    """one library call each way (dgsct_patch_merge_*); gradient for x only: a frozen merge (_PatchMergeTrainFn is the trainable one)"""

    @staticmethod
    def forward(ctx, lib, x, w, ln_w, ln_b, eps, H, W, mode):
        B, L, C_ = x.shape
        rows = B * (H // 2) * (W // 2)
        out = torch.empty(B, rows // B, 2 * C_, dtype=x.dtype, device=x.device)
        pre = torch.empty_like(out) if mode == PMERGE_NORM_LAST else None
        mu = torch.empty(rows, dtype=torch.float32, device=x.device)
        rstd = torch.empty(rows, dtype=torch.float32, device=x.device)
        _mark_stream_use(x, w, ln_w, ln_b)
        with _dev_guard(x):
            lib.patch_merge_forward(mode, B, H, W, C_, x.data_ptr(), w.data_ptr(), ln_w.data_ptr(), ln_b.data_ptr(), float(eps), out.data_ptr(),
                                    pre.data_ptr() if pre is not None else None, mu.data_ptr(), rstd.data_ptr(), _stream_of(x))
        ctx.lib, ctx.geom, ctx.eps = lib, (mode, B, H, W, C_), float(eps)
        # NORM_FIRST's backward re-gathers x; NORM_LAST's reads `pre` instead, so the stage map is not kept alive for it
        ctx.save_for_backward(w, ln_w, mu, rstd, x if pre is None else pre)
        return out

    @staticmethod
    def backward(ctx, dout):
        w, ln_w, mu, rstd, kept = ctx.saved_tensors
        mode, B, H, W, C_ = ctx.geom
        x, pre = (kept, None) if mode == PMERGE_NORM_FIRST else (None, kept)
        dout = dout.contiguous()
        if dout.dtype != kept.dtype:
            dout = dout.to(kept.dtype)
        dx = torch.empty(B, H * W, C_, dtype=kept.dtype, device=kept.device)
        ws = torch.empty(ctx.lib.patch_merge_ws_bytes(*ctx.geom), dtype=torch.uint8, device=kept.device)
        _mark_stream_use(kept, w, ln_w, mu, rstd, dout)
        with _dev_guard(kept):
            ctx.lib.patch_merge_backward(*ctx.geom, dout.data_ptr(), x.data_ptr() if x is not None else None, w.data_ptr(), ln_w.data_ptr(),
                                         pre.data_ptr() if pre is not None else None, mu.data_ptr(), rstd.data_ptr(), ctx.eps, dx.data_ptr(),
                                         ws.data_ptr(), _stream_of(kept))
        return None, dx, None, None, None, None, None, None, None


def patch_merge(x: torch.Tensor, w_bf16: torch.Tensor, ln_w: torch.Tensor, ln_b: torch.Tensor, eps: float, H: int, W: int, mode: int,
                lib: Optional[Lib] = None) -> torch.Tensor:
    """The 2 x 2 patch merge between two stages on x [B, H*W, C] (bf16, token-major) -> [B, (H/2)(W/2), 2C]:
    PMERGE_NORM_FIRST (HTS-AT) `LN_4C(gather(x)) @ w^T`, PMERGE_NORM_LAST (Swin-V2) `LN_2C(gather(x) @ w^T)`; gather = the four tokens
    (2i,2j), (2i+1,2j), (2i,2j+1), (2i+1,2j+1) side by side.  w_bf16 [2C, 4C] bf16, ln_w / ln_b fp32 ([4C] / [2C]).  One launch forward
    (NORM_LAST: two), two backward; the gradient reaches x only (w and the norm vectors are frozen inputs)."""
    who = "patch_merge"
    if mode not in (PMERGE_NORM_FIRST, PMERGE_NORM_LAST):
        raise RuntimeError(f"dg-sct_amd: {who}: unknown mode {mode}")
    if not patch_merge_supported(x, H, W, mode):
        raise RuntimeError(f"dg-sct_amd: {who} takes a bf16 CUDA/HIP map [B, H*W, C] with H, W even, C a multiple of 32 and "
                           f"{'4C' if mode == PMERGE_NORM_FIRST else '2C'} <= 1536 (got {tuple(getattr(x, 'shape', ()))} "
                           f"{getattr(x, 'dtype', None)}, map {H} x {W}; no CPU kernels: fused=False is the ATen formulation)")
    C_ = x.shape[-1]
    dev = x.device
    if (not isinstance(w_bf16, torch.Tensor) or w_bf16.dtype != torch.bfloat16 or tuple(w_bf16.shape) != (2 * C_, 4 * C_) or w_bf16.device != dev
            or not w_bf16.is_contiguous()):
        raise RuntimeError(f"dg-sct_amd: {who}: w_bf16 must be a contiguous bf16 tensor [{2 * C_}, {4 * C_}] on {dev}")
    cn = 4 * C_ if mode == PMERGE_NORM_FIRST else 2 * C_
    _dev_f32(who, "ln_w", ln_w, (cn,), dev)
    _dev_f32(who, "ln_b", ln_b, (cn,), dev)
    if any(t.requires_grad for t in (w_bf16, ln_w, ln_b)):
        raise RuntimeError(f"dg-sct_amd: {who} returns no weight gradients: pass detached w_bf16 / ln_w / ln_b (a trainable merge takes the ATen formulation)")
    return _PatchMergeFn.apply(lib or _lib.default_lib(), x.contiguous(), w_bf16, ln_w, ln_b, float(eps), int(H), int(W), int(mode))


class _PatchMergeTrainFn(torch.autograd.Function):
    """_PatchMergeFn for a trainable merge: the parameters are inputs, and backward is dgsct_patch_merge_backward_params"""

    @staticmethod
    def forward(ctx, lib, x, weight, ln_weight, ln_bias, w, ln_w, ln_b, eps, H, W, mode):
        B, L, C_ = x.shape
        rows = B * (H // 2) * (W // 2)
        out = torch.empty(B, rows // B, 2 * C_, dtype=x.dtype, device=x.device)
        pre = torch.empty_like(out) if mode == PMERGE_NORM_LAST else None
        mu = torch.empty(rows, dtype=torch.float32, device=x.device)
        rstd = torch.empty(rows, dtype=torch.float32, device=x.device)
        _mark_stream_use(x, w, ln_w, ln_b)
        with _dev_guard(x):
            lib.patch_merge_forward(mode, B, H, W, C_, x.data_ptr(), w.data_ptr(), ln_w.data_ptr(), ln_b.data_ptr(), float(eps), out.data_ptr(),
                                    pre.data_ptr() if pre is not None else None, mu.data_ptr(), rstd.data_ptr(), _stream_of(x))
        ctx.lib, ctx.geom, ctx.eps = lib, (mode, B, H, W, C_), float(eps)
        ctx.param_dtypes = (weight.dtype, ln_weight.dtype, ln_bias.dtype)
        # the weight gradient needs the operand the forward multiplied with W, which is re-made from x in both modes: NORM_LAST keeps
        # the stage map alive as well as `pre`
        ctx.save_for_backward(x, w, ln_w, ln_b, mu, rstd, *(() if pre is None else (pre,)))
        return out

    @staticmethod
    def backward(ctx, dout):
        x, w, ln_w, ln_b, mu, rstd = ctx.saved_tensors[:6]
        pre = ctx.saved_tensors[6] if len(ctx.saved_tensors) > 6 else None
        mode, B, H, W, C_ = ctx.geom
        dout = dout.contiguous()
        if dout.dtype != x.dtype:
            dout = dout.to(x.dtype)
        dx = torch.empty(B, H * W, C_, dtype=x.dtype, device=x.device)
        f32 = dict(dtype=torch.float32, device=x.device)
        dw, dln_w, dln_b = torch.empty(2 * C_, 4 * C_, **f32), torch.empty_like(ln_w), torch.empty_like(ln_b)      # (zeroed by the call)
        ws = torch.empty(ctx.lib.patch_merge_params_ws_bytes(*ctx.geom), dtype=torch.uint8, device=x.device)
        _mark_stream_use(x, w, ln_w, ln_b, mu, rstd, dout, pre)
        with _dev_guard(x):
            ctx.lib.patch_merge_backward_params(*ctx.geom, dout.data_ptr(), x.data_ptr(), w.data_ptr(), ln_w.data_ptr(), ln_b.data_ptr(),
                                                pre.data_ptr() if pre is not None else None, mu.data_ptr(), rstd.data_ptr(), ctx.eps,
                                                dx.data_ptr(), dw.data_ptr(), dln_w.data_ptr(), dln_b.data_ptr(), ws.data_ptr(), _stream_of(x))
        need = ctx.needs_input_grad
        grads = [g.to(dt) if n else None for g, dt, n in zip((dw, dln_w, dln_b), ctx.param_dtypes, need[2:5])]
        return (None, dx if need[1] else None, *grads, None, None, None, None, None, None, None)


def patch_merge_train(x: torch.Tensor, weight: torch.Tensor, ln_w: torch.Tensor, ln_b: torch.Tensor, eps: float, H: int, W: int, mode: int,
                      lib: Optional[Lib] = None) -> torch.Tensor:
    """`patch_merge` for a TRAINABLE merge: `weight` [2C, 4C], `ln_w`, `ln_b` ([4C] NORM_FIRST / [2C] NORM_LAST) are the parameters
    themselves, in any floating dtype (fp32 masters or bf16), and receive gradients.  The forward runs the same kernels on a bf16 copy of
    the weight and fp32 copies of the norm vectors; backward is
    dgsct_patch_merge_backward_params: dx bit for bit as `patch_merge` returns it, and dW / d ln_w / d ln_b accumulated in fp32 and cast
    to each parameter's dtype (fp32 masters get fp32 gradients).  NORM_LAST saves x as well as the product before the norm: the weight
    gradient re-gathers its operand from x, so the stage map stays alive until backward (the frozen `patch_merge` keeps only `pre`)."""
    return _patch_merge_train(x, weight, ln_w, ln_b, eps, H, W, mode, lib)


def _patch_merge_train(x, weight, ln_w, ln_b, eps, H, W, mode, lib=None, cached=None):
    """`patch_merge_train`; `cached` = (weight in bf16, ln_w, ln_b in fp32) where the caller keeps those copies, as the merge modules do"""
    who = "patch_merge_train"
    if mode not in (PMERGE_NORM_FIRST, PMERGE_NORM_LAST):
        raise RuntimeError(f"dg-sct_amd: {who}: unknown mode {mode}")
    if not patch_merge_supported(x, H, W, mode):
        raise RuntimeError(f"dg-sct_amd: {who} takes a bf16 CUDA/HIP map [B, H*W, C] with H, W even, C a multiple of 32 and "
                           f"{'4C' if mode == PMERGE_NORM_FIRST else '2C'} <= 1536 (got {tuple(getattr(x, 'shape', ()))} "
                           f"{getattr(x, 'dtype', None)}, map {H} x {W}; no CPU kernels: fused=False is the ATen formulation)")
    lib = lib or _lib.default_lib()
    if not lib.has_patch_merge_params():
        raise RuntimeError(f"dg-sct_amd: {who}: {lib.path} does not export dgsct_patch_merge_backward_params (a library without the merge's "
                           f"parameter gradients; the ATen formulation trains a merge without it)")
    C_ = x.shape[-1]
    dev = x.device
    cn = 4 * C_ if mode == PMERGE_NORM_FIRST else 2 * C_
    for name, t, shape in (("weight", weight, (2 * C_, 4 * C_)), ("ln_w", ln_w, (cn,)), ("ln_b", ln_b, (cn,))):
        if not isinstance(t, torch.Tensor) or not t.is_floating_point() or tuple(t.shape) != shape or t.device != dev:
            raise RuntimeError(f"dg-sct_amd: {who}: {name} must be a floating-point tensor {list(shape)} on {dev}")
    if cached is None:
        with torch.no_grad():
            cached = (weight.detach().to(torch.bfloat16).contiguous(), ln_w.detach().float().contiguous(), ln_b.detach().float().contiguous())
    return _PatchMergeTrainFn.apply(lib, x.contiguous(), weight, ln_w, ln_b, *cached, float(eps), int(H), int(W), int(mode))


# ---- the live part of the CMBS event head (csrc/head.hip) -----------------------------------------------------------------------
CMBS_TOPK, CMBS_MAX_T, CMBS_MAX_D, CMBS_MAX_K = 4, 32, 512, 32


class _CMBSHeadFn(torch.autograd.Function):
    """(v, a, video_cas.{weight, bias}, audio_cas.{weight, bias}, classifier.{weight, bias}, event_classifier.{weight, bias}) ->
    (is_event_scores [T, B, 1], event_scores [B, K], av_score [B, K]): one HIP launch forward, two backward (csrc/head.hip)."""

    @staticmethod
    def forward(ctx, lib, gamma, v, a, Wvc, bvc, Wac, bac, wc, bc, We, be):
        T, B, D = v.shape
        K = Wvc.shape[0]
        dev = v.device
        v, a = v.contiguous().float(), a.contiguous().float()
        ps = [t.detach().contiguous().float() for t in (Wvc, bvc, Wac, bac, wc, bc, We, be)]
        f32 = dict(dtype=torch.float32, device=dev)
        is_event, event, av = torch.empty(T, B, 1, **f32), torch.empty(B, K, **f32), torch.empty(B, K, **f32)
        topmask = torch.empty(B, 2, K, dtype=torch.int32, device=dev)
        argmax = torch.empty(B, D, dtype=torch.int32, device=dev)
        _mark_stream_use(v, a, *ps)
        with _dev_guard(v):
            lib.cmbs_head_forward(T, B, D, K, float(gamma), v.data_ptr(), a.data_ptr(), *[t.data_ptr() for t in ps], is_event.data_ptr(),
                                  event.data_ptr(), av.data_ptr(), topmask.data_ptr(), argmax.data_ptr(), _stream_of(v))
        ctx.lib, ctx.gamma, ctx.dims = lib, float(gamma), (T, B, D, K)
        ctx.param_shapes = tuple((t.shape, t.dtype) for t in (Wvc, bvc, Wac, bac, wc, bc, We, be))
        ctx.save_for_backward(v, a, ps[0], ps[2], ps[4], ps[6], topmask, argmax)
        ctx.mark_non_differentiable(topmask, argmax)
        ctx.set_materialize_grads(False)                   # an unused output's cotangent arrives as None -> a NULL pointer, no zero fill
        return is_event, event, av, topmask, argmax

    @staticmethod
    def backward(ctx, d_is, d_ev, d_av, _dm, _da):
        v, a, Wvc, Wac, wc, We, topmask, argmax = ctx.saved_tensors
        T, B, D, K = ctx.dims
        dev = v.device
        need = ctx.needs_input_grad
        if d_is is None and d_ev is None and d_av is None:
            return (None,) * 12
        cots = [t.contiguous().float() if t is not None else None for t in (d_is, d_ev, d_av)]
        f32 = dict(dtype=torch.float32, device=dev)
        want_x = need[2] or need[3]
        dv, da = (torch.empty(T, B, D, **f32), torch.empty(T, B, D, **f32)) if want_x else (None, None)
        grads = ws = None
        if any(need[4:12]):                                # (all eight are computed together; the ones not asked for are dropped below)
            grads = [torch.empty(s, **f32) for s in ((K, D), (K,), (K, D), (K,), (1, D), (1,), (K, D), (K,))]
            ws = torch.empty(ctx.lib.cmbs_head_ws_bytes(T, B, D, K), dtype=torch.uint8, device=dev)
        ptr = lambda t: t.data_ptr() if t is not None else None      # noqa: E731
        _mark_stream_use(v, a, Wvc, Wac, wc, We, topmask, argmax, *cots)
        with _dev_guard(v):
            ctx.lib.cmbs_head_backward(T, B, D, K, ctx.gamma, v.data_ptr(), a.data_ptr(), Wvc.data_ptr(), Wac.data_ptr(), wc.data_ptr(),
                                       We.data_ptr(), topmask.data_ptr(), argmax.data_ptr(), *[ptr(t) for t in cots], ptr(dv), ptr(da),
                                       [g.data_ptr() for g in grads] if grads is not None else None, ptr(ws), _stream_of(v))
        out = [None, None, dv if need[2] else None, da if need[3] else None]
        for i, (shape, dtype) in enumerate(ctx.param_shapes):
            out.append(grads[i].view(shape).to(dtype) if grads is not None and need[4 + i] else None)
        return tuple(out)


def cmbs_head_supported(v: torch.Tensor, a: torch.Tensor, K: int) -> bool:
    """the kernels take these inputs: fp32 [T, B, D] on a ROCm device inside the limits of include/dgsct.h"""
    if not (isinstance(v, torch.Tensor) and isinstance(a, torch.Tensor) and v.dim() == 3 and v.shape == a.shape):
        return False
    T, B, D = v.shape
    return (v.is_cuda and a.device == v.device and v.dtype == torch.float32 and a.dtype == torch.float32 and CMBS_TOPK <= T <= CMBS_MAX_T
            and B >= 1 and D % 64 == 0 and 64 <= D <= CMBS_MAX_D and 1 <= K <= CMBS_MAX_K)


def cmbs_head(v: torch.Tensor, a: torch.Tensor, video_cas_w, video_cas_b, audio_cas_w, audio_cas_b, cls_w, cls_b, event_w, event_b,
              gamma: float, lib: Optional[Lib] = None, return_saved: bool = False):
    """The live part of ``CMBS.forward`` (net_trans.py:273-292) on fp32 time-major ``v``, ``a`` [T, B, D]: returns
    ``(is_event_scores [T, B, 1], event_scores [B, K], av_score [B, K])``; with ``return_saved`` also the two tensors the backward reads
    instead of a sort permutation, ``topmask [B, 2, K]`` and ``argmax [B, D]`` (int32).  Shapes outside the limits are refused by the
    launcher (nothing is launched); a library without the export raises naming the symbol.  No CPU kernels."""
    if not (isinstance(v, torch.Tensor) and isinstance(a, torch.Tensor) and v.dim() == 3 and v.shape == a.shape):
        raise RuntimeError("dg-sct_amd: cmbs_head takes v, a of one shape [T, B, D]")
    if v.dtype != torch.float32 or a.dtype != torch.float32:
        raise RuntimeError(f"dg-sct_amd: cmbs_head runs in fp32, as the reference runs this head (got {v.dtype}, {a.dtype})")
    if lib is None:
        if not v.is_cuda:
            raise RuntimeError("dg-sct_amd: cmbs_head runs on MI355X through libdgsct.so; there is no CPU path (CMBS(fused=False) is the "
                               "ATen formulation)")
        lib = _lib.default_lib()
    if not lib.has_cmbs_head():
        raise RuntimeError(f"dg-sct_amd: {lib.path} does not export dgsct_cmbs_head_forward (a library without the CMBS event head)")
    K, D = video_cas_w.shape
    for name, t, n in (("video_cas.weight", video_cas_w, K * D), ("video_cas.bias", video_cas_b, K), ("audio_cas.weight", audio_cas_w, K * D),
                       ("audio_cas.bias", audio_cas_b, K), ("classifier.weight", cls_w, D), ("classifier.bias", cls_b, 1),
                       ("event_classifier.weight", event_w, K * D), ("event_classifier.bias", event_b, K)):
        if t.numel() != n or t.device != v.device or D != v.shape[-1]:
            raise RuntimeError(f"dg-sct_amd: cmbs_head: {name} must hold {n} elements on {v.device} for D = {v.shape[-1]}, K = {K}")
    outs = _CMBSHeadFn.apply(lib, float(gamma), v, a, video_cas_w, video_cas_b, audio_cas_w, audio_cas_b, cls_w, cls_b, event_w, event_b)
    return outs if return_saved else outs[:3]


# ---- the audio-visual TPAVI block in linear form (csrc/tpavi.hip) ------------------------------------------------------------------
TPAVI_MIN_C, TPAVI_MAX_C, TPAVI_MAX_T = 64, 256, 16


def _tpavi_view(x: torch.Tensor, T: Optional[int]):
    """x [B, C, T, H, W] or frames [B*T, C, H, W] -> (x with contiguous planes, (B, C, T, H, W), element strides of (b, c, t)): what the
    kernels address.  Copies only if a plane's H*W positions are not contiguous."""
    if x.dim() == 5:
        B, C_, T_, H, W = x.shape
        if not (x.stride(4) == 1 and x.stride(3) == W):
            x = x.contiguous()
        return x, (B, C_, T_, H, W), (x.stride(0), x.stride(1), x.stride(2))
    BT, C_, H, W = x.shape
    if not (x.stride(3) == 1 and x.stride(2) == W):
        x = x.contiguous()
    return x, (BT // T, C_, T, H, W), (T * x.stride(0), x.stride(1), x.stride(0))


def tpavi_setup(s, audio, align_w, align_b, g_w, g_b, wz_w, wz_b, theta_w, theta_b, phi_w, phi_b, HW: int):
    """The per-clip setup of the linear form, plain torch under autograd: frame sums ``s [B, T, C]`` and
    ``audio [B, T, 128]`` -> ``(A [B, C, C], c [B, C], audio_temp [B, T, C])`` with ``u = A_b x_p + c_b`` the block's value in front of
    its BatchNorm.  The 1x1x1 convolutions' weights come as stored (5-D)."""
    T = s.shape[1]
    Wg, Wz, Wt, Wp = (w.flatten(1) for w in (g_w, wz_w, theta_w, phi_w))
    a = torch.nn.functional.linear(audio, align_w, align_b)                  # [B, T, C]   (the module's second result)
    phi = torch.nn.functional.linear(a, Wp, phi_b)                           # [B, T, Ci]
    gbar = torch.nn.functional.linear(s, Wg) + HW * g_b                      # [B, T, Ci]
    K = torch.matmul(phi.transpose(1, 2), gbar) / (T * HW)                   # [B, Ci, Ci]
    WK = torch.matmul(Wz, K.transpose(1, 2))                                 # [B, C, Ci]
    return torch.matmul(WK, Wt), torch.matmul(WK, theta_b) + wz_b, a


class _TPAVISumFn(torch.autograd.Function):
    """x -> frame sums s [B, T, C] (one launch).  The backward hands autograd the broadcast of ds as an expanded view: its accumulation
    into dx is the extra pass."""

    @staticmethod
    def forward(ctx, lib, x, T):
        x, dims, xs = _tpavi_view(x, T)
        B, C_, T_ = dims[:3]
        s = torch.empty(B, T_, C_, dtype=torch.float32, device=x.device)
        _mark_stream_use(x)
        with _dev_guard(x):
            lib.tpavi_frame_sum(dims, x.data_ptr(), xs, s.data_ptr(), _stream_of(x))
        ctx.dims, ctx.five = dims, x.dim() == 5
        return s

    @staticmethod
    def backward(ctx, ds):
        B, C_, T_, H, W = ctx.dims
        if ctx.five:
            return None, ds.permute(0, 2, 1)[:, :, :, None, None].expand(B, C_, T_, H, W), None
        return None, ds.reshape(B * T_, C_)[:, :, None, None].expand(B * T_, C_, H, W), None


class _TPAVIFn(torch.autograd.Function):
    """(x, A, c, bn_w, bn_b, ln_w, ln_b) -> z = LayerNorm_C(BatchNorm(A_b x + c_b) + x).  ``mu0`` None: no BatchNorm inside (eval: folded
    into A, c by the caller).  Forward: two passes over x and a finalising launch (one pass without BatchNorm); backward: three passes and
    three reductions.  Saves x, A, c and the [2, C] statistics: nothing else of x's size."""

    @staticmethod
    def forward(ctx, lib, T, x, A, c, bn_w, bn_b, ln_w, ln_b, mu0, run_mean, run_var, momentum, bn_eps, ln_eps):
        x, dims, xs = _tpavi_view(x, T)
        C_ = dims[1]
        dev = x.device
        z = torch.empty_like(x)
        z, _, zs = _tpavi_view(z, T)
        A, c = A.contiguous(), c.contiguous()
        ln_w, ln_b = ln_w.detach().contiguous(), ln_b.detach().contiguous()
        stat = ws = None
        if mu0 is not None:
            bn_w, bn_b = bn_w.detach().contiguous(), bn_b.detach().contiguous()
            stat = torch.empty(2, C_, dtype=torch.float32, device=dev)
            ws = torch.empty(2048 * C_, dtype=torch.uint8, device=dev)
        ptr = lambda t: t.data_ptr() if t is not None else None      # noqa: E731
        _mark_stream_use(x, A, c, ln_w, ln_b, *[t for t in (bn_w, bn_b, mu0, run_mean, run_var) if t is not None])
        with _dev_guard(x):
            lib.tpavi_forward(dims, x.data_ptr(), xs, A.data_ptr(), c.data_ptr(), ptr(mu0), ptr(bn_w) if stat is not None else None,
                              ptr(bn_b) if stat is not None else None, ptr(run_mean), ptr(run_var), float(momentum), float(bn_eps),
                              ln_w.data_ptr(), ln_b.data_ptr(), float(ln_eps), z.data_ptr(), zs, ptr(stat), ptr(ws), _stream_of(x))
        ctx.lib, ctx.T, ctx.dims, ctx.ln_eps, ctx.bn = lib, T, dims, float(ln_eps), stat is not None
        ctx.save_for_backward(x, A, c, ln_w, *((stat, bn_w, bn_b) if stat is not None else ()))
        return z

    @staticmethod
    def backward(ctx, dz):
        x, A, c, ln_w, *bn = ctx.saved_tensors
        stat, bn_w, bn_b = bn if ctx.bn else (None, None, None)
        lib, dims = ctx.lib, ctx.dims
        B, C_ = dims[:2]
        dev = x.device
        x, _, xs = _tpavi_view(x, ctx.T)
        dz, _, gs = _tpavi_view(dz.float(), ctx.T)
        dx = torch.empty_like(x)
        dx, _, dxs = _tpavi_view(dx, ctx.T)
        f32 = dict(dtype=torch.float32, device=dev)
        dA, dc = torch.empty(B, C_, C_, **f32), torch.empty(B, C_, **f32)
        dln_w, dln_b = torch.empty(C_, **f32), torch.empty(C_, **f32)
        dbn_w, dbn_b = (torch.empty(C_, **f32), torch.empty(C_, **f32)) if ctx.bn else (None, None)
        ws = torch.empty(lib.tpavi_ws_bytes(*dims), dtype=torch.uint8, device=dev)
        ptr = lambda t: t.data_ptr() if t is not None else None      # noqa: E731
        _mark_stream_use(x, A, c, ln_w, dz, *[t for t in (stat, bn_w, bn_b) if t is not None])
        with _dev_guard(x):
            lib.tpavi_backward(dims, x.data_ptr(), xs, A.data_ptr(), c.data_ptr(), ptr(stat), ptr(bn_w), ptr(bn_b), ln_w.data_ptr(), ctx.ln_eps,
                               dz.data_ptr(), gs, None, dx.data_ptr(), dxs, dA.data_ptr(), dc.data_ptr(), ptr(dbn_w), ptr(dbn_b),
                               dln_w.data_ptr(), dln_b.data_ptr(), ws.data_ptr(), _stream_of(x))
        return None, None, dx, dA, dc, dbn_w, dbn_b, dln_w, dln_b, None, None, None, None, None, None


def tpavi_supported(x: torch.Tensor, audio: torch.Tensor, T: Optional[int] = None) -> bool:
    """the kernels take these inputs: fp32 ``x [B, C, T, H, W]`` (or frames ``[B*T, C, H, W]`` with ``T``) and ``audio [B, T, 128]`` on one
    ROCm device, inside the limits of include/dgsct.h"""
    if not (isinstance(x, torch.Tensor) and isinstance(audio, torch.Tensor) and x.dim() in (4, 5) and audio.dim() == 3):
        return False
    if x.dim() == 4 and (not T or x.shape[0] % T):
        return False
    B, C_, T_ = (x.shape[0], x.shape[1], x.shape[2]) if x.dim() == 5 else (x.shape[0] // T, x.shape[1], T)
    return (x.is_cuda and audio.device == x.device and x.dtype == torch.float32 and audio.dtype == torch.float32 and B >= 1
            and tuple(audio.shape[:2]) == (B, T_) and C_ % 64 == 0 and TPAVI_MIN_C <= C_ <= TPAVI_MAX_C and 1 <= T_ <= TPAVI_MAX_T
            and x.shape[-1] >= 1 and x.shape[-2] >= 1)


def tpavi(x: torch.Tensor, audio: torch.Tensor, align_w, align_b, g_w, g_b, wz_w, wz_b, theta_w, theta_b, phi_w, phi_b, bn_w, bn_b,
          run_mean, run_var, ln_w, ln_b, training: bool, T: Optional[int] = None, momentum: float = 0.1, bn_eps: float = 1e-5,
          ln_eps: float = 1e-5, lib: Optional[Lib] = None):
    """``TPAVIModule.forward`` (mode 'dot', audio branch, BatchNorm layer) through the kernels of csrc/tpavi.hip: returns
    ``(z, audio_temp)``, ``z`` in ``x``'s shape and layout.  ``x`` is ``[B, C, T, H, W]``, or the model's frames ``[B*T, C, H, W]`` with
    ``T`` given; neither is copied.  The per-clip setup (``tpavi_setup``) runs in torch under autograd, so the gradients of ``theta``,
    ``phi``, ``g``, ``W_z.0``, ``align_channel`` and ``audio`` come from its backward; the passes over ``x`` are the kernels.
    ``training``: batch statistics, and ``run_mean`` / ``run_var`` are updated in place (the caller counts ``num_batches_tracked``);
    otherwise the BatchNorm is folded into ``A`` and ``c`` here.  Inputs outside the limits raise; there is no CPU path."""
    if not (isinstance(x, torch.Tensor) and x.dim() in (4, 5) and isinstance(audio, torch.Tensor)):
        raise RuntimeError("dg-sct_amd: tpavi takes x [B, C, T, H, W] or frames [B*T, C, H, W] with T, and audio [B, T, 128]")
    if x.dtype != torch.float32 or audio.dtype != torch.float32:
        raise RuntimeError(f"dg-sct_amd: tpavi runs in fp32 (got {x.dtype}, {audio.dtype})")
    if lib is None:
        if not x.is_cuda:
            raise RuntimeError("dg-sct_amd: tpavi runs on MI355X through libdgsct.so; there is no CPU path (TPAVIModule(fused=False) is the "
                               "ATen linear form)")
        lib = _lib.default_lib()
    if not lib.has_tpavi():
        raise RuntimeError(f"dg-sct_amd: {lib.path} does not export dgsct_tpavi_forward (a library without the TPAVI kernels)")
    if x.dim() == 4 and (not T or x.shape[0] % T):
        raise RuntimeError(f"dg-sct_amd: tpavi on frames {list(x.shape)} needs T dividing the first dimension (got T={T})")
    if x.dim() == 4:
        audio = audio.reshape(-1, T, audio.shape[-1])
    if not tpavi_supported(x, audio, T):
        raise RuntimeError(f"dg-sct_amd: tpavi: the kernels take fp32 x with C a multiple of 64 in [{TPAVI_MIN_C}, {TPAVI_MAX_C}] and "
                           f"1 <= T <= {TPAVI_MAX_T}, and audio [B, T, 128] on the same ROCm device (got x {list(x.shape)}, audio "
                           f"{list(audio.shape)} on {x.device})")
    T5 = T if x.dim() == 4 else None
    xv, dims, _ = _tpavi_view(x, T5)
    B, C_, T_, H, W = dims
    s = _TPAVISumFn.apply(lib, xv, T5)
    A, c, a_temp = tpavi_setup(s, audio, align_w, align_b, g_w, g_b, wz_w, wz_b, theta_w, theta_b, phi_w, phi_b, H * W)
    if training:
        with torch.no_grad():                              # the shift of the centred variance accumulation: mean of u from the frame sums
            mu0 = ((torch.bmm(A, s.sum(1)[:, :, None])[:, :, 0] + T_ * H * W * c).sum(0) / (B * T_ * H * W)).contiguous()
        z = _TPAVIFn.apply(lib, T5, xv, A, c, bn_w, bn_b, ln_w, ln_b, mu0, run_mean, run_var, momentum, bn_eps, ln_eps)
    else:
        k = bn_w * torch.rsqrt(run_var + bn_eps)
        z = _TPAVIFn.apply(lib, T5, xv, k[None, :, None] * A, k * (c - run_mean) + bn_b, None, None, ln_w, ln_b, None, None, None, momentum,
                           bn_eps, ln_eps)
    return z, a_temp
