"""ctypes binding of libdgsct.so (include/dgsct.h).  No CPU fallback: if the HIP library is missing
or does not load, importing the product path raises -- build it with ``python -m dgsct_amd.build``
(or ``__graft_entry__.build()``)."""
from __future__ import annotations

import ctypes as C
import os
from typing import List, Optional, Sequence

HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(HERE, "libdgsct.so")

F32, BF16, BF16_FP8 = 0, 1, 2
REMAP_CONV, REMAP_FIXED = 0, 1
PATCH_IMAGE, PATCH_AUDIO = 0, 1
PMERGE_NORM_FIRST, PMERGE_NORM_LAST = 0, 1

# parameter table order == enum in include/dgsct.h; values are the reference state_dict names
PARAM_NAMES: List[str] = [
    "gate", "my_tokens", "gate_av", "conv_adapter.weight", "conv_adapter.bias", "fc.weight", "fc.bias",
    "fc_affine_audio_1.weight", "fc_affine_audio_1.bias", "fc_affine_video_1.weight", "fc_affine_video_1.bias",
    "fc_affine_bottleneck.weight", "fc_affine_bottleneck.bias", "fc_affine_video_2.weight", "fc_affine_video_2.bias",
    "fc_affine_audio_2.weight", "fc_affine_audio_2.bias", "fc_affine_v_s_att.weight", "fc_affine_v_s_att.bias",
    "fc_affine_v_c_att.weight", "fc_affine_v_c_att.bias", "down_sampler.weight", "up_sampler.weight",
    "bn1.weight", "bn1.bias", "bn1.running_mean", "bn1.running_var",
    "bn2.weight", "bn2.bias", "bn2.running_mean", "bn2.running_var",
    "ln_before.weight", "ln_before.bias", "ln_post.weight", "ln_post.bias",
    "temporal_gated.0.weight", "temporal_gated.0.bias",
]
P_COUNT = len(PARAM_NAMES)
P_INDEX = {n: i for i, n in enumerate(PARAM_NAMES)}
P_WN = P_INDEX["conv_adapter.weight"]


class AdapterDesc(C.Structure):
    _fields_ = [(n, C.c_int32) for n in ("BT", "T", "N", "C", "No", "Co", "tk", "r", "g", "dtype", "remap", "use_bn", "use_gate",
                                         "ln_before", "ln_post", "gate_before_ln_post", "temporal", "training")] + \
               [(n, C.c_float) for n in ("alpha", "beta", "gamma", "eps", "bn_momentum")]


class Sizes(C.Structure):
    _fields_ = [("prep_bytes", C.c_int64), ("saved_bytes", C.c_int64), ("ws_fwd_bytes", C.c_int64),
                ("ws_bwd_bytes", C.c_int64), ("grad_floats", C.c_int64),
                ("grad_offset", C.c_int64 * P_COUNT), ("grad_numel", C.c_int64 * P_COUNT)]


class GemmArgs(C.Structure):
    _fields_ = [("mode", C.c_int32), ("M", C.c_int32), ("N", C.c_int32), ("K", C.c_int32), ("KB", C.c_int32),
                ("batch", C.c_int32), ("splitk", C.c_int32), ("atomic", C.c_int32),
                ("A", C.c_void_p), ("lda", C.c_int64), ("a_kmajor", C.c_int32), ("a_bs", C.c_int64), ("a_kbs", C.c_int64),
                ("B", C.c_void_p), ("ldb", C.c_int64), ("b_kmajor", C.c_int32), ("b_bs", C.c_int64), ("b_kbs", C.c_int64),
                ("D", C.c_void_p), ("ddt", C.c_int32), ("ldd", C.c_int64), ("dbs", C.c_int64),
                ("alpha", C.c_float), ("alpha_ptr", C.c_void_p),
                ("bias_m", C.c_void_p), ("bias_n", C.c_void_p), ("bias_n_bs", C.c_int64), ("m_mod", C.c_int32),
                ("r1_m", C.c_void_p), ("r1_n", C.c_void_p), ("act", C.c_int32),
                ("R", C.c_void_p), ("rdt", C.c_int32), ("ldr", C.c_int64), ("rbs", C.c_int64), ("beta", C.c_float),
                ("mask", C.c_void_p), ("ldmask", C.c_int64), ("maskbs", C.c_int64),
                ("R2", C.c_void_p), ("sm_scale", C.c_void_p), ("sm_dot", C.c_void_p)]


class AttnArgs(C.Structure):
    _fields_ = [(n, C.c_int32) for n in ("mode", "B", "N", "C", "tk")] + \
               [(n, C.c_void_p) for n in ("X", "Yp", "dX1", "R2", "out", "T0", "tok", "lse", "a", "aE", "gate_av", "dtok", "dgate",
                                          "da")] + [("invN", C.c_float), ("dT0b", C.c_void_p), ("scratch", C.c_void_p), ("tokpk", C.c_void_p), ("T0pk", C.c_void_p),
                                                               ("dtokpk", C.c_void_p)]


EXPORTS = ["dgsct_test_gemm_fp8", "dgsct_temporal_gate_forward", "dgsct_temporal_gate_backward", "dgsct_test_attn", "dgsct_test_attn_scratch_floats", "dgsct_version", "dgsct_arch", "dgsct_last_error", "dgsct_query", "dgsct_prepare", "dgsct_adapter_forward",
           "dgsct_adapter_forward_ex", "dgsct_adapter_backward", "dgsct_adapter_backward_ex", "dgsct_adapter_backward_ex2", "dgsct_saved_region", "dgsct_test_gemm", "dgsct_test_tune", "dgsct_frame_scale_forward", "dgsct_frame_scale_backward", "dgsct_prof_enable", "dgsct_prof_collect",
           "dgsct_stream_create", "dgsct_stream_destroy", "dgsct_map_pool_forward", "dgsct_map_pool_backward",
           "dgsct_window_attn_forward", "dgsct_window_attn_backward", "dgsct_window_attn_forward_ex", "dgsct_window_attn_backward_ex",
           "dgsct_layer_norm_scratch_floats", "dgsct_layer_norm_forward", "dgsct_layer_norm_backward"]

_PP = C.POINTER(C.c_void_p)


class BwdOpts(C.Structure):
    """dgsct_bwd_opts (include/dgsct.h)"""
    _fields_ = [("flags", C.c_int32), ("dy_residual", C.c_void_p), ("dx_ready_event", C.c_void_p), ("dy_wait_event", C.c_void_p)]


BWD_SKIP_INTO_DX, BWD_NO_JOIN, BWD_HOLD_DY, BWD_ONLY_DY = 1, 2, 4, 8


class Lib:
    """One loaded instance of the C ABI."""

    def __init__(self, path: str = LIB_PATH):
        if not os.path.exists(path):
            raise RuntimeError(f"dg-sct_amd: HIP library not found at {path}; there is no CPU fallback. "
                               f"Build it with `python -c 'import __graft_entry__ as g; g.build()'`.")
        self.path = path
        self.c = C.CDLL(path)
        for name in EXPORTS:
            if not hasattr(self.c, name):
                raise RuntimeError(f"dg-sct_amd: {path} does not export {name}")
        c = self.c
        c.dgsct_version.restype = C.c_int
        c.dgsct_arch.restype = C.c_char_p
        c.dgsct_last_error.restype = C.c_char_p
        c.dgsct_query.argtypes = [C.POINTER(AdapterDesc), C.POINTER(Sizes)]
        c.dgsct_prepare.argtypes = [C.POINTER(AdapterDesc), _PP, C.c_void_p, C.c_void_p]
        c.dgsct_adapter_forward.argtypes = [C.POINTER(AdapterDesc), _PP, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p,
                                            C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
        c.dgsct_adapter_backward.argtypes = [C.POINTER(AdapterDesc), _PP, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p,
                                             C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p,
                                             C.c_void_p, C.c_void_p]
        c.dgsct_adapter_backward_ex.argtypes = c.dgsct_adapter_backward.argtypes + [C.c_void_p, C.c_int]
        c.dgsct_adapter_backward_ex2.argtypes = c.dgsct_adapter_backward.argtypes + [C.c_void_p, C.POINTER(BwdOpts)]
        fa = list(c.dgsct_adapter_forward.argtypes)
        c.dgsct_adapter_forward_ex.argtypes = fa[:5] + [C.c_void_p] + fa[5:] + [C.c_void_p]
        c.dgsct_saved_region.argtypes = [C.POINTER(AdapterDesc), C.c_int, C.c_char_p, C.c_int, C.POINTER(C.c_int64),
                                         C.POINTER(C.c_int64)]
        c.dgsct_test_gemm.argtypes = [C.POINTER(GemmArgs), C.c_void_p]
        c.dgsct_test_tune.argtypes = [C.c_char_p, C.c_int]
        c.dgsct_test_tune.restype = C.c_int
        c.dgsct_test_attn.argtypes = [C.c_int, C.POINTER(AttnArgs), C.c_void_p]
        c.dgsct_test_gemm_fp8.argtypes = [C.c_int] * 3 + [C.c_void_p] * 3 + [C.c_int] + [C.c_void_p] * 4
        c.dgsct_temporal_gate_forward.argtypes = [C.c_int, C.c_int, C.c_float] + [C.c_void_p] * 14
        c.dgsct_temporal_gate_backward.argtypes = [C.c_int, C.c_int, C.c_float] + [C.c_void_p] * 20
        c.dgsct_frame_scale_forward.argtypes = [C.c_int, C.c_int, C.c_int64, C.c_float] + [C.c_void_p] * 4
        c.dgsct_frame_scale_backward.argtypes = [C.c_int, C.c_int, C.c_int64, C.c_float] + [C.c_void_p] * 6
        c.dgsct_test_attn_scratch_floats.argtypes = [C.c_int] * 4
        c.dgsct_test_attn_scratch_floats.restype = C.c_int64
        c.dgsct_stream_create.argtypes = [C.c_int, C.POINTER(C.c_void_p)]
        c.dgsct_stream_destroy.argtypes = [C.c_void_p]
        c.dgsct_map_pool_forward.argtypes = [C.c_int] * 4 + [C.c_void_p] * 4
        c.dgsct_map_pool_backward.argtypes = [C.c_int] * 4 + [C.c_void_p] * 6
        c.dgsct_window_attn_forward.argtypes = [C.c_int] * 8 + [C.c_void_p] * 6
        c.dgsct_window_attn_backward.argtypes = [C.c_int] * 8 + [C.c_void_p] * 8
        c.dgsct_window_attn_forward_ex.argtypes = [C.c_int] * 9 + [C.c_void_p] * 6
        c.dgsct_window_attn_backward_ex.argtypes = [C.c_int] * 9 + [C.c_void_p] * 8
        c.dgsct_layer_norm_scratch_floats.argtypes = [C.c_int]
        c.dgsct_layer_norm_scratch_floats.restype = C.c_int64
        c.dgsct_layer_norm_forward.argtypes = [C.c_int, C.c_int64, C.c_int] + [C.c_void_p] * 3 + [C.c_float] + [C.c_void_p] * 5
        c.dgsct_layer_norm_backward.argtypes = [C.c_int, C.c_int64, C.c_int] + [C.c_void_p] * 6 + [C.c_float] + [C.c_void_p] * 5
        # optional (include/dgsct.h): the table-gradient backward of the window attention; the host emulation of the CPU tests lacks it
        self._wattn_tables = getattr(c, "dgsct_window_attn_backward_tables", None)
        if self._wattn_tables is not None:
            self._wattn_tables.argtypes = [C.c_int] * 9 + [C.c_void_p] * 10
        # optional (include/dgsct.h): the audio / image front ends (csrc/frontend.hip); the host emulation lacks them
        self._logmel = getattr(c, "dgsct_logmel_forward", None)
        self._logmel_scratch = getattr(c, "dgsct_logmel_scratch_floats", None)
        self._patch_embed = getattr(c, "dgsct_patch_embed_forward", None)
        if self._logmel is not None:
            self._logmel.argtypes = [C.c_int, C.c_int64] + [C.c_int] * 3 + [C.c_void_p] * 7
        if self._logmel_scratch is not None:
            self._logmel_scratch.argtypes = [C.c_int, C.c_int64] + [C.c_int] * 3
            self._logmel_scratch.restype = C.c_int64
        if self._patch_embed is not None:
            self._patch_embed.argtypes = [C.c_int] * 9 + [C.c_void_p] * 7 + [C.c_float] + [C.c_void_p] * 2
        # optional (include/dgsct.h): the parameter gradients of the patch embedding, for a trainable front end
        self._patch_embed_pws = getattr(c, "dgsct_patch_embed_params_ws_floats", None)
        self._patch_embed_bwd_params = getattr(c, "dgsct_patch_embed_backward_params", None)
        if self._patch_embed_pws is not None:
            self._patch_embed_pws.argtypes = [C.c_int] * 6
            self._patch_embed_pws.restype = C.c_int64
        if self._patch_embed_bwd_params is not None:
            self._patch_embed_bwd_params.argtypes = [C.c_int] * 9 + [C.c_void_p] * 8 + [C.c_float] + [C.c_void_p] * 8
        # optional (include/dgsct.h): the audio mode of both with SpecAugment stripes and mix-up folded into the loads
        self._patch_embed_aug = getattr(c, "dgsct_patch_embed_forward_aug", None)
        self._patch_embed_bwd_params_aug = getattr(c, "dgsct_patch_embed_backward_params_aug", None)
        if self._patch_embed_aug is not None:
            self._patch_embed_aug.argtypes = [C.c_int] * 4 + [C.c_void_p] * 9 + [C.c_float] + [C.c_void_p] * 2
        if self._patch_embed_bwd_params_aug is not None:
            self._patch_embed_bwd_params_aug.argtypes = [C.c_int] * 4 + [C.c_void_p] * 10 + [C.c_float] + [C.c_void_p] * 8
        # optional (include/dgsct.h): patch merging between two stages (csrc/pmerge.hip); the host emulation lacks it
        self._pmerge_ws = getattr(c, "dgsct_patch_merge_ws_bytes", None)
        self._pmerge_fwd = getattr(c, "dgsct_patch_merge_forward", None)
        self._pmerge_bwd = getattr(c, "dgsct_patch_merge_backward", None)
        if self._pmerge_ws is not None:
            self._pmerge_ws.argtypes = [C.c_int] * 5
            self._pmerge_ws.restype = C.c_int64
        if self._pmerge_fwd is not None:
            self._pmerge_fwd.argtypes = [C.c_int] * 5 + [C.c_void_p] * 4 + [C.c_float] + [C.c_void_p] * 5
        if self._pmerge_bwd is not None:
            self._pmerge_bwd.argtypes = [C.c_int] * 5 + [C.c_void_p] * 7 + [C.c_float] + [C.c_void_p] * 3
        # optional (include/dgsct.h): the merge's backward with parameter gradients, for a trainable merge
        self._pmerge_pws = getattr(c, "dgsct_patch_merge_params_ws_bytes", None)
        self._pmerge_bwd_params = getattr(c, "dgsct_patch_merge_backward_params", None)
        if self._pmerge_pws is not None:
            self._pmerge_pws.argtypes = [C.c_int] * 5
            self._pmerge_pws.restype = C.c_int64
        if self._pmerge_bwd_params is not None:
            self._pmerge_bwd_params.argtypes = [C.c_int] * 5 + [C.c_void_p] * 8 + [C.c_float] + [C.c_void_p] * 6
        # optional (include/dgsct.h): the live part of the CMBS event head (csrc/head.hip); the host emulation lacks it
        self._cmbs_ws = getattr(c, "dgsct_cmbs_head_ws_bytes", None)
        self._cmbs_fwd = getattr(c, "dgsct_cmbs_head_forward", None)
        self._cmbs_bwd = getattr(c, "dgsct_cmbs_head_backward", None)
        if self._cmbs_ws is not None:
            self._cmbs_ws.argtypes = [C.c_int] * 4
            self._cmbs_ws.restype = C.c_int64
        if self._cmbs_fwd is not None:
            self._cmbs_fwd.argtypes = [C.c_int] * 4 + [C.c_float] + [C.c_void_p] * 16
        if self._cmbs_bwd is not None:
            self._cmbs_bwd.argtypes = [C.c_int] * 4 + [C.c_float] + [C.c_void_p] * 23
        # optional (include/dgsct.h): the audio-visual TPAVI block in linear form (csrc/tpavi.hip); the host emulation lacks it
        self._tpavi_ws = getattr(c, "dgsct_tpavi_ws_bytes", None)
        self._tpavi_sum = getattr(c, "dgsct_tpavi_frame_sum", None)
        self._tpavi_fwd = getattr(c, "dgsct_tpavi_forward", None)
        self._tpavi_bwd = getattr(c, "dgsct_tpavi_backward", None)
        if self._tpavi_ws is not None:
            self._tpavi_ws.argtypes = [C.c_int] * 5
            self._tpavi_ws.restype = C.c_int64
        if self._tpavi_sum is not None:
            self._tpavi_sum.argtypes = [C.c_int] * 5 + [C.c_void_p] + [C.c_int64] * 3 + [C.c_void_p] * 2
        if self._tpavi_fwd is not None:
            self._tpavi_fwd.argtypes = ([C.c_int] * 5 + [C.c_void_p] + [C.c_int64] * 3 + [C.c_void_p] * 7 + [C.c_float] * 2 + [C.c_void_p] * 2
                                        + [C.c_float] + [C.c_void_p] + [C.c_int64] * 3 + [C.c_void_p] * 3)
        if self._tpavi_bwd is not None:
            self._tpavi_bwd.argtypes = ([C.c_int] * 5 + [C.c_void_p] + [C.c_int64] * 3 + [C.c_void_p] * 6 + [C.c_float] + [C.c_void_p]
                                        + [C.c_int64] * 3 + [C.c_void_p] * 2 + [C.c_int64] * 3 + [C.c_void_p] * 8)
        if c.dgsct_version() != 101:
            raise RuntimeError("dg-sct_amd: libdgsct version mismatch")

    # ------------------------------------------------------------------
    def _check(self, rc: int, what: str):
        if rc != 0:
            raise RuntimeError(f"{what} failed ({rc}): {self.c.dgsct_last_error().decode()}")

    def query(self, desc: AdapterDesc) -> Sizes:
        s = Sizes()
        self._check(self.c.dgsct_query(C.byref(desc), C.byref(s)), "dgsct_query")
        return s

    @staticmethod
    def ptr_table(ptrs: Sequence[Optional[int]]):
        arr = (C.c_void_p * P_COUNT)()
        for i, p in enumerate(ptrs):
            arr[i] = p if p else None
        return arr

    def prepare(self, desc, ptrs, prep: int, stream: int):
        self._check(self.c.dgsct_prepare(C.byref(desc), C.cast(ptrs, _PP), prep, stream), "dgsct_prepare")

    def forward(self, desc, ptrs, prep, X, Y, out, amap, tmap, saved, ws, stream, residual=None, aux_stream=None):
        self._check(self.c.dgsct_adapter_forward_ex(C.byref(desc), C.cast(ptrs, _PP), prep, X, Y, residual, out, amap, tmap,
                                                    saved, ws, stream, aux_stream), "dgsct_adapter_forward")

    def backward(self, desc, ptrs, prep, X, Y, saved, dOut, dMap, dTmap, dX, dY, grads, ws, stream, aux_stream=None,
                 skip_into_dx=False, no_join=False):
        flags = (1 if skip_into_dx else 0) | (2 if no_join else 0)       # DGSCT_BWD_SKIP_INTO_DX | DGSCT_BWD_NO_JOIN
        self._check(self.c.dgsct_adapter_backward_ex(C.byref(desc), C.cast(ptrs, _PP), prep, X, Y, saved, dOut, dMap, dTmap,
                                                     dX, dY, grads, ws, stream, aux_stream, flags),
                    "dgsct_adapter_backward")

    def backward_hold_dy(self, desc, ptrs, prep, X, Y, saved, dOut, dMap, dTmap, dX, grads, ws, stream, aux_stream=None,
                         skip_into_dx=False, no_join=False, dx_ready_event=None):
        """everything of the backward except the product that writes dY (DGSCT_BWD_HOLD_DY); `dx_ready_event` (raw hipEvent_t) is
        recorded on `stream` once dX is complete"""
        o = BwdOpts((BWD_SKIP_INTO_DX if skip_into_dx else 0) | (BWD_NO_JOIN if no_join else 0) | BWD_HOLD_DY, None, dx_ready_event, None)
        self._check(self.c.dgsct_adapter_backward_ex2(C.byref(desc), C.cast(ptrs, _PP), prep, X, Y, saved, dOut, dMap, dTmap,
                                                      dX, None, grads, ws, stream, aux_stream, C.byref(o)),
                    "dgsct_adapter_backward_ex2 (HOLD_DY)")

    def backward_only_dy(self, desc, ptrs, prep, dY, ws, stream, dy_residual=None, dy_wait_event=None):
        """the held-back product: dY = dy_residual + d adapter / dY, behind `dy_wait_event` (DGSCT_BWD_ONLY_DY)"""
        o = BwdOpts(BWD_ONLY_DY, dy_residual, None, dy_wait_event)
        self._check(self.c.dgsct_adapter_backward_ex2(C.byref(desc), C.cast(ptrs, _PP), prep, None, None, None, None, None, None,
                                                      None, dY, None, ws, stream, None, C.byref(o)),
                    "dgsct_adapter_backward_ex2 (ONLY_DY)")

    def saved_regions(self, desc):
        out = {}
        i = 0
        name = C.create_string_buffer(64)
        off, nb = C.c_int64(), C.c_int64()
        while self.c.dgsct_saved_region(C.byref(desc), i, name, 64, C.byref(off), C.byref(nb)) == 0:
            out[name.value.decode()] = (off.value, nb.value)
            i += 1
        return out

    def stream_create(self, priority_class: int) -> int:
        """raw hipStream_t in its own priority class (-1 high, 0 normal, +1 low) = its own hardware-queue pool"""
        out = C.c_void_p()
        self._check(self.c.dgsct_stream_create(int(priority_class), C.byref(out)), "dgsct_stream_create")
        return int(out.value or 0)

    def map_pool_forward(self, dtype: int, BT: int, N: int, C_: int, F: int, amap: int, pooled: int, stream: int):
        self._check(self.c.dgsct_map_pool_forward(dtype, BT, N, C_, F, amap, pooled, stream), "dgsct_map_pool_forward")

    def map_pool_backward(self, dtype: int, BT: int, N: int, C_: int, F: int, amap: int, dpooled: int, dF, dmap, stream: int):
        self._check(self.c.dgsct_map_pool_backward(dtype, BT, N, C_, F, amap, dpooled, dF, dmap, stream), "dgsct_map_pool_backward")

    def window_attn_forward(self, geom, qkv, bm, scale, out, lse, stream, flags=0):
        """geom = (B, H, W, ws, shift, heads, hd, nwm); pointers as ints; flags: WATTN_COSINE (include/dgsct.h: dgsct_window_attn_forward_ex)"""
        self._check(self.c.dgsct_window_attn_forward_ex(*geom, flags, qkv, bm, scale, out, lse, stream), "dgsct_window_attn_forward")

    def window_attn_backward(self, geom, qkv, bm, scale, out, lse, dout, dqkv, stream, flags=0):
        self._check(self.c.dgsct_window_attn_backward_ex(*geom, flags, qkv, bm, scale, out, lse, dout, dqkv, stream), "dgsct_window_attn_backward")

    @property
    def has_window_attn_tables(self) -> bool:
        """whether this library exports dgsct_window_attn_backward_tables (bias-table / logit-scale gradients of trainable blocks)"""
        return self._wattn_tables is not None

    def window_attn_backward_tables(self, geom, qkv, bm, scale, out, lse, dout, dqkv, dbm, dscale, stream, flags=0):
        """dqkv as window_attn_backward, plus dbm [nwm, heads, n, n] / dscale [heads] (fp32, zeroed by the call; None = not wanted)"""
        if self._wattn_tables is None:
            raise RuntimeError(f"dg-sct_amd: {self.path} does not export dgsct_window_attn_backward_tables")
        self._check(self._wattn_tables(*geom, flags, qkv, bm, scale, out, lse, dout, dqkv, dbm, dscale, stream),
                    "dgsct_window_attn_backward_tables")

    def _front_end(self, fn, name: str):
        if fn is None:
            raise RuntimeError(f"dg-sct_amd: {self.path} does not export {name} (a library without the audio / image front end)")
        return fn

    def logmel_scratch_floats(self, B: int, L: int, n_fft: int = 1024, hop: int = 320, n_mels: int = 64) -> int:
        n = self._front_end(self._logmel_scratch, "dgsct_logmel_scratch_floats")(B, L, n_fft, hop, n_mels)
        if n < 0:
            raise RuntimeError(f"dgsct_logmel_scratch_floats failed: {self.c.dgsct_last_error().decode()}")
        return int(n)

    def logmel_forward(self, B, L, waveform, melW, ranges, out, stats, scratch, stream, n_fft: int = 1024, hop: int = 320, n_mels: int = 64):
        """pointers as ints; ranges / stats / scratch may be None (include/dgsct.h: dgsct_logmel_forward)"""
        self._check(self._front_end(self._logmel, "dgsct_logmel_forward")(B, L, n_fft, hop, n_mels, waveform, melW, ranges, out, stats,
                                                                           scratch, stream), "dgsct_logmel_forward")

    def patch_embed_forward(self, mode, in_dtype, out_dtype, B, in_chans, H, W, T, C_, x, bn_scale, bn_shift, w, b, ln_w, ln_b, eps, out, stream):
        """mode: PATCH_IMAGE | PATCH_AUDIO (include/dgsct.h: dgsct_patch_embed_forward)"""
        self._check(self._front_end(self._patch_embed, "dgsct_patch_embed_forward")(mode, in_dtype, out_dtype, B, in_chans, H, W, T, C_, x,
                                                                                     bn_scale, bn_shift, w, b, ln_w, ln_b, eps, out, stream),
                    "dgsct_patch_embed_forward")

    def has_patch_embed_params(self) -> bool:
        """whether this library exports dgsct_patch_embed_backward_params / dgsct_patch_embed_params_ws_floats (the gradients of
        `patch_embed.*` and `bn0.*`, for a trainable front end) on top of dgsct_patch_embed_forward"""
        return None not in (self._patch_embed, self._patch_embed_pws, self._patch_embed_bwd_params)

    def patch_embed_params_ws_floats(self, mode: int, B: int, in_chans: int, H: int, W: int, C_: int) -> int:
        n = self._front_end(self._patch_embed_pws, "dgsct_patch_embed_params_ws_floats")(mode, B, in_chans, H, W, C_)
        if n < 0:
            raise RuntimeError(f"dgsct_patch_embed_params_ws_floats failed: {self.c.dgsct_last_error().decode()}")
        return int(n)

    def patch_embed_backward_params(self, mode, in_dtype, dout_dtype, B, in_chans, H, W, T, C_, x, bn_scale, bn_shift, bn_pivot, w, b, ln_w, ln_b,
                                    eps, dout, dw, db, dln_w, dln_b, dbn, ws, stream):
        """dw [C, in_chans, 4, 4], db / dln_w / dln_b [C], audio mode: dbn [2, 64] = (g1, g0); all fp32 and all written by the call
        (include/dgsct.h: dgsct_patch_embed_backward_params)"""
        self._check(self._front_end(self._patch_embed_bwd_params, "dgsct_patch_embed_backward_params")(
            mode, in_dtype, dout_dtype, B, in_chans, H, W, T, C_, x, bn_scale, bn_shift, bn_pivot, w, b, ln_w, ln_b, eps, dout, dw, db, dln_w,
            dln_b, dbn, ws, stream), "dgsct_patch_embed_backward_params")

    def has_patch_embed_aug(self) -> bool:
        """whether this library exports dgsct_patch_embed_forward_aug / dgsct_patch_embed_backward_params_aug (audio mode with the
        SpecAugment stripes and the mix-up inside the kernels) on top of the parameter-gradient backward"""
        return self.has_patch_embed_params() and None not in (self._patch_embed_aug, self._patch_embed_bwd_params_aug)

    def patch_embed_forward_aug(self, out_dtype, B, T, C_, logmel, bn_scale, bn_shift, stripes, lam, w, b, ln_w, ln_b, eps, out, stream):
        """stripes int32 [B, 4, 2] / lam fp32 [B] device pointers or None (include/dgsct.h: dgsct_patch_embed_forward_aug)"""
        self._check(self._front_end(self._patch_embed_aug, "dgsct_patch_embed_forward_aug")(
            out_dtype, B, T, C_, logmel, bn_scale, bn_shift, stripes, lam, w, b, ln_w, ln_b, eps, out, stream), "dgsct_patch_embed_forward_aug")

    def patch_embed_backward_params_aug(self, dout_dtype, B, T, C_, logmel, bn_scale, bn_shift, bn_pivot, stripes, lam, w, b, ln_w, ln_b, eps,
                                        dout, dw, db, dln_w, dln_b, dbn, ws, stream):
        """the outputs and the workspace of `patch_embed_backward_params` in audio mode (include/dgsct.h: dgsct_patch_embed_backward_params_aug)"""
        self._check(self._front_end(self._patch_embed_bwd_params_aug, "dgsct_patch_embed_backward_params_aug")(
            dout_dtype, B, T, C_, logmel, bn_scale, bn_shift, bn_pivot, stripes, lam, w, b, ln_w, ln_b, eps, dout, dw, db, dln_w, dln_b, dbn, ws,
            stream), "dgsct_patch_embed_backward_params_aug")

    @property
    def has_patch_merge(self) -> bool:
        """whether this library exports dgsct_patch_merge_* (csrc/pmerge.hip)"""
        return None not in (self._pmerge_ws, self._pmerge_fwd, self._pmerge_bwd)

    def _pmerge(self, fn, name: str):
        if fn is None:
            raise RuntimeError(f"dg-sct_amd: {self.path} does not export {name} (a library without patch merging)")
        return fn

    def patch_merge_ws_bytes(self, mode: int, B: int, H: int, W: int, C_: int) -> int:
        n = self._pmerge(self._pmerge_ws, "dgsct_patch_merge_ws_bytes")(mode, B, H, W, C_)
        if n < 0:
            raise RuntimeError(f"dgsct_patch_merge_ws_bytes failed: {self.c.dgsct_last_error().decode()}")
        return int(n)

    def patch_merge_forward(self, mode, B, H, W, C_, x, w_bf16, ln_w, ln_b, eps, out, pre, mu, rstd, stream):
        """pointers as ints; pre: NORM_LAST only, else None (include/dgsct.h: dgsct_patch_merge_forward)"""
        self._check(self._pmerge(self._pmerge_fwd, "dgsct_patch_merge_forward")(mode, B, H, W, C_, x, w_bf16, ln_w, ln_b, eps, out, pre, mu,
                                                                                 rstd, stream), "dgsct_patch_merge_forward")

    def patch_merge_backward(self, mode, B, H, W, C_, dout, x, w_bf16, ln_w, pre, mu, rstd, eps, dx, ws, stream):
        self._check(self._pmerge(self._pmerge_bwd, "dgsct_patch_merge_backward")(mode, B, H, W, C_, dout, x, w_bf16, ln_w, pre, mu, rstd, eps,
                                                                                  dx, ws, stream), "dgsct_patch_merge_backward")

    def has_patch_merge_params(self) -> bool:
        """whether this library exports dgsct_patch_merge_backward_params / dgsct_patch_merge_params_ws_bytes (the weight and norm gradients
        of a trainable merge) on top of dgsct_patch_merge_*"""
        return self.has_patch_merge and None not in (self._pmerge_pws, self._pmerge_bwd_params)

    def patch_merge_params_ws_bytes(self, mode: int, B: int, H: int, W: int, C_: int) -> int:
        n = self._pmerge(self._pmerge_pws, "dgsct_patch_merge_params_ws_bytes")(mode, B, H, W, C_)
        if n < 0:
            raise RuntimeError(f"dgsct_patch_merge_params_ws_bytes failed: {self.c.dgsct_last_error().decode()}")
        return int(n)

    def patch_merge_backward_params(self, mode, B, H, W, C_, dout, x, w_bf16, ln_w, ln_b, pre, mu, rstd, eps, dx, dw, dln_w, dln_b, ws, stream):
        """dx as patch_merge_backward (bit for bit) + dw [2C, 4C] / dln_w / dln_b in fp32, zeroed by the call; NORM_LAST needs x AND pre
        (include/dgsct.h: dgsct_patch_merge_backward_params)"""
        self._check(self._pmerge(self._pmerge_bwd_params, "dgsct_patch_merge_backward_params")(
            mode, B, H, W, C_, dout, x, w_bf16, ln_w, ln_b, pre, mu, rstd, eps, dx, dw, dln_w, dln_b, ws, stream), "dgsct_patch_merge_backward_params")

    def has_cmbs_head(self) -> bool:
        """whether this library exports dgsct_cmbs_head_forward / _backward / _ws_bytes (csrc/head.hip)"""
        return None not in (self._cmbs_ws, self._cmbs_fwd, self._cmbs_bwd)

    def _cmbs(self, fn, name: str):
        if fn is None:
            raise RuntimeError(f"dg-sct_amd: {self.path} does not export {name} (a library without the CMBS event head)")
        return fn

    def cmbs_head_ws_bytes(self, T: int, B: int, D: int, K: int) -> int:
        n = self._cmbs(self._cmbs_ws, "dgsct_cmbs_head_ws_bytes")(T, B, D, K)
        if n < 0:
            raise RuntimeError(f"dgsct_cmbs_head_ws_bytes failed: {self.c.dgsct_last_error().decode()}")
        return int(n)

    def cmbs_head_forward(self, T, B, D, K, gamma, v, a, Wvc, bvc, Wac, bac, wc, bc, We, be, is_event, event, av, topmask, argmax, stream):
        """pointers as ints (include/dgsct.h: dgsct_cmbs_head_forward)"""
        self._check(self._cmbs(self._cmbs_fwd, "dgsct_cmbs_head_forward")(T, B, D, K, gamma, v, a, Wvc, bvc, Wac, bac, wc, bc, We, be, is_event,
                                                                          event, av, topmask, argmax, stream), "dgsct_cmbs_head_forward")

    def cmbs_head_backward(self, T, B, D, K, gamma, v, a, Wvc, Wac, wc, We, topmask, argmax, d_is, d_ev, d_av, dv, da, grads, ws, stream):
        """grads: the eight gradient pointers (dWvc, dbvc, dWac, dbac, dwc, dbc, dWe, dbe) or None for a frozen head; cotangents, dv / da
        and ws may be None (include/dgsct.h: dgsct_cmbs_head_backward)"""
        grads = tuple(grads) if grads is not None else (None,) * 8
        self._check(self._cmbs(self._cmbs_bwd, "dgsct_cmbs_head_backward")(T, B, D, K, gamma, v, a, Wvc, Wac, wc, We, topmask, argmax, d_is, d_ev,
                                                                           d_av, dv, da, *grads, ws, stream), "dgsct_cmbs_head_backward")

    def has_tpavi(self) -> bool:
        """whether this library exports dgsct_tpavi_frame_sum / _forward / _backward / _ws_bytes (csrc/tpavi.hip)"""
        return None not in (self._tpavi_ws, self._tpavi_sum, self._tpavi_fwd, self._tpavi_bwd)

    def _tpavi(self, fn, name: str):
        if fn is None:
            raise RuntimeError(f"dg-sct_amd: {self.path} does not export {name} (a library without the TPAVI kernels)")
        return fn

    def tpavi_ws_bytes(self, B: int, C_: int, T: int, H: int, W: int) -> int:
        n = self._tpavi(self._tpavi_ws, "dgsct_tpavi_ws_bytes")(B, C_, T, H, W)
        if n < 0:
            raise RuntimeError(f"dgsct_tpavi_ws_bytes failed: {self.c.dgsct_last_error().decode()}")
        return int(n)

    def tpavi_frame_sum(self, dims, x, xs, s, stream):
        """dims (B, C, T, H, W); xs the element strides of (b, c, t); pointers as ints (include/dgsct.h: dgsct_tpavi_frame_sum)"""
        self._check(self._tpavi(self._tpavi_sum, "dgsct_tpavi_frame_sum")(*dims, x, *xs, s, stream), "dgsct_tpavi_frame_sum")

    def tpavi_forward(self, dims, x, xs, A, c, mu0, bn_w, bn_b, run_mean, run_var, momentum, bn_eps, ln_w, ln_b, ln_eps, z, zs, stat, ws, stream):
        """mu0 None: no BatchNorm inside (eval: the caller folded it into A, c); then bn_*, run_*, stat, ws may be None
        (include/dgsct.h: dgsct_tpavi_forward)"""
        self._check(self._tpavi(self._tpavi_fwd, "dgsct_tpavi_forward")(*dims, x, *xs, A, c, mu0, bn_w, bn_b, run_mean, run_var, momentum, bn_eps,
                                                                        ln_w, ln_b, ln_eps, z, *zs, stat, ws, stream), "dgsct_tpavi_forward")

    def tpavi_backward(self, dims, x, xs, A, c, stat, bn_w, bn_b, ln_w, ln_eps, dz, gs, ds, dx, dxs, dA, dc, dbn_w, dbn_b, dln_w, dln_b, ws, stream):
        """stat None: no BatchNorm inside; then bn_*, dbn_* may be None; ds may be None (include/dgsct.h: dgsct_tpavi_backward)"""
        self._check(self._tpavi(self._tpavi_bwd, "dgsct_tpavi_backward")(*dims, x, *xs, A, c, stat, bn_w, bn_b, ln_w, ln_eps, dz, *gs, ds, dx, *dxs,
                                                                         dA, dc, dbn_w, dbn_b, dln_w, dln_b, ws, stream), "dgsct_tpavi_backward")

    def layer_norm_forward(self, dtype, rows, C_, x, w, b, eps, residual, out, mu, rstd, stream):
        self._check(self.c.dgsct_layer_norm_forward(dtype, rows, C_, x, w, b, eps, residual, out, mu, rstd, stream), "dgsct_layer_norm_forward")

    def layer_norm_backward(self, dtype, rows, C_, dout, x, w, b, mu, rstd, eps, dx, dw, db, scratch, stream):
        self._check(self.c.dgsct_layer_norm_backward(dtype, rows, C_, dout, x, w, b, mu, rstd, eps, dx, dw, db, scratch, stream),
                    "dgsct_layer_norm_backward")

    def prof_enable(self, on: bool):
        self.c.dgsct_prof_enable(int(on))

    def prof_collect(self):
        n, ms, fl = C.c_int64(), C.c_double(), C.c_double()
        self.c.dgsct_prof_collect(C.byref(n), C.byref(ms), C.byref(fl))
        return n.value, ms.value, fl.value

    def frame_scale_forward(self, dtype, rows, inner, gamma, x, g, y, stream):
        self._check(self.c.dgsct_frame_scale_forward(dtype, rows, inner, gamma, x, g, y, stream), "dgsct_frame_scale_forward")

    def frame_scale_backward(self, dtype, rows, inner, gamma, x, g, dy, dx, dg, stream):
        self._check(self.c.dgsct_frame_scale_backward(dtype, rows, inner, gamma, x, g, dy, dx, dg, stream), "dgsct_frame_scale_backward")

    def temporal_gate_forward(self, R, D, gamma, *ptrs):
        self._check(self.c.dgsct_temporal_gate_forward(R, D, gamma, *ptrs), "dgsct_temporal_gate_forward")

    def temporal_gate_backward(self, R, D, gamma, *ptrs):
        self._check(self.c.dgsct_temporal_gate_backward(R, D, gamma, *ptrs), "dgsct_temporal_gate_backward")

    def test_gemm_fp8(self, M, N, K, A, W, bias, relu, D, w8, scale, stream):
        self._check(self.c.dgsct_test_gemm_fp8(M, N, K, A, W, bias, int(relu), D, w8, scale, stream), "dgsct_test_gemm_fp8")

    def test_attn(self, op: int, args: "AttnArgs", stream: int):
        self._check(self.c.dgsct_test_attn(int(op), C.byref(args), stream), "dgsct_test_attn")

    def test_tune(self, key: str, value: int) -> int:
        return int(self.c.dgsct_test_tune(key.encode(), int(value)))

    def test_gemm(self, args: GemmArgs, stream: int):
        self._check(self.c.dgsct_test_gemm(C.byref(args), stream), "dgsct_test_gemm")


_DEFAULT: Optional[Lib] = None


def default_lib() -> Lib:
    """The product library (hand-written gfx950 kernels).  Raises if it has not been built."""
    global _DEFAULT
    if _DEFAULT is None:
        _DEFAULT = Lib(LIB_PATH)
    return _DEFAULT
