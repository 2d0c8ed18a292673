"""What carries a token map from one stage of the layer loop to the next: the backbones' 2 x 2 patch merging
(``f_v = my_blk.downsample(f_v)`` / ``f_a = htsat_blk.downsample(f_a)``, DG-SCT/AVE/nets/net_trans.py:914-916), and the trunk that chains the
four stages so that a loss on the last stage's output trains the adapters of the first (``:880-924``).

    HTSATPatchMerging   ``PatchMerging`` of htsat.py:259-295:         reduction(norm(gather(x))),  norm = LayerNorm(4 dim)
    SwinV2PatchMerging  timm 0.6.12 ``swin_transformer_v2.PatchMerging``: norm(reduction(gather(x))),  norm = LayerNorm(2 dim)
    AVETrunk            AdapterStack (chained) + FrozenBlocks + the merges + ``swin.norm`` + the two map poolings

``gather`` puts the tokens (2i, 2j), (2i+1, 2j), (2i, 2j+1), (2i+1, 2j+1) of a map side by side (the reference's x0 | x1 | x2 | x3);
``reduction = Linear(4 dim, 2 dim, bias=False)``; state_dict keys ``reduction.weight``, ``norm.weight``, ``norm.bias`` in both.

The HIP path (csrc/pmerge.hip: one launch forward for HTS-AT, two for Swin-V2, two backward, the [rows, 4 dim] concatenation never written
by a forward) takes bf16 GPU maps inside the kernel's limits -- H, W even, dim a multiple of 32, 4 dim <= 1536 (HTS-AT) / 2 dim <= 1536
(Swin-V2).  ``fused=True`` selects it and raises on anything it does not take (a trainable parameter without ``weight_grads=True`` included); ``fused=False`` is the
ATen formulation (the one pinned to the reference on the CPU); ``fused=None`` takes the kernels only at the shapes where they have been
measured faster than ATen in both directions (``_KERNELS_FASTER``, from profiles/patch_merging_bench.txt: seven of the nine merges of
the AVE trunk at the Swin-V2-B / -L widths; the two widest last merges lose their forward and stay ATen) and ATen at every other shape,
unmeasured ones included; ``fused=True`` is the opt-in to the kernels anywhere inside the limits.

A merge with a parameter that requires grad (AVS-S4 trains HTS-AT): **the kernels return weight gradients only on request**,
``weight_grads=True``.  Without the keyword such a merge takes the ATen formulation under ``fused=None`` and raises under ``fused=True``,
as before.  With it, ``fused=True`` runs the kernels with ``dgsct_patch_merge_backward_params`` as the backward (dx bit for bit the frozen
path's, plus ``reduction.weight`` / ``norm.weight`` / ``norm.bias`` gradients accumulated in fp32 and returned in each parameter's dtype:
fp32 masters get fp32 gradients) and raises when the library lacks that export; ``fused=None`` takes them only at the shapes of
``_KERNELS_FASTER_TRAIN`` (profiles/patch_merging_train_bench.txt: the first two HTS-AT merges) and ATen elsewhere; ``fused=False`` is ATen.  The Swin-V2 form then
keeps the stage map alive until backward as well as the product before the norm (the weight gradient re-gathers its operand).  A frozen
merge is unaffected by the keyword.

Parity: ``HTSATPatchMerging`` is pinned against the reference class and ``SwinV2PatchMerging`` against Hugging Face transformers'
``Swinv2PatchMerging`` (tools/make_golden_patch_merging.py -> tests/golden/ref_patch_merging.pt); **parity against timm itself stays
unpinned** (timm is not installed here)."""
from __future__ import annotations

import math
from typing import Dict, Optional, Sequence, Tuple

import torch
import torch.nn as nn

from . import ops
from .backbone import FrozenBlocks, _linear, _ln, _norm
from .stack import AdapterStack

# Where fused=None takes the kernels: the (mode, map tokens H*W, dim) at which tools/patch_merging_bench.py has MEASURED them faster than
# the ATen formulation on an MI355X in BOTH directions (profiles/patch_merging_bench.txt, BT = 160).  Every other shape -- an unmeasured
# one included -- goes to ATen under fused=None; fused=True is the opt-in to the kernels at any supported shape.  Measured and NOT
# listed, because the forward loses there (0.41 x / 0.86 x of ATen's speed): the last audio merge 16^2 x 384 and the last Swin-V2-L
# merge 12^2 x 768.
_KERNELS_FASTER: frozenset = frozenset({
    (ops.PMERGE_NORM_FIRST, 4096, 96), (ops.PMERGE_NORM_FIRST, 1024, 192),                                          # HTS-AT stages 0, 1
    (ops.PMERGE_NORM_LAST, 2304, 128), (ops.PMERGE_NORM_LAST, 576, 256), (ops.PMERGE_NORM_LAST, 144, 512),          # Swin-V2-B stages 0 - 2
    (ops.PMERGE_NORM_LAST, 2304, 192), (ops.PMERGE_NORM_LAST, 576, 384),                                            # Swin-V2-L stages 0, 1
})

# The same for a TRAINABLE merge with weight_grads=True (forward + backward with parameter gradients together): the shapes at which
# `tools/patch_merging_bench.py --train` measured the kernels' slowest window faster than the fastest window of the formulation
# AVETrunk(train_htsat=True) runs without the keyword (fp32 masters through ATen); profiles/patch_merging_train_bench.txt, BT = 160:
# 411 against 1822 us and 302 against 778 us.  The last audio merge (256 tokens x 384: 469 against 476 us, the windows overlap, the
# forward alone loses) is NOT listed and stays ATen under fused=None.
_KERNELS_FASTER_TRAIN: frozenset = frozenset({(ops.PMERGE_NORM_FIRST, 4096, 96), (ops.PMERGE_NORM_FIRST, 1024, 192)})


def gather_2x2(x: torch.Tensor, H: int, W: int) -> torch.Tensor:
    """[B, H*W, C] -> [B, (H/2)(W/2), 4C]: the reference's four strided slices and their cat (== view(B,H/2,2,W/2,2,C).permute(0,1,3,4,2,5))"""
    B, L, C = x.shape
    x = x.view(B, H, W, C)
    x = torch.cat([x[:, 0::2, 0::2, :], x[:, 1::2, 0::2, :], x[:, 0::2, 1::2, :], x[:, 1::2, 1::2, :]], -1)
    return x.view(B, -1, 4 * C)


class _PatchMerging(nn.Module):
    _MODE = -1
    _NORM_MULT = 0

    def __init__(self, input_resolution: Tuple[int, int], dim: int, fused: Optional[bool] = None, lib=None, weight_grads: bool = False):
        super().__init__()
        self.input_resolution, self.dim = tuple(input_resolution), dim
        self.fused, self._lib, self.weight_grads = fused, lib, bool(weight_grads)
        self.reduction = nn.Linear(4 * dim, 2 * dim, bias=False)
        self.norm = nn.LayerNorm(self._NORM_MULT * dim)

    def _cached(self):
        """(reduction.weight in bf16, norm.weight / norm.bias in fp32), remade when a parameter changes (as backbone._ln)"""
        ps = (self.reduction.weight, self.norm.weight, self.norm.bias)
        key = (tuple((p._version, p.dtype, p.data_ptr()) for p in ps), ps[0].device)       # (.to(dtype) bumps no version: dtype and storage too)
        c = self.__dict__.get("_fused_params")
        if c is None or c[0] != key:
            with torch.no_grad():
                c = self.__dict__["_fused_params"] = (key, ps[0].detach().to(torch.bfloat16).contiguous(), ps[1].detach().float().contiguous(),
                                                      ps[2].detach().float().contiguous())
        return c[1:]

    def _supported(self, x: torch.Tensor) -> bool:
        """the kernels take x; ``fused=True`` raises where they do not"""
        H, W = self.input_resolution
        ok = ops.patch_merge_supported(x, H, W, self._MODE) and x.device == self.reduction.weight.device
        if self.fused and not ok:
            raise RuntimeError(f"dg-sct_amd: {type(self).__name__}(fused=True) takes bf16 CUDA/HIP maps with dim a multiple of 32 and "
                               f"{self._NORM_MULT} dim <= 1536 (got {tuple(x.shape)} {x.dtype} on "
                               f"{x.device}; fused=False is the ATen formulation)")
        return ok

    def _use_fused(self, x: torch.Tensor) -> bool:
        """a FROZEN merge (no parameter requires grad, or grad mode is off)"""
        if self.fused is False:
            return False
        H, W = self.input_resolution
        if self.fused is None and (self._MODE, H * W, self.dim) not in _KERNELS_FASTER:
            return False
        return self._supported(x)

    def _use_fused_train(self, x: torch.Tensor) -> bool:
        """a TRAINABLE merge: the kernels only with ``weight_grads=True``, and under ``fused=None`` only at the measured shapes"""
        if self.fused is False:
            return False
        H, W = self.input_resolution
        if not self.weight_grads:
            if self.fused and self._supported(x):
                raise RuntimeError(f"dg-sct_amd: {type(self).__name__}(fused=True): a parameter requires grad and without weight_grads=True "
                                   f"the kernels return the input gradient only (pass weight_grads=True, freeze the module, or "
                                   f"fused=None / False for the ATen formulation)")
            return False                                   # dx only without the keyword
        if self.fused is None and (self._MODE, H * W, self.dim) not in _KERNELS_FASTER_TRAIN:
            return False
        lib = self._lib or ops._lib.default_lib()
        if not lib.has_patch_merge_params():
            if self.fused:
                raise RuntimeError(f"dg-sct_amd: {type(self).__name__}(fused=True, weight_grads=True): {lib.path} does not export "
                                   f"dgsct_patch_merge_backward_params (fused=None / False for the ATen formulation)")
            return False
        return self._supported(x)

    def _aten(self, g: torch.Tensor) -> torch.Tensor:
        raise NotImplementedError

    def forward(self, x: torch.Tensor) -> torch.Tensor:
        """x: [B, H*W, C] -> [B, (H/2)(W/2), 2C]"""
        H, W = self.input_resolution
        B, L, C = x.shape
        assert L == H * W, "input feature has wrong size"
        assert H % 2 == 0 and W % 2 == 0, f"x size ({H}*{W}) are not even."
        if torch.is_grad_enabled() and any(p.requires_grad for p in self.parameters()):
            if self._use_fused_train(x):
                return ops._patch_merge_train(x, self.reduction.weight, self.norm.weight, self.norm.bias, self.norm.eps, H, W, self._MODE,
                                              self._lib, self._cached())
        elif self._use_fused(x):
            w, ln_w, ln_b = self._cached()
            return ops.patch_merge(x, w, ln_w, ln_b, self.norm.eps, H, W, self._MODE, self._lib)
        return self._aten(gather_2x2(x, H, W))

    def extra_repr(self):
        return f"input_resolution={self.input_resolution}, dim={self.dim}"


class HTSATPatchMerging(_PatchMerging):
    """``PatchMerging`` of htsat.py:259-295: ``reduction(norm(cat(x0, x1, x2, x3)))`` with ``norm = LayerNorm(4 dim)``.  Fused: one launch
    forward (csrc/pmerge.hip, DGSCT_PMERGE_NORM_FIRST), two backward, dx only -- with a trainable parameter fused=None is ATen and fused=True
    raises, unless ``weight_grads=True`` asks for the backward that also returns the three parameter gradients (module docstring)."""
    _MODE = ops.PMERGE_NORM_FIRST
    _NORM_MULT = 4

    def _aten(self, g):
        return _linear(self.reduction, _norm(self.norm, g))


class SwinV2PatchMerging(_PatchMerging):
    """timm 0.6.12 ``swin_transformer_v2.PatchMerging`` as the AVE loop calls it: ``norm(reduction(cat(x0, x1, x2, x3)))`` with
    ``norm = LayerNorm(2 dim)``.  Fused: two launches each way (DGSCT_PMERGE_NORM_LAST), dx only -- with a trainable parameter fused=None is
    ATen and fused=True raises, unless ``weight_grads=True`` (which keeps the input map alive until backward as well as the product before
    the norm).  Parity against timm unpinned (see the module docstring)."""
    _MODE = ops.PMERGE_NORM_LAST
    _NORM_MULT = 2

    def _aten(self, g):
        return _norm(self.norm, _linear(self.reduction, g))


class _ChainedStack(AdapterStack):
    """AdapterStack whose layer loop carries ONE pair of maps through all stages: ``feats[0]`` enters stage 0, and the merges of the owning
    trunk take what leaves a stage into the next (net_trans.py:914-916; the last stage has no downsample)."""

    def _layers(self, feats, step, outs, maps):
        vis_merge, aud_merge = self._merges
        f_v, f_a = feats[0]
        idx = 0
        for s, st in enumerate(self.stages):
            for _ in range(st["layers"]):
                f_a, f_v, _, _ = step(self.audio_adapter_blocks_p1[idx], self.vis_adapter_blocks_p1[idx], f_a, f_v, idx, 0, True)
                f_a, f_v, a_map, v_map = step(self.audio_adapter_blocks_p2[idx], self.vis_adapter_blocks_p2[idx], f_a, f_v, idx, 1, False)
                maps = (v_map, a_map)
                idx += 1
            outs.append((f_v, f_a))
            if s + 1 < len(self.stages):
                f_v = vis_merge[s](f_v)
                f_a = aud_merge[s](f_a)
        return outs, maps


class AVETrunk(nn.Module):
    """The trunk of the AVE model between the front ends and the temporal head (net_trans.py:880-924): the adapter / frozen-block loop of
    every stage, patch merging between the stages, ``swin.norm`` on the last visual map and the two spatial-map poolings.

    ``forward(f_v [BT, Nv0, Cv0], f_a [BT, Na0, Ca0])`` (the stage-0 tokens of ``PatchEmbed`` / ``HTSATFrontEnd``) returns
    ``(pooled_v [BT, 1, Cv_last], pooled_a [BT, 1, Ca_last], outs, maps)``: outs[s] = (f_v, f_a) leaving stage s (before its merge and before
    ``norm``), maps = (map_v, map_a) of the last p2 adapters.  Sub-modules: ``stack`` (the adapters, the only trainable part), ``blocks``
    (FrozenBlocks), ``vis_merge`` / ``aud_merge`` (one per stage boundary, frozen like the blocks; ``train_htsat=True`` keeps the audio
    merges fp32 masters and trainable, which sends them down the ATen formulation unless ``merge_weight_grads=True`` hands them
    ``weight_grads=True``: see the module docstring; the Swin-V2 merges are frozen in every reference task and never get it), ``norm``.  ``stack_kw`` goes to AdapterStack (``lib=``,
    ``concurrent=``, ...).  Consecutive stages must quarter the tokens and double the width.  CPU tensors are taken only with ``lib=`` (the
    host emulation of the adapter kernels): that path exists for the tests."""

    def __init__(self, stages: Sequence[Dict[str, int]], opt=None, dtype: torch.dtype = torch.bfloat16, fused: Optional[bool] = None,
                 train_htsat: bool = False, merge_weight_grads: bool = False, **stack_kw):
        super().__init__()
        stages = [dict(s) for s in stages]
        for s, (a, b) in enumerate(zip(stages[:-1], stages[1:])):
            for n, c, who in (("Nv", "Cv", "visual"), ("Na", "Ca", "audio")):
                if a[n] != 4 * b[n] or b[c] != 2 * a[c]:
                    raise ValueError(f"dg-sct_amd: AVETrunk: {who} stage {s + 1} must have a quarter of the tokens and twice the width of stage "
                                     f"{s} (got {a[n]} x {a[c]} -> {b[n]} x {b[c]})")
        for s in stages:
            for n in ("Nv", "Na"):
                if int(round(math.sqrt(s[n]))) ** 2 != s[n]:
                    raise ValueError(f"dg-sct_amd: AVETrunk: the maps are square; {n} = {s[n]} is no square number")
        stack_kw.setdefault("compute_dtype", dtype)
        self._lib = stack_kw.get("lib")
        self.stack = _ChainedStack(stages, opt, **stack_kw)
        self.blocks = FrozenBlocks(stages, dtype=dtype, fused=fused, train_htsat=train_htsat)
        side = lambda n: int(round(math.sqrt(n)))             # noqa: E731
        self.vis_merge = nn.ModuleList([SwinV2PatchMerging((side(s["Nv"]),) * 2, s["Cv"], fused=fused, lib=self._lib) for s in stages[:-1]])
        self.aud_merge = nn.ModuleList([HTSATPatchMerging((side(s["Na"]),) * 2, s["Ca"], fused=fused, lib=self._lib, weight_grads=merge_weight_grads)
                                        for s in stages[:-1]])
        self.norm = nn.LayerNorm(stages[-1]["Cv"])
        self.vis_merge.to(dtype)
        self.norm.to(dtype)
        self.aud_merge.to(torch.float32 if train_htsat else dtype)
        for m in (self.vis_merge, self.norm):
            m.requires_grad_(False)
        self.aud_merge.requires_grad_(bool(train_htsat))
        object.__setattr__(self.stack, "_merges", (self.vis_merge, self.aud_merge))      # a plain attribute: the trunk owns the modules

    def _final_norm(self, f_v: torch.Tensor) -> torch.Tensor:
        if (f_v.is_cuda or self._lib is not None) and ops.layer_norm_supported(f_v):
            return _ln(self.norm, f_v, None, self._lib)
        return _norm(self.norm, f_v)

    def _pool(self, f: torch.Tensor, amap: torch.Tensor) -> torch.Tensor:
        if not f.is_cuda and self._lib is None:
            raise RuntimeError("dg-sct_amd: AVETrunk needs CUDA/HIP tensors (CPU tensors only with lib=, the host emulation of the tests)")
        return ops.map_pool(f, amap, self._lib)

    def forward(self, f_v: torch.Tensor, f_a: torch.Tensor):
        outs, maps = self.stack([(f_v, f_a)], vis_block=self.blocks.vis_block_map, aud_block=self.blocks.aud_block)
        f_v, f_a = outs[-1]
        f_v = self._final_norm(f_v)
        return self._pool(f_v, maps[0]), self._pool(f_a, maps[1]), outs, maps
