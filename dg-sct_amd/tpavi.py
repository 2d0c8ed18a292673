"""Drop-in ``TPAVIModule`` -- the audio-visual attention block the AVS decoder runs once per scale (``Pred_endecoder.tpavi_va``).

Mirrors reference ``DG-SCT/AVS/avs_scripts/avs_s4/model/TPAVI.py``: the same constructor signature, the same sub-modules built in the same
order (``align_channel``, ``norm_layer``, ``g``, ``W_z`` = Conv3d + BatchNorm3d with weight and bias 0, ``theta``, ``phi``; the Conv3d
weights stay 5-D) -- hence the same ``state_dict`` keys in the same order and, under one seed, the same parameter values.
``avs_ms3/model/TPAVI.py`` is the same file byte for byte, so this class serves both AVS tasks.  Only what the AVS models build is
supported: ``mode='dot'`` and ``dimension=3``; anything else raises ``NotImplementedError``.

What is computed.  The reference materialises ``f = theta(x)^T phi(audio)`` of shape ``[B, THW, THW]`` (983 MB
of fp32 per clip at 56 x 56) and then ``y = (f / N) g(x)``.  'dot' has no softmax, so ``(theta^T phi) g = theta^T (phi g^T)``, and in the
audio branch ``phi`` is constant over h, w: up to its BatchNorm the block is a per-clip ``C x C`` linear map of ``x``,

    u = A_b x_p + c_b,    A_b = Wz K_b^T Wtheta,    c_b = Wz K_b^T btheta + bz,    K_b = (1/N) sum_t phi_t gbar_t^T

with ``gbar_t = Wg (sum_hw x) + H W bg`` -- no ``N x N`` tensor and about 60 x fewer FLOP (derived, not measured).  Three formulations:

* ``fused=True``: the passes over ``x`` are the HIP kernels of csrc/tpavi.hip (``ops.tpavi``), the per-clip setup is torch.  Raises where
  the kernels cannot run (CPU tensors, a library without the exports, shapes outside the limits, bf16): it never falls back.
* ``fused=False``: the linear form in ATen.  Works on the CPU; the honest baseline of tools/tpavi_bench.py.
* ``fused=None``: the kernels on a ROCm device only at the ``(B*T, H, W)`` in ``_KERNELS_FASTER`` (where tools/tpavi_bench.py measured
  their slowest window, forward + backward, faster than the ATen linear form's fastest), the ATen linear form everywhere else.
* ``reference_order=True`` selects the formulation that materialises ``f``, written like the reference: ATen only, for the parity tests
  and the bench.  ``audio=None`` (the video-video branch, which both training scripts switch off) and ``bn_layer=False`` always take it.

``forward(x [B, C, T, H, W], audio [B, T, 128]) -> (z [B, C, T, H, W], audio_temp [B, T, C])`` is the reference's contract.
``forward_frames(x [B*T, C, H, W], audio [B*T, 128] or [B, T, 128], T=5)`` does what ``tpavi_va`` does around the call
without its two permute copies: the kernels address the frames through strides.
"""
from __future__ import annotations

from typing import Optional

import torch
import torch.nn as nn

from . import ops

# (B*T, H, W) at C = 256 where forward + backward of the kernels have been MEASURED faster than the ATen linear form on an MI355X
# (tools/tpavi_bench.py -> profiles/tpavi_bench.txt; the rule: the kernels' slowest window beats ATen's fastest)
_KERNELS_FASTER: frozenset = frozenset()


class TPAVIModule(nn.Module):
    """TPAVI.py:6-153; ``fused`` / ``reference_order`` / ``lib``: module docstring."""

    def __init__(self, in_channels, inter_channels=None, mode='dot', dimension=3, bn_layer=True, fused: Optional[bool] = None,
                 reference_order: bool = False, lib=None):
        super().__init__()
        if mode not in ['gaussian', 'embedded', 'dot', 'concatenate']:
            raise ValueError('`mode` must be one of `gaussian`, `embedded`, `dot` or `concatenate`')
        if mode != 'dot':
            raise NotImplementedError(f"dg-sct_amd: TPAVIModule supports mode='dot' only (the AVS models build nothing else); got {mode!r}")
        if dimension != 3:
            raise NotImplementedError(f"dg-sct_amd: TPAVIModule supports dimension=3 only (the AVS models build nothing else); got "
                                      f"{dimension!r}")
        self.mode, self.dimension = mode, dimension
        self.fused, self.reference_order, self._lib = fused, reference_order, lib
        self.in_channels = in_channels
        self.inter_channels = inter_channels
        if self.inter_channels is None:
            self.inter_channels = in_channels // 2
            if self.inter_channels == 0:
                self.inter_channels = 1
        self.bn_layer = bn_layer
        self.align_channel = nn.Linear(128, in_channels)
        self.norm_layer = nn.LayerNorm(in_channels)
        self.g = nn.Conv3d(in_channels=self.in_channels, out_channels=self.inter_channels, kernel_size=1)
        if bn_layer:
            self.W_z = nn.Sequential(nn.Conv3d(in_channels=self.inter_channels, out_channels=self.in_channels, kernel_size=1),
                                     nn.BatchNorm3d(self.in_channels))
            nn.init.constant_(self.W_z[1].weight, 0)
            nn.init.constant_(self.W_z[1].bias, 0)
        else:
            self.W_z = nn.Conv3d(in_channels=self.inter_channels, out_channels=self.in_channels, kernel_size=1)
            nn.init.constant_(self.W_z.weight, 0)
            nn.init.constant_(self.W_z.bias, 0)
        self.theta = nn.Conv3d(in_channels=self.in_channels, out_channels=self.inter_channels, kernel_size=1)
        self.phi = nn.Conv3d(in_channels=self.in_channels, out_channels=self.inter_channels, kernel_size=1)

    # ---- the formulation that materialises f, in the reference's order (TPAVI.py:82-153) ----
    def _reference(self, x, audio=None):
        audio_temp = 0
        batch_size = x.size(0)
        if audio is not None:
            H, W = x.shape[-2], x.shape[-1]
            audio_temp = self.align_channel(audio)                               # [B, T, C]
            audio = audio_temp.permute(0, 2, 1).unsqueeze(-1).unsqueeze(-1).repeat(1, 1, 1, H, W)
        else:
            audio = x
        g_x = self.g(x).view(batch_size, self.inter_channels, -1).permute(0, 2, 1)          # [B, THW, Ci]
        theta_x = self.theta(x).view(batch_size, self.inter_channels, -1).permute(0, 2, 1)  # [B, THW, Ci]
        phi_x = self.phi(audio).view(batch_size, self.inter_channels, -1)                   # [B, Ci, THW]
        f = torch.matmul(theta_x, phi_x)                                                    # [B, THW, THW]
        y = torch.matmul(f / f.size(-1), g_x)                                               # [B, THW, Ci]
        y = y.permute(0, 2, 1).contiguous().view(batch_size, self.inter_channels, *x.size()[2:])
        z = self.W_z(y) + x
        z = self.norm_layer(z.permute(0, 2, 3, 4, 1)).permute(0, 4, 1, 2, 3)
        return z, audio_temp

    def _params(self):
        conv, bn = self.W_z[0], self.W_z[1]
        return (self.align_channel.weight, self.align_channel.bias, self.g.weight, self.g.bias, conv.weight, conv.bias, self.theta.weight,
                self.theta.bias, self.phi.weight, self.phi.bias), bn

    # ---- the linear form in ATen ----
    def _linear(self, x, audio):
        setup, bn = self._params()
        H, W = x.shape[-2:]
        s = x.sum(dim=(3, 4)).permute(0, 2, 1)                                   # [B, T, C]
        A, c, audio_temp = ops.tpavi_setup(s, audio, *setup, H * W)
        u = torch.einsum('bij,bjthw->bithw', A, x) + c[:, :, None, None, None]
        z = self.norm_layer((bn(u) + x).permute(0, 2, 3, 4, 1)).permute(0, 4, 1, 2, 3)
        return z, audio_temp

    def _fused(self, x, audio, T=None):
        setup, bn = self._params()
        if bn.momentum is None or not bn.track_running_stats or not bn.affine:
            raise RuntimeError("dg-sct_amd: TPAVIModule(fused=True) takes the BatchNorm3d the constructor builds (affine, momentum 0.1, "
                               "running statistics)")
        z, audio_temp = ops.tpavi(x, audio, *setup, bn.weight, bn.bias, bn.running_mean, bn.running_var, self.norm_layer.weight,
                                  self.norm_layer.bias, self.training, T, bn.momentum, bn.eps, self.norm_layer.eps, self._lib)
        if self.training:
            with torch.no_grad():
                bn.num_batches_tracked += 1
        return z, audio_temp

    def _use_fused(self, x: torch.Tensor, audio: torch.Tensor, T: Optional[int]) -> bool:
        if self.fused is False:
            return False
        if self.fused:
            return True                                        # ops.tpavi raises on what the kernels do not take
        a3 = audio.reshape(-1, T, audio.shape[-1]) if T else audio
        if not ops.tpavi_supported(x, a3, T):
            return False
        key = (x.shape[0] * x.shape[2], x.shape[3], x.shape[4]) if x.dim() == 5 else (x.shape[0], x.shape[2], x.shape[3])
        if key not in _KERNELS_FASTER:
            return False
        return (self._lib or ops._lib.default_lib()).has_tpavi()

    def _reference_only(self, audio) -> bool:
        return self.reference_order or audio is None or not self.bn_layer

    def forward(self, x, audio=None):
        if self._reference_only(audio):
            return self._reference(x, audio)
        if self._use_fused(x, audio, None):
            return self._fused(x, audio)
        return self._linear(x, audio)

    def forward_frames(self, x, audio=None, T: int = 5):
        """``x [B*T, C, H, W]``, ``audio [B*T, 128]`` or ``[B, T, 128]`` -> ``(z [B*T, C, H, W], audio_temp [B, T, C])``: ``tpavi_va``
        (PVT_AVSModel.py:766-778) around ``forward``, without its two permute copies where the kernels run."""
        BT, C_, H, W = x.shape
        if audio is not None:
            audio = audio.reshape(-1, T, audio.shape[-1])
        if not self._reference_only(audio) and self._use_fused(x, audio, T):
            return self._fused(x, audio, T)
        x5 = x.reshape(-1, T, C_, H, W).permute(0, 2, 1, 3, 4)
        if self._reference_only(audio):
            z, audio_temp = self._reference(x5.contiguous(), audio)
        else:
            z, audio_temp = self._linear(x5, audio)
        return z.permute(0, 2, 1, 3, 4).reshape(BT, C_, H, W), audio_temp
