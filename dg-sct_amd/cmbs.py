"""Drop-in ``CMBS`` -- the event head of the AVE model, the last call of ``forward_swin``.

Mirrors reference ``DG-SCT/AVE/nets/net_trans.py:254-292`` and its building blocks ``AudioVideoInter`` (``:165-179``) and
``SupvLocalizeModule`` (``:116-138``): the same constructor signature (``CMBS(config)``, ``config`` unused), the same attributes built in
the same order -- hence the same 24 ``state_dict`` keys in the same order and, under one seed, the same parameter values.

What the forward computes is the LIVE part of the reference's: the two class-activation Linears, the mean of the four largest scores
over time, the fused feature's per-timestep score, its max over time and the event classifier.  The reference also runs its two
``AudioVideoInter`` blocks (``:286-287``) and reads neither result; like the decoders of ``TemporalAttentionAVS`` they are constructed
here for the checkpoint format and skipped in forward.  Their 12 parameters and the 4 of the never-called ``video_norm`` /
``audio_norm`` receive no gradient in the reference either.  One consequence: in train mode the reference's dead branches draw dropout
masks from the RNG and this module does not, so a seeded train-mode run leaves the head with a different RNG state than the
reference's (eval mode is unaffected).

``fused=True`` runs the head as one HIP launch forward and two backward (csrc/head.hip, ``ops.cmbs_head``) and raises where the kernels
cannot run (CPU tensors, a library without the export, shapes outside the limits): it never falls back.  ``fused=False`` is the ATen
formulation, written like the reference (sort, ``[:4]``, mean), and works on the CPU.  ``fused=None`` takes the kernels on a ROCm device
only at the ``(T, B)`` where tools/head_bench.py measured their slowest window faster than ATen's fastest (``_KERNELS_FASTER``, from
profiles/cmbs_head_bench.txt), and ATen everywhere else, unmeasured shapes included.
"""
from __future__ import annotations

from typing import Optional

import torch
import torch.nn as nn
from torch.nn import MultiheadAttention

from . import ops

# (T, B) at d_model 256, 28 classes where forward + backward of the kernels have been MEASURED faster than the ATen formulation on an
# MI355X (tools/head_bench.py -> profiles/cmbs_head_bench.txt; the rule: the kernels' slowest window beats ATen's fastest)
_KERNELS_FASTER: frozenset = frozenset()


class AudioVideoInter(nn.Module):
    """net_trans.py:165-179"""

    def __init__(self, d_model, n_head, head_dropout=0.1):
        super().__init__()
        self.dropout = nn.Dropout(0.1)
        self.video_multihead = MultiheadAttention(d_model, num_heads=n_head, dropout=head_dropout)
        self.norm1 = nn.LayerNorm(d_model)

    def forward(self, video_feat, audio_feat):
        raise RuntimeError("dg-sct_amd: AudioVideoInter is built for CMBS's state_dict only: the reference computes it and reads the "
                           "result nowhere, and CMBS.forward here skips it")


class SupvLocalizeModule(nn.Module):
    """net_trans.py:116-138"""

    def __init__(self, d_model):
        super().__init__()
        self.relu = nn.ReLU(inplace=True)
        self.classifier = nn.Linear(d_model, 1)
        self.event_classifier = nn.Linear(d_model, 28)

    def forward(self, fused_content):
        """fused_content [T, B, d] -> (per-timestep score [T, B, 1], class scores of the feature's max over time [B, 28])"""
        return self.classifier(fused_content), self.event_classifier(fused_content.max(dim=0)[0])


class CMBS(nn.Module):
    """net_trans.py:254-292.  ``forward(visual_feature [T, B, 256], audio_feature [T, B, 256]) ->
    (is_event_scores [T, B, 1], event_scores [B, 28], av_score [B, 28])``; ``fused`` / ``lib``: module docstring."""

    def __init__(self, config=None, fused: Optional[bool] = None, lib=None):
        super().__init__()
        self.config = config
        self.fused, self._lib = fused, lib
        self.beta = 0.4
        self.d_model = 256
        self.AVInter = AudioVideoInter(self.d_model, n_head=4, head_dropout=0.2)        # constructed, skipped in forward
        self.VAInter = AudioVideoInter(self.d_model, n_head=4, head_dropout=0.2)        # constructed, skipped in forward
        self.localize_module = SupvLocalizeModule(self.d_model)
        self.video_norm = nn.LayerNorm(self.d_model)                                    # never called by the reference
        self.audio_norm = nn.LayerNorm(self.d_model)                                    # never called by the reference
        self.audio_cas = nn.Linear(self.d_model, 28)
        self.video_cas = nn.Linear(self.d_model, 28)
        self.alpha = 0.1
        self.gamma = 0.3

    def _aten(self, visual_feature, audio_feature):
        video_cas = self.video_cas(visual_feature).permute(1, 0, 2)                     # [B, T, 28]
        audio_cas = self.audio_cas(audio_feature).permute(1, 0, 2)
        score_video = torch.mean(video_cas.sort(descending=True, dim=1)[0][:, :4, :], dim=1)
        score_audio = torch.mean(audio_cas.sort(descending=True, dim=1)[0][:, :4, :], dim=1)
        av_score = (score_video + score_audio) / 2
        is_event_scores, event_scores = self.localize_module((visual_feature + audio_feature) / 2)
        return is_event_scores, event_scores + self.gamma * av_score, av_score

    def _use_fused(self, v: torch.Tensor, a: torch.Tensor) -> bool:
        if self.fused is False:
            return False
        if self.fused:
            return True                                        # ops.cmbs_head raises on what the kernels do not take
        if not ops.cmbs_head_supported(v, a, self.video_cas.out_features) or tuple(v.shape[:2]) not in _KERNELS_FASTER:
            return False
        return (self._lib or ops._lib.default_lib()).has_cmbs_head()

    def forward(self, visual_feature, audio_feature):
        if not self._use_fused(visual_feature, audio_feature):
            return self._aten(visual_feature, audio_feature)
        loc = self.localize_module
        return ops.cmbs_head(visual_feature, audio_feature, self.video_cas.weight, self.video_cas.bias, self.audio_cas.weight,
                             self.audio_cas.bias, loc.classifier.weight, loc.classifier.bias, loc.event_classifier.weight,
                             loc.event_classifier.bias, self.gamma, self._lib)
