"""What feeds the layer loop (the part in front of the first block): the reference's audio front end
``spectrogram_extractor -> logmel_extractor -> bn0 -> reshape_wav2img -> patch_embed`` (DG-SCT/AVE/nets/net_trans.py:857-876;
htsat.py:443-459, 719-734; layers.py:56-86) and the visual ``swin.patch_embed`` (net_trans.py:855), as two modules with the reference's
``state_dict`` names, frozen and forward-only unless built with ``trainable=True``:

    HTSATFrontEnd   waveform [B, L] -> tokens [B, 4096, embed_dim]      two or three launches of csrc/frontend.hip (ops.logmel, its
                    statistics reduction in train mode, ops.patch_embed in audio mode); no tensor larger than the log-mel exists
    PatchEmbed      image [B, in_chans, H, W] -> tokens [B, (H/4)(W/4), embed_dim]      one launch (ops.patch_embed)

Both dispatch like the backbone blocks: ``fused=None`` runs the HIP path on GPU tensors; ``fused=False`` (or CPU tensors) runs an ATen
formulation of the same maths (torch.stft, matmul, F.batch_norm, F.interpolate, F.conv2d, F.layer_norm) -- the CPU-testable restatement
and the A/B partner on the GPU.

``trainable=True`` (AVS-S4 trains everything outside ``'ViT'`` / ``'swin'``, avs_s4/train.py:145-163, so ``htsat.bn0.*`` and
``htsat.patch_embed.*`` train, ``bn0`` on batch statistics) leaves ``proj.*``, ``norm.*``, ``bn0.weight`` and ``bn0.bias`` requiring grad --
never ``melW``, the waveform or the image -- and runs the forward under autograd.  On the kernel path the forward is the same launches and the
backward is ONE call, ``dgsct_patch_embed_backward_params`` (``ops.patch_embed_train``), which recomputes the convolution and the
LayerNorm statistics from the log-mel / the image: nothing token-sized is kept for it.  ``fused=True`` takes the kernels (and raises when the
library lacks the export), ``fused=False`` / CPU is the ATen formulation under plain autograd, and ``fused=None`` follows
``_KERNELS_FASTER_TRAIN`` (the kinds measured faster, profiles/frontend_train_bench.txt).  With grad disabled, or with every one of those parameters frozen again, a
trainable module runs exactly the frozen path.

``spec_augment=True`` (HTSATFrontEnd) keeps the reference's train-time augmentation: ``spec_augmenter`` (htsat.py:451: torchlibrosa's
``SpecAugmentation(time_drop_width=64, time_stripes_num=2, freq_drop_width=8, freq_stripes_num=2)``) zeroes two time and two mel stripes per
sample of the ``bn0`` output, and ``do_mixup`` (nets/utils.py:143-153) then mixes sample b with sample B-1-b by ``mixup_lambda``
(``forward(waveform, mixup_lambda, stripes)``), both before the stretch and both only in train mode (net_trans.py:862-866).  The stripes are
drawn by ``draw_stripes`` from torch's CPU generator, draw for draw as the published ``DropStripes`` does; an explicit ``stripes=`` table
replays a run.  On the kernel path both are part of the loads of ``patch_embed_k`` / ``patch_embed_bwd_k`` (a zero at a tap, a second tap from
the mirrored sample: ``dgsct_patch_embed_forward_aug`` / ``dgsct_patch_embed_backward_params_aug``), so neither the ``bn0`` output nor the
image exists in memory; ``fused=False`` / CPU multiplies by the keep mask and mixes with ``torch.flip`` in ATen.  ``fused=None`` with an
augmentation active follows ``_KERNELS_FASTER_AUG``.  Parity with torchlibrosa's ``DropStripes`` is unpinned like the rest (next paragraph):
the pin is to the published algorithm (tests/test_frontend_aug_cpu.py).

**Parity against torchlibrosa / librosa is unpinned**: neither is installed here, and the oracle cannot import the front end of
``htsat.py``.  The pin is to the published formulas evaluated in float64 (tests/test_frontend_cpu.py, tests/test_frontend_gpu.py): the
centred, reflect-padded, periodic-Hann STFT; librosa's default (Slaney-scale, Slaney-normalised) mel filterbank; PyTorch's bicubic
kernel.  A real HTS-AT checkpoint supplies its own ``logmel_extractor.melW``, which replaces the one built here.

Out of scope: ``do_mixup_label`` (the label side of the mix-up belongs to the task's loss), ``ape`` /
``pos_drop`` (off / identity in every reference config), the random ``crop_wav`` branch (more than 1024 frames raises here), image-side
augmentation.  Patch merging and the Swin-V2 final norm live in ``merging.py`` (``AVETrunk``)."""
from __future__ import annotations

import math
from typing import Optional

import torch
import torch.nn as nn
import torch.nn.functional as F

from . import ops
from .ops import HOP, MAX_FRAMES, N_FFT, N_MELS


def slaney_mel_filterbank(sample_rate: int = 32000, n_fft: int = N_FFT, n_mels: int = N_MELS, fmin: float = 50.0,
                          fmax: float = 14000.0) -> torch.Tensor:
    """librosa.filters.mel's default (htk=False, norm='slaney') transposed to [n_fft // 2 + 1, n_mels], built in float64: triangles
    between n_mels + 2 points evenly spaced on the Slaney mel scale (linear below 1 kHz, logarithmic above), each scaled by
    2 / (its width in Hz)."""
    f_sp, min_log_hz, logstep = 200.0 / 3.0, 1000.0, math.log(6.4) / 27.0
    min_log_mel = min_log_hz / f_sp

    def to_mel(f: float) -> float:
        return f / f_sp if f < min_log_hz else min_log_mel + math.log(f / min_log_hz) / logstep

    mels = torch.linspace(to_mel(fmin), to_mel(fmax), n_mels + 2, dtype=torch.float64)
    hz = torch.where(mels < min_log_mel, mels * f_sp, min_log_hz * torch.exp(logstep * (mels - min_log_mel)))
    bins = torch.linspace(0.0, sample_rate / 2.0, n_fft // 2 + 1, dtype=torch.float64)
    ramps = hz[:, None] - bins[None, :]                                       # [n_mels + 2, bins]
    fdiff = hz[1:] - hz[:-1]
    lower = -ramps[:-2] / fdiff[:-1, None]
    upper = ramps[2:] / fdiff[1:, None]
    w = torch.minimum(lower, upper).clamp_min(0.0) * (2.0 / (hz[2:] - hz[:-2]))[:, None]
    return w.t().contiguous().float()


def hann_dft_basis(n_fft: int = N_FFT):
    """(real, imag) [n_fft // 2 + 1, 1, n_fft] float64: the periodic-Hann-windowed DFT basis the reference's STFT convolves with
    (`spectrogram_extractor.stft.conv_real / conv_imag`): cos(2 pi k n / N) w[n] and -sin(2 pi k n / N) w[n]"""
    n = torch.arange(n_fft, dtype=torch.float64)
    k = torch.arange(n_fft // 2 + 1, dtype=torch.float64)
    win = 0.5 - 0.5 * torch.cos(2.0 * math.pi * n / n_fft)
    ang = 2.0 * math.pi * torch.outer(k, n) / n_fft
    return (torch.cos(ang) * win).unsqueeze(1), (-torch.sin(ang) * win).unsqueeze(1)


def _use_fused(fused: Optional[bool], x: torch.Tensor, who: str) -> bool:
    if fused is None:
        return x.is_cuda
    if fused and not x.is_cuda:
        raise RuntimeError(f"dg-sct_amd: {who}(fused=True) needs CUDA/HIP tensors (no CPU kernels; fused=False is the ATen formulation)")
    return bool(fused)


def _refuse_grad(who: str, x: torch.Tensor):
    if x.requires_grad:
        raise RuntimeError(f"dg-sct_amd: {who} is forward-only: its input requires grad (detach it; no input gradient is built, trainable or not)")


# `fused=None` with trainable=True takes the kernels only for the kinds listed here: those where `tools/frontend_bench.py --train` measured
# the kernels' slowest forward + backward window faster than the fastest window of the ATen formulation on the same GPU
# (profiles/frontend_train_bench.txt).  A kind that is not listed stays ATen under fused=None, and fused=True is the opt-in.
_KERNELS_FASTER_TRAIN: frozenset = frozenset({"audio", "image"})


def _train_through_kernels(fused: Optional[bool], x: torch.Tensor, lib, who: str, kind: str) -> bool:
    """which formulation a forward that wants parameter gradients takes; kind: "audio" (HTSATFrontEnd) | "image" (PatchEmbed)"""
    if fused is None and not (x.is_cuda and kind in _KERNELS_FASTER_TRAIN):
        return False
    if not _use_fused(fused, x, who):
        return False
    lib = lib or ops._lib.default_lib()
    if not lib.has_patch_embed_params():
        if fused:
            raise RuntimeError(f"dg-sct_amd: {who}(trainable=True, fused=True): {lib.path} does not export dgsct_patch_embed_backward_params "
                               f"(fused=None / False for the ATen formulation)")
        return False
    return True


# `fused=None` with an augmentation active (stripes and / or mixup_lambda, train mode) takes the kernels only for the kinds listed here:
# "frozen" (forward only) | "train" (forward + backward of a trainable module), by the same rule on the rows of `tools/frontend_bench.py
# --augment` (profiles/frontend_aug_bench.txt).  A call without augmentation never looks at it.
_KERNELS_FASTER_AUG: frozenset = frozenset({"frozen", "train"})

TIME_DROP_WIDTH, TIME_STRIPES, FREQ_DROP_WIDTH, FREQ_STRIPES = 64, 2, 8, 2          # htsat.py:451


def draw_stripes(B: int, T: int, generator: Optional[torch.Generator] = None) -> torch.Tensor:
    """The stripes `spec_augmenter` would drop from a [B, 1, T, 64] batch, as int32 [B, 4, 2] of half-open (begin, end): rows 0 and 1 the
    time stripes (frames of the un-stretched log-mel), rows 2 and 3 the mel stripes.  The published DropStripes algorithm, draw for draw on
    the CPU generator (None: torch's default one): the time dropper first, for samples 0 .. B-1 in order and twice per sample
    ``distance = randint(0, drop_width)`` then ``bgn = randint(0, total_width - distance)``; the mel dropper follows the same way.
    T < 64 raises: a distance of up to 63 frames can leave the second range empty."""
    if T < TIME_DROP_WIDTH:
        raise ValueError(f"dg-sct_amd: draw_stripes: {T} frames are fewer than the time drop width {TIME_DROP_WIDTH} (the reference's "
                         f"randint(0, total_width - distance) can have an empty range)")
    out = torch.zeros(B, 4, 2, dtype=torch.int32)
    for row0, total, width, num in ((0, T, TIME_DROP_WIDTH, TIME_STRIPES), (TIME_STRIPES, N_MELS, FREQ_DROP_WIDTH, FREQ_STRIPES)):
        for n in range(B):
            for j in range(num):
                distance = int(torch.randint(low=0, high=width, size=(1,), generator=generator)[0])
                bgn = int(torch.randint(low=0, high=total - distance, size=(1,), generator=generator)[0])
                out[n, row0 + j, 0], out[n, row0 + j, 1] = bgn, bgn + distance
    return out


def keep_mask(stripes: torch.Tensor, T: int) -> torch.Tensor:
    """stripes int32 [B, 4, 2] -> bool [B, T, 64]: False inside any of a sample's stripes"""
    s = stripes.long()
    t = torch.arange(T, device=s.device).view(1, T, 1)
    f = torch.arange(N_MELS, device=s.device).view(1, 1, N_MELS)
    drop = torch.zeros(s.shape[0], T, N_MELS, dtype=torch.bool, device=s.device)
    for r, idx in ((0, t), (1, t), (2, f), (3, f)):
        drop = drop | ((idx >= s[:, r, 0].view(-1, 1, 1)) & (idx < s[:, r, 1].view(-1, 1, 1)))
    return ~drop


class PatchEmbed(nn.Module):
    """``PatchEmbed`` of timm 0.6.12 / layers.py:56-86 at patch 4, stride 4: ``norm(proj(x).flatten(2).transpose(1, 2))``; keys
    ``proj.{weight,bias}``, ``norm.{weight,bias}``.  Frozen and forward-only; trainable=True: the four parameters require grad and the forward
    runs under autograd (no input gradient either way).  out_dtype None: the image's dtype."""

    def __init__(self, img_size, patch_size: int = 4, in_chans: int = 3, embed_dim: int = 128, fused: Optional[bool] = None, lib=None,
                 out_dtype: Optional[torch.dtype] = None, trainable: bool = False):
        super().__init__()
        if patch_size != 4:
            raise ValueError("dg-sct_amd: PatchEmbed is built for 4 x 4 patches at stride 4 (every reference backbone)")
        self.img_size = (img_size, img_size) if isinstance(img_size, int) else tuple(img_size)
        if self.img_size[0] % 4 or self.img_size[1] % 4:
            raise ValueError("dg-sct_amd: PatchEmbed: the image sides must be multiples of 4")
        if in_chans not in (1, 3) or embed_dim % 32 or not 32 <= embed_dim <= 192:
            raise ValueError("dg-sct_amd: PatchEmbed takes in_chans 1 or 3 and an embed_dim that is a multiple of 32 up to 192")
        self.grid_size = (self.img_size[0] // 4, self.img_size[1] // 4)
        self.num_patches = self.grid_size[0] * self.grid_size[1]
        self.in_chans, self.embed_dim = in_chans, embed_dim
        self.fused, self.lib, self.out_dtype = fused, lib, out_dtype
        self.proj = nn.Conv2d(in_chans, embed_dim, kernel_size=4, stride=4)
        self.norm = nn.LayerNorm(embed_dim)
        self.trainable = bool(trainable)
        self.requires_grad_(self.trainable)

    def _wants_grad(self) -> bool:
        return self.trainable and torch.is_grad_enabled() and any(p.requires_grad for p in self.parameters())

    def _tokens_aten(self, img: torch.Tensor) -> torch.Tensor:
        x = F.conv2d(img.float(), self.proj.weight, self.proj.bias, stride=4)
        return F.layer_norm(x.flatten(2).transpose(1, 2), (self.embed_dim,), self.norm.weight, self.norm.bias, self.norm.eps)

    def forward(self, x: torch.Tensor) -> torch.Tensor:
        if x.dim() != 4 or x.shape[1] != self.in_chans or tuple(x.shape[2:]) != self.img_size:
            raise RuntimeError(f"dg-sct_amd: PatchEmbed: input {tuple(x.shape)} does not match [B, {self.in_chans}, {self.img_size[0]}, {self.img_size[1]}]")
        _refuse_grad("PatchEmbed", x)
        out_dtype = self.out_dtype or x.dtype
        if self._wants_grad():
            if _train_through_kernels(self.fused, x, self.lib, "PatchEmbed", "image"):
                return ops.patch_embed_train(x.contiguous(), self.proj.weight, self.proj.bias, self.norm.weight, self.norm.bias, self.norm.eps,
                                             out_dtype=out_dtype, lib=self.lib)
            return self._tokens_aten(x).to(out_dtype)
        with torch.no_grad():
            return self._forward_frozen(x, out_dtype)

    def _frozen_params(self):
        """proj.weight, proj.bias, norm.weight, norm.bias as `ops.patch_embed` takes them (it refuses tensors that require grad: a trainable
        module evaluated without a graph hands it detached views)"""
        ps = (self.proj.weight, self.proj.bias, self.norm.weight, self.norm.bias)
        return tuple(t.detach() for t in ps) if self.trainable else ps

    def _forward_frozen(self, x: torch.Tensor, out_dtype: torch.dtype) -> torch.Tensor:
        if _use_fused(self.fused, x, "PatchEmbed"):
            return ops.patch_embed(x.contiguous(), *self._frozen_params(), self.norm.eps, out_dtype=out_dtype, lib=self.lib)
        return self._tokens_aten(x).to(out_dtype)


class _MelBank(nn.Module):
    """holder of `logmel_extractor.melW` (torchlibrosa's LogmelFilterBank keeps it as a frozen Parameter)"""

    def __init__(self, melW: torch.Tensor):
        super().__init__()
        self.melW = nn.Parameter(melW, requires_grad=False)


class HTSATFrontEnd(nn.Module):
    """waveform [B, L] fp32 -> HTS-AT patch tokens [B, 4096, embed_dim] (``f_a`` as the first HTS-AT block sees it, net_trans.py:857-876).
    state_dict: ``logmel_extractor.melW`` [513, 64], ``bn0.*``, ``patch_embed.proj.*``, ``patch_embed.norm.*``; a checkpoint's
    ``spectrogram_extractor.stft.conv_{real,imag}.weight`` are checked against the Hann-windowed DFT basis and dropped (they are functions
    of the constants; a basis more than 1e-5 away -- entries are <= 1, so fp32 rounding plus margin -- raises; ``conv_imag`` is accepted
    with either sign, +sin or -sin, because only the power is used).  ``bn0`` follows the module's mode: running statistics in eval mode, batch statistics
    over (B, T) per mel bin plus the running-statistics update in train mode.  Frozen and forward-only; trainable=True: ``bn0.weight``,
    ``bn0.bias`` and the four ``patch_embed`` parameters require grad (``melW`` never does) and the forward runs under autograd; the statistics
    of ``bn0`` are functions of the waveform and carry no gradient.  out_dtype None: fp32."""

    _DERIVED = ("spectrogram_extractor.stft.conv_real.weight", "spectrogram_extractor.stft.conv_imag.weight")

    def __init__(self, embed_dim: int = 96, spec_size: int = 256, sample_rate: int = 32000, fmin: float = 50, fmax: float = 14000,
                 fused: Optional[bool] = None, lib=None, out_dtype: Optional[torch.dtype] = None, trainable: bool = False,
                 spec_augment: bool = False):
        super().__init__()
        if spec_size != 256:
            raise ValueError("dg-sct_amd: HTSATFrontEnd is built for spec_size 256 (64 mel bins x 4 time quarters, every reference config)")
        self.spec_size, self.freq_ratio = spec_size, spec_size // N_MELS
        self.fused, self.lib, self.out_dtype = fused, lib, out_dtype
        self.logmel_extractor = _MelBank(slaney_mel_filterbank(sample_rate, N_FFT, N_MELS, fmin, fmax))
        self.bn0 = nn.BatchNorm2d(N_MELS)
        self.patch_embed = PatchEmbed(spec_size, 4, 1, embed_dim, fused=fused, lib=lib, out_dtype=out_dtype, trainable=trainable)
        self.trainable = bool(trainable)
        self.spec_augment = bool(spec_augment)
        self.requires_grad_(False)
        if self.trainable:
            self.bn0.requires_grad_(True)
            self.patch_embed.requires_grad_(True)
        self._ranges = None            # (melW version, device, ops.mel_ranges(melW))

    # -- checkpoint loading ------------------------------------------------------------------------------------------------------------
    def _load_from_state_dict(self, state_dict, prefix, local_metadata, strict, missing_keys, unexpected_keys, error_msgs):
        basis = None
        for name, which in zip(self._DERIVED, (0, 1)):
            w = state_dict.pop(prefix + name, None)
            if w is None:
                continue
            basis = basis or hann_dft_basis()
            ref = basis[which]
            ok = tuple(w.shape) == tuple(ref.shape)
            if ok:
                w64 = w.detach().double().cpu()
                ok = torch.allclose(w64, ref, rtol=0.0, atol=1e-5) or (which == 1 and torch.allclose(w64, -ref, rtol=0.0, atol=1e-5))
            if not ok:
                error_msgs.append(f"{prefix + name} is not the periodic-Hann-windowed {N_FFT}-point DFT basis this front end computes "
                                  f"(shape {tuple(w.shape)}); a checkpoint with another STFT cannot be loaded")
        super()._load_from_state_dict(state_dict, prefix, local_metadata, strict, missing_keys, unexpected_keys, error_msgs)

    # -- pieces ------------------------------------------------------------------------------------------------------------------------
    def _mel_ranges(self) -> torch.Tensor:
        m = self.logmel_extractor.melW
        key = (m._version, m.device, m.data_ptr())
        if self._ranges is None or self._ranges[0] != key:
            self._ranges = (key, ops.mel_ranges(m))
        return self._ranges[1]

    def logmel_aten(self, waveform: torch.Tensor) -> torch.Tensor:
        """[B, L] -> [B, T, 64]: torch.stft (centred, reflect, periodic Hann), power, melW, 10 log10(max(., 1e-10))"""
        win = torch.hann_window(N_FFT, periodic=True, dtype=waveform.dtype, device=waveform.device)
        z = torch.stft(waveform, N_FFT, hop_length=HOP, win_length=N_FFT, window=win, center=True, pad_mode="reflect", return_complex=True)
        power = (z.real * z.real + z.imag * z.imag).transpose(1, 2)            # [B, T, 513]
        return 10.0 * torch.log10(torch.clamp(power @ self.logmel_extractor.melW.to(waveform.dtype), min=1e-10))

    def _bn_statistics(self, mean: Optional[torch.Tensor], var: Optional[torch.Tensor], n: int):
        """the (mean, biased variance) bn0 normalises with: the batch statistics (train mode: also the running-statistics update) or the
        running ones"""
        bn = self.bn0
        if mean is not None:
            if bn.track_running_stats and bn.running_mean is not None:
                bn.num_batches_tracked += 1
                mom = bn.momentum if bn.momentum is not None else 1.0 / float(bn.num_batches_tracked)
                bn.running_mean.mul_(1.0 - mom).add_(mean, alpha=mom)
                bn.running_var.mul_(1.0 - mom).add_(var * (n / max(n - 1, 1)), alpha=mom)
        else:
            mean, var = bn.running_mean, bn.running_var
        return mean, var

    def _bn_affine(self, mean: Optional[torch.Tensor], var: Optional[torch.Tensor], n: int):
        """scale / shift [64] of bn0 from `_bn_statistics`"""
        bn = self.bn0
        mean, var = self._bn_statistics(mean, var, n)
        scale = bn.weight * torch.rsqrt(var + bn.eps)
        return scale.contiguous(), (bn.bias - mean * scale).contiguous()

    def _tokens_aten(self, lm: torch.Tensor, stripes: Optional[torch.Tensor] = None, lam: Optional[torch.Tensor] = None) -> torch.Tensor:
        B, T, _ = lm.shape
        bn = self.bn0
        x = lm.transpose(1, 2).unsqueeze(-1)                                   # [B, 64, T, 1] = the reference's `audio.transpose(1, 3)`
        if self.training:
            bn.num_batches_tracked += 1
        x = F.batch_norm(x, bn.running_mean, bn.running_var, bn.weight, bn.bias, self.training, bn.momentum, bn.eps)
        x = x.transpose(1, 3)                                                  # [B, 1, T, 64]
        if stripes is not None:                                                # `spec_augmenter` (out of place: autograd keeps the bn0 output)
            stripes = ops.check_stripes(stripes, B, T, "HTSATFrontEnd")
            x = x * keep_mask(stripes.to(x.device), T).unsqueeze(1).to(x.dtype)
        if lam is not None:                                                    # `do_mixup`
            la = lam.to(x.device).view(B, 1, 1, 1)
            x = la * x + (1.0 - la) * torch.flip(x, [0])
        if T < MAX_FRAMES:
            x = F.interpolate(x, (MAX_FRAMES, N_MELS), mode="bicubic", align_corners=True)
        x = x.permute(0, 1, 3, 2).reshape(B, 1, N_MELS, self.freq_ratio, MAX_FRAMES // self.freq_ratio)
        x = x.permute(0, 1, 3, 2, 4).reshape(B, 1, self.spec_size, self.spec_size)     # image[q*64 + f][t'] = x[q*256 + t'][f]
        return self.patch_embed._tokens_aten(x)

    def _wants_grad(self) -> bool:
        if not (self.trainable and torch.is_grad_enabled()):
            return False
        if self.logmel_extractor.melW.requires_grad:
            raise RuntimeError("dg-sct_amd: HTSATFrontEnd: logmel_extractor.melW requires grad, and no gradient into the mel matrix is built "
                               "(freeze it: a name rule that unfreezes everything under 'htsat' unfreezes it too)")
        return any(p.requires_grad for p in self.parameters())

    def _augmentation(self, B: int, T: int, mixup_lambda, stripes):
        """(stripes int32 [B, 4, 2] | None, lam fp32 [B] | None) of this call: both None outside train mode, as the reference applies neither
        (`if self.htsat.training`); drawn stripes live on the CPU, where `draw_stripes` makes them.  The table is range-checked once, where it
        is consumed: by `ops.patch_embed` on the kernel path, by `_tokens_aten` otherwise"""
        if not self.training:
            return None, None
        if stripes is None and self.spec_augment:
            stripes = draw_stripes(B, T)
        if mixup_lambda is not None:
            if not isinstance(mixup_lambda, torch.Tensor) or tuple(mixup_lambda.shape) != (B,) or mixup_lambda.dtype != torch.float32:
                raise RuntimeError(f"dg-sct_amd: HTSATFrontEnd: mixup_lambda must be an fp32 tensor [{B}], one lambda per waveform (got "
                                   f"{tuple(getattr(mixup_lambda, 'shape', ()))} {getattr(mixup_lambda, 'dtype', type(mixup_lambda).__name__)})")
            _refuse_grad("HTSATFrontEnd (mixup_lambda)", mixup_lambda)
        return stripes, mixup_lambda

    def _aug_through_kernels(self, waveform: torch.Tensor, kind: str) -> bool:
        """which formulation a call with an augmentation active takes; kind: "frozen" (forward only) | "train" (with parameter gradients)"""
        if self.fused is None and not (waveform.is_cuda and kind in _KERNELS_FASTER_AUG):
            return False
        if not _use_fused(self.fused, waveform, "HTSATFrontEnd"):
            return False
        lib = self.lib or ops._lib.default_lib()
        if not lib.has_patch_embed_aug():
            if self.fused:
                raise RuntimeError(f"dg-sct_amd: HTSATFrontEnd(fused=True) with stripes / mixup_lambda: {lib.path} does not export "
                                   f"dgsct_patch_embed_forward_aug / dgsct_patch_embed_backward_params_aug (fused=None / False for the ATen formulation)")
            return False
        return True

    def forward(self, waveform: torch.Tensor, mixup_lambda: Optional[torch.Tensor] = None, stripes: Optional[torch.Tensor] = None) -> torch.Tensor:
        """mixup_lambda fp32 [B] and stripes int32 [B, 4, 2] (`draw_stripes`; None with spec_augment=True: drawn here) apply in train mode
        only; eval mode ignores both"""
        if waveform.dim() != 2 or waveform.dtype != torch.float32:
            raise RuntimeError(f"dg-sct_amd: HTSATFrontEnd takes an fp32 waveform [B, L] (got {tuple(waveform.shape)} {waveform.dtype})")
        _refuse_grad("HTSATFrontEnd", waveform)
        B, L = waveform.shape
        if L <= N_FFT // 2:
            raise RuntimeError(f"dg-sct_amd: HTSATFrontEnd: {L} samples are too few for the reflect padding (need more than {N_FFT // 2})")
        T = ops.logmel_frames(L)
        if T > MAX_FRAMES:
            raise RuntimeError(f"dg-sct_amd: HTSATFrontEnd: {L} samples give {T} frames, more than the {MAX_FRAMES} the {self.spec_size} x "
                               f"{self.spec_size} image holds (the reference's random crop_wav branch is not built)")
        out_dtype = self.out_dtype or torch.float32
        stripes, lam = self._augmentation(B, T, mixup_lambda, stripes)
        if self._wants_grad():
            return self._forward_trainable(waveform, B, T, out_dtype, stripes, lam)
        with torch.no_grad():
            return self._forward_frozen(waveform, B, T, out_dtype, stripes, lam)

    def _forward_trainable(self, waveform: torch.Tensor, B: int, T: int, out_dtype: torch.dtype, stripes=None, lam=None) -> torch.Tensor:
        """the waveform and melW are data: the log-mel (and the statistics of bn0) are made without a graph, autograd starts at bn0"""
        melW, pe, bn = self.logmel_extractor.melW, self.patch_embed, self.bn0
        aug = stripes is not None or lam is not None
        if not _train_through_kernels(self.fused, waveform, self.lib, "HTSATFrontEnd", "audio") or (aug and not self._aug_through_kernels(waveform, "train")):
            with torch.no_grad():
                lm = self.logmel_aten(waveform)
            return self._tokens_aten(lm, stripes, lam).to(out_dtype)
        with torch.no_grad():
            if self.training:
                lm, mean, var = ops.logmel(waveform.contiguous(), melW, want_stats=True, lib=self.lib, ranges=self._mel_ranges())
                mean, var = self._bn_statistics(mean, var, B * T)
            else:
                lm = ops.logmel(waveform.contiguous(), melW, lib=self.lib, ranges=self._mel_ranges())
                mean, var = self._bn_statistics(None, None, B * T)
        return ops.patch_embed_train(lm, pe.proj.weight, pe.proj.bias, pe.norm.weight, pe.norm.bias, pe.norm.eps, out_dtype=out_dtype,
                                     bn_weight=bn.weight, bn_bias=bn.bias, mean=mean, var=var, bn_eps=bn.eps, lib=self.lib, stripes=stripes,
                                     mixup_lambda=lam)

    def _forward_frozen(self, waveform: torch.Tensor, B: int, T: int, out_dtype: torch.dtype, stripes=None, lam=None) -> torch.Tensor:
        aug = stripes is not None or lam is not None
        if not _use_fused(self.fused, waveform, "HTSATFrontEnd") or (aug and not self._aug_through_kernels(waveform, "frozen")):
            return self._tokens_aten(self.logmel_aten(waveform), stripes, lam).to(out_dtype)
        melW, pe = self.logmel_extractor.melW, self.patch_embed
        if self.training:
            lm, mean, var = ops.logmel(waveform.contiguous(), melW, want_stats=True, lib=self.lib, ranges=self._mel_ranges())
            scale, shift = self._bn_affine(mean, var, B * T)
        else:
            lm = ops.logmel(waveform.contiguous(), melW, lib=self.lib, ranges=self._mel_ranges())
            scale, shift = self._bn_affine(None, None, B * T)
        return ops.patch_embed(lm, *pe._frozen_params(), pe.norm.eps, out_dtype=out_dtype, bn_scale=scale, bn_shift=shift, lib=self.lib,
                               stripes=stripes, mixup_lambda=lam)
