"""float64 reference of the audio / image front ends for tests/test_frontend_*.py, written from the published formulas and
independently of dg-sct_amd/frontend.py (nothing is imported from the package): centred reflect-padded periodic-Hann STFT through
np.fft.rfft, the Slaney mel filterbank, 10 log10, BatchNorm, PyTorch's bicubic kernel (A = -0.75, align_corners) as a dense matrix, the
HTS-AT fold, and conv + LayerNorm in float64."""
import functools
import math

import numpy as np
import torch
import torch.nn.functional as F

SR, N_FFT, HOP, N_MELS, FMIN, FMAX = 32000, 1024, 320, 64, 50.0, 14000.0


def signal(B, L, seed=0):
    """broadband test input [B, L] fp32: 0.1 randn + 0.3 sin(2 pi 440 t) + 0.2 sin(2 pi 5000 t)"""
    g = torch.Generator().manual_seed(seed)
    t = torch.arange(L, dtype=torch.float64) / SR
    x = 0.1 * torch.randn(B, L, generator=g, dtype=torch.float64) + 0.3 * torch.sin(2 * math.pi * 440 * t) + 0.2 * torch.sin(2 * math.pi * 5000 * t)
    return x.float()


def _hz_to_mel(f):
    f = np.asarray(f, dtype=np.float64)
    return np.where(f >= 1000.0, 15.0 + np.log(np.maximum(f, 1e-30) / 1000.0) / (np.log(6.4) / 27.0), f * 3.0 / 200.0)


def _mel_to_hz(m):
    m = np.asarray(m, dtype=np.float64)
    return np.where(m >= 15.0, 1000.0 * np.exp((np.log(6.4) / 27.0) * (m - 15.0)), m * 200.0 / 3.0)


@functools.lru_cache(maxsize=None)
def slaney_melW():
    """[513, 64] float64 numpy: triangular filters on the Slaney mel scale, area-normalised (2 / bandwidth)"""
    edges = _mel_to_hz(np.linspace(_hz_to_mel(FMIN), _hz_to_mel(FMAX), N_MELS + 2))
    freqs = np.arange(N_FFT // 2 + 1, dtype=np.float64) * SR / N_FFT
    W = np.zeros((N_FFT // 2 + 1, N_MELS))
    for m in range(N_MELS):
        lo, ce, hi = edges[m], edges[m + 1], edges[m + 2]
        tri = np.minimum((freqs - lo) / (ce - lo), (hi - freqs) / (hi - ce))
        W[:, m] = np.maximum(tri, 0.0) * 2.0 / (hi - lo)
    return W


def hann_basis():
    """(real, imag) [513, 1, 1024] float64 torch: the Hann-windowed DFT basis of the reference checkpoint's STFT convolutions"""
    n = np.arange(N_FFT)
    win = 0.5 - 0.5 * np.cos(2 * np.pi * n / N_FFT)
    ang = 2 * np.pi * np.outer(np.arange(N_FFT // 2 + 1), n) / N_FFT
    return torch.from_numpy(np.cos(ang) * win).unsqueeze(1), torch.from_numpy(-np.sin(ang) * win).unsqueeze(1)


def logmel(wave, melW=None):
    """wave [B, L] -> [B, T, 64] float64 torch"""
    x = wave.detach().double().cpu().numpy()
    melW = slaney_melW() if melW is None else melW.detach().double().cpu().numpy()
    B, L = x.shape
    T = L // HOP + 1
    xp = np.pad(x, ((0, 0), (N_FFT // 2, N_FFT // 2)), mode="reflect")
    idx = HOP * np.arange(T)[:, None] + np.arange(N_FFT)[None, :]
    win = 0.5 - 0.5 * np.cos(2 * np.pi * np.arange(N_FFT) / N_FFT)
    spec = np.fft.rfft(xp[:, idx] * win, axis=-1)                              # [B, T, 513]
    power = spec.real ** 2 + spec.imag ** 2
    return torch.from_numpy(10.0 * np.log10(np.maximum(power @ melW, 1e-10)))


def bicubic_matrix(n_in, n_out):
    """[n_out, n_in] float64: PyTorch's bicubic interpolation along one axis, align_corners=True, A = -0.75, taps clamped"""
    A = -0.75
    M = np.zeros((n_out, n_in))
    if n_in == n_out:
        return np.eye(n_in)
    inner = lambda x: ((A + 2.0) * x - (A + 3.0)) * x * x + 1.0               # |x| <= 1
    outer = lambda x: ((A * x - 5.0 * A) * x + 8.0 * A) * x - 4.0 * A          # 1 < |x| < 2
    for o in range(n_out):
        src = o * (n_in - 1) / (n_out - 1)
        i0 = int(math.floor(src))
        t = src - i0
        for tap, wgt in zip((i0 - 1, i0, i0 + 1, i0 + 2), (outer(t + 1.0), inner(t), inner(1.0 - t), outer(2.0 - t))):
            M[o, min(max(tap, 0), n_in - 1)] += wgt
    return M


def patch_tokens(img, sd, prefix=""):
    """img [B, C, H, W] -> [B, (H/4)(W/4), E] float64: F.conv2d + F.layer_norm in float64 on the CPU"""
    w, b = sd[prefix + "proj.weight"].double().cpu(), sd[prefix + "proj.bias"].double().cpu()
    x = F.conv2d(img.detach().double().cpu(), w, b, stride=4).flatten(2).transpose(1, 2)
    return F.layer_norm(x, (w.shape[0],), sd[prefix + "norm.weight"].double().cpu(), sd[prefix + "norm.bias"].double().cpu(), 1e-5)


def audio_tokens(lm, sd, training):
    """log-mel [B, T, 64] float64 + the module's state dict (BEFORE the call) -> (tokens [B, 4096, E], running_mean', running_var') float64.
    bn0: batch statistics over (B, T) per mel bin in training mode (biased variance normalises, the unbiased one updates), else running."""
    lm = lm.double()
    B, T, _ = lm.shape
    g, be = sd["bn0.weight"].double().cpu(), sd["bn0.bias"].double().cpu()
    rm, rv = sd["bn0.running_mean"].double().cpu(), sd["bn0.running_var"].double().cpu()
    if training:
        n = B * T
        mean, var = lm.mean((0, 1)), lm.var((0, 1), unbiased=False)
        rm, rv = 0.9 * rm + 0.1 * mean, 0.9 * rv + 0.1 * var * n / (n - 1)
    else:
        mean, var = rm, rv
    x = (lm - mean) / torch.sqrt(var + 1e-5) * g + be
    x = torch.einsum("ot,btf->bof", torch.from_numpy(bicubic_matrix(T, 1024)), x)          # [B, 1024, 64]
    img = x.reshape(B, 4, 256, N_MELS).permute(0, 1, 3, 2).reshape(B, 1, 256, 256)           # image[q*64 + f][t'] = x[q*256 + t'][f]
    return patch_tokens(img, sd, "patch_embed."), rm, rv


def randomise(module, seed):
    """non-trivial frozen parameters: BatchNorm / LayerNorm affines and running statistics away from their identity defaults"""
    g = torch.Generator().manual_seed(seed)
    with torch.no_grad():
        for name, t in module.state_dict().items():
            if name.endswith("num_batches_tracked") or name.endswith("melW"):
                continue
            r = torch.randn(t.shape, generator=g)
            if name.endswith("running_var"):
                t.copy_(30.0 + 20.0 * torch.rand(t.shape, generator=g))
            elif name.endswith("running_mean"):
                t.copy_(-5.0 + 3.0 * r)
            elif name.endswith("norm.weight") or name.endswith("bn0.weight"):
                t.copy_(1.0 + 0.2 * r)
            elif name.endswith("bias"):
                t.copy_(0.2 * r)
            else:
                t.copy_(0.25 * r)
    return module
