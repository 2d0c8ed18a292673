"""The audio / image front ends on the device (csrc/frontend.hip through default_lib()) against the float64 reference of
tests/frontend_ref.py.

Log-mel bound: 8 x the error of an fp32 ATen evaluation (the module's fused=False path on the CPU) of the same input against the same
reference, in dB -- a few ulp of log10 at |20 dB|; reduced-precision twiddles, a wrong reflection index or an off-by-one frame start near
1e-2 dB.  Tokens: helpers.fp32_err < 1e-3 (fp32 output), helpers.nrm_err < 1e-2 (bf16 output), the project's two bounds."""
import functools
import os
import sys

import pytest
import torch

import dgsct_amd
from dgsct_amd import HTSATFrontEnd, PatchEmbed, ops

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import frontend_ref as R                    # noqa: E402
from helpers import fp32_err, nrm_err       # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda:0"

#        (B, L)            frames   what it exercises
CASES = [(2, 3200),      # T = 11   smallest interpolation source, odd T
         (3, 5000),      # T = 16   L not a multiple of the hop, odd B T
         (1, 327360),    # T = 1024 exact-copy path (no interpolation)
         (1, 320000)]    # T = 1001 one real-length waveform
IDS = ["smallest", "ragged", "no-interp", "real-length"]


@functools.lru_cache(maxsize=None)
def _case(B, L):
    """(waveform, float64 log-mel, error of the fp32 ATen log-mel on the CPU in dB): computed once, shared, never modified"""
    x = R.signal(B, L)
    ref = R.logmel(x)
    aten = HTSATFrontEnd(fused=False).logmel_aten(x)
    return x, ref, (aten.double() - ref).abs().max().item()


@functools.lru_cache(maxsize=None)
def _tokens_ref(B, L, training):
    _, ref, _ = _case(B, L)
    return R.audio_tokens(ref, _module().state_dict(), training)


def _module(**kw):
    return R.randomise(HTSATFrontEnd(**kw), 2)


@pytest.mark.parametrize("B,L", CASES, ids=IDS)
def test_logmel(B, L):
    x, ref, aten_err = _case(B, L)
    m = HTSATFrontEnd().to(DEV)
    lm = ops.logmel(x.to(DEV), m.logmel_extractor.melW)
    assert lm.shape == ref.shape and lm.dtype == torch.float32
    err = (lm.double().cpu() - ref).abs().max().item()
    print(f"logmel [{B}, {L}]: device {err:.3e} dB, fp32 ATen {aten_err:.3e} dB, ratio {err / aten_err:.2f}; "
          f"range {ref.min().item():.1f} .. {ref.max().item():.1f} dB")
    assert err <= 8.0 * aten_err
    # the dense product (no ranges table) gives the same numbers up to the order of the sum
    dense = torch.stack([torch.zeros(64), torch.full((64,), 513.0)], 1).to(torch.int32).to(DEV)
    lm2 = ops.logmel(x.to(DEV), m.logmel_extractor.melW, ranges=dense)
    assert (lm2.double().cpu() - ref).abs().max().item() <= 8.0 * aten_err


@pytest.mark.parametrize("B,L", CASES[:2], ids=IDS[:2])
def test_logmel_statistics(B, L):
    x, ref, _ = _case(B, L)
    m = HTSATFrontEnd().to(DEV)
    lm, mean, var = ops.logmel(x.to(DEV), m.logmel_extractor.melW, want_stats=True)
    assert torch.equal(lm, ops.logmel(x.to(DEV), m.logmel_extractor.melW))
    rmean, rvar = ref.mean((0, 1)), ref.var((0, 1), unbiased=False)
    # both within 1e-4 (the mean in units of the bin's spread).  The narrowest bins hold the two tones: variance ~0.05 dB^2 (spread 0.23 dB)
    # around a mean near 20 dB.  A log-mel error of e ~ 2e-5 dB, uncorrelated over the n >= 22 frames, moves the mean by e / sqrt(n) and the
    # variance by 2 e sigma / sqrt(n): ~2e-5 and ~4e-5 relative to the spread / the variance.  The accumulation itself must add nothing
    # visible to that: plain fp32 sums of v and v^2 do not qualify (E[v^2] - mean^2 cancels ~400 against 0.05: ~2e-4 here)
    assert ((mean.double().cpu() - rmean).abs() / rvar.sqrt()).max().item() < 1e-4
    assert ((var.double().cpu() - rvar).abs() / rvar).max().item() < 1e-4


@pytest.mark.parametrize("training", [False, True], ids=["eval", "train"])
@pytest.mark.parametrize("B,L", CASES, ids=IDS)
def test_tokens_fp32(B, L, training):
    x = _case(B, L)[0]
    ref, rm, rv = _tokens_ref(B, L, training)
    m = _module().to(DEV).train(training)
    tok = m(x.to(DEV))
    assert tok.shape == (B, 4096, 96) and tok.dtype == torch.float32
    err = fp32_err(tok, ref)
    print(f"tokens fp32 [{B}, {L}] training={training}: {err:.3e}")
    assert err < 1e-3
    if training:
        assert int(m.bn0.num_batches_tracked) == 1
        assert ((m.bn0.running_mean.double().cpu() - rm).abs() / rm.abs().clamp_min(1e-3)).max().item() < 1e-4
        assert ((m.bn0.running_var.double().cpu() - rv).abs() / rv).max().item() < 1e-4
    else:
        assert int(m.bn0.num_batches_tracked) == 0


@pytest.mark.parametrize("B,L", CASES, ids=IDS)
def test_tokens_bf16(B, L):
    x = _case(B, L)[0]
    ref = _tokens_ref(B, L, False)[0]
    tok = _module(out_dtype=torch.bfloat16).to(DEV).eval()(x.to(DEV))
    assert tok.dtype == torch.bfloat16
    err = nrm_err(tok, ref)
    print(f"tokens bf16 [{B}, {L}]: {err:.3e}")
    assert err < 1e-2


@pytest.mark.parametrize("training", [False, True], ids=["eval", "train"])
@pytest.mark.parametrize("B,L", CASES, ids=IDS)
def test_fused_against_aten(B, L, training):
    x = _case(B, L)[0].to(DEV)
    fused, aten = _module().to(DEV).train(training), _module(fused=False).to(DEV).train(training)
    a, b = fused(x), aten(x)
    assert fp32_err(a, b) < 1e-3
    if training:
        assert ((fused.bn0.running_mean - aten.bn0.running_mean).abs() / aten.bn0.running_mean.abs().clamp_min(1e-3)).max().item() < 1e-4
        assert ((fused.bn0.running_var - aten.bn0.running_var).abs() / aten.bn0.running_var).max().item() < 1e-4
    fused.out_dtype = torch.bfloat16
    fused.eval(); aten.eval()
    assert nrm_err(fused(x), aten(x)) < 1e-2


@pytest.mark.parametrize("in_dtype,out_dtype", [(torch.float32, torch.float32), (torch.bfloat16, torch.bfloat16),
                                                (torch.bfloat16, torch.float32), (torch.float32, torch.bfloat16)],
                         ids=["f32-f32", "bf16-bf16", "bf16-f32", "f32-bf16"])
@pytest.mark.parametrize("shape,C", [((2, 3, 192, 192), 128), ((1, 3, 192, 192), 192), ((2, 1, 32, 32), 96)], ids=["swinB", "swinL", "mono32"])
def test_patch_embed_image(shape, C, in_dtype, out_dtype):
    g = torch.Generator().manual_seed(7)
    img = torch.randn(shape, generator=g).to(in_dtype)
    m = R.randomise(PatchEmbed(shape[2:], in_chans=shape[1], embed_dim=C, out_dtype=out_dtype), 8)
    ref = R.patch_tokens(img, m.state_dict())
    m = m.to(DEV)
    tok = m(img.to(DEV))
    assert tok.shape == ref.shape and tok.dtype == out_dtype
    if out_dtype == torch.float32:
        assert fp32_err(tok, ref) < 1e-3
    else:
        assert nrm_err(tok, ref) < 1e-2
    aten = PatchEmbed(shape[2:], in_chans=shape[1], embed_dim=C, out_dtype=out_dtype, fused=False).to(DEV)
    aten.load_state_dict(m.state_dict())
    if out_dtype == torch.float32:
        assert fp32_err(tok, aten(img.to(DEV))) < 1e-3
    else:
        assert nrm_err(tok, aten(img.to(DEV))) < 1e-2


def test_calls_go_through_default_lib(monkeypatch):
    lib = dgsct_amd.default_lib()
    seen = []
    for name in ("logmel_forward", "patch_embed_forward"):
        real = getattr(lib, name)
        monkeypatch.setattr(lib, name, lambda *a, _real=real, _name=name, **k: (seen.append(_name), _real(*a, **k))[1])
    x = _case(2, 3200)[0].to(DEV)
    _module().to(DEV).train()(x)
    PatchEmbed(32, in_chans=3, embed_dim=96).to(DEV)(torch.zeros(1, 3, 32, 32, device=DEV))
    assert seen == ["logmel_forward", "patch_embed_forward", "patch_embed_forward"]      # three launches' worth of calls, then the image


def test_device_argument_checks():
    m = HTSATFrontEnd().to(DEV)
    W = m.logmel_extractor.melW
    with pytest.raises(RuntimeError, match="contiguous fp32"):
        ops.logmel(torch.zeros(2, 6400, device=DEV)[:, ::2], W)
    with pytest.raises(RuntimeError, match="melW"):
        ops.logmel(torch.zeros(2, 3200, device=DEV), W[:, :32].contiguous())
    with pytest.raises(RuntimeError, match="forward-only"):
        ops.logmel(torch.zeros(2, 3200, device=DEV, requires_grad=True), W)
    with pytest.raises(RuntimeError, match="frames"):
        ops.logmel(torch.zeros(1, 320 * 1024, device=DEV), W)
    pe = m.patch_embed
    with pytest.raises(RuntimeError, match="log-mel"):
        ops.patch_embed(torch.zeros(1, 11, 32, device=DEV), pe.proj.weight, pe.proj.bias, pe.norm.weight, pe.norm.bias,
                        bn_scale=torch.ones(64, device=DEV), bn_shift=torch.zeros(64, device=DEV))
    with pytest.raises(RuntimeError, match="weight"):
        ops.patch_embed(torch.zeros(1, 3, 32, 32, device=DEV), pe.proj.weight, pe.proj.bias, pe.norm.weight, pe.norm.bias)
