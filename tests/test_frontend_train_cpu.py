"""The trainable front end (``HTSATFrontEnd(trainable=True)`` / ``PatchEmbed(trainable=True)``) without a GPU: the ATen formulation
(fused=False) under plain autograd against a differentiable float64 restatement, what stays frozen, the state-dict keys, the AVS-S4 name
rule, and the C symbols of the parameter-gradient backward.

Reference: ``F.batch_norm`` -> stretch with ``frontend_ref.bicubic_matrix`` -> fold -> ``F.conv2d`` -> ``F.layer_norm`` in float64, fed
``frontend_ref.logmel(frontend_ref.signal(B, L))`` and the parameters of ``frontend_ref.randomise(module, 2)``; the cotangent is
``randn`` with seed 11, rounded to the token dtype before both sides use it.  Bound: ``helpers.fp32_err < 1e-3`` on each of the six
gradients (the fp32 ATen evaluation of this restatement sits at 2e-7 .. 4e-6 from float64 on all six)."""
import ctypes
import os
import re
import sys

import pytest
import torch
import torch.nn.functional as F

import dgsct_amd
from dgsct_amd import HTSATFrontEnd, PatchEmbed, ops, train

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import frontend_ref as R                    # noqa: E402
from helpers import ROOT, fp32_err          # noqa: E402

SIX = ("bn0.weight", "bn0.bias", "patch_embed.proj.weight", "patch_embed.proj.bias", "patch_embed.norm.weight", "patch_embed.norm.bias")
FOUR = ("proj.weight", "proj.bias", "norm.weight", "norm.bias")


def cotangent(shape, dtype=torch.float32):
    """randn with seed 11, rounded to the token dtype"""
    return torch.randn(shape, generator=torch.Generator().manual_seed(11)).to(dtype)


def audio_grads64(lm, sd, training, cot):
    """float64 gradients of the six tensors: sum(tokens * cot) differentiated through batch_norm -> stretch -> fold -> conv2d -> layer_norm.
    lm [B, T, 64] float64, sd the module's state dict before the call, cot [B, 4096, E]."""
    lm = lm.double()
    B, T, _ = lm.shape
    p = {k: sd[k].detach().double().cpu().clone().requires_grad_(True) for k in SIX}
    x = F.batch_norm(lm.transpose(1, 2).unsqueeze(-1), sd["bn0.running_mean"].double().cpu().clone(), sd["bn0.running_var"].double().cpu().clone(),
                     p["bn0.weight"], p["bn0.bias"], training, 0.1, 1e-5)                 # [B, 64, T, 1]
    x = x.squeeze(-1).transpose(1, 2)                                                      # [B, T, 64]
    x = torch.einsum("ot,btf->bof", torch.from_numpy(R.bicubic_matrix(T, 1024)), x)        # [B, 1024, 64]
    img = x.reshape(B, 4, 256, R.N_MELS).permute(0, 1, 3, 2).reshape(B, 1, 256, 256)       # image[q*64 + f][t'] = x[q*256 + t'][f]
    y = F.conv2d(img, p["patch_embed.proj.weight"], p["patch_embed.proj.bias"], stride=4).flatten(2).transpose(1, 2)
    tok = F.layer_norm(y, (y.shape[-1],), p["patch_embed.norm.weight"], p["patch_embed.norm.bias"], 1e-5)
    (tok * cot.double().cpu()).sum().backward()
    return {k: v.grad for k, v in p.items()}, tok.detach()


def image_grads64(img, sd, cot):
    """float64 gradients of proj.* / norm.* through conv2d + layer_norm"""
    p = {k: sd[k].detach().double().cpu().clone().requires_grad_(True) for k in FOUR}
    y = F.conv2d(img.detach().double().cpu(), p["proj.weight"], p["proj.bias"], stride=4).flatten(2).transpose(1, 2)
    tok = F.layer_norm(y, (y.shape[-1],), p["norm.weight"], p["norm.bias"], 1e-5)
    (tok * cot.double().cpu()).sum().backward()
    return {k: v.grad for k, v in p.items()}, tok.detach()


def module_grads(m, names=SIX):
    g = dict(m.named_parameters())
    return {k: g[k].grad for k in names}


@pytest.mark.parametrize("training", [False, True], ids=["eval", "train"])
def test_aten_gradients_against_float64(training):
    B, L = 2, 3200
    x = R.signal(B, L)
    m = R.randomise(HTSATFrontEnd(fused=False, trainable=True), 2).train(training)
    sd0 = {k: v.clone() for k, v in m.state_dict().items()}
    cot = cotangent((B, 4096, 96))
    ref, tok64 = audio_grads64(R.logmel(x), sd0, training, cot)
    tok = m(x)
    assert tok.requires_grad and tok.dtype == torch.float32 and fp32_err(tok, tok64) < 1e-3
    tok.backward(cot)
    got = module_grads(m)
    for k in SIX:
        err = fp32_err(got[k], ref[k])
        print(f"{k} training={training}: {err:.3e}")
        assert err < 1e-3, k
    assert m.logmel_extractor.melW.grad is None
    assert int(m.bn0.num_batches_tracked) == int(training)                  # once per forward, as the frozen module


def test_patch_embed_aten_gradients_against_float64():
    g = torch.Generator().manual_seed(7)
    img = torch.randn(2, 3, 32, 32, generator=g)
    m = R.randomise(PatchEmbed(32, in_chans=3, embed_dim=128, fused=False, trainable=True), 8)
    cot = cotangent((2, 64, 128))
    ref, _ = image_grads64(img, m.state_dict(), cot)
    m(img).backward(cot)
    for k in FOUR:
        assert fp32_err(dict(m.named_parameters())[k].grad, ref[k]) < 1e-3, k


def test_default_modules_stay_frozen_and_unchanged():
    x = R.signal(2, 3200)
    a, b = R.randomise(HTSATFrontEnd(fused=False), 2).eval(), R.randomise(HTSATFrontEnd(fused=False, trainable=True), 2).eval()
    assert not any(p.requires_grad for p in a.parameters()) and not a.trainable
    ta = a(x)
    assert not ta.requires_grad
    tb = b(x)
    assert tb.requires_grad and torch.equal(ta, tb.detach())
    with torch.no_grad():
        assert not b(x).requires_grad
    # a trainable module whose parameters were all frozen again runs the frozen path
    b.requires_grad_(False)
    assert not b(x).requires_grad
    p = PatchEmbed(32, in_chans=3, embed_dim=96, fused=False)
    assert not any(q.requires_grad for q in p.parameters()) and not p(torch.zeros(1, 3, 32, 32)).requires_grad
    with pytest.raises(RuntimeError, match="requires grad"):
        HTSATFrontEnd(fused=False, trainable=True)(torch.zeros(1, 3200, requires_grad=True))
    with pytest.raises(RuntimeError, match="requires grad"):
        PatchEmbed(32, fused=False, trainable=True)(torch.zeros(1, 3, 32, 32, requires_grad=True))


def test_trainable_never_unfreezes_melW():
    m = HTSATFrontEnd(trainable=True)
    req = {k for k, p in m.named_parameters() if p.requires_grad}
    assert req == set(SIX)
    assert not m.logmel_extractor.melW.requires_grad
    assert {k for k, p in PatchEmbed(32, trainable=True).named_parameters() if p.requires_grad} == set(FOUR)
    m.logmel_extractor.melW.requires_grad_(True)                            # ... and a gradient into it is refused, not dropped
    with pytest.raises(RuntimeError, match="melW"):
        m(torch.zeros(1, 3200))


def test_state_dict_keys_do_not_change():
    assert set(HTSATFrontEnd(trainable=True).state_dict()) == set(HTSATFrontEnd().state_dict())
    assert set(PatchEmbed(32, trainable=True).state_dict()) == set(PatchEmbed(32).state_dict())
    src = R.randomise(HTSATFrontEnd(), 1)
    dst = HTSATFrontEnd(trainable=True)
    res = dst.load_state_dict(src.state_dict(), strict=True)
    assert not res.missing_keys and not res.unexpected_keys


def test_avs_s4_name_rule_selects_the_six_tensors():
    class Model(torch.nn.Module):
        def __init__(self):
            super().__init__()
            self.htsat = HTSATFrontEnd(fused=False, trainable=True)
            self.swin = PatchEmbed(32, in_chans=3, embed_dim=96, fused=False, trainable=True)

    model = Model()
    train.trainable_by_name(model.named_parameters(), task="avs_s4")
    req = {k for k, p in model.named_parameters() if p.requires_grad}
    assert {"htsat." + k for k in SIX} <= req
    assert not any(k.startswith("swin.") for k in req)
    # the reference's loop sets requires_grad on EVERY parameter outside 'ViT' / 'swin', its mel matrix included; no gradient into melW is
    # built here, so it is frozen again by hand (HTSATFrontEnd raises otherwise)
    assert req - {"htsat." + k for k in SIX} == {"htsat.logmel_extractor.melW"}
    # "ave" freezes everything under 'htsat'
    train.trainable_by_name(model.named_parameters(), task="ave")
    assert not any(p.requires_grad for k, p in model.named_parameters() if k.startswith("htsat."))


def test_header_and_library_declare_the_backward():
    with open(os.path.join(ROOT, "include", "dgsct.h")) as f:
        text = f.read()
    assert re.search(r"int64_t\s+dgsct_patch_embed_params_ws_floats\s*\(", text)
    assert re.search(r"int\s+dgsct_patch_embed_backward_params\s*\(", text)
    assert re.search(r"#define\s+DGSCT_VERSION\s+101\b", text)
    lib = dgsct_amd.default_lib()
    c = ctypes.CDLL(lib.path)
    assert c.dgsct_patch_embed_params_ws_floats is not None and c.dgsct_patch_embed_backward_params is not None
    assert c.dgsct_version() == 101
    assert lib.has_patch_embed_params()
    assert callable(ops.patch_embed_train)
    # workspace: one row per workgroup, a workgroup per 16 tokens up to 1024; row = (K + 3) C (+ 2 x 64 bn0 sums in audio mode)
    assert lib.patch_embed_params_ws_floats(ops._lib.PATCH_AUDIO, 2, 1, 256, 256, 96) == 512 * (19 * 96 + 128)
    assert lib.patch_embed_params_ws_floats(ops._lib.PATCH_AUDIO, 160, 1, 256, 256, 96) == 1024 * (19 * 96 + 128)
    assert lib.patch_embed_params_ws_floats(ops._lib.PATCH_IMAGE, 1, 1, 4, 12, 96) == 1 * 19 * 96
    assert lib.patch_embed_params_ws_floats(ops._lib.PATCH_IMAGE, 2, 3, 32, 32, 128) == 8 * 51 * 128
    with pytest.raises(RuntimeError, match="multiple of 32"):
        lib.patch_embed_params_ws_floats(ops._lib.PATCH_IMAGE, 2, 3, 32, 32, 100)
    with pytest.raises(RuntimeError, match="in_chans 1 or 3"):
        lib.patch_embed_params_ws_floats(ops._lib.PATCH_IMAGE, 2, 2, 32, 32, 96)


def test_emulation_has_no_backward_and_the_kernel_path_says_so():
    sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "emu"))
    from build_emu import build_emu
    from dgsct_amd._lib import Lib
    emu = Lib(build_emu())
    assert not emu.has_patch_embed_params()
    with pytest.raises(RuntimeError, match="dgsct_patch_embed_params_ws_floats"):
        emu.patch_embed_params_ws_floats(0, 1, 3, 32, 32, 96)
    with pytest.raises(RuntimeError, match="CUDA/HIP"):
        HTSATFrontEnd(fused=True, trainable=True)(torch.zeros(1, 3200))
    p = PatchEmbed(32, fused=False, trainable=True)
    with pytest.raises(RuntimeError, match="CUDA/HIP"):
        ops.patch_embed_train(torch.zeros(1, 3, 32, 32), p.proj.weight, p.proj.bias, p.norm.weight, p.norm.bias)
