"""SpecAugment stripes and mix-up inside the front-end kernels: ``dgsct_patch_embed_forward_aug`` / ``dgsct_patch_embed_backward_params_aug``
(csrc/frontend.hip, the AUG instantiations of ``patch_embed_k`` / ``patch_embed_bwd_k``) through ``HTSATFrontEnd(fused=True)`` in train mode
with explicit ``stripes=`` / ``mixup_lambda=``, against the float64 restatement of tests/frontend_aug_ref.py.

Bounds, those of tests/test_frontend_train_gpu.py: ``helpers.fp32_err < 1e-3`` on fp32 tokens and on every gradient for fp32 AND bf16 tokens
(the backward recomputes in fp32 from a dOut that is exact in either dtype), ``helpers.nrm_err < 1e-2`` on bf16 tokens.

Shapes (the smallest ones of the un-augmented tests) and what the stripe tables put on them:
    (2, 3200)    T = 11    every stretched frame has taps on both sides of a stripe edge or clamped at an end; overlapping time stripes from
                           frame 0, a stripe holding frame T-1, an empty stripe, mel stripes [3, 6) (across a patch row), at bin 0 and at bin 63;
                           the partner is the other sample
    (3, 5000)    T = 16    odd B: the middle sample mixes with itself; sample 2 loses every frame (R = K = 0: its tokens are LayerNorm(bias));
                           lambda 0.3 / 0 / 1
    (1, 327360)  T = 1024  the one-tap path; the sample is its own partner
    (8, 3200)    T = 11    one backward with the grid-stride loop carried (see test_frontend_train_gpu.test_carried_accumulators)"""
import functools
import os
import sys

import pytest
import torch
import torch.nn.functional as F

import dgsct_amd
from dgsct_amd import HTSATFrontEnd, frontend, ops

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import frontend_aug_ref as A                # noqa: E402
import frontend_ref as R                    # noqa: E402
from helpers import fp32_err, nrm_err       # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
SIX = A.SIX


def _table(rows):
    return torch.tensor(rows, dtype=torch.int32)


#         name          B  L        stripes [B][4][2]: time, time, mel, mel                                              lambda
CASES = {
    "smallest":  (2, 3200,   [[[0, 3], [2, 5], [3, 6], [0, 2]], [[10, 11], [4, 4], [60, 64], [7, 7]]],                    [0.3, 1.0]),
    "odd-B":     (3, 5000,   [[[15, 16], [0, 1], [31, 33], [63, 64]], [[5, 9], [7, 12], [0, 1], [20, 20]],
                              [[0, 16], [3, 3], [8, 12], [40, 47]]],                                                       [0.3, 0.0, 1.0]),
    "no-interp": (1, 327360, [[[0, 40], [1000, 1024], [3, 6], [58, 64]]],                                                  [0.3]),
    "carried":   (8, 3200,   [[[(3 * i) % 11, min((3 * i) % 11 + i % 4, 11)], [10 - i, 11 - (i % 2)], [(9 * i) % 64, min((9 * i) % 64 + i, 64)],
                               [4 * i + 3, 4 * i + 6]] for i in range(8)],                                                 [0.0, 1.0, 0.3, 0.5, 0.9, 0.3, 1.0, 0.0]),
}


def _operands(case, what="both"):
    """(B, L, stripes int32 [B, 4, 2] | None, lam fp32 [B] | None) on the host"""
    B, L, rows, lam = CASES[case]
    return B, L, (_table(rows) if what in ("both", "stripes") else None), (torch.tensor(lam) if what in ("both", "lambda") else None)


def cotangent(shape, dtype=torch.float32):
    """randn with seed 11, rounded to the token dtype"""
    return torch.randn(shape, generator=torch.Generator().manual_seed(11)).to(dtype)


@functools.lru_cache(maxsize=None)
def _wave(B, L):
    """(waveform, float64 log-mel): computed once, shared, never modified"""
    x = R.signal(B, L)
    return x, R.logmel(x)


def _module(embed=96, **kw):
    return R.randomise(HTSATFrontEnd(embed_dim=embed, **kw), 2)


@functools.lru_cache(maxsize=None)
def _reference(case, what, embed, dtype):
    """(float64 gradients, float64 tokens, running_mean', running_var') for the cotangent of this dtype"""
    B, L, stripes, lam = _operands(case, what)
    lm = _wave(B, L)[1]
    sd = _module(embed).state_dict()
    grads, tok = A.audio_grads64(lm, sd, True, cotangent((B, 4096, embed), dtype), stripes, lam)
    _, rm, rv = R.audio_tokens(lm, sd, True)
    return grads, tok, rm, rv


def module_grads(m):
    g = dict(m.named_parameters())
    return {k: g[k].grad for k in SIX}


def _check(case, what, embed, dtype):
    B, L, stripes, lam = _operands(case, what)
    x = _wave(B, L)[0].to(DEV)
    ref, tok64, rm, rv = _reference(case, what, embed, dtype)
    m = _module(embed, out_dtype=dtype, trainable=True, fused=True).to(DEV).train()
    tok = m(x, mixup_lambda=lam, stripes=stripes)
    assert tok.shape == (B, 4096, embed) and tok.dtype == dtype and tok.requires_grad
    assert "PatchEmbedTrain" in type(tok.grad_fn).__name__
    err = fp32_err(tok, tok64) if dtype == torch.float32 else nrm_err(tok, tok64)
    print(f"{case} {what} embed={embed} {dtype} tokens: {err:.3e}")
    assert err < (1e-3 if dtype == torch.float32 else 1e-2)
    frozen = _module(embed, out_dtype=dtype, fused=True).to(DEV).train()
    assert torch.equal(tok.detach(), frozen(x, mixup_lambda=lam, stripes=stripes))       # bit for bit the frozen module's tokens
    tok.backward(cotangent((B, 4096, embed), dtype).to(DEV))
    got = module_grads(m)
    for k in SIX:
        assert got[k].dtype == torch.float32 and got[k].shape == ref[k].shape, k
        err = fp32_err(got[k], ref[k])
        print(f"{case} {what} embed={embed} {dtype} {k}: {err:.3e}")
        assert err < 1e-3, k
    assert m.logmel_extractor.melW.grad is None
    # bn0 saw the un-augmented log-mel: the running statistics are those of a plain run, bit for bit
    plain = _module(embed, out_dtype=dtype, fused=True).to(DEV).train()
    plain(x)
    assert int(m.bn0.num_batches_tracked) == 1
    for mod in (m, frozen):
        assert torch.equal(mod.bn0.running_mean, plain.bn0.running_mean) and torch.equal(mod.bn0.running_var, plain.bn0.running_var)
    assert ((m.bn0.running_mean.double().cpu() - rm).abs() / rm.abs().clamp_min(1e-3)).max().item() < 1e-4
    assert ((m.bn0.running_var.double().cpu() - rv).abs() / rv).max().item() < 1e-4
    return m, tok.detach(), tok64


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["fp32", "bf16"])
@pytest.mark.parametrize("case", ["smallest", "odd-B", "no-interp"])
def test_stripes_and_lambda(case, dtype):
    m, tok, tok64 = _check(case, "both", 96, dtype)
    if case == "odd-B":
        # sample 2 has every frame dropped and lambda 1: R = K = 0, the convolution is its bias, every token LayerNorm(bias)
        pe = m.patch_embed
        want = F.layer_norm(pe.proj.bias.detach(), (96,), pe.norm.weight.detach(), pe.norm.bias.detach(), pe.norm.eps)
        assert torch.equal(tok[2], tok[2, :1].expand(4096, 96))
        assert (fp32_err(tok[2, 0], want) < 1e-3) if dtype == torch.float32 else (nrm_err(tok[2, 0], want) < 1e-2)
        # sample 1 is its own partner with lambda 0: its own stripes, nothing of the others
        assert not torch.equal(tok[1], tok[2])


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["fp32", "bf16"])
@pytest.mark.parametrize("what", ["stripes", "lambda"])
def test_one_augmentation_alone(what, dtype):
    """stripes with lam = NULL, lam with stripes = NULL: the two operands are independent"""
    _check("odd-B", what, 96, dtype)


def test_own_partner_at_1024_frames():
    """B = 1: the sample mixes with itself, lam x + (1 - lam) x, so lambda changes nothing but rounding"""
    B, L, stripes, lam = _operands("no-interp")
    x = _wave(B, L)[0].to(DEV)
    m = _module(fused=True).to(DEV).train()
    with_lam, without = m(x, mixup_lambda=lam, stripes=stripes), m(x, stripes=stripes)
    tok64 = _reference("no-interp", "stripes", 96, torch.float32)[1]
    assert fp32_err(with_lam, without) < 1e-3 and fp32_err(with_lam, tok64) < 1e-3 and fp32_err(without, tok64) < 1e-3
    assert fp32_err(m(x), tok64) > 1e-2                                      # ... and the stripes are visible


@pytest.mark.parametrize("embed,dtype", [(32, torch.float32), (160, torch.bfloat16)], ids=["NJ1", "NJ3-lanes-past-C"])
def test_other_widths(embed, dtype):
    """embed 32: one channel per lane and half the lanes past C; embed 160: three channels per lane, lanes 32 .. 63 past C in the third"""
    _check("odd-B", "both", embed, dtype)


def test_carried_accumulators():
    """8 x 4096 tokens = 8192 four-token groups on at most 1024 workgroups of 4 waves: every wave runs its loop at least twice and carries
    its register accumulators and its LDS bins (now fed by K as well) from one group to the next"""
    lib = dgsct_amd.default_lib()
    assert lib.patch_embed_params_ws_floats(ops._lib.PATCH_AUDIO, 8, 1, 256, 256, 96) // (19 * 96 + 128) == 1024
    _check("carried", "both", 96, torch.float32)


def test_repeated_backward_is_bit_identical():
    B, L, stripes, lam = _operands("odd-B")
    x = _wave(B, L)[0].to(DEV)
    cot = cotangent((B, 4096, 96), torch.bfloat16).to(DEV)
    m = _module(out_dtype=torch.bfloat16, trainable=True, fused=True).to(DEV).train()
    runs = []
    for _ in range(2):
        m.zero_grad(set_to_none=True)
        tok = m(x, mixup_lambda=lam, stripes=stripes)
        tok.backward(cot, retain_graph=True)
        first = {k: v.clone() for k, v in module_grads(m).items()}
        m.zero_grad(set_to_none=True)
        tok.backward(cot)                                                    # the same graph again: the saved stripes and lambda are intact
        runs.append((tok.detach(), first, module_grads(m)))
    for k in SIX:
        assert torch.isfinite(runs[0][1][k]).all()
        assert torch.equal(runs[0][1][k], runs[0][2][k]) and torch.equal(runs[0][1][k], runs[1][1][k]) and torch.equal(runs[0][1][k], runs[1][2][k]), k
    assert torch.equal(runs[0][0], runs[1][0])


def test_without_augmentation_the_old_exports_are_called(monkeypatch):
    lib = dgsct_amd.default_lib()
    calls = {"fwd": 0, "bwd": 0, "fwd_aug": 0, "bwd_aug": 0}

    def count(name, key):
        real = getattr(lib, name)
        monkeypatch.setattr(lib, name, lambda *a, **k: (calls.__setitem__(key, calls[key] + 1), real(*a, **k))[1])

    count("patch_embed_forward", "fwd"); count("patch_embed_backward_params", "bwd")
    count("patch_embed_forward_aug", "fwd_aug"); count("patch_embed_backward_params_aug", "bwd_aug")
    B, L, stripes, lam = _operands("smallest")
    x = _wave(B, L)[0].to(DEV)
    cot = cotangent((B, 4096, 96)).to(DEV)
    old = _module(trainable=True, fused=True).to(DEV).train()
    new = _module(trainable=True, fused=True, spec_augment=False).to(DEV).train()
    a, b = old(x), new(x, mixup_lambda=None, stripes=None)
    a.backward(cot); b.backward(cot)
    assert torch.equal(a, b)
    ga, gb = module_grads(old), module_grads(new)
    for k in SIX:
        assert torch.equal(ga[k], gb[k]), k
    # eval mode ignores stripes, lambda and the flag (T = 11: a draw would raise)
    ev = _module(trainable=True, fused=True, spec_augment=True).to(DEV).eval()
    assert torch.equal(ev(x, mixup_lambda=lam, stripes=stripes), _module(trainable=True, fused=True).to(DEV).eval()(x))
    assert calls == {"fwd": 4, "bwd": 2, "fwd_aug": 0, "bwd_aug": 0}
    # ... and with an augmentation active, one call of each new export per step
    t = new(x, mixup_lambda=lam, stripes=stripes)
    t.backward(cot)
    assert calls == {"fwd": 4, "bwd": 2, "fwd_aug": 1, "bwd_aug": 1}
    assert not torch.equal(t, b)


def test_fused_against_aten():
    B, L, stripes, lam = _operands("odd-B")
    x = _wave(B, L)[0].to(DEV)
    cot = cotangent((B, 4096, 96)).to(DEV)
    fused = _module(trainable=True, fused=True).to(DEV).train()
    aten = _module(trainable=True, fused=False).to(DEV).train()
    a, b = fused(x, lam, stripes), aten(x, lam.to(DEV), stripes.to(DEV))      # (host or device operands: both are taken)
    assert fp32_err(a, b) < 1e-3 and "PatchEmbedTrain" not in type(b.grad_fn).__name__
    a.backward(cot); b.backward(cot)
    ga, gb = module_grads(fused), module_grads(aten)
    for k in SIX:
        assert fp32_err(ga[k], gb[k]) < 1e-3, k
    fz, az = _module(out_dtype=torch.bfloat16, fused=True).to(DEV).train(), _module(out_dtype=torch.bfloat16, fused=False).to(DEV).train()
    assert nrm_err(fz(x, lam, stripes), az(x, lam, stripes)) < 1e-2


def test_dispatch_and_errors():
    B, L, stripes, lam = _operands("smallest")
    x = _wave(B, L)[0].to(DEV)
    # fused=None with an augmentation active follows the measured policy; without one it never looks at it
    m = _module(trainable=True).to(DEV).train()
    assert ("PatchEmbedTrain" in type(m(x, lam, stripes).grad_fn).__name__) == ("train" in frontend._KERNELS_FASTER_AUG and "audio" in frontend._KERNELS_FASTER_TRAIN)
    assert ("PatchEmbedTrain" in type(m(x).grad_fn).__name__) == ("audio" in frontend._KERNELS_FASTER_TRAIN)
    fz = _module().to(DEV).train()
    ref = _module(fused="frozen" in frontend._KERNELS_FASTER_AUG).to(DEV).train()
    assert torch.equal(fz(x, lam, stripes), ref(x, lam, stripes))

    class NoAug:                                                             # a library whose probe says the two exports are missing
        path = "libstub.so"

        def has_patch_embed_params(self):
            return True

        def has_patch_embed_aug(self):
            return False

    for mod in (HTSATFrontEnd(fused=True, lib=NoAug()), HTSATFrontEnd(fused=True, trainable=True, lib=NoAug())):
        with pytest.raises(RuntimeError, match="dgsct_patch_embed_forward_aug"):
            mod.to(DEV).train()(x, lam, stripes)
    # raw calls
    mm = _module().to(DEV)
    lmel = ops.logmel(x, mm.logmel_extractor.melW)
    scale, shift = mm._bn_affine(None, None, B * 11)
    pe = mm.patch_embed._frozen_params()
    bad = stripes.clone()
    bad[0, 1, 1] = 12                                                        # a time stripe past the 11 frames
    with pytest.raises(RuntimeError, match="outside"):
        ops.patch_embed(lmel, *pe, 1e-5, None, scale, shift, stripes=bad)
    bad = stripes.clone()
    bad[1, 2, 1] = 65                                                        # a mel stripe past bin 63
    with pytest.raises(RuntimeError, match="outside"):
        ops.patch_embed(lmel, *pe, 1e-5, None, scale, shift, stripes=bad.to(DEV))
    with pytest.raises(RuntimeError, match="mixup_lambda"):
        ops.patch_embed(lmel, *pe, 1e-5, None, scale, shift, mixup_lambda=torch.ones(3, device=DEV))
    with pytest.raises(RuntimeError, match="mixup_lambda"):
        mm.train()(x, mixup_lambda=torch.ones(3))
    with pytest.raises(RuntimeError, match="audio mode"):
        ops.patch_embed(torch.zeros(1, 3, 32, 32, device=DEV), torch.zeros(96, 3, 4, 4, device=DEV), *(torch.zeros(96, device=DEV),) * 3,
                        stripes=torch.zeros(1, 4, 2, dtype=torch.int32))
    # the raw call with both operands NULL is the plain call
    out = ops.patch_embed(lmel, *pe, 1e-5, None, scale, shift)
    raw = torch.empty_like(out)
    dgsct_amd.default_lib().patch_embed_forward_aug(ops._lib.F32, B, 11, 96, lmel.data_ptr(), scale.data_ptr(), shift.data_ptr(), None, None,
                                                    *(t.data_ptr() for t in pe), 1e-5, raw.data_ptr(), torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    assert torch.equal(raw, out)
