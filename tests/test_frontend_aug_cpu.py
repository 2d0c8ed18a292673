"""SpecAugment stripes and mix-up of the HTS-AT front end (``HTSATFrontEnd(spec_augment=True)``, ``forward(waveform, mixup_lambda, stripes)``)
without a GPU: the ATen formulation (fused=False) under plain autograd against the float64 restatement of tests/frontend_aug_ref.py, the
draw of the stripes against the published DropStripes algorithm written out inline, what eval mode and the defaults leave untouched, and
the C symbols of the in-kernel variant.

Bound: ``helpers.fp32_err < 1e-3`` on the tokens and each of the six gradients, the bound of tests/test_frontend_train_cpu.py (the fp32 ATen
evaluation of the un-augmented restatement sits at 2e-7 .. 4e-6 from float64; a mask and a convex mix add two roundings per element)."""
import ctypes
import os
import re
import sys

import numpy as np
import pytest
import torch

import dgsct_amd
from dgsct_amd import AVENet, HTSATFrontEnd, ave_stage_shapes, frontend, ops, train

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import frontend_aug_ref as A                # noqa: E402
import frontend_ref as R                    # noqa: E402
from helpers import ROOT, fp32_err          # noqa: E402

SIX = A.SIX


def cotangent(shape, dtype=torch.float32):
    """randn with seed 11, rounded to the token dtype"""
    return torch.randn(shape, generator=torch.Generator().manual_seed(11)).to(dtype)


def table(rows):
    return torch.tensor(rows, dtype=torch.int32)


# T = 11: sample 0 loses frames [0, 3) and [2, 5) (overlapping, frame 0 included) and mel bins [3, 6) (across a patch row) and [0, 2);
# sample 1 loses the last frame, has one empty stripe and loses mel bins [60, 64)
STRIPES_2x11 = table([[[0, 3], [2, 5], [3, 6], [0, 2]], [[10, 11], [4, 4], [60, 64], [7, 7]]])


def module_grads(m):
    g = dict(m.named_parameters())
    return {k: g[k].grad for k in SIX}


@pytest.mark.parametrize("what", ["stripes+lambda", "stripes", "lambda"])
def test_aten_tokens_and_gradients_against_float64(what):
    B, L, T = 2, 3200, 11
    x = R.signal(B, L)
    stripes = STRIPES_2x11 if "stripes" in what else None
    lam = torch.tensor([0.3, 0.8]) if "lambda" in what else None
    m = R.randomise(HTSATFrontEnd(fused=False, trainable=True), 2).train()
    sd0 = {k: v.clone() for k, v in m.state_dict().items()}
    cot = cotangent((B, 4096, 96))
    ref, tok64 = A.audio_grads64(R.logmel(x), sd0, True, cot, stripes, lam)
    plain = R.audio_tokens(R.logmel(x), sd0, True)[0]
    assert fp32_err(tok64, plain) > 1e-2                                     # the augmentation is visible at this shape
    tok = m(x, mixup_lambda=lam, stripes=stripes)
    assert tok.requires_grad and tok.dtype == torch.float32
    err = fp32_err(tok, tok64)
    print(f"{what} tokens: {err:.3e}")
    assert err < 1e-3
    tok.backward(cot)
    got = module_grads(m)
    for k in SIX:
        err = fp32_err(got[k], ref[k])
        print(f"{what} {k}: {err:.3e}")
        assert err < 1e-3, k
    assert m.logmel_extractor.melW.grad is None
    # bn0 normalises with (and tracks) the statistics of the un-augmented log-mel
    _, rm, rv = R.audio_tokens(R.logmel(x), sd0, True)
    assert ((m.bn0.running_mean.double() - rm).abs() / rm.abs().clamp_min(1e-3)).max().item() < 1e-4
    assert ((m.bn0.running_var.double() - rv).abs() / rv).max().item() < 1e-4


def _inline_drop_stripes(B, T):
    """the published DropStripes loop (time dropper: dim 2, width 64, 2 stripes; then mel dropper: dim 3, width 8, 2 stripes), each over
    the samples in order, on torch's default generator"""
    out = torch.zeros(B, 4, 2, dtype=torch.int32)
    for row0, total_width, drop_width in ((0, T, 64), (2, 64, 8)):
        for n in range(B):
            for j in range(2):
                distance = torch.randint(low=0, high=drop_width, size=(1,))[0]
                bgn = torch.randint(low=0, high=total_width - distance, size=(1,))[0]
                out[n, row0 + j, 0] = int(bgn)
                out[n, row0 + j, 1] = int(bgn + distance)
    return out


def test_draw_stripes_is_the_published_algorithm_draw_for_draw():
    B, T = 4, 101
    torch.manual_seed(1234)
    want = _inline_drop_stripes(B, T)
    state_want = torch.get_rng_state()
    torch.manual_seed(1234)
    got = frontend.draw_stripes(B, T)
    assert got.dtype == torch.int32 and tuple(got.shape) == (B, 4, 2) and torch.equal(got, want)
    assert torch.equal(torch.get_rng_state(), state_want)                    # the default generator is left where the reference leaves it
    for width, rows, longest in ((T, got[:, :2], 64), (64, got[:, 2:], 8)):
        bgn, end = rows[..., 0], rows[..., 1]
        assert bool((bgn >= 0).all() and (bgn <= end).all() and (end <= width).all() and (end - bgn < longest).all())
    # an explicit generator is used instead of the default one
    g = torch.Generator().manual_seed(1234)
    before = torch.get_rng_state()
    assert torch.equal(frontend.draw_stripes(B, T, generator=g), want) and torch.equal(torch.get_rng_state(), before)
    # the module draws them itself in train mode: the same call on the same seed
    m = R.randomise(HTSATFrontEnd(fused=False, spec_augment=True), 2).train()
    x = R.signal(2, 20480)                                                   # T = 65
    torch.manual_seed(7)
    a = m(x)
    torch.manual_seed(7)
    drawn = frontend.draw_stripes(2, 65)
    assert torch.equal(a, R.randomise(HTSATFrontEnd(fused=False), 2).train()(x, stripes=drawn))


def test_draw_stripes_refuses_fewer_frames_than_the_drop_width():
    with pytest.raises(ValueError, match="frames"):
        frontend.draw_stripes(2, 11)
    assert tuple(frontend.draw_stripes(1, 64).shape) == (1, 4, 2)


def test_eval_mode_ignores_stripes_and_lambda():
    x = R.signal(2, 3200)
    lam = torch.tensor([0.3, 0.8])
    for kw in (dict(), dict(trainable=True)):
        m = R.randomise(HTSATFrontEnd(fused=False, spec_augment=True, **kw), 2).eval()
        assert torch.equal(m(x, mixup_lambda=lam, stripes=STRIPES_2x11).detach(), m(x).detach())
    m = R.randomise(HTSATFrontEnd(fused=False, spec_augment=True), 2).eval()
    m(x)                                                                     # T = 11 < 64: nothing is drawn in eval mode
    with pytest.raises(ValueError):
        m.train()(x)


def test_defaults_are_the_un_augmented_module():
    x = R.signal(2, 3200)
    for training in (False, True):
        a = R.randomise(HTSATFrontEnd(fused=False), 2).train(training)
        b = R.randomise(HTSATFrontEnd(fused=False, spec_augment=False), 2).train(training)
        sd0 = {k: v.clone() for k, v in a.state_dict().items()}
        ta, tb = a(x), b(x, mixup_lambda=None, stripes=None)
        assert torch.equal(ta, tb) and not a.spec_augment
        assert fp32_err(ta, R.audio_tokens(R.logmel(x), sd0, training)[0]) < 1e-3      # ... which is the un-augmented front end
        assert torch.equal(a.bn0.running_mean, b.bn0.running_mean)
    # a table of empty stripes and lambda = 1 change nothing but rounding
    a = R.randomise(HTSATFrontEnd(fused=False), 2).train()
    assert fp32_err(a(x, torch.ones(2), torch.zeros(2, 4, 2, dtype=torch.int32)), ta) < 1e-6


def test_wrong_operands_raise():
    x = R.signal(2, 3200)
    m = HTSATFrontEnd(fused=False).train()
    with pytest.raises(RuntimeError, match="mixup_lambda"):
        m(x, mixup_lambda=torch.ones(3))
    with pytest.raises(RuntimeError, match="mixup_lambda"):
        m(x, mixup_lambda=torch.ones(2, dtype=torch.float64))
    with pytest.raises(RuntimeError, match="stripes"):
        m(x, stripes=torch.zeros(2, 4, 2, dtype=torch.int64))
    with pytest.raises(RuntimeError, match="stripes"):
        m(x, stripes=torch.zeros(3, 4, 2, dtype=torch.int32))
    bad = STRIPES_2x11.clone()
    bad[1, 0, 1] = 12                                                        # past the 11 frames
    with pytest.raises(RuntimeError, match="outside"):
        m(x, stripes=bad)
    bad = STRIPES_2x11.clone()
    bad[0, 3, 0] = -1
    with pytest.raises(RuntimeError, match="outside"):
        ops.check_stripes(bad, 2, 11)
    with pytest.raises(RuntimeError, match="CUDA/HIP"):
        HTSATFrontEnd(fused=True).train()(x, stripes=STRIPES_2x11)


def test_state_dict_keys_do_not_change():
    assert set(HTSATFrontEnd(spec_augment=True).state_dict()) == set(HTSATFrontEnd().state_dict())
    assert set(HTSATFrontEnd(spec_augment=True, trainable=True).state_dict()) == set(HTSATFrontEnd().state_dict())
    res = HTSATFrontEnd(spec_augment=True).load_state_dict(R.randomise(HTSATFrontEnd(), 1).state_dict(), strict=True)
    assert not res.missing_keys and not res.unexpected_keys


def test_header_and_library_declare_the_exports():
    with open(os.path.join(ROOT, "include", "dgsct.h")) as f:
        text = f.read()
    assert re.search(r"int\s+dgsct_patch_embed_forward_aug\s*\(", text)
    assert re.search(r"int\s+dgsct_patch_embed_backward_params_aug\s*\(", text)
    assert re.search(r"#define\s+DGSCT_VERSION\s+101\b", text)
    lib = dgsct_amd.default_lib()
    c = ctypes.CDLL(lib.path)
    assert c.dgsct_patch_embed_forward_aug is not None and c.dgsct_patch_embed_backward_params_aug is not None
    assert c.dgsct_version() == 101
    assert lib.has_patch_embed_aug() and lib.has_patch_embed_params()
    # the host emulation has no front end at all, and says so
    sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "emu"))
    from build_emu import build_emu
    from dgsct_amd._lib import Lib
    emu = Lib(build_emu())
    assert not emu.has_patch_embed_aug()
    with pytest.raises(RuntimeError, match="dgsct_patch_embed_forward_aug"):
        emu.patch_embed_forward_aug(0, 1, 11, 96, *([None] * 9), 1e-5, None, None)


def test_policy_set_names_known_kinds_and_is_backed_by_the_profile():
    assert isinstance(frontend._KERNELS_FASTER_AUG, frozenset) and frontend._KERNELS_FASTER_AUG <= {"frozen", "train"}
    path = os.path.join(ROOT, "profiles", "frontend_aug_bench.txt")
    if frontend._KERNELS_FASTER_AUG:                                         # a kind is listed only on the strength of measured rows
        with open(path) as f:
            won = {k for k, v in re.findall(r"_KERNELS_FASTER_AUG should hold '(\w+)'\): (yes|no)", f.read()) if v == "yes"}
        assert set(frontend._KERNELS_FASTER_AUG) <= won


def test_mix_lambda_is_the_list_of_single_draws():
    np.random.seed(5)
    want = np.array([np.random.beta(0.5, 0.5, 1)[0] for _ in range(7)]).astype(np.float32)
    after = np.random.get_state()[1].copy()
    np.random.seed(5)
    got = train.mix_lambda(0.5, 7)
    assert got.dtype == torch.float32 and tuple(got.shape) == (7,) and np.array_equal(got.numpy(), want)
    assert np.array_equal(np.random.get_state()[1], after)
    assert bool((got >= 0).all() and (got <= 1).all())


def test_avenet_hands_the_flag_and_the_lambda_to_its_front_end(monkeypatch):
    stages = ave_stage_shapes("swinv2_base")[:2]
    assert not AVENet(stages, T=4).frontend.spec_augment
    net = AVENet(stages, T=4, spec_augment=True)
    assert net.frontend.spec_augment
    seen = {}

    class Stop(Exception):
        pass

    def spy(waveform, mixup_lambda=None, stripes=None):
        seen["lam"] = mixup_lambda
        raise Stop

    monkeypatch.setattr(net.frontend, "forward", spy)
    monkeypatch.setattr(net.patch_embed, "forward", lambda x: None)
    lam = train.mix_lambda(0.5, 4)
    with pytest.raises(Stop):
        net(torch.zeros(4, 3200), torch.zeros(1, 4, 3, 192, 192), lam)
    assert seen["lam"] is lam
    with pytest.raises(Stop):
        net(torch.zeros(4, 3200), torch.zeros(1, 4, 3, 192, 192))
    assert seen["lam"] is None
