"""CPU-only: the patch-merging modules (dg-sct_amd/merging.py) in their ATen formulation against the reference-generated fixture
(tools/make_golden_patch_merging.py -> tests/golden/ref_patch_merging.pt: the reference's HTS-AT ``PatchMerging`` and Hugging Face
transformers' ``Swinv2PatchMerging``), their assertions, and ``AVETrunk`` on the host-emulated library: the chained layer loop against a
hand-written stage-by-stage loop, and the gradient of a loss on the pooled outputs reaching the stage-0 adapters."""
import os
import sys

import pytest
import torch
import torch.nn as nn

from helpers import GOLDEN, ROOT

sys.path.insert(0, os.path.join(ROOT, "tests", "emu"))
from build_emu import build_emu  # noqa: E402

import dgsct_amd  # noqa: E402,F401
from dgsct_amd import AdapterStack, AVETrunk, HTSATPatchMerging, SwinV2PatchMerging  # noqa: E402
from dgsct_amd._lib import Lib  # noqa: E402
from dgsct_amd.stack import default_opt  # noqa: E402

FORMS = {"htsat": HTSATPatchMerging, "swinv2": SwinV2PatchMerging}
CASE_IDS = [f"{f}-{s}" for f in FORMS for s in ("3x6x4x32", "2x8x8x96")]
STAGES = [dict(layers=1, Nv=144, Cv=128, Na=256, Ca=96), dict(layers=1, Nv=36, Cv=256, Na=64, Ca=192)]


def _fixture():
    return torch.load(os.path.join(GOLDEN, "ref_patch_merging.pt"), weights_only=True)


def test_fixture_holds_both_forms_and_both_cases():
    assert sorted(_fixture()) == sorted(CASE_IDS)


@pytest.mark.parametrize("case", CASE_IDS)
def test_aten_formulation_matches_the_reference(case):
    fx = _fixture()[case]
    B, H, W, C = fx["shape"]
    m = FORMS[fx["form"]]((H, W), C, fused=False).eval()
    assert set(m.state_dict()) == set(fx["state"]) == {"reduction.weight", "norm.weight", "norm.bias"}
    m.load_state_dict(fx["state"])
    assert all(p.dtype == torch.float32 for p in m.parameters())
    x = fx["x"].clone().requires_grad_(True)
    y = m(x)
    y.backward(fx["cot"])
    assert y.shape == (B, (H // 2) * (W // 2), 2 * C)
    assert (y - fx["y"]).abs().max().item() <= 1e-5
    assert (x.grad - fx["dx"]).abs().max().item() <= 1e-5


@pytest.mark.parametrize("cls", list(FORMS.values()), ids=list(FORMS))
def test_assertions_and_dispatch_errors(cls):
    with pytest.raises(AssertionError, match="not even"):
        cls((5, 4), 32, fused=False)(torch.randn(1, 20, 32))
    with pytest.raises(AssertionError, match="not even"):
        cls((4, 3), 32, fused=False)(torch.randn(1, 12, 32))
    with pytest.raises(AssertionError, match="wrong size"):
        cls((4, 4), 32, fused=False)(torch.randn(1, 15, 32))
    with pytest.raises(RuntimeError, match="fused=True"):
        cls((4, 4), 32, fused=True)(torch.randn(1, 16, 32))
    with pytest.raises(RuntimeError, match="fused=True"):
        cls((4, 4), 32, fused=True).bfloat16()(torch.randn(1, 16, 32).bfloat16())         # bf16, but on the CPU: no CPU kernels
    y = cls((4, 4), 32)(torch.randn(2, 16, 32))                                        # fused=None on the CPU: the ATen formulation
    assert y.shape == (2, 4, 64)


def test_trunk_rejects_stages_that_do_not_chain():
    with pytest.raises(ValueError, match="quarter"):
        AVETrunk([STAGES[0], dict(STAGES[1], Nv=144)], dtype=torch.float32)
    with pytest.raises(ValueError, match="twice the width"):
        AVETrunk([STAGES[0], dict(STAGES[1], Ca=96)], dtype=torch.float32)


def _trunk(emu):
    torch.manual_seed(0)
    tr = AVETrunk(STAGES, opt=default_opt(num_tokens=4), dtype=torch.float32, fused=False, lib=emu, concurrent=False)
    with torch.no_grad():
        for n, p in tr.stack.named_parameters():                                      # open the gates (they start at 0: every adapter a no-op)
            if n.endswith("gate") or n.endswith("gate_av"):
                p.fill_(0.5)
        for m in (tr.vis_merge, tr.aud_merge, tr.norm):
            for p in m.parameters():
                p.add_(0.1 * torch.randn_like(p))
    return tr.train()


def _inputs(BT=2):
    g = torch.Generator().manual_seed(1)
    return (torch.randn(BT, STAGES[0]["Nv"], STAGES[0]["Cv"], generator=g), torch.randn(BT, STAGES[0]["Na"], STAGES[0]["Ca"], generator=g))


def test_trunk_chain_equals_a_stage_by_stage_loop():
    """outs of the chained loop == a plain AdapterStack called once per stage with the SAME adapter / block modules, the merges applied
    by hand in between: exactly"""
    emu = Lib(build_emu())
    tr = _trunk(emu)
    ref = _trunk(emu)                                                                  # a twin: BatchNorm running statistics move in train mode
    ref.load_state_dict(tr.state_dict())
    f_v, f_a = _inputs()
    pooled_v, pooled_a, outs, maps = tr(f_v, f_a)
    assert len(outs) == 2 and pooled_v.shape == (2, 1, 256) and pooled_a.shape == (2, 1, 192)
    assert outs[1][0].shape == (2, 36, 256) and outs[1][1].shape == (2, 64, 192)

    hand = []
    hv, ha = f_v, f_a
    for s, st in enumerate(STAGES):
        plain = AdapterStack([st], opt=default_opt(num_tokens=4), lib=emu, concurrent=False, compute_dtype=torch.float32).train()
        for name in ("audio_adapter_blocks_p1", "vis_adapter_blocks_p1", "audio_adapter_blocks_p2", "vis_adapter_blocks_p2"):
            setattr(plain, name, nn.ModuleList([getattr(ref.stack, name)[s]]))         # one layer per stage: global index s

        def vis_block(i, half, f, s=s):
            return ref.blocks.vis_block_map(s + i, half, f)
        vis_block.returns_map = True
        o, m = plain([(hv, ha)], vis_block=vis_block, aud_block=lambda i, f, s=s: ref.blocks.aud_block(s + i, f))
        hand.append(o[0])
        hv, ha = o[0]
        if s + 1 < len(STAGES):
            hv, ha = ref.vis_merge[s](hv), ref.aud_merge[s](ha)
    for (a, b), (c, d) in zip(outs, hand):
        assert torch.equal(a, c) and torch.equal(b, d)
    assert torch.equal(maps[0], m[0]) and torch.equal(maps[1], m[1])


def test_loss_on_the_pooled_outputs_trains_the_stage0_adapters():
    emu = Lib(build_emu())
    tr = _trunk(emu)
    f_v, f_a = _inputs()
    pooled_v, pooled_a, outs, maps = tr(f_v, f_a)
    g = torch.Generator().manual_seed(2)
    torch.autograd.backward([pooled_v, pooled_a], [torch.randn(pooled_v.shape, generator=g), torch.randn(pooled_a.shape, generator=g)])
    for name in ("audio_adapter_blocks_p1", "vis_adapter_blocks_p1", "audio_adapter_blocks_p2", "vis_adapter_blocks_p2"):
        ad = getattr(tr.stack, name)[0]                                                # layer 0 = stage 0
        for n, p in ad.named_parameters():
            if n == "gate_tk":                                                         # declared and never read by the reference forward either
                assert p.grad is None
                continue
            assert p.grad is not None and torch.isfinite(p.grad).all() and float(p.grad.abs().sum()) > 0, (name, n)
    for mod in (tr.blocks, tr.vis_merge, tr.aud_merge, tr.norm):
        assert all(p.grad is None for p in mod.parameters())
