"""CPU-only: the surface of the trainable fused patch merging -- the `weight_grads` / `merge_weight_grads` keywords and their defaults,
unchanged state-dict names, the two C declarations, and the error of a library that lacks the export."""
import inspect
import os
import re
import sys

import pytest
import torch

from helpers import ROOT

sys.path.insert(0, os.path.join(ROOT, "tests", "emu"))
from build_emu import build_emu  # noqa: E402

import dgsct_amd  # noqa: E402,F401
from dgsct_amd import AVETrunk, HTSATPatchMerging, SwinV2PatchMerging, merging, ops  # noqa: E402
from dgsct_amd._lib import Lib  # noqa: E402

FORMS = {"htsat": HTSATPatchMerging, "swinv2": SwinV2PatchMerging}
STAGES = [dict(layers=1, Nv=144, Cv=128, Na=256, Ca=96), dict(layers=1, Nv=36, Cv=256, Na=64, Ca=192)]


@pytest.mark.parametrize("cls", list(FORMS.values()), ids=list(FORMS))
def test_keyword_exists_and_defaults_to_off(cls):
    assert inspect.signature(cls.__init__).parameters["weight_grads"].default is False
    assert cls((4, 4), 32).weight_grads is False and cls((4, 4), 32, weight_grads=True).weight_grads is True
    for wg in (False, True):
        assert set(cls((4, 4), 32, weight_grads=wg).state_dict()) == {"reduction.weight", "norm.weight", "norm.bias"}
    y = cls((4, 4), 32, weight_grads=True)(torch.randn(2, 16, 32))           # fused=None on the CPU stays the ATen formulation
    assert y.shape == (2, 4, 64) and "PatchMerge" not in type(y.grad_fn).__name__


def test_trunk_keyword_reaches_the_audio_merges_only():
    assert inspect.signature(AVETrunk.__init__).parameters["merge_weight_grads"].default is False
    keys = None
    for kw in ({}, dict(merge_weight_grads=True)):
        tr = AVETrunk(STAGES, dtype=torch.float32, train_htsat=True, **kw)
        assert all(m.weight_grads is bool(kw) for m in tr.aud_merge)
        assert all(m.weight_grads is False for m in tr.vis_merge)
        assert all(p.requires_grad and p.dtype == torch.float32 for p in tr.aud_merge.parameters())
        assert not any(p.requires_grad for p in tr.vis_merge.parameters())
        assert keys is None or keys == list(tr.state_dict())
        keys = list(tr.state_dict())
    assert "aud_merge.0.reduction.weight" in keys and "aud_merge.0.norm.bias" in keys


def test_header_declares_the_two_exports():
    with open(os.path.join(ROOT, "include", "dgsct.h")) as f:
        text = f.read()
    assert re.search(r"int64_t\s+dgsct_patch_merge_params_ws_bytes\s*\(", text)
    assert re.search(r"int\s+dgsct_patch_merge_backward_params\s*\(", text)
    assert re.search(r"#define\s+DGSCT_VERSION\s+101\b", text)
    assert isinstance(merging._KERNELS_FASTER_TRAIN, frozenset)
    assert callable(ops.patch_merge_train)


@pytest.mark.parametrize("cls", list(FORMS.values()), ids=list(FORMS))
def test_library_without_the_export_is_an_error_under_fused_true(cls):
    emu = Lib(build_emu())                                     # the host emulation has no patch merging at all
    assert not emu.has_patch_merge_params()
    m = cls((4, 4), 32, fused=True, lib=emu, weight_grads=True)
    with pytest.raises(RuntimeError, match="dgsct_patch_merge_backward_params"):
        m(torch.randn(1, 16, 32).bfloat16())
    with pytest.raises(RuntimeError, match="dgsct_patch_merge_params_ws_bytes"):
        emu.patch_merge_params_ws_bytes(0, 1, 4, 4, 32)
