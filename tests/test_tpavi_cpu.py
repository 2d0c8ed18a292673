"""CPU-only: the drop-in ``TPAVIModule`` (dg-sct_amd/tpavi.py) in its ATen formulations against the reference-generated float64 fixture
(tools/make_golden_tpavi.py -> tests/golden/ref_tpavi.pt, ref_tpavi_eval.pt) and against tests/tpavi_ref.py, and the surface of the
feature: the C header, the optional exports, the dispatch rules.

Bounds (relative to scale, tests/tpavi_ref.py ``check`` / ``grad_scales``): float64 runs <= 1e-9; fp32 outputs 1e-5 x max(1, |ref|max),
fp32 gradients 1e-4 x max(1, |ref|max) -- the project's own for fp32 kernels (test_cmbs_gpu.py); the two analytically zero gradients
take the largest scale among the case's other parameter gradients."""
import os
import re
import sys

import pytest
import torch

from helpers import GOLDEN, ROOT
import tpavi_ref as R

sys.path.insert(0, os.path.join(ROOT, "tests", "emu"))
from build_emu import build_emu  # noqa: E402

import dgsct_amd  # noqa: E402,F401
from dgsct_amd import TPAVIModule  # noqa: E402
from dgsct_amd import _lib, ops, tpavi as tpavi_mod  # noqa: E402

NEW_EXPORTS = ("dgsct_tpavi_frame_sum", "dgsct_tpavi_forward", "dgsct_tpavi_backward", "dgsct_tpavi_ws_bytes")


@pytest.fixture(scope="module")
def fx():
    d = torch.load(os.path.join(GOLDEN, "ref_tpavi.pt"), weights_only=True)
    d.update(torch.load(os.path.join(GOLDEN, "ref_tpavi_eval.pt"), weights_only=True))
    return d


def _module(fx, dtype=torch.float32, **kw):
    m = TPAVIModule(64, **kw)
    m.load_state_dict(fx["state"])
    return m.to(dtype)


def _run(m, fx, dtype):
    x, audio = fx["x"].to(dtype).clone().requires_grad_(True), fx["audio"].to(dtype).clone().requires_grad_(True)
    z, a = m(x, audio)
    torch.autograd.backward([z, a], [fx["cot_z"].to(dtype), fx["cot_a"].to(dtype)])
    return z, a, x.grad, audio.grad


def _compare(m, got, rec, out_bound, grad_bound):
    z, a, dx, da = got
    assert tuple(z.shape) == (2, 64, 5, 7, 7) and tuple(a.shape) == (2, 5, 64)
    R.check(z, rec["z"], out_bound, "z")
    R.check(a, rec["audio_temp"], out_bound, "audio_temp")
    R.check(dx, rec["dx"], grad_bound, "dx")
    R.check(da, rec["daudio"], grad_bound, "daudio")
    scales = R.grad_scales(rec["grads"])
    params = dict(m.named_parameters())
    assert sorted(params) == sorted(R.PARAMS)
    for k in R.PARAMS:
        R.check(params[k].grad, rec["grads"][k], grad_bound, "d " + k, scales[k])
    bn = m.W_z[1]
    R.check(bn.running_mean, rec["running_mean"], out_bound, "running_mean")
    R.check(bn.running_var, rec["running_var"], out_bound, "running_var")
    assert int(bn.num_batches_tracked) == rec["num_batches_tracked"]


def test_seeded_construction_reproduces_the_reference_parameters(fx):
    torch.manual_seed(fx["seed"])
    m = TPAVIModule(in_channels=64, mode='dot')
    sd = m.state_dict()
    assert list(sd) == fx["keys"] == list(R.KEYS) and len(sd) == 17
    assert sd["g.weight"].dim() == 5 and sd["W_z.0.weight"].dim() == 5
    R.set_nontrivial(sd, fx["seed"] + 1)
    for k in sd:
        assert torch.equal(sd[k], fx["state"][k]), k


@pytest.mark.parametrize("mode", ["train", "eval"])
@pytest.mark.parametrize("kw", [dict(fused=False), dict(reference_order=True)], ids=["linear", "reference_order"])
def test_float64_aten_formulations_reproduce_the_fixture(fx, mode, kw):
    m = _module(fx, torch.float64, **kw).train(mode == "train")
    _compare(m, _run(m, fx, torch.float64), fx[mode], 1e-9, 1e-9)
    assert fx["train"]["num_batches_tracked"] == 1 and fx["eval"]["num_batches_tracked"] == 0


@pytest.mark.parametrize("mode", ["train", "eval"])
def test_fp32_linear_form_within_the_kernel_bounds(fx, mode):
    m = _module(fx, fused=False).train(mode == "train")
    _compare(m, _run(m, fx, torch.float32), fx[mode], 1e-5, 1e-4)


def test_restatement_matches_the_fixture(fx):
    for mode in ("train", "eval"):
        ref = R.tpavi_f64(fx["state"], fx["x"], fx["audio"], mode == "train", fx["cot_z"], fx["cot_a"])
        for k in ("z", "audio_temp", "dx", "daudio", "running_mean", "running_var"):
            assert (ref[k] - fx[mode][k]).abs().max().item() <= 1e-10, (mode, k)
        for k in R.PARAMS:
            assert (ref["grads"][k] - fx[mode]["grads"][k]).abs().max().item() <= 1e-10, (mode, k)


@pytest.mark.parametrize("shape", [(1, 64, 5, 3, 5), (2, 128, 2, 6, 10)], ids=["B1", "T2"])
def test_linear_form_matches_the_restatement_off_the_fixture(shape):
    state, x, audio, cz, ca = R.make_case(*shape, seed=11)
    m = TPAVIModule(shape[1], fused=False)
    m.load_state_dict(state)
    m = m.double().train()
    xx, aa = x.double().requires_grad_(True), audio.double().requires_grad_(True)
    z, a = m(xx, aa)
    torch.autograd.backward([z, a], [cz.double(), ca.double()])
    ref = R.tpavi_f64(state, x, audio, True, cz, ca)
    R.check(z, ref["z"], 1e-9, "z")
    R.check(xx.grad, ref["dx"], 1e-9, "dx")
    R.check(aa.grad, ref["daudio"], 1e-9, "daudio")
    scales = R.grad_scales(ref["grads"])
    for k, p in m.named_parameters():
        R.check(p.grad, ref["grads"][k], 1e-9, "d " + k, scales[k])
    if shape[0] == 1:
        assert ref["grads"]["theta.bias"].abs().max().item() < 1e-9         # analytically zero at B = 1
    assert ref["grads"]["W_z.0.bias"].abs().max().item() < 1e-9             # a bias in front of a batch-statistics BatchNorm


@pytest.mark.parametrize("kw", [dict(fused=False), dict(reference_order=True)], ids=["linear", "reference_order"])
def test_forward_frames_equals_the_permuted_forward(fx, kw):
    m = _module(fx, torch.float64, **kw).eval()
    x, audio = fx["x"].double(), fx["audio"].double()
    z, a = m(x, audio)
    frames = x.permute(0, 2, 1, 3, 4).reshape(10, 64, 7, 7)                    # pre_reshape_for_tpavi, inverted
    for au in (audio, audio.reshape(10, 128)):
        zf, af = m.forward_frames(frames, au, T=5)
        assert tuple(zf.shape) == (10, 64, 7, 7)
        assert (zf - z.permute(0, 2, 1, 3, 4).reshape(10, 64, 7, 7)).abs().max().item() <= 1e-12
        assert torch.equal(af, a)


def test_at_constructor_initialisation_z_is_the_layer_norm_of_x(fx):
    torch.manual_seed(0)
    m = TPAVIModule(64, fused=False).train()
    x, audio = fx["x"], fx["audio"]
    z, _ = m(x, audio)
    want = torch.nn.functional.layer_norm(x.permute(0, 2, 3, 4, 1), (64,)).permute(0, 4, 1, 2, 3)
    assert (z - want).abs().max().item() <= 1e-6


def test_video_video_branch_and_no_bn_layer_take_the_reference_order(fx):
    m = _module(fx, fused=True).eval()                          # fused=True, and still ATen: audio=None is not built as kernels
    z, a = m(fx["x"])
    assert tuple(z.shape) == (2, 64, 5, 7, 7) and a == 0
    m2 = TPAVIModule(64, bn_layer=False, fused=True).eval()
    assert isinstance(m2.W_z, torch.nn.Conv3d) and list(m2.state_dict())[4:8] == ["g.weight", "g.bias", "W_z.weight", "W_z.bias"]
    z2, _ = m2(fx["x"], fx["audio"])
    assert tuple(z2.shape) == (2, 64, 5, 7, 7)


def test_unsupported_modes_raise_naming_what_is_supported():
    for mode in ("gaussian", "embedded", "concatenate"):
        with pytest.raises(NotImplementedError, match="mode='dot'"):
            TPAVIModule(64, mode=mode)
    for dim in (1, 2):
        with pytest.raises(NotImplementedError, match="dimension=3"):
            TPAVIModule(64, dimension=dim)
    with pytest.raises(ValueError):
        TPAVIModule(64, mode="nonsense")


def test_header_declares_the_exports_and_keeps_the_version():
    h = open(os.path.join(ROOT, "include", "dgsct.h")).read()
    assert re.search(r"^#define DGSCT_VERSION 101\s*$", h, re.M)
    for name in NEW_EXPORTS:
        assert re.search(r"^int(64_t)? " + name + r"\(", h, re.M), name
        assert name not in _lib.EXPORTS


def test_emulation_library_lacks_the_kernels_and_fused_true_raises(fx):
    lib = _lib.Lib(build_emu())
    assert not lib.has_tpavi()
    m = _module(fx, fused=True, lib=lib)
    with pytest.raises(RuntimeError, match="dgsct_tpavi_forward"):
        m(fx["x"], fx["audio"])
    with pytest.raises(RuntimeError, match="dgsct_tpavi_ws_bytes"):
        lib.tpavi_ws_bytes(2, 64, 5, 7, 7)


def test_fused_true_never_falls_back_on_cpu_tensors(fx):
    m = _module(fx, fused=True)
    with pytest.raises(RuntimeError, match="no CPU path"):
        m(fx["x"], fx["audio"])
    with pytest.raises(RuntimeError, match="no CPU path"):
        m.forward_frames(fx["x"].permute(0, 2, 1, 3, 4).reshape(10, 64, 7, 7), fx["audio"], T=5)


def test_fused_none_with_an_empty_set_is_the_aten_linear_form(fx, monkeypatch):
    assert isinstance(tpavi_mod._KERNELS_FASTER, frozenset)
    monkeypatch.setattr(tpavi_mod, "_KERNELS_FASTER", frozenset())
    m = _module(fx).eval()
    assert m.fused is None and not m._use_fused(fx["x"], fx["audio"], None)
    called = []
    monkeypatch.setattr(ops, "tpavi", lambda *a, **k: called.append(1))
    z, _ = m(fx["x"], fx["audio"])
    z2, _ = _module(fx, fused=False).eval()(fx["x"], fx["audio"])
    assert not called and torch.equal(z, z2)
    # a listed shape still needs a ROCm tensor: CPU tensors stay on ATen
    monkeypatch.setattr(tpavi_mod, "_KERNELS_FASTER", frozenset({(10, 7, 7)}))
    assert not m._use_fused(fx["x"], fx["audio"], None)
    assert not ops.tpavi_supported(fx["x"], fx["audio"])
