"""GPU: the TPAVI kernels (csrc/tpavi.hip) through ``TPAVIModule(fused=True)`` against the float64 CPU reference -- the
reference-generated fixture (tests/golden/ref_tpavi.pt, ref_tpavi_eval.pt) at its shape, tests/tpavi_ref.py (the reference's order: it
materialises f) everywhere else -- and their determinism, layouts, memory and limits.

Bounds are the project's own for fp32 kernels (test_cmbs_gpu.py), relative to scale: outputs and running statistics within
1e-5 x max(1, |ref|max), input and parameter gradients within 1e-4 x max(1, |ref|max); a gradient whose float64 reference is below 1e-9
(``W_z.0.bias`` in train mode; ``theta.bias`` at B = 1) takes the largest |ref|max among the case's other parameter gradients
(tpavi_ref.grad_scales).

The grids are capped: the tile passes run at most 256 persistent workgroups over the 64-position tiles (B * T * ceil(H W / 64) of them) and
the dA / dc pass at most 16 workgroups per clip and 64-column block.  The last case has 17 * 2 * 9 = 306 tiles, 18 per clip: past both."""
import os

import pytest
import torch

from helpers import GOLDEN
import tpavi_ref as R

import dgsct_amd  # noqa: F401
from dgsct_amd import TPAVIModule, ops
from dgsct_amd._lib import default_lib

pytestmark = pytest.mark.gpu
SEED = 21
# (B, C, T, H, W): the fixture, odd unaligned planes | the smallest: H != W, one clip, the zero d theta.bias | the real width, several
# position tiles per frame with a tail | T != 5, the middle width | more tiles than the capped grids have workgroups (module docstring)
CASES = [(2, 64, 5, 7, 7), (1, 64, 5, 3, 5), (3, 256, 5, 14, 14), (2, 128, 2, 6, 10), (17, 64, 2, 19, 27)]
_REF = {}


def _fixture():
    d = torch.load(os.path.join(GOLDEN, "ref_tpavi.pt"), weights_only=True)
    d.update(torch.load(os.path.join(GOLDEN, "ref_tpavi_eval.pt"), weights_only=True))
    return d


def _case(shape, mode):
    """inputs + the float64 CPU reference, computed once per (case, mode) and shared"""
    key = (shape, mode)
    if key not in _REF:
        if shape == CASES[0]:
            fx = _fixture()
            for m in ("train", "eval"):
                _REF[(shape, m)] = (fx["state"], fx["x"], fx["audio"], fx["cot_z"], fx["cot_a"], fx[m])
        else:
            state, x, audio, cz, ca = R.make_case(*shape, seed=SEED)
            _REF[key] = (state, x, audio, cz, ca, R.tpavi_f64(state, x, audio, mode == "train", cz, ca))
    return _REF[key]


def _module(state, C, dev, train, **kw):
    m = TPAVIModule(C, **kw)
    m.load_state_dict(state)
    return m.to(dev).train(train)


def _run(m, x, audio, cz, ca, dev, frames=False):
    x, audio = x.to(dev), audio.to(dev)
    B, C, T, H, W = x.shape
    if frames:
        x = x.permute(0, 2, 1, 3, 4).reshape(B * T, C, H, W).contiguous()
        cz = cz.permute(0, 2, 1, 3, 4).reshape(B * T, C, H, W)
    x.requires_grad_(True)
    audio.requires_grad_(True)
    z, a = m.forward_frames(x, audio, T=T) if frames else m(x, audio)
    torch.autograd.backward([z, a], [cz.to(dev), ca.to(dev)])
    torch.cuda.synchronize()
    return z.detach(), a.detach(), x.grad, audio.grad


@pytest.mark.parametrize("mode", ["train", "eval"])
@pytest.mark.parametrize("shape", CASES, ids=["x".join(map(str, c)) for c in CASES])
def test_kernels_vs_the_float64_reference(shape, mode):
    dev = torch.device("cuda:0")
    state, x, audio, cz, ca, ref = _case(shape, mode)
    m = _module(state, shape[1], dev, mode == "train", fused=True)
    z, a, dx, da = _run(m, x, audio, cz, ca, dev)
    R.check(z, ref["z"], 1e-5, "z")
    R.check(a, ref["audio_temp"], 1e-5, "audio_temp")
    R.check(dx, ref["dx"], 1e-4, "dx")
    R.check(da, ref["daudio"], 1e-4, "daudio")
    scales = R.grad_scales(ref["grads"])
    params = dict(m.named_parameters())
    assert sorted(params) == sorted(R.PARAMS) and len(params) == 14
    for k in R.PARAMS:
        assert params[k].grad is not None, k
        R.check(params[k].grad, ref["grads"][k], 1e-4, "d " + k, scales[k])
    bn = m.W_z[1]
    R.check(bn.running_mean, ref["running_mean"], 1e-5, "running_mean")
    R.check(bn.running_var, ref["running_var"], 1e-5, "running_var")
    assert int(bn.num_batches_tracked) == (1 if mode == "train" else 0)
    if mode == "train":
        assert ref["grads"]["W_z.0.bias"].abs().max().item() < 1e-9
        if shape[0] == 1:
            assert ref["grads"]["theta.bias"].abs().max().item() < 1e-9


@pytest.mark.parametrize("mode", ["train", "eval"])
def test_two_calls_and_both_layouts_are_bit_identical(mode):
    dev = torch.device("cuda:0")
    shape = CASES[3]
    state, x, audio, cz, ca, _ = _case(shape, mode)
    B, C, T, H, W = shape
    runs = []
    for frames in (False, False, True):
        m = _module(state, C, dev, mode == "train", fused=True)
        z, a, dx, da = _run(m, x, audio, cz, ca, dev, frames=frames)
        if frames:
            assert tuple(z.shape) == (B * T, C, H, W) and tuple(dx.shape) == (B * T, C, H, W)
            z, dx = (t.reshape(B, T, C, H, W).permute(0, 2, 1, 3, 4) for t in (z, dx))
        grads = [p.grad for p in m.parameters()]
        runs.append([z, a, dx, da, m.W_z[1].running_mean, m.W_z[1].running_var] + grads)
    for other in runs[1:]:
        for i, (p, q) in enumerate(zip(runs[0], other)):
            assert torch.equal(p, q), i


def test_frame_sum_cotangent_argument_of_the_export():
    """``ds`` of dgsct_tpavi_backward (the cotangent of the frame sums, broadcast into dx by the last kernel) against the broadcast
    added afterwards; the autograd path adds it in an extra pass and leaves the argument NULL"""
    dev = torch.device("cuda:0")
    lib = default_lib()
    B, C, T, H, W = 2, 64, 3, 5, 9
    g = torch.Generator().manual_seed(3)
    r = lambda *s: torch.randn(*s, generator=g).to(dev)      # noqa: E731
    x, dz, A, c, ds, ln_w = r(B, C, T, H, W), r(B, C, T, H, W), r(B, C, C) / 8, r(B, C), r(B, T, C), r(C)
    st = (C * T * H * W, T * H * W, H * W)
    outs = []
    for d in (None, ds):
        dx, dA, dc, dlw, dlb = torch.empty_like(x), torch.empty(B, C, C, device=dev), torch.empty(B, C, device=dev), r(C), r(C)
        ws = torch.empty(lib.tpavi_ws_bytes(B, C, T, H, W), dtype=torch.uint8, device=dev)
        lib.tpavi_backward((B, C, T, H, W), x.data_ptr(), st, A.data_ptr(), c.data_ptr(), None, None, None, ln_w.data_ptr(), 1e-5, dz.data_ptr(),
                           st, d.data_ptr() if d is not None else None, dx.data_ptr(), st, dA.data_ptr(), dc.data_ptr(), None, None,
                           dlw.data_ptr(), dlb.data_ptr(), ws.data_ptr(), torch.cuda.current_stream().cuda_stream)
        torch.cuda.synchronize()
        outs.append((dx, dA, dc))
    want = outs[0][0] + ds.permute(0, 2, 1)[:, :, :, None, None]
    assert (outs[1][0] - want).abs().max().item() <= 1e-6 * max(1.0, want.abs().max().item())
    assert torch.equal(outs[0][1], outs[1][1]) and torch.equal(outs[0][2], outs[1][2])


def test_nothing_n_by_n_is_allocated():
    """(1, 64, 5, 28, 28): f alone would be 61 MB, x is 1 MB; forward + backward must stay under 16 x the bytes of x"""
    dev = torch.device("cuda:0")
    B, C, T, H, W = 1, 64, 5, 28, 28
    state, x, audio, cz, ca = R.make_case(B, C, T, H, W, seed=SEED)
    m = _module(state, C, dev, True, fused=True)
    x, audio, cz, ca = x.to(dev).requires_grad_(True), audio.to(dev).requires_grad_(True), cz.to(dev), ca.to(dev)
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    before = torch.cuda.memory_allocated()
    z, a = m(x, audio)
    torch.autograd.backward([z, a], [cz, ca])
    torch.cuda.synchronize()
    rise = torch.cuda.max_memory_allocated() - before
    xbytes = x.numel() * 4
    print(f"peak rise {rise} bytes = {rise / xbytes:.2f} x the bytes of x")
    assert rise < 16 * xbytes, (rise, xbytes)


def test_limits_raise_with_fused_true():
    dev = torch.device("cuda:0")
    for C, T, dtype in ((96, 5, torch.float32), (512, 5, torch.float32), (64, 17, torch.float32), (64, 5, torch.bfloat16)):
        m = TPAVIModule(C, fused=True).to(dev)
        x = torch.zeros(1, C, T, 4, 4, device=dev, dtype=dtype)
        audio = torch.zeros(1, T, 128, device=dev, dtype=dtype)
        with pytest.raises(RuntimeError, match="tpavi"):
            m(x, audio)
    assert not ops.tpavi_supported(torch.zeros(1, 96, 5, 4, 4, device=dev), torch.zeros(1, 5, 128, device=dev))
    assert ops.tpavi_supported(torch.zeros(1, 64, 5, 4, 4, device=dev), torch.zeros(1, 5, 128, device=dev))
    with pytest.raises(RuntimeError, match="C a multiple of 64"):
        default_lib().tpavi_ws_bytes(1, 96, 5, 4, 4)
