"""GPU: the CMBS event head kernels (csrc/head.hip) against the plain-torch formulation on the CPU (tests/cmbs_ref.py) and against the
reference-generated fixture (tests/golden/ref_cmbs.pt), their saved state, determinism and limits, and ``AVENet`` from waveform + frames
through ``ave_loss`` and back at the real stage-0 geometry.

Bounds are the project's own for its fp32 head kernel (test_temporal_gate_kernel_vs_torch): outputs < 1e-5, input and parameter
gradients < 1e-4 x max(1, |ref|max).  Every case asserts on the CPU that its inputs are >= 1e-4 away from a tie in the top-4 selection and
in the arg-max over time before it compares anything (the generator seeds were picked for that)."""
import os

import pytest
import torch

from helpers import GOLDEN
from cmbs_ref import PARAMS, head_torch, make_case, tie_margins

import dgsct_amd  # noqa: F401
from dgsct_amd import AVENet, CMBS, ave_stage_shapes, ops
from dgsct_amd._lib import default_lib
from dgsct_amd.train import ave_loss, trainable_by_name

pytestmark = pytest.mark.gpu
GAMMA = 0.3
# (T, B, D, K, generator seed): the fixture's shape | the smallest, T = top-k so every mask bit is set | exactly one timestep excluded |
# every limit at once | more clips than the capped grid of the backward has workgroups (several clips per partial row)
CASES = [(10, 3, 256, 28, 1), (4, 1, 64, 5, 1), (5, 2, 128, 28, 1), (32, 5, 512, 32, 1), (10, 67, 256, 28, 657)]
_REF = {}


def _case(T, B, D, K, seed):
    """inputs + the CPU reference (outputs, gradients), computed once per case and shared"""
    key = (T, B, D, K, seed)
    if key not in _REF:
        v, a, params, cots = make_case(T, B, D, K, seed)
        top, amax = tie_margins(v, a, params["Wvc"], params["bvc"], params["Wac"], params["bac"])
        assert top >= 1e-4 and amax >= 1e-4, (key, top, amax)
        ins = [t.clone().requires_grad_(True) for t in (v, a, *[params[n] for n in PARAMS])]
        outs = head_torch(*ins, GAMMA)
        torch.autograd.backward(list(outs), cots)
        _REF[key] = (v, a, params, cots, [o.detach() for o in outs], [t.grad for t in ins])
    return _REF[key]


def _dev_inputs(v, a, params, dev, requires_grad=True):
    return [t.to(dev).requires_grad_(requires_grad) for t in (v, a, *[params[n] for n in PARAMS])]


def _close_out(got, ref, what):
    err = (got.detach().cpu() - ref).abs().max().item()
    print(f"{what}: max abs err {err:.3e}")
    assert err < 1e-5, (what, err)


def _close_grad(got, ref, what):
    err, scale = (got.cpu() - ref).abs().max().item(), max(1.0, ref.abs().max().item())
    print(f"{what}: max abs err {err:.3e} (bound {1e-4 * scale:.3e})")
    assert err < 1e-4 * scale, (what, err, scale)


@pytest.mark.parametrize("T,B,D,K,seed", CASES, ids=[f"T{c[0]}-B{c[1]}-D{c[2]}-K{c[3]}" for c in CASES])
def test_head_kernels_vs_torch(T, B, D, K, seed):
    dev = torch.device("cuda:0")
    v, a, params, cots, ref_out, ref_grad = _case(T, B, D, K, seed)
    ins = _dev_inputs(v, a, params, dev)
    outs = ops.cmbs_head(*ins, GAMMA, default_lib(), return_saved=True)
    torch.autograd.backward(list(outs[:3]), [c.to(dev) for c in cots])
    torch.cuda.synchronize()
    assert [tuple(o.shape) for o in outs[:3]] == [(T, B, 1), (B, K), (B, K)]
    for o, r, n in zip(outs[:3], ref_out, ("is_event", "event", "av")):
        _close_out(o, r, n)
    for t, r, n in zip(ins, ref_grad, ("d_v", "d_a") + tuple("d_" + p for p in PARAMS)):
        assert t.grad.shape == r.shape
        _close_grad(t.grad, r, n)
    # the saved state: exactly four selected timesteps per (clip, modality, class), inside T; the arg-max inside T and the CPU's
    topmask, argmax = outs[3].cpu(), outs[4].cpu()
    assert topmask.shape == (B, 2, K) and argmax.shape == (B, D) and topmask.dtype == argmax.dtype == torch.int32
    bits = torch.stack([(topmask >> t) & 1 for t in range(32)], -1)
    assert (bits.sum(-1) == 4).all() and (bits[..., T:] == 0).all()
    assert ((argmax >= 0) & (argmax < T)).all()
    assert torch.equal(argmax.long(), ((v + a) / 2).max(dim=0)[1])
    for m, (W, b_) in enumerate(((params["Wvc"], params["bvc"]), (params["Wac"], params["bac"]))):
        sel = ((v, a)[m] @ W.t() + b_).topk(4, dim=0)[1]                                 # [4, B, K]
        want = torch.zeros(B, K, dtype=torch.int64)
        for j in range(4):
            want |= 1 << sel[j]
        assert torch.equal(topmask[:, m].long() & 0xFFFFFFFF, want)


def _module(fx, dev, **kw):
    torch.manual_seed(fx["seed"])
    m = CMBS(None, **kw)
    assert all(torch.equal(m.state_dict()[k], t) for k, t in fx["state"].items())
    return m.to(dev).eval()


@pytest.fixture(scope="module")
def fx():
    return torch.load(os.path.join(GOLDEN, "ref_cmbs.pt"), weights_only=True)


def test_module_matches_the_reference_fixture(fx):
    dev = torch.device("cuda:0")
    m = _module(fx, dev, fused=True)
    v, a = fx["v"].to(dev).requires_grad_(True), fx["a"].to(dev).requires_grad_(True)
    outs = m(v, a)
    torch.autograd.backward(list(outs), [fx[k].to(dev) for k in ("cot_is", "cot_ev", "cot_av")])
    torch.cuda.synchronize()
    for o, n in zip(outs, ("is_event", "event", "av")):
        assert o.shape == fx[n].shape
        _close_out(o, fx[n], n)
    _close_grad(v.grad, fx["d_v"], "d_v")
    _close_grad(a.grad, fx["d_a"], "d_a")
    params = dict(m.named_parameters())
    for k, r in fx["grads"].items():
        _close_grad(params[k].grad, r, k)
    assert [n for n, p in params.items() if p.grad is None] == fx["no_grad"]


def test_parameter_gradients_are_bit_identical_from_call_to_call():
    """fixed-order reduction of per-workgroup partial rows, no atomics: two backward calls on one saved state agree bit for bit
    (B = 67: the capped grid sums several clips per row)"""
    dev = torch.device("cuda:0")
    v, a, params, cots, _, _ = _case(*CASES[4])
    ins = _dev_inputs(v, a, params, dev)
    outs = ops.cmbs_head(*ins, GAMMA, default_lib())
    cd = [c.to(dev) for c in cots]
    g1 = torch.autograd.grad(list(outs), ins, cd, retain_graph=True)
    g2 = torch.autograd.grad(list(outs), ins, cd)
    torch.cuda.synchronize()
    for x, y in zip(g1, g2):
        assert torch.equal(x, y)


def test_only_event_scores_in_the_loss(monkeypatch):
    """is_event and av_score unused: the op does not materialise their cotangents, so the library call really gets NULL for d_is and
    d_av (checked on the call's arguments) and the kernel reads them as zero"""
    dev = torch.device("cuda:0")
    lib = default_lib()
    v, a, params, cots, _, _ = _case(*CASES[0])
    ref_in = [t.clone().requires_grad_(True) for t in (v, a, *[params[n] for n in PARAMS])]
    (head_torch(*ref_in, GAMMA)[1] * cots[1]).sum().backward()
    seen = []
    real = lib.cmbs_head_backward
    monkeypatch.setattr(lib, "cmbs_head_backward", lambda *args: (seen.append(args[13:16]), real(*args))[1])
    ins = _dev_inputs(v, a, params, dev)
    (ops.cmbs_head(*ins, GAMMA, lib)[1] * cots[1].to(dev)).sum().backward()
    torch.cuda.synchronize()
    assert len(seen) == 1 and seen[0][0] is None and seen[0][1] is not None and seen[0][2] is None, seen
    for t, r, n in zip(ins, ref_in, ("d_v", "d_a") + tuple("d_" + p for p in PARAMS)):
        if r.grad is None:                                          # (classifier.{weight, bias} feed is_event only: the kernel returns zeros)
            assert t.grad is not None and not t.grad.abs().sum(), n
        else:
            _close_grad(t.grad, r.grad, n)


@pytest.mark.parametrize("keep", [0, 1, 2], ids=["only_d_is", "only_d_ev", "only_d_av"])
def test_backward_with_null_cotangents_direct_call(keep):
    """dgsct_cmbs_head_backward with two of the three cotangent pointers NULL, called directly, against torch with those two outputs
    left out of the loss; B = 67, so partial rows hold several clips"""
    dev = torch.device("cuda:0")
    lib = default_lib()
    T, B, D, K, seed = CASES[4]
    v, a, params, cots, _, _ = _case(T, B, D, K, seed)
    ref_in = [t.clone().requires_grad_(True) for t in (v, a, *[params[n] for n in PARAMS])]
    (head_torch(*ref_in, GAMMA)[keep] * cots[keep]).sum().backward()
    ins = _dev_inputs(v, a, params, dev, False)
    topmask, argmax = ops.cmbs_head(*ins, GAMMA, lib, return_saved=True)[3:]
    cd = [cots[i].to(dev).contiguous() if i == keep else None for i in range(3)]
    f32 = dict(dtype=torch.float32, device=dev)
    dv, da = torch.full((T, B, D), float("nan"), **f32), torch.full((T, B, D), float("nan"), **f32)
    grads = [torch.full(s, float("nan"), **f32) for s in ((K, D), (K,), (K, D), (K,), (1, D), (1,), (K, D), (K,))]
    ws = torch.empty(lib.cmbs_head_ws_bytes(T, B, D, K), dtype=torch.uint8, device=dev)
    d = dict(zip(("v", "a") + PARAMS, ins))
    ptr = lambda t: t.data_ptr() if t is not None else None        # noqa: E731
    lib.cmbs_head_backward(T, B, D, K, GAMMA, ptr(d["v"]), ptr(d["a"]), ptr(d["Wvc"]), ptr(d["Wac"]), ptr(d["wc"]), ptr(d["We"]), ptr(topmask),
                           ptr(argmax), *[ptr(c) for c in cd], ptr(dv), ptr(da), [g.data_ptr() for g in grads], ptr(ws),
                           torch.cuda.current_stream(dev).cuda_stream)
    torch.cuda.synchronize()
    for got, r, n in zip([dv, da] + grads, ref_in, ("d_v", "d_a") + tuple("d_" + p for p in PARAMS)):
        ref = r.grad if r.grad is not None else torch.zeros_like(r)
        _close_grad(got, ref, n)


def test_frozen_head_returns_input_gradients_only(fx):
    dev = torch.device("cuda:0")
    m = _module(fx, dev, fused=True).requires_grad_(False)
    v, a = fx["v"].to(dev).requires_grad_(True), fx["a"].to(dev).requires_grad_(True)
    torch.autograd.backward(list(m(v, a)), [fx[k].to(dev) for k in ("cot_is", "cot_ev", "cot_av")])
    torch.cuda.synchronize()
    _close_grad(v.grad, fx["d_v"], "d_v")
    _close_grad(a.grad, fx["d_a"], "d_a")
    assert all(p.grad is None for p in m.parameters())


@pytest.mark.parametrize("T,D,K", [(3, 256, 28), (10, 96, 28), (10, 256, 33)], ids=["T3", "D96", "K33"])
def test_out_of_limit_shapes_raise_with_the_launchers_message(T, D, K):
    dev = torch.device("cuda:0")
    v, a, params, _ = make_case(T, 2, D, K, 1)
    with pytest.raises(RuntimeError, match=r"dgsct_cmbs_head_forward failed.*need 4 <= T <= 32 \(top-k is fixed at 4\), D a multiple of 64 and <= 512, 1 <= K <= 32"):
        ops.cmbs_head(*_dev_inputs(v, a, params, dev, False), GAMMA, default_lib())
    with pytest.raises(RuntimeError, match="dgsct_cmbs_head_ws_bytes failed"):
        default_lib().cmbs_head_ws_bytes(T, 2, D, K)


def test_avenet_waveform_and_frames_to_loss_and_back():
    """two-stage trunk at the real stage-0 geometry (4096 x 96 audio / 2304 x 128 visual tokens), B = 1 clip of T = 4 frames"""
    dev = torch.device("cuda:0")
    torch.manual_seed(0)
    B, T = 1, 4
    net = AVENet(ave_stage_shapes("swinv2_base")[:2], T=T, head_fused=True).to(dev)
    trainable_by_name(net.named_parameters())
    net.eval()
    # MIOpen's LSTM backward only exists in training mode: train() with every dropout probability set to 0 (tests/test_temporal.py)
    net.temporal_attn.train()
    for mod in net.temporal_attn.modules():
        if isinstance(mod, torch.nn.Dropout):
            mod.p = 0.0
        elif isinstance(mod, (torch.nn.MultiheadAttention, torch.nn.LSTM)):
            mod.dropout = 0.0
    net.trunk.train()
    with torch.no_grad():
        for n, p in net.trunk.stack.named_parameters():
            if n.endswith("gate") or n.endswith("gate_av"):
                p.fill_(0.5)                                   # the adapters are live
    wave = 0.1 * torch.randn(B * T, 160000, device=dev)
    frames = torch.randn(B, T, 3, 192, 192, device=dev)
    labels = torch.zeros(B, T, 29, device=dev)
    labels[0, :2, 7] = 1.0
    labels[0, 2:, 28] = 1.0
    outs = net(wave, frames)
    loss = ave_loss(*outs, labels)
    loss.backward()
    torch.cuda.synchronize()
    assert [tuple(o.shape) for o in outs] == [(T, B, 1), (B, 28), (T, B, 1), (B, 28)]
    assert all(torch.isfinite(o).all() for o in outs) and torch.isfinite(loss)
    nonzero = lambda p: p.grad is not None and bool(torch.isfinite(p.grad).all()) and float(p.grad.abs().sum()) > 0      # noqa: E731
    for name in ("audio_adapter_blocks_p1", "vis_adapter_blocks_p1", "audio_adapter_blocks_p2", "vis_adapter_blocks_p2"):
        for n, p in getattr(net.trunk.stack, name)[0].named_parameters():
            if n != "gate_tk":                                 # declared and never read by the reference forward either
                assert nonzero(p), (name, n)
    dead = ("AVInter.", "VAInter.", "video_norm.", "audio_norm.")
    for n, p in net.CMBS.named_parameters():
        assert (p.grad is None) if n.startswith(dead) else nonzero(p), n
    # temporal_attn: the never-called prototypes / self_attn of the decoder layers have no gradient (as in the reference); what has one is
    # finite, and every live weight matrix's is non-zero (a key bias's is zero by the softmax's shift invariance: not asked of vectors)
    live = [(n, p) for n, p in net.temporal_attn.named_parameters() if p.grad is not None]
    assert len(live) > 60
    for n, p in live:
        assert torch.isfinite(p.grad).all(), n
        if p.dim() >= 2:
            assert nonzero(p), n
    for mod in (net.patch_embed, net.frontend, net.trunk.blocks, net.trunk.vis_merge, net.trunk.aud_merge, net.trunk.norm):
        assert all(p.grad is None for p in mod.parameters())
