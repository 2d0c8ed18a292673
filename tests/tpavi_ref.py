"""TEST INFRASTRUCTURE: the audio-visual TPAVI block (mode 'dot', audio branch, BatchNorm layer) in plain torch, float64, in the
REFERENCE's order -- it materialises ``f = theta(x)^T phi(audio)`` [B, THW, THW] (DG-SCT/AVS/avs_scripts/avs_s4/model/TPAVI.py:82-153) --
at any (B, C, T, H, W), the seeded case generator, and the comparison rule of the TPAVI tests.  It is the yardstick at the shapes
tests/golden/ref_tpavi.pt does not cover; tools/make_golden_tpavi.py asserts it is <= 1e-10 from the reference module.
Shared by tests/test_tpavi_cpu.py and tests/test_tpavi_gpu.py."""
import math

import torch
import torch.nn.functional as F

PARAMS = ("align_channel.weight", "align_channel.bias", "norm_layer.weight", "norm_layer.bias", "g.weight", "g.bias", "W_z.0.weight",
          "W_z.0.bias", "W_z.1.weight", "W_z.1.bias", "theta.weight", "theta.bias", "phi.weight", "phi.bias")
BUFFERS = ("W_z.1.running_mean", "W_z.1.running_var", "W_z.1.num_batches_tracked")
KEYS = PARAMS[:10] + BUFFERS + PARAMS[10:]                 # the reference's state_dict order
NONTRIVIAL = ("W_z.1.weight", "W_z.1.bias", "norm_layer.weight", "norm_layer.bias", "align_channel.bias", "g.bias", "W_z.0.bias",
              "theta.bias", "phi.bias")


def set_nontrivial(state, seed):
    """overwrite (in place) what the constructor leaves at or near zero -- the BatchNorm affine (0, 0: z would be LayerNorm(x)), the
    LayerNorm affine (1, 0) and the five biases -- with seeded values; weights near 1, biases within +-0.5"""
    g = torch.Generator().manual_seed(seed)
    for k in NONTRIVIAL:
        t = state[k]
        r = torch.rand(t.shape, generator=g, dtype=torch.float32)
        t.copy_((0.5 + r) if k in ("W_z.1.weight", "norm_layer.weight") else (r - 0.5))
    return state


def make_case(B, C, T, H, W, seed):
    """(state in the reference's key order, x [B, C, T, H, W], audio [B, T, 128], cotangent of z, cotangent of audio_temp), fp32, from one
    seeded generator; Linear / Conv3d weights uniform in +-1/sqrt(fan_in) as the constructor draws them"""
    g = torch.Generator().manual_seed(seed)
    Ci = C // 2
    u = lambda fan, *s: (torch.rand(*s, generator=g) * 2 - 1) / math.sqrt(fan)          # noqa: E731
    shapes = {"align_channel.weight": (128, (C, 128)), "align_channel.bias": (128, (C,)), "norm_layer.weight": (1, (C,)),
              "norm_layer.bias": (1, (C,)), "g.weight": (C, (Ci, C, 1, 1, 1)), "g.bias": (C, (Ci,)), "W_z.0.weight": (Ci, (C, Ci, 1, 1, 1)),
              "W_z.0.bias": (Ci, (C,)), "W_z.1.weight": (1, (C,)), "W_z.1.bias": (1, (C,)), "theta.weight": (C, (Ci, C, 1, 1, 1)),
              "theta.bias": (C, (Ci,)), "phi.weight": (C, (Ci, C, 1, 1, 1)), "phi.bias": (C, (Ci,))}
    state = {}
    for k in KEYS:
        if k == "W_z.1.running_mean":
            state[k] = torch.randn(C, generator=g) * 0.1
        elif k == "W_z.1.running_var":
            state[k] = torch.rand(C, generator=g) + 0.5
        elif k == "W_z.1.num_batches_tracked":
            state[k] = torch.tensor(0)
        else:
            state[k] = u(*shapes[k][:1], *shapes[k][1])
    set_nontrivial(state, seed + 1)
    x = torch.randn(B, C, T, H, W, generator=g)
    audio = torch.randn(B, T, 128, generator=g)
    return state, x, audio, torch.randn(B, C, T, H, W, generator=g), torch.randn(B, T, C, generator=g)


def tpavi_f64(state, x, audio, training, cot_z=None, cot_a=None):
    """the block in the reference's order, float64.  Returns a dict: ``z``, ``audio_temp``, ``running_mean`` / ``running_var`` after the
    call, and with cotangents ``dx``, ``daudio`` and ``grads`` {parameter name: gradient} (one backward of both outputs)."""
    P = {k: state[k].detach().double().requires_grad_(True) for k in PARAMS}
    rm, rv = state["W_z.1.running_mean"].detach().double().clone(), state["W_z.1.running_var"].detach().double().clone()
    x, audio = x.detach().double().requires_grad_(True), audio.detach().double().requires_grad_(True)
    B, C = x.shape[:2]
    Ci = P["g.weight"].shape[0]
    H, W = x.shape[-2:]
    audio_temp = F.linear(audio, P["align_channel.weight"], P["align_channel.bias"])
    au = audio_temp.permute(0, 2, 1).unsqueeze(-1).unsqueeze(-1).repeat(1, 1, 1, H, W)
    g_x = F.conv3d(x, P["g.weight"], P["g.bias"]).view(B, Ci, -1).permute(0, 2, 1)
    theta_x = F.conv3d(x, P["theta.weight"], P["theta.bias"]).view(B, Ci, -1).permute(0, 2, 1)
    phi_x = F.conv3d(au, P["phi.weight"], P["phi.bias"]).view(B, Ci, -1)
    f = torch.matmul(theta_x, phi_x)                                             # [B, THW, THW]
    y = torch.matmul(f / f.size(-1), g_x)
    y = y.permute(0, 2, 1).contiguous().view(B, Ci, *x.shape[2:])
    w = F.batch_norm(F.conv3d(y, P["W_z.0.weight"], P["W_z.0.bias"]), rm, rv, P["W_z.1.weight"], P["W_z.1.bias"], training, 0.1, 1e-5)
    z = F.layer_norm((w + x).permute(0, 2, 3, 4, 1), (C,), P["norm_layer.weight"], P["norm_layer.bias"], 1e-5).permute(0, 4, 1, 2, 3)
    out = dict(z=z.detach(), audio_temp=audio_temp.detach(), running_mean=rm, running_var=rv)
    if cot_z is not None:
        torch.autograd.backward([z, audio_temp], [cot_z.double(), cot_a.double()])
        out.update(dx=x.grad, daudio=audio.grad, grads={k: P[k].grad for k in PARAMS})
    return out


def grad_scales(grads):
    """{name: the scale a gradient's error is taken relative to}: max(1, |ref|max); a gradient whose float64 reference is below 1e-9 is
    analytically zero (``W_z.0.bias`` in front of a batch-statistics BatchNorm; ``theta.bias`` at B = 1) and takes the largest |ref|max
    among the case's other parameter gradients"""
    mx = {k: g.abs().max().item() for k, g in grads.items()}
    big = max(mx.values())
    return {k: max(1.0, big if m < 1e-9 else m) for k, m in mx.items()}


def check(got, ref, bound, what, scale=None):
    """|got - ref|max < bound x max(1, |ref|max) (or x ``scale``); prints the figure first"""
    ref = ref.double()
    scale = max(1.0, ref.abs().max().item()) if scale is None else scale
    assert got.shape == ref.shape, (what, got.shape, ref.shape)
    err = (got.detach().cpu().double() - ref).abs().max().item()
    print(f"{what}: max abs err {err:.3e} (bound {bound * scale:.3e})")
    assert err < bound * scale, (what, err, bound * scale)
