"""SURVEY.md 8(f) row f4 (round 5, first step): the frozen blocks either side of the adapter calls (dg-sct_amd/backbone.py).

* `HTSATBlock` against the reference class (`DG-SCT/AVE/nets/htsat.py:135-251`) through the committed fixture
  `tests/golden/htsat_block.pt` (oracle/make_golden_backbone.py: the restatement matches the imported reference bit for bit on CPU).
* `SwinV2Block` restates timm 0.6.12 (not vendored, not installed): parity UNPINNED.  What can be checked without timm is checked:
  the window partition / cyclic shift / shift mask / relative-offset plumbing against a direct per-token evaluation of the published
  formulas over the whole map (every token against every token, membership and offsets computed from coordinates).
* On the GPU: the blocks as `AdapterStack(vis_block=, aud_block=)` callables in bf16 -- gradients flow through the frozen blocks to
  the adapters below, their own parameters get none."""
import math
import os

import pytest
import torch

from helpers import ROOT
import sys
sys.path.insert(0, os.path.join(ROOT, "tests", "emu"))
from dgsct_amd.backbone import FrozenBlocks, HTSATBlock, SwinV2Block


def _cases():
    return torch.load(os.path.join(ROOT, "tests", "golden", "htsat_block.pt"), weights_only=False)


@pytest.mark.parametrize("name", ["plain", "shifted", "one_window"])
def test_htsat_block_matches_reference_fixture(name):
    fx = _cases()[name]
    dim, res, heads, ws, shift = fx["cfg"]
    blk = HTSATBlock(dim, (res, res), heads, window_size=ws, shift_size=shift).eval()
    blk.load_state_dict(fx["state"])
    x = fx["x"].clone().requires_grad_(True)
    y, attn = blk(x)
    y.backward(fx["cot"])
    assert (y - fx["y"]).abs().max() < 1e-5 and (x.grad - fx["dx"]).abs().max() < 1e-5
    assert attn.shape == (3 * (res // blk.window_size) ** 2, heads, blk.window_size ** 2, blk.window_size ** 2)


def _swin_cases():
    return torch.load(os.path.join(ROOT, "tests", "golden", "swinv2_block.pt"), weights_only=False)


def _swin_block(fx, **kw):
    dim, res, heads, ws, shift = fx["cfg"]
    blk = SwinV2Block(dim, (res, res), heads, window_size=ws, shift_size=shift, **kw).eval()
    r = blk.load_timm_state_dict(fx["state"], strict=False)          # the geometry-derived buffers are not in the fixture
    assert set(r.missing_keys) <= {"attn_mask", "attn.relative_coords_table", "attn.relative_position_index"} and not r.unexpected_keys
    return blk


@pytest.mark.parametrize("name", ["plain", "shifted", "one_window", "small_shifted"])
def test_swinv2_block_matches_the_independent_implementation_fixture(name):
    """timm 0.6.12 (the reference's Swin-V2 blocks) is absent: parity against timm stays unpinned.  This pins `SwinV2Block` against an
    INDEPENDENT implementation of the same published block -- Hugging Face transformers' `Swinv2Layer`, run by oracle/make_golden_swinv2.py
    with its parameters renamed to timm's layout -- in float64 (oracle/make_golden_swinv2.py --f64) output and input gradient to 1e-10;
    in fp32 the output to 1e-5 and the input gradient no further from the float64 result than twice the HF layer's own fp32 gradient
    (fp32 rounding alone puts dx ~2e-5 from exact here, and where on that scale it lands depends on the host's BLAS) -- plain / shifted
    12 x 12 windows on a 24 x 24 map, the map as one 6 x 6 window, shifted 8 x 8 windows."""
    fx = _swin_cases()[name]
    ref = torch.load(os.path.join(ROOT, "tests", "golden", "swinv2_block_f64.pt"), weights_only=False)[name]
    x64 = fx["x"].double().requires_grad_(True)
    y64 = _swin_block(fx, fused=False).double()(x64)
    y64.backward(fx["cot"].double())
    assert (y64 - ref["y"]).abs().max() < 1e-10 and (x64.grad - ref["dx"]).abs().max() < 1e-10
    blk = _swin_block(fx, fused=False)
    x = fx["x"].clone().requires_grad_(True)
    y = blk(x)
    y.backward(fx["cot"])
    assert (y - fx["y"]).abs().max() < 1e-5
    assert (x.grad.double() - ref["dx"]).abs().max() <= 2 * (fx["dx"].double() - ref["dx"]).abs().max()
    # the two halves as the AVE loop calls them (net_trans.py:894, :903) compose to the block
    h = fx["x"] + blk.attn_branch(fx["x"])
    assert torch.allclose(h + blk.mlp_branch(h), y.detach(), atol=1e-6)


@pytest.mark.parametrize("name", ["plain", "shifted", "one_window", "small_shifted"])
def test_swinv2_block_fused_path_against_the_fixture_on_the_host_emulation(name):
    """the same fixture through the fused path (cosine window attention + LayerNorm / residual of the C ABI, host-loop emulation) in bf16"""
    from build_emu import build_emu
    from dgsct_amd._lib import Lib
    fx = _swin_cases()[name]
    blk = _swin_block(fx, fused=True, lib=Lib(build_emu())).to(torch.bfloat16)
    x = fx["x"].bfloat16().requires_grad_(True)
    y = blk(x)
    y.backward(fx["cot"].bfloat16())
    assert _L2(y, fx["y"]) < 3e-2 and _L2(x.grad, fx["dx"]) < 5e-2


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["plain", "shifted", "one_window", "small_shifted"])
def test_swinv2_block_bf16_on_gpu(name):
    """bf16 on the GPU against the fp32 fixture: the ATen formulation sets the yardstick (a post-norm block in bf16: 1.5 % / 3 % on these
    tiny widths), the path THROUGH THE KERNELS (wattn cosine mode, dgsct_layer_norm_*) may be no further than 1.5 x that"""
    fx = _swin_cases()[name]
    dev = torch.device("cuda:0")
    err = {}
    for fused in (False, True):
        blk = _swin_block(fx, fused=fused).to(dev, torch.bfloat16)
        x = fx["x"].to(dev, torch.bfloat16).requires_grad_(True)
        y = blk(x)
        y.backward(fx["cot"].to(dev, torch.bfloat16))
        err[fused] = (_L2(y, fx["y"]), _L2(x.grad, fx["dx"]))
    assert err[False][0] < 3e-2 and err[False][1] < 5e-2, err
    assert err[True][0] < 1.5 * err[False][0] + 2e-3 and err[True][1] < 1.5 * err[False][1] + 2e-3, err


def _naive_swinv2_attn(blk: SwinV2Block, x: torch.Tensor) -> torch.Tensor:
    """`blk._attn(x)` evaluated token against token over the whole map: two tokens interact iff the cyclic shift puts them into the same
    window; inside a window, tokens that the shift brought together from different sides of the map border get -100 on their logit;
    the position bias is 16 sigmoid(cpb_mlp(log-spaced (dy, dx))) of their offset in the shifted frame (Liu et al. 2022, eqs. 3-4)."""
    H, W = blk.input_resolution
    ws, s, h = blk.window_size, blk.shift_size, blk.num_heads
    a = blk.attn
    B, L, C = x.shape
    ys, xs = torch.meshgrid(torch.arange(H), torch.arange(W), indexing="ij")
    sy, sx = ((ys - s) % H).reshape(-1), ((xs - s) % W).reshape(-1)            # coordinates after the roll by -s
    same_win = (sy[:, None] // ws == sy[None, :] // ws) & (sx[:, None] // ws == sx[None, :] // ws)
    reg = lambda c, n: torch.where(c < n - ws, 0, torch.where(c < n - s, 1, 2)) if s else torch.zeros_like(c)
    region = reg(sy, H) * 3 + reg(sx, W)
    masked = region[:, None] != region[None, :]
    bias3 = torch.cat([a.q_bias, torch.zeros_like(a.v_bias), a.v_bias])
    q, k, v = torch.nn.functional.linear(x, a.qkv.weight, bias3).reshape(B, L, 3, h, C // h).permute(2, 0, 3, 1, 4)
    qn, kn = q / q.norm(dim=-1, keepdim=True).clamp_min(1e-12), k / k.norm(dim=-1, keepdim=True).clamp_min(1e-12)
    logits = (qn @ kn.transpose(-2, -1)) * torch.clamp(a.logit_scale, max=math.log(100.0)).exp()
    dy, dx = (sy[:, None] - sy[None, :]).float(), (sx[:, None] - sx[None, :]).float()
    off = torch.stack([dy, dx], -1) / (ws - 1) * 8
    off = torch.sign(off) * torch.log2(off.abs() + 1) / math.log2(8)
    bias = 16 * torch.sigmoid(a.cpb_mlp(off)).permute(2, 0, 1)                  # [h, L, L]
    logits = logits + bias[None] + torch.where(masked, -100.0, 0.0)[None, None]
    logits = logits.masked_fill(~same_win[None, None], float("-inf"))
    return a.proj((logits.softmax(-1) @ v).transpose(1, 2).reshape(B, L, C))


@pytest.mark.parametrize("res,ws,shift", [(24, 12, 0), (24, 12, 6), (12, 12, 6), (16, 8, 4)])
def test_swinv2_block_windowing_against_a_per_token_evaluation(res, ws, shift):
    torch.manual_seed(5)
    blk = SwinV2Block(32, (res, res), 2, window_size=ws, shift_size=shift).eval()
    with torch.no_grad():
        for p in blk.parameters():
            p.add_(0.2 * torch.randn_like(p))
    x = torch.randn(2, res * res, 32)
    with torch.no_grad():
        got, ref = blk._attn(x), _naive_swinv2_attn(blk, x)
    assert (got - ref).abs().max() < 2e-5, (got - ref).abs().max()
    if res <= ws:
        assert blk.shift_size == 0 and blk.attn_mask is None                 # a window as large as the map: no shift (stages 2-3 at 192^2)


def test_swinv2_block_loads_a_timm_style_state_dict():
    """a timm checkpoint names the block's tensors `attn.{qkv.weight, q_bias, v_bias, logit_scale, cpb_mlp.0.*, cpb_mlp.2.weight,
    proj.*}`, `norm1 / norm2.*`, `mlp.fc1 / fc2.*`, `attn_mask`, and -- depending on the release -- the derived buffers
    `attn.relative_coords_table` / `attn.relative_position_index`.  Both key sets must load by name (parity itself stays UNPINNED: timm is
    not installed here)."""
    blk = SwinV2Block(128, (24, 24), 4, window_size=12, shift_size=6)
    own = blk.state_dict()
    expect = {"attn.logit_scale", "attn.cpb_mlp.0.weight", "attn.cpb_mlp.0.bias", "attn.cpb_mlp.2.weight", "attn.qkv.weight", "attn.q_bias",
              "attn.v_bias", "attn.proj.weight", "attn.proj.bias", "norm1.weight", "norm1.bias", "mlp.fc1.weight", "mlp.fc1.bias",
              "mlp.fc2.weight", "mlp.fc2.bias", "norm2.weight", "norm2.bias", "attn_mask"}
    assert set(own) == expect, set(own) ^ expect
    torch.manual_seed(1)
    sd = {k: torch.randn_like(v) for k, v in own.items()}
    blk.load_timm_state_dict(sd)                                              # release without the derived buffers
    sd2 = dict(sd, **{"attn.relative_coords_table": blk.attn.relative_coords_table.clone(),
                      "attn.relative_position_index": blk.attn.relative_position_index.clone()})
    blk.load_timm_state_dict(sd2)                                             # release that stores them
    assert all(torch.equal(blk.state_dict()[k], v) for k, v in sd.items())
    with pytest.raises(RuntimeError):
        blk.load_timm_state_dict(dict(sd, bogus=torch.zeros(1)))


def test_frozen_blocks_are_frozen_and_shaped_for_the_ave_stack():
    from dgsct_amd import ave_stage_shapes
    fb = FrozenBlocks(ave_stage_shapes("swinv2_base"), dtype=torch.float32)
    assert len(fb.vis) == len(fb.aud) == 12 and not any(p.requires_grad for p in fb.parameters())
    assert [b.window_size for b in fb.vis] == [12, 12, 12, 12] + [12] * 6 + [6, 6]
    assert [b.shift_size for b in fb.vis][:4] == [0, 6, 0, 6] and all(b.shift_size == 0 for b in fb.vis[4:])     # stages 2-3: one window
    assert [b.shift_size for b in fb.aud] == [0, 4, 0, 4, 0, 4, 0, 4, 0, 4, 0, 0]                               # 8 x 8 map at stage 3
    f_a = torch.randn(2, 64, 768, requires_grad=True)
    y = fb.aud_block(11, f_a)
    y.sum().backward()
    assert f_a.grad is not None and y.shape == f_a.shape


@pytest.mark.gpu
def test_adapter_stack_with_frozen_blocks_on_gpu():
    """harness B of SURVEY.md 8(d): two stages of the AVE stack with the frozen half-blocks / blocks in the loop, bf16, fwd + bwd"""
    from dgsct_amd import AdapterStack
    dev = torch.device("cuda:0")
    stages = [dict(layers=1, Nv=576, Cv=256, Na=1024, Ca=192), dict(layers=2, Nv=144, Cv=512, Na=256, Ca=384)]
    torch.manual_seed(0)
    st = AdapterStack(stages, compute_dtype=torch.bfloat16).to(dev)
    with torch.no_grad():
        for n, p in st.named_parameters():
            if n.endswith("gate") or n.endswith("gate_av"):
                p.fill_(0.5)
    st.flatten_parameters().train()
    fb = FrozenBlocks(stages, dtype=torch.bfloat16).to(dev)
    feats = [(torch.randn(4, s["Nv"], s["Cv"], device=dev, dtype=torch.bfloat16, requires_grad=True),
              torch.randn(4, s["Na"], s["Ca"], device=dev, dtype=torch.bfloat16, requires_grad=True)) for s in stages]
    outs, maps = st(feats, vis_block=fb.vis_block, aud_block=fb.aud_block)
    plain, _ = st([(a.detach(), b.detach()) for a, b in feats])
    torch.autograd.backward([t for pr in outs for t in pr], [torch.randn_like(t) for pr in outs for t in pr])
    torch.cuda.synchronize()
    for (fv, fa), (pv, pa) in zip(outs, plain):
        assert torch.isfinite(fv.float()).all() and torch.isfinite(fa.float()).all()
        assert (fv.float() - pv.float()).abs().max() > 1e-2                  # the blocks are in the loop
    assert all(torch.isfinite(f.grad.float()).all() and f.grad.abs().sum() > 0 for pr in feats for f in pr)
    assert all(p.grad is None for p in fb.parameters())
    assert all(torch.isfinite(m.flat_param.grad).all() for m in st.modules() if hasattr(m, "flat_param"))


@pytest.mark.gpu
@pytest.mark.parametrize("fused", [False, True], ids=["aten", "fused"])
@pytest.mark.parametrize("name", ["plain", "shifted", "one_window"])
def test_htsat_block_bf16_on_gpu(name, fused):
    """bf16 on the GPU against the REFERENCE class's fp32 results (fixture): the ATen formulation and the fused window-attention kernel
    (csrc/wattn.hip), output and input gradient"""
    fx = _cases()[name]
    dim, res, heads, ws, shift = fx["cfg"]
    dev = torch.device("cuda:0")
    blk = HTSATBlock(dim, (res, res), heads, window_size=ws, shift_size=shift, fused=fused).eval()
    blk.load_state_dict(fx["state"])
    blk = blk.to(dev, torch.bfloat16)
    x = fx["x"].to(dev, torch.bfloat16).requires_grad_(True)
    y, attn = blk(x)
    assert (attn is None) == fused
    y.backward(fx["cot"].to(dev, torch.bfloat16))
    assert ((y.float().cpu() - fx["y"]).norm() / fx["y"].norm()) < 2e-2
    assert ((x.grad.float().cpu() - fx["dx"]).norm() / fx["dx"].norm()) < 3e-2


_L2 = lambda a, b: ((a.float().cpu() - b.float().cpu()).norm() / b.float().cpu().norm().clamp_min(1e-30)).item()     # noqa: E731
# (block class, width, map side, heads, window, shift): HTS-AT stage-0 / stage-3 geometry (head width 24), Swin-V2-B stage 0 (12 x 12 windows of
# 144 tokens, shifted), Swin-V2 with the map as ONE 6 x 6 window (stage 3 at 192^2: 36 tokens)
_FUSED_CASES = [(HTSATBlock, 96, 16, 4, 8, 0), (HTSATBlock, 96, 16, 4, 8, 4), (HTSATBlock, 192, 8, 8, 8, 0), (SwinV2Block, 128, 24, 4, 12, 6),
                (SwinV2Block, 128, 24, 4, 12, 0), (SwinV2Block, 256, 6, 8, 12, 0)]


def _block_pair(cls, dim, res, heads, ws, shift, lib, device):
    torch.manual_seed(3)
    ref = cls(dim, (res, res), heads, window_size=ws, shift_size=shift, fused=False)
    with torch.no_grad():
        for n_, p_ in ref.named_parameters():
            if "bias_table" in n_:
                p_.copy_(0.5 * torch.randn_like(p_))                          # (trunc_normal(0.02) would leave the bias invisible)
    fused = cls(dim, (res, res), heads, window_size=ws, shift_size=shift, fused=True, lib=lib)
    fused.load_state_dict(ref.state_dict())
    x = torch.randn(3, res * res, dim).bfloat16()
    g = torch.randn(3, res * res, dim).bfloat16()
    out = {}
    for tag, m, dt in (("fp32", ref, torch.float32), ("aten", ref, torch.bfloat16), ("fused", fused, torch.bfloat16)):
        m = m.to(device, dt)
        xi = x.clone().to(device, dt).requires_grad_(True)              # (a fresh leaf: .to() of a bf16 CPU tensor to bf16 / cpu is the tensor itself)
        y = m(xi)
        y = y[0] if isinstance(y, tuple) else y
        y.backward(g.to(device, dt))
        out[tag] = (y.detach().float().cpu(), xi.grad.float().cpu())
    return out


def _check_fused(out):
    """the fused path is held to the fp32 evaluation of the SAME block: no further from it than 1.5 x the bf16 ATen path is (+ 2e-3)"""
    for k in (0, 1):
        e_f, e_a = _L2(out["fused"][k], out["fp32"][k]), _L2(out["aten"][k], out["fp32"][k])
        assert e_f < 1.5 * e_a + 2e-3, (k, e_f, e_a)


@pytest.mark.parametrize("case", _FUSED_CASES, ids=lambda c: f"{c[0].__name__}-{c[1]}-{c[2]}-s{c[5]}")
def test_fused_window_attention_semantics_on_the_host_emulation(case):
    """CPU: the C ABI's window attention (dgsct_window_attn_*, here the host-loop emulation of tests/emu with the kernel's addressing:
    window partition + cyclic shift as index arithmetic on the un-partitioned qkv map, bias + mask as one table) inside the blocks,
    against the ATen formulation that is pinned to the reference class"""
    from build_emu import build_emu
    from dgsct_amd._lib import Lib
    _check_fused(_block_pair(*case, Lib(build_emu()), torch.device("cpu")))


@pytest.mark.gpu
@pytest.mark.parametrize("case", _FUSED_CASES, ids=lambda c: f"{c[0].__name__}-{c[1]}-{c[2]}-s{c[5]}")
def test_fused_window_attention_kernel_on_gpu(case):
    _check_fused(_block_pair(*case, None, torch.device("cuda:0")))


@pytest.mark.gpu
@pytest.mark.parametrize("geom", [(2, 16, 16, 8, 4, 4, 24), (2, 24, 24, 12, 6, 4, 32), (3, 6, 6, 6, 0, 8, 32), (2, 8, 8, 8, 0, 3, 16), (1, 24, 12, 12, 0, 2, 8)])
@pytest.mark.parametrize("cosine", [False, True], ids=["dot", "cosine"])
def test_window_attention_kernel_against_the_emulation(geom, cosine):
    """the gfx950 kernel against the host loops on identical bf16 inputs through the same C-ABI entry points: forward O and lse, backward
    dqkv -- shifted and un-shifted windows, head widths 8 ... 32, 36 / 64 / 144-token windows, non-square maps; cosine: q / k rows
    normalised inside (DGSCT_WATTN_COSINE), the gradient returned for the raw rows"""
    from build_emu import build_emu
    from dgsct_amd import ops
    from dgsct_amd._lib import Lib, default_lib
    B, H, W, ws, shift, heads, hd = geom
    n, nW = ws * ws, (H // ws) * (W // ws)
    gen = torch.Generator().manual_seed(11)
    qkv = torch.randn(B, H * W, 3 * heads * hd, generator=gen).bfloat16()
    bm = torch.randn(nW if shift else 1, heads, n, n, generator=gen)
    if shift:
        bm[:, :, : n // 2, n // 2:] -= 100.0                                  # mask-like entries
    scale = torch.rand(heads, generator=gen) + 0.2
    dout = torch.randn(B, H * W, heads * hd, generator=gen).bfloat16()
    res = {}
    for tag, lib, dev in (("emu", Lib(build_emu()), torch.device("cpu")), ("hip", default_lib(), torch.device("cuda:0"))):
        q = qkv.detach().clone().to(dev).requires_grad_(True)
        o = ops.window_attention(q, bm.to(dev), scale.to(dev) * (8.0 if cosine else 1.0), H, W, ws, shift, heads, lib, cosine=cosine)
        o.backward(dout.to(dev))
        res[tag] = (o.detach(), q.grad)
    assert _L2(res["hip"][0], res["emu"][0]) < 6e-3
    assert _L2(res["hip"][1], res["emu"][1]) < 1e-2
    if cosine:      # against autograd through F.normalize on the CPU (fp32 evaluation of the same bf16 inputs)
        q = qkv.float().requires_grad_(True)
        x = q.reshape(B, H * W, 3, heads, hd)
        qn = torch.cat([torch.nn.functional.normalize(x[:, :, :2], dim=-1), x[:, :, 2:]], dim=2).reshape(B, H * W, -1)
        o = ops.window_attention(qn.bfloat16(), bm, scale * 8.0, H, W, ws, shift, heads, Lib(build_emu()))
        o.backward(dout)
        assert _L2(res["hip"][0], o) < 2e-2 and _L2(res["hip"][1], q.grad) < 4e-2


# ---- LayerNorm (+ residual) on the library's row kernels (dgsct_layer_norm_*) -------------------------------------------
def _layer_norm_case(lib, device, dtype, rows, C, residual, train_affine):
    from dgsct_amd import ops
    torch.manual_seed(rows + C)
    x = torch.randn(rows, C).to(dtype)
    r = torch.randn(rows, C).to(dtype) if residual else None
    w, b = (1 + 0.2 * torch.randn(C)), 0.2 * torch.randn(C)
    g = torch.randn(rows, C).to(dtype)
    # reference: fp32 evaluation of the same (dtype-representable) inputs
    xr, wr, br = x.float().clone().requires_grad_(True), w.clone().requires_grad_(True), b.clone().requires_grad_(True)
    rr = r.float().clone().requires_grad_(True) if residual else None
    yr = torch.nn.functional.layer_norm(xr, (C,), wr, br, 1e-5) + (rr if residual else 0)
    yr.backward(g.float())
    xd = x.clone().to(device).requires_grad_(True)
    rd = r.clone().to(device).requires_grad_(True) if residual else None
    wd, bd = w.clone().to(device).requires_grad_(train_affine), b.clone().to(device).requires_grad_(train_affine)
    y = ops.layer_norm(xd.reshape(2, rows // 2, C), wd, bd, 1e-5, rd.reshape(2, rows // 2, C) if residual else None, lib)
    y.backward(g.to(device).reshape(2, rows // 2, C))
    tol = 1e-5 if dtype == torch.float32 else 1.2e-2
    assert _L2(y.reshape(rows, C), yr) < tol and _L2(xd.grad, xr.grad) < (tol if dtype == torch.float32 else 2e-2)
    if residual:
        assert torch.equal(rd.grad.cpu(), g)
    if train_affine:
        assert _L2(wd.grad, wr.grad) < max(tol, 1e-4) and _L2(bd.grad, br.grad) < max(tol, 1e-4)
    else:
        assert wd.grad is None and bd.grad is None


_LN_CASES = [(torch.float32, 64, 96, False, True), (torch.float32, 50, 132, True, False), (torch.bfloat16, 64, 128, True, True),
             (torch.bfloat16, 36, 1024, False, False), (torch.bfloat16, 30, 1536, True, False)]


@pytest.mark.parametrize("case", _LN_CASES, ids=lambda c: f"{str(c[0])[6:]}-{c[1]}x{c[2]}-res{int(c[3])}-aff{int(c[4])}")
def test_layer_norm_c_abi_on_the_host_emulation(case):
    from build_emu import build_emu
    from dgsct_amd._lib import Lib
    _layer_norm_case(Lib(build_emu()), torch.device("cpu"), *case)


@pytest.mark.gpu
@pytest.mark.parametrize("case", _LN_CASES + [(torch.bfloat16, 23040, 512, True, False), (torch.bfloat16, 40960, 96, False, True)],
                         ids=lambda c: f"{str(c[0])[6:]}-{c[1]}x{c[2]}-res{int(c[3])}-aff{int(c[4])}")
def test_layer_norm_kernels_on_gpu(case):
    _layer_norm_case(None, torch.device("cuda:0"), *case)


def test_vis_block_map_is_the_branch_plus_its_input():
    """FrozenBlocks.vis_block_map (what bench.py --blocks hands to AdapterStack: `returns_map`) = f_v + vis_block(f_v)"""
    fb = FrozenBlocks([dict(Nv=36, Cv=128, Na=64, Ca=96, layers=1)], dtype=torch.float32, fused=False)
    f = torch.randn(2, 36, 128)
    for half in (0, 1):
        assert torch.allclose(fb.vis_block_map(0, half, f), f + fb.vis_block(0, half, f), atol=1e-6)
    assert fb.vis_block_map.returns_map and not getattr(fb.vis_block, "returns_map", False)
