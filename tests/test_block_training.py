"""Training the backbone blocks through the fused window attention (AVS-S4 trains the HTS-AT blocks: DG-SCT/AVS/avs_scripts/avs_s4/
train.py:145-163; its block is htsat.py's SwinTransformerBlock, restated as `HTSATBlock`).

* Fixtures (tools/make_golden_block_grads.py): the reference HTS-AT block's parameter gradients (tests/golden/htsat_block_grads.pt) and
  those of an independent Swin-V2 implementation, fp32 and float64 (tests/golden/swinv2_block_grads.pt).
* CPU: the ATen path against both; the differentiable table graph (a known dbm reaches the bias table as the window-summed scatter-add);
  frozen tables stay cached; the AVS-S4 freeze rule and `FrozenBlocks(train_htsat=True)`.
* GPU: the table-gradient backward of csrc/wattn.hip (dgsct_window_attn_backward_tables) at kernel level against an fp32 autograd
  evaluation, dqkv / O bit-identical to the frozen backward; trainable blocks on the fused path against the fixtures; one Adam step of
  an adapter stack with trainable HTS-AT blocks."""
import math
import os
import sys

import pytest
import torch
import torch.nn.functional as F

from helpers import ROOT
sys.path.insert(0, os.path.join(ROOT, "tests", "emu"))
from dgsct_amd.backbone import FrozenBlocks, HTSATBlock, SwinV2Block, _from_windows, _to_windows

_L2 = lambda a, b: ((a.float().cpu() - b.float().cpu()).norm() / b.float().cpu().norm().clamp_min(1e-30)).item()     # noqa: E731


def _htsat_fx():
    return torch.load(os.path.join(ROOT, "tests", "golden", "htsat_block_grads.pt"), weights_only=False)


def _swin_fx():
    return torch.load(os.path.join(ROOT, "tests", "golden", "swinv2_block_grads.pt"), weights_only=False)


def _htsat_block(fx, **kw):
    dim, res, heads, ws, shift = fx["cfg"]
    blk = HTSATBlock(dim, (res, res), heads, window_size=ws, shift_size=shift, mlp_ratio=fx["mlp_ratio"], **kw).eval()
    r = blk.load_state_dict(fx["state"], strict=False)
    assert set(r.missing_keys) <= {"attn_mask", "attn.relative_position_index"} and not r.unexpected_keys
    return blk


def _swin_block(fx, **kw):
    dim, res, heads, ws, shift = fx["cfg"]
    blk = SwinV2Block(dim, (res, res), heads, window_size=ws, shift_size=shift, **kw).eval()
    r = blk.load_timm_state_dict(fx["state"], strict=False)
    assert set(r.missing_keys) <= {"attn_mask", "attn.relative_coords_table", "attn.relative_position_index"} and not r.unexpected_keys
    return blk


def _run(blk, x, cot):
    x = x.clone().requires_grad_(True)
    y = blk(x)
    y = y[0] if isinstance(y, tuple) else y
    y.backward(cot)
    return y.detach(), x.grad, {n: p.grad for n, p in blk.named_parameters()}


# ---- CPU ----------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["plain", "shifted", "one_window", "hw24_shifted"])
def test_htsat_parameter_gradients_match_the_reference_fixture(name):
    fx = _htsat_fx()[name]
    y, dx, g = _run(_htsat_block(fx, fused=False), fx["x"], fx["cot"])
    assert (y - fx["y"]).abs().max() < 1e-5 and (dx - fx["dx"]).abs().max() < 1e-5
    assert g.keys() == fx["grads"].keys() and "attn.relative_position_bias_table" in g
    for k in g:
        assert (g[k] - fx["grads"][k]).abs().max() < 1e-5, k


@pytest.mark.parametrize("name", ["shifted", "small_plain"])
def test_swinv2_parameter_gradients_match_the_independent_fixture(name):
    """no further from the float64 evaluation than twice the independent implementation's own fp32 result (the rule test_backbone.py
    applies to dx: fp32 rounding alone puts these sums ~1e-4 from exact)"""
    fx = _swin_fx()[name]
    _, _, g = _run(_swin_block(fx, fused=False), fx["x"], fx["cot"])
    assert g.keys() == fx["grads"].keys()
    assert {"attn.cpb_mlp.0.weight", "attn.cpb_mlp.0.bias", "attn.cpb_mlp.2.weight", "attn.logit_scale", "attn.q_bias", "attn.v_bias"} <= set(g)
    for k in g:
        ref = fx["grads_f64"][k]
        e_m, e_fx = (g[k].double() - ref).abs().max().item(), (fx["grads"][k].double() - ref).abs().max().item()
        assert e_m <= 2 * e_fx + 1e-6 * ref.abs().max().item(), (k, e_m, e_fx)


def test_bias_table_gets_the_window_summed_scatter_add_of_dbm():
    """the trainable table graph: bm = bias_table[pair index] (+ mask) per window type; d/d(table) of <dbm, bm> is dbm summed over the window
    types, then scatter-added by pair index"""
    torch.manual_seed(2)
    blk = HTSATBlock(32, (16, 16), 4, window_size=8, shift_size=4)
    a = blk.attn
    bm, scale = a._tables(blk.attn_mask)
    assert bm.requires_grad and bm.shape == (4, 4, 64, 64) and not scale.requires_grad
    dbm = torch.randn_like(bm)
    (got,) = torch.autograd.grad(bm, a.relative_position_bias_table, dbm)
    summed = dbm.sum(0).permute(1, 2, 0).reshape(64 * 64, 4)                # [i * n + j, head]
    want = torch.zeros_like(a.relative_position_bias_table).index_add_(0, a.relative_position_index.reshape(-1), summed)
    assert torch.allclose(got, want, rtol=1e-5, atol=1e-5)
    with torch.no_grad():                                                  # the same values as the frozen (cached) table
        bm0, _ = a._tables(blk.attn_mask)
    assert torch.equal(bm.detach(), bm0)


def test_swinv2_tables_carry_gradients_to_cpb_mlp_and_logit_scale():
    torch.manual_seed(3)
    blk = SwinV2Block(32, (16, 16), 4, window_size=8, shift_size=4)
    a = blk.attn
    bm, scale = a._tables(blk.attn_mask)
    assert bm.requires_grad and scale.requires_grad and scale.shape == (4,)
    srcs = list(a.cpb_mlp.parameters()) + [a.logit_scale]
    gs = torch.autograd.grad((bm * torch.randn_like(bm)).sum() + (scale * torch.randn_like(scale)).sum(), srcs)
    assert all(g is not None and g.abs().sum() > 0 for g in gs)


def test_frozen_tables_stay_cached_and_unchanged():
    torch.manual_seed(4)
    for blk in (HTSATBlock(32, (16, 16), 4, window_size=8, shift_size=4), SwinV2Block(32, (16, 16), 4, window_size=8, shift_size=4)):
        for p in blk.parameters():
            p.requires_grad_(False)
        a = blk.attn
        bm1, s1 = a._tables(blk.attn_mask)
        bm2, s2 = a._tables(blk.attn_mask)
        assert bm1 is bm2 and s1 is s2 and not bm1.requires_grad
        n, h = a.window_size[0] ** 2, a.num_heads
        if isinstance(a, SwinV2Block.__init__.__globals__["_WindowAttentionV2"]):
            table = a.cpb_mlp(a.relative_coords_table).reshape(-1, h)
            want = (16 * torch.sigmoid(table[a.relative_position_index.reshape(-1)].reshape(n, n, h).permute(2, 0, 1)))[None]
            with torch.no_grad():
                a.cpb_mlp[0].bias.add_(1.0)                                 # every cpb_mlp parameter is in the cache key
            assert a._tables(blk.attn_mask)[0] is not bm1
        else:
            want = a.relative_position_bias_table[a.relative_position_index.reshape(-1)].reshape(n, n, h).permute(2, 0, 1)[None]
        assert torch.equal(bm1, (want + blk.attn_mask[:, None]).detach())


def test_trainable_fused_block_on_a_library_without_the_table_entry_keeps_todays_behaviour():
    """the host emulation has no dgsct_window_attn_backward_tables: dqkv as before, no table gradient, one warning"""
    from build_emu import build_emu
    from dgsct_amd._lib import Lib
    lib = Lib(build_emu())
    assert not lib.has_window_attn_tables
    fx = _htsat_fx()["shifted"]
    blk = _htsat_block(fx, fused=True, lib=lib).to(torch.bfloat16)
    with pytest.warns(RuntimeWarning, match="no dgsct_window_attn_backward_tables") if not _warned(lib) else _nullctx():
        _, dx, g = _run(blk, fx["x"].bfloat16(), fx["cot"].bfloat16())
    assert g["attn.relative_position_bias_table"] is None and g["attn.qkv.weight"] is not None
    assert _L2(dx, fx["dx"]) < 5e-2


def _warned(lib):
    from dgsct_amd import ops
    return lib.path in ops._WARNED_NO_TABLES


class _nullctx:
    def __enter__(self):
        return self

    def __exit__(self, *a):
        return False


def test_avs_s4_freeze_rule_and_the_default_rule():
    from dgsct_amd.train import trainable_by_name
    names = ["module.encoder_backbone.swin.layers.0.blocks.0.attn.qkv.weight", "module.ViT.norm.weight", "module.audio_backbone.htsat.layers.0."
             "blocks.0.attn.relative_position_bias_table", "module.adapter_blocks.0.fc.weight", "module.temporal_attn.0.weight",
             "module.decoder.conv1.weight", "module.mlp_class.weight"]
    mk = lambda: [(n, torch.nn.Parameter(torch.zeros(1))) for n in names]                                  # noqa: E731
    ps = mk()
    groups = trainable_by_name(ps, task="avs_s4")
    assert [p.requires_grad for _, p in ps] == [False, False, True, True, True, True, True]
    assert len(groups) == len(names) and all(g["lr"] == 5e-4 for g in groups)
    ps = mk()
    trainable_by_name(ps)                                                   # "ave": main_trans.py:211-256, unchanged
    assert [p.requires_grad for _, p in ps] == [False, False, False, True, True, False, True]
    ps = mk()
    trainable_by_name(ps, is_vit_ln=True, task="ave")
    assert [p.requires_grad for _, p in ps] == [False, True, False, True, True, False, True]
    with pytest.raises(ValueError):
        trainable_by_name(mk(), task="avs_ms3")


def test_frozen_blocks_train_htsat_option():
    stages = [dict(layers=2, Nv=36, Cv=128, Na=64, Ca=96)]
    fb = FrozenBlocks(stages, dtype=torch.bfloat16, train_htsat=True)
    assert all(p.requires_grad and p.dtype == torch.float32 for p in fb.aud.parameters())
    assert all(not p.requires_grad and p.dtype == torch.bfloat16 for p in fb.vis.parameters())
    assert all(b.compute_dtype == torch.bfloat16 for b in fb.aud) and all(b.compute_dtype is None for b in fb.vis)
    f_a = torch.randn(2, 64, 96).bfloat16()
    y = fb.aud_block(1, f_a)                                                # (CPU: the ATen path on bf16 casts of the fp32 masters)
    assert y.dtype == torch.bfloat16
    y.float().sum().backward()
    assert all(p.grad is not None and p.grad.dtype == torch.float32 for p in fb.aud[1].parameters())
    fb0 = FrozenBlocks(stages, dtype=torch.bfloat16)                        # default: unchanged
    assert not any(p.requires_grad for p in fb0.parameters()) and all(p.dtype == torch.bfloat16 for p in fb0.parameters())


def test_window_attention_argument_checks():
    from build_emu import build_emu
    from dgsct_amd import ops
    from dgsct_amd._lib import Lib
    lib = Lib(build_emu())
    qkv = torch.randn(1, 64, 3 * 32).bfloat16()
    bm, sc = torch.zeros(1, 2, 16, 16), torch.ones(2)
    ops.window_attention(qkv, bm, sc, 8, 8, 4, 0, 2, lib)
    for bad in (dict(qkv=torch.randn(1, 60, 96).bfloat16()), dict(sc=torch.ones(2, 1)), dict(bm=torch.zeros(3, 2, 16, 16))):
        a = dict(dict(qkv=qkv, bm=bm, sc=sc), **bad)
        with pytest.raises(RuntimeError):
            ops.window_attention(a["qkv"], a["bm"], a["sc"], 8, 8, 4, 0, 2, lib)


# ---- GPU ----------------------------------------------------------------------------------------------------------------------------------
def _wattn_autograd(qkv, bm, scale, H, W, ws, shift, heads, cosine):
    """the window attention in ATen (roll, partition, logits tensor): what the kernel computes, evaluated by autograd in qkv's dtype"""
    B, L, C3 = qkv.shape
    hd, n, nW = C3 // (3 * heads), ws * ws, (H // ws) * (W // ws)
    x = qkv.reshape(B, H, W, C3)
    if shift:
        x = torch.roll(x, (-shift, -shift), (1, 2))
    q, k, v = _to_windows(x, ws).reshape(B * nW, n, 3, heads, hd).permute(2, 0, 3, 1, 4)
    if cosine:
        q, k = F.normalize(q, dim=-1), F.normalize(k, dim=-1)
    logits = (q @ k.transpose(-2, -1)) * scale.to(q.dtype)[None, :, None, None]
    logits = (logits.reshape(B, nW, heads, n, n) + bm.to(q.dtype)[None]).reshape(B * nW, heads, n, n)
    o = (logits.softmax(-1) @ v).transpose(1, 2).reshape(B * nW, n, heads * hd)
    o = _from_windows(o, ws, H, W)
    if shift:
        o = torch.roll(o, (shift, shift), (1, 2))
    return o.reshape(B, L, heads * hd)


def _kernel_geoms():
    from dgsct_amd import ave_stage_shapes
    from dgsct_amd.backbone import _HTSAT_HEADS, _SWIN_HEADS
    g = [(2, 16, 16, 8, 4, 4, 24), (2, 24, 24, 12, 6, 4, 32), (3, 6, 6, 6, 0, 8, 32), (2, 8, 8, 8, 0, 3, 16), (1, 24, 12, 12, 0, 2, 8)]
    for s in ave_stage_shapes("swinv2_base"):                               # the eight AVE geometries of tools/wattn_bench.py, B = 2
        for N, C, ws0, heads in ((s["Nv"], s["Cv"], 12, _SWIN_HEADS[s["Cv"]]), (s["Na"], s["Ca"], 8, _HTSAT_HEADS[s["Ca"]])):
            R = int(round(math.sqrt(N)))
            ws = min(ws0, R)
            g.append((2, R, R, ws, ws // 2 if R > ws else 0, heads, C // heads))
    return g


@pytest.mark.gpu
@pytest.mark.parametrize("geom", _kernel_geoms(), ids=lambda g: "B{}-{}x{}-ws{}-s{}-h{}-hd{}".format(*g))
@pytest.mark.parametrize("nwm_all", [False, True], ids=["nwm1", "nwmW"])
@pytest.mark.parametrize("cosine", [False, True], ids=["dot", "cosine"])
def test_window_attention_table_gradients_on_gpu(geom, nwm_all, cosine):
    from dgsct_amd import ops
    from dgsct_amd._lib import default_lib
    lib = default_lib()
    assert lib.has_window_attn_tables
    B, H, W, ws, shift, heads, hd = geom
    n, nW = ws * ws, (H // ws) * (W // ws)
    nwm = nW if nwm_all else 1
    dev = torch.device("cuda:0")
    gen = torch.Generator().manual_seed(17)
    qkv = torch.randn(B, H * W, 3 * heads * hd, generator=gen).bfloat16()
    bm = torch.randn(nwm, heads, n, n, generator=gen)
    if shift and nwm_all:
        bm[:, :, : n // 2, n // 2:] -= 100.0
    scale = (torch.rand(heads, generator=gen) + 0.2) * (8.0 if cosine else 1.0)
    dout = torch.randn(B, H * W, heads * hd, generator=gen).bfloat16()
    # fp32 and bf16 autograd of the same bf16 inputs (CPU)
    ref = {}
    for dt in (torch.float32, torch.bfloat16):
        b_, s_ = bm.clone().requires_grad_(True), scale.clone().requires_grad_(True)
        o = _wattn_autograd(qkv.to(dt), b_, s_, H, W, ws, shift, heads, cosine)
        o.backward(dout.to(dt))
        ref[dt] = (b_.grad, s_.grad)
    # the kernel, table variant and frozen variant
    q0 = qkv.to(dev)
    runs = []
    for _ in range(2):
        qd = q0.clone().requires_grad_(True)
        bd, sd = bm.to(dev).requires_grad_(True), scale.to(dev).requires_grad_(True)
        o = ops.window_attention(qd, bd, sd, H, W, ws, shift, heads, lib, cosine=cosine)
        o.backward(dout.to(dev))
        runs.append((o.detach(), qd.grad, bd.grad, sd.grad))
    qf = q0.clone().requires_grad_(True)
    of = ops.window_attention(qf, bm.to(dev), scale.to(dev), H, W, ws, shift, heads, lib, cosine=cosine)
    of.backward(dout.to(dev))
    torch.cuda.synchronize()
    o_t, dq_t, dbm, dsc = runs[0]
    assert torch.equal(o_t, of.detach()) and torch.equal(dq_t, qf.grad)          # dqkv of the table variant: bit-identical
    assert dbm.shape == bm.shape and dsc.shape == scale.shape and dbm.dtype == dsc.dtype == torch.float32
    for got, k in ((dbm, 0), (dsc, 1)):
        e, e_a = _L2(got, ref[torch.float32][k]), _L2(ref[torch.bfloat16][k], ref[torch.float32][k])
        assert e < 1.5 * e_a + 2e-3 and e < 3e-2, (k, e, e_a)
    assert _L2(runs[1][2], dbm) < 1e-5 and _L2(runs[1][3], dsc) < 1e-5        # run to run: atomic order only


_FIXTURE_BLOCKS = [("htsat", "plain"), ("htsat", "shifted"), ("htsat", "one_window"), ("htsat", "hw24_shifted"), ("swin", "shifted"),
                   ("swin", "small_plain")]


@pytest.mark.gpu
@pytest.mark.parametrize("case", _FIXTURE_BLOCKS, ids=lambda c: f"{c[0]}-{c[1]}")
@pytest.mark.parametrize("masters", [False, True], ids=["bf16", "fp32-masters"])
def test_trainable_block_parameter_gradients_on_gpu(case, masters):
    """a trainable block on the default fused path (fused=None) in bf16 -- parameters bf16, or fp32 masters with compute_dtype=bf16 --
    gets EVERY parameter gradient, the bias table / cpb_mlp.* / logit_scale included (None before the table-gradient backward), no
    further from the fixture than 1.5 x the bf16 ATen path (+ 2e-3)"""
    kind, name = case
    fx = (_htsat_fx() if kind == "htsat" else _swin_fx())[name]
    mk = _htsat_block if kind == "htsat" else _swin_block
    dev = torch.device("cuda:0")
    res = {}
    for tag, fused in (("aten", False), ("fused", None)):
        blk = mk(fx, fused=fused)
        if masters:
            blk.compute_dtype = torch.bfloat16
            blk = blk.to(dev)
        else:
            blk = blk.to(dev, torch.bfloat16)
        y, dx, g = _run(blk, fx["x"].to(dev, torch.bfloat16), fx["cot"].to(dev, torch.bfloat16))
        res[tag] = (y, dx, g)
    must = ["attn.relative_position_bias_table"] if kind == "htsat" else ["attn.cpb_mlp.0.weight", "attn.cpb_mlp.0.bias", "attn.cpb_mlp.2.weight",
                                                                          "attn.logit_scale"]
    g_f, g_a = res["fused"][2], res["aten"][2]
    assert all(g_f[k] is not None for k in must)
    assert g_f.keys() == fx["grads"].keys()
    for k, ref in fx["grads"].items():
        assert g_f[k] is not None and torch.isfinite(g_f[k].float()).all(), k
        if masters:
            assert g_f[k].dtype == torch.float32, k
        e_f, e_a = _L2(g_f[k], ref), _L2(g_a[k], ref)
        assert e_f < 1.5 * e_a + 2e-3, (k, e_f, e_a)
    assert _L2(res["fused"][1], fx["dx"]) < 1.5 * _L2(res["aten"][1], fx["dx"]) + 2e-3


@pytest.mark.gpu
def test_adapter_stack_with_trainable_htsat_blocks_one_adam_step_on_gpu():
    """AVS-S4's setting: adapters + HTS-AT blocks train (fp32 masters, bf16 compute through the fused kernels), Swin-V2 frozen"""
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
    fb = FrozenBlocks(stages, dtype=torch.bfloat16, train_htsat=True).to(dev)
    with torch.no_grad():
        for n, p in fb.aud.named_parameters():
            if "bias_table" in n:
                p.copy_(0.5 * torch.randn_like(p))
    feats = [(torch.randn(4, s["Nv"], s["Cv"], device=dev, dtype=torch.bfloat16, requires_grad=True),
              torch.randn(4, s["Na"], s["Ca"], device=dev, dtype=torch.bfloat16, requires_grad=True)) for s in stages]
    outs, maps = st(feats, vis_block=fb.vis_block, aud_block=fb.aud_block)
    params = [p for p in list(st.parameters()) + list(fb.parameters()) if p.requires_grad]
    opt = torch.optim.Adam(params, lr=1e-3)
    tabs0 = [b.attn.relative_position_bias_table.detach().clone() for b in fb.aud]
    torch.autograd.backward([t for pr in outs for t in pr], [torch.randn_like(t) for pr in outs for t in pr])
    torch.cuda.synchronize()
    for n, p in fb.aud.named_parameters():
        assert p.grad is not None and p.grad.dtype == torch.float32 and torch.isfinite(p.grad).all() and p.grad.abs().sum() > 0, n
    assert all(p.grad is None for p in fb.vis.parameters())
    assert all(torch.isfinite(m.flat_param.grad).all() for m in st.modules() if hasattr(m, "flat_param"))
    opt.step()
    torch.cuda.synchronize()
    assert all(not torch.equal(t0, b.attn.relative_position_bias_table.detach()) for t0, b in zip(tabs0, fb.aud))
