"""GPU: the patch-merging kernels (csrc/pmerge.hip) behind HTSATPatchMerging / SwinV2PatchMerging and the chained AVETrunk.

The accuracy criterion is the project's own (tests/test_backbone.py::_check_fused): the fused bf16 path may be no further from the fp32
evaluation of the SAME module than 1.5 x the bf16 ATen formulation is, + 2e-3, in relative L2 -- for the output and for the input gradient.
The exact-data tests need no tolerance: with a 0/1 selection matrix as W and small integers as data every product and sum is exact, so the
gather (forward) and the scatter (backward) are compared bit for bit against index arithmetic."""
import os

import pytest
import torch

from helpers import GOLDEN

import dgsct_amd  # noqa: F401
from dgsct_amd import AVETrunk, HTSATFrontEnd, HTSATPatchMerging, PatchEmbed, SwinV2PatchMerging, ave_stage_shapes, ops
from dgsct_amd._lib import PMERGE_NORM_FIRST, PMERGE_NORM_LAST, default_lib

pytestmark = pytest.mark.gpu
FORMS = {"htsat": HTSATPatchMerging, "swinv2": SwinV2PatchMerging}
_L2 = lambda a, b: ((a.float().cpu() - b.float().cpu()).norm() / b.float().cpu().norm().clamp_min(1e-30)).item()     # noqa: E731
# non-square maps, 4C no power of two (C = 96), one token cell, 45 output rows (a ragged last row block)
_COMMON = [(3, 6, 4, 32), (1, 2, 2, 96), (2, 4, 8, 96), (5, 6, 6, 128)]
_SWEEP = [("htsat", c) for c in _COMMON] + [("swinv2", c) for c in _COMMON] + [
    ("htsat", (2, 4, 4, 192)),        # the two-chunks-per-lane row kernels (4C = 768: the audio stage-1 merge's width)
    ("swinv2", (2, 4, 4, 384)),       # ... and the Swin-V2 form's (2C = 768)
    ("htsat", (1, 4, 4, 384)),        # NORM_FIRST at its widest: three output-column tiles, the whole LDS image
    ("swinv2", (1, 4, 4, 768))]       # NORM_LAST at its deepest contraction (K = 3072)


def _rule(e_fused, e_aten, what):
    print(f"{what}: fused {e_fused:.3e}  aten {e_aten:.3e}  bound {1.5 * e_aten + 2e-3:.3e}")
    assert e_fused < 1.5 * e_aten + 2e-3, (what, e_fused, e_aten)


def _run(m, x, cot, dev, dt):
    m = m.to(dev, dt)
    xi = x.clone().to(dev, dt).requires_grad_(True)
    y = m(xi)
    y.backward(cot.to(dev, dt))
    torch.cuda.synchronize()
    return y.detach().float().cpu(), xi.grad.float().cpu()


@pytest.mark.parametrize("form,shape", _SWEEP, ids=[f"{f}-{'x'.join(map(str, s))}" for f, s in _SWEEP])
def test_fused_merge_against_fp32_on_the_same_module(form, shape):
    B, H, W, C = shape
    dev = torch.device("cuda:0")
    torch.manual_seed(7)
    ref = FORMS[form]((H, W), C, fused=False).eval()
    with torch.no_grad():
        for p in ref.parameters():
            p.add_(0.1 * torch.randn_like(p))
    fused = FORMS[form]((H, W), C, fused=True).eval().requires_grad_(False)
    fused.load_state_dict(ref.state_dict())
    x = torch.randn(B, H * W, C).bfloat16()
    cot = torch.randn(B, (H // 2) * (W // 2), 2 * C).bfloat16()
    out = {"fp32": _run(ref, x, cot, dev, torch.float32), "aten": _run(ref, x, cot, dev, torch.bfloat16),
           "fused": _run(fused, x, cot, dev, torch.bfloat16)}
    for k, what in ((0, "y"), (1, "dx")):
        _rule(_L2(out["fused"][k], out["fp32"][k]), _L2(out["aten"][k], out["fp32"][k]), f"{form} {shape} {what}")


def _ramp(B, H, W, C):
    """x[b, h, w, c] = a small integer made from its own index (exact in bf16: |v| <= 125)"""
    b, h, w, c = torch.meshgrid(torch.arange(B), torch.arange(H), torch.arange(W), torch.arange(C), indexing="ij")
    return ((b * 7 + h * 5 + w * 3 + c * 11 + (h * w) % 13) % 251 - 125).float()


def _token_and_offset(H, W, C):
    """for element k of the virtual 4C row of output cell (i, j): (row offset dh, column offset dw, channel) = segment order
    (0,0) (1,0) (0,1) (1,1), stated on its own (not through the module's gather)"""
    k = torch.arange(4 * C)
    seg = k // C
    return seg % 2, seg // 2, k % C


def _selection(C):
    """W [2C][4C] with one 1 per row at column sel[n] = (5 n + 3) mod 4C (4C is a multiple of 128, so sel is one-to-one): far from symmetric"""
    sel = (torch.arange(2 * C) * 5 + 3) % (4 * C)
    w = torch.zeros(2 * C, 4 * C)
    w[torch.arange(2 * C), sel] = 1.0
    return w, sel


def _zero_mean_ints(rows, n):
    r, c = torch.meshgrid(torch.arange(rows), torch.arange(n), indexing="ij")
    d = ((r * 3 + c * 7) % 17 - 8).float()
    d[:, 1::2] = -d[:, 0::2]                                  # every row sums to exactly 0
    return d


@pytest.mark.parametrize("shape", [(2, 4, 6, 32), (3, 6, 10, 96)], ids=lambda s: "x".join(map(str, s)))
def test_gather_and_scatter_are_exact_on_integer_data(shape):
    B, H, W, C = shape
    dev = torch.device("cuda:0")
    lib = default_lib()
    H2, W2, rows = H // 2, W // 2, B * (H // 2) * (W // 2)
    x = _ramp(B, H, W, C)
    w, sel = _selection(C)
    dh, dw, ch = _token_and_offset(H, W, C)
    st = torch.cuda.current_stream().cuda_stream
    xd = x.reshape(B, H * W, C).to(dev, torch.bfloat16).contiguous()
    wd = w.to(dev, torch.bfloat16).contiguous()
    one2, zero2 = torch.ones(2 * C, device=dev), torch.zeros(2 * C, device=dev)
    out = torch.empty(B, H2 * W2, 2 * C, device=dev, dtype=torch.bfloat16)
    pre = torch.full_like(out, float("nan"))
    mu, rstd = torch.empty(rows, device=dev), torch.empty(rows, device=dev)
    lib.patch_merge_forward(PMERGE_NORM_LAST, B, H, W, C, xd.data_ptr(), wd.data_ptr(), one2.data_ptr(), zero2.data_ptr(), 1e-5, out.data_ptr(),
                            pre.data_ptr(), mu.data_ptr(), rstd.data_ptr(), st)
    torch.cuda.synchronize()
    # index arithmetic: pre[b, i, j, n] = x[b, 2i + dh[sel n], 2j + dw[sel n], ch[sel n]]
    b_, i_, j_, n_ = torch.meshgrid(torch.arange(B), torch.arange(H2), torch.arange(W2), torch.arange(2 * C), indexing="ij")
    k_ = sel[n_]
    want = x[b_, 2 * i_ + dh[k_], 2 * j_ + dw[k_], ch[k_]].reshape(B, H2 * W2, 2 * C)
    assert torch.equal(pre.float().cpu(), want)
    assert torch.allclose(mu.cpu(), want.reshape(rows, -1).mean(1), atol=1e-4)

    # backward with mu = 0, rstd = 1 and a zero `pre` / `x`: x^ = 0, and zero-mean rows make the LayerNorm backward the identity
    zeros_r, ones_r = torch.zeros(rows, device=dev), torch.ones(rows, device=dev)
    dout = _zero_mean_ints(rows, 2 * C)
    g = (dout @ w).reshape(B, H2, W2, 4 * C)                  # both forms: dx = scatter(dout . W); its rows have zero mean too (a selection
    for mode in (PMERGE_NORM_LAST, PMERGE_NORM_FIRST):        # matrix only moves the entries of dout), which NORM_FIRST's row pass needs
        dx = torch.full((B, H * W, C), float("nan"), device=dev, dtype=torch.bfloat16)
        ws = torch.empty(lib.patch_merge_ws_bytes(mode, B, H, W, C), dtype=torch.uint8, device=dev)
        dd = dout.to(dev, torch.bfloat16).contiguous()
        cn = 2 * C if mode == PMERGE_NORM_LAST else 4 * C
        lw = torch.ones(cn, device=dev)
        zx = torch.zeros_like(xd)
        zp = torch.zeros_like(out)
        lib.patch_merge_backward(mode, B, H, W, C, dd.data_ptr(), zx.data_ptr(), wd.data_ptr(), lw.data_ptr(), zp.data_ptr(), zeros_r.data_ptr(),
                                 ones_r.data_ptr(), 1e-5, dx.data_ptr(), ws.data_ptr(), st)
        torch.cuda.synchronize()
        want_dx = torch.zeros(B, H, W, C)
        b4, i4, j4, k4 = torch.meshgrid(torch.arange(B), torch.arange(H2), torch.arange(W2), torch.arange(4 * C), indexing="ij")
        want_dx[b4, 2 * i4 + dh[k4], 2 * j4 + dw[k4], ch[k4]] = g
        assert torch.equal(dx.float().cpu().reshape(B, H, W, C), want_dx), mode


@pytest.mark.parametrize("case", [f"{f}-{s}" for f in FORMS for s in ("3x6x4x32", "2x8x8x96")])
def test_fused_merge_against_the_reference_fixture(case):
    """bf16 on the GPU against the REFERENCE's fp32 results (fixture), held to the same rule with the fixture as the fp32 side"""
    fx = torch.load(os.path.join(GOLDEN, "ref_patch_merging.pt"), weights_only=True)[case]
    B, H, W, C = fx["shape"]
    dev = torch.device("cuda:0")
    got = {}
    for tag, fused in (("aten", False), ("fused", True)):
        m = FORMS[fx["form"]]((H, W), C, fused=fused).eval().requires_grad_(False)
        m.load_state_dict(fx["state"])
        got[tag] = _run(m, fx["x"], fx["cot"], dev, torch.bfloat16)
    for k, what in ((0, "y"), (1, "dx")):
        _rule(_L2(got["fused"][k], fx[what]), _L2(got["aten"][k], fx[what]), f"{case} {what}")


@pytest.mark.parametrize("mode,shape", [(PMERGE_NORM_FIRST, (5, 6, 6, 128)), (PMERGE_NORM_FIRST, (2, 4, 8, 96)), (PMERGE_NORM_LAST, (5, 6, 6, 128)),
                                        (PMERGE_NORM_LAST, (2, 4, 8, 96))], ids=lambda v: str(v).replace(", ", "x"))
def test_backward_writes_every_element_of_dx(mode, shape):
    B, H, W, C = shape
    dev = torch.device("cuda:0")
    lib = default_lib()
    torch.manual_seed(1)
    rows, cn = B * (H // 2) * (W // 2), (4 * C if mode == PMERGE_NORM_FIRST else 2 * C)
    x = torch.randn(B, H * W, C, device=dev).bfloat16()
    w = (0.05 * torch.randn(2 * C, 4 * C, device=dev)).bfloat16()
    lw, lb = 1 + 0.1 * torch.randn(cn, device=dev), 0.1 * torch.randn(cn, device=dev)
    out = torch.empty(B, rows // B, 2 * C, device=dev, dtype=torch.bfloat16)
    pre = torch.empty_like(out)
    mu, rstd = torch.empty(rows, device=dev), torch.empty(rows, device=dev)
    st = torch.cuda.current_stream().cuda_stream
    lib.patch_merge_forward(mode, B, H, W, C, x.data_ptr(), w.data_ptr(), lw.data_ptr(), lb.data_ptr(), 1e-5, out.data_ptr(),
                            pre.data_ptr() if mode == PMERGE_NORM_LAST else None, mu.data_ptr(), rstd.data_ptr(), st)
    dout = torch.randn_like(out)
    dx = torch.full_like(x, float("nan"))
    ws = torch.empty(lib.patch_merge_ws_bytes(mode, B, H, W, C), dtype=torch.uint8, device=dev)
    lib.patch_merge_backward(mode, B, H, W, C, dout.data_ptr(), x.data_ptr(), w.data_ptr(), lw.data_ptr(),
                             pre.data_ptr() if mode == PMERGE_NORM_LAST else None, mu.data_ptr(), rstd.data_ptr(), 1e-5, dx.data_ptr(), ws.data_ptr(), st)
    torch.cuda.synchronize()
    assert torch.isfinite(out.float()).all() and torch.isfinite(mu).all() and torch.isfinite(rstd).all()
    assert not torch.isnan(dx.float()).any()


def test_limits_are_enforced_by_the_library():
    lib = default_lib()
    for mode, B, H, W, C in ((PMERGE_NORM_FIRST, 1, 4, 4, 416), (PMERGE_NORM_LAST, 1, 4, 4, 800), (PMERGE_NORM_FIRST, 1, 3, 4, 32),
                             (PMERGE_NORM_LAST, 1, 4, 0, 32), (PMERGE_NORM_FIRST, 1, 4, 4, 48), (2, 1, 4, 4, 32)):
        with pytest.raises(RuntimeError, match="dgsct_patch_merge_ws_bytes"):
            lib.patch_merge_ws_bytes(mode, B, H, W, C)
    with pytest.raises(RuntimeError, match="fused=True"):
        HTSATPatchMerging((4, 4), 416, fused=True).to("cuda:0", torch.bfloat16)(torch.randn(1, 16, 416, device="cuda:0", dtype=torch.bfloat16))
    with pytest.raises(RuntimeError, match="fused=True"):
        SwinV2PatchMerging((4, 4), 32, fused=True).to("cuda:0")(torch.randn(1, 16, 32, device="cuda:0"))             # fp32


def test_trainable_merge_takes_the_aten_formulation():
    """the kernels return dx only: a merge with a parameter that requires grad runs ATen and its parameters get their gradients;
    fused=True raises instead of falling back, as everywhere"""
    dev = torch.device("cuda:0")
    m = HTSATPatchMerging((4, 4), 32).to(dev, torch.bfloat16)
    x = torch.randn(2, 16, 32, device=dev, dtype=torch.bfloat16, requires_grad=True)
    m(x).float().sum().backward()
    assert all(p.grad is not None for p in m.parameters()) and x.grad is not None
    m.fused = True
    with pytest.raises(RuntimeError, match="requires grad"):
        m(x)
    with torch.no_grad():
        assert m(x).shape == (2, 4, 64)                       # nothing to differentiate: the kernels take it


def test_cached_parameters_follow_a_cast_of_the_module():
    """the bf16 weight / fp32 norm vectors of the fused path are remade when the module is cast after a first call (a cast bumps no
    parameter version): fp32 masters first, then the module in bf16, whose norm vectors are the ROUNDED ones"""
    dev = torch.device("cuda:0")
    torch.manual_seed(0)
    m = SwinV2PatchMerging((4, 4), 32, fused=True).to(dev).requires_grad_(False)
    with torch.no_grad():
        m.norm.weight.add_(0.1 * torch.randn_like(m.norm.weight))
    x = torch.randn(2, 16, 32, device=dev, dtype=torch.bfloat16)
    m(x)
    assert torch.equal(m._cached()[1], m.norm.weight)
    m = m.to(torch.bfloat16)
    assert not torch.equal(m.norm.weight.float(), m.__dict__["_fused_params"][2])      # the stale entry differs ...
    m(x)
    assert torch.equal(m._cached()[1], m.norm.weight.float())                                            # ... and is replaced


def test_default_dispatch_takes_the_kernels_only_where_they_were_measured_faster():
    from dgsct_amd import merging
    dev = torch.device("cuda:0")
    x = torch.randn(1, 16, 32, device=dev, dtype=torch.bfloat16, requires_grad=True)
    for cls in FORMS.values():
        m = cls((4, 4), 32).to(dev, torch.bfloat16).requires_grad_(False)
        listed = (m._MODE, 16, 32) in merging._KERNELS_FASTER
        assert ("PatchMergeFn" in type(m(x).grad_fn).__name__) == listed                # fused=None: by the table
        m.fused = True
        assert "PatchMergeFn" in type(m(x).grad_fn).__name__                            # the opt-in
        m.fused = False
        assert "PatchMergeFn" not in type(m(x).grad_fn).__name__
    # a merge the table lists (Swin-V2-B stage 2, 12 x 12 x 512) and one it measured slower (Swin-V2-L stage 2, 12 x 12 x 768)
    for dim, fused_by_default in ((512, True), (768, False)):
        m = SwinV2PatchMerging((12, 12), dim).to(dev, torch.bfloat16).requires_grad_(False)
        xx = torch.randn(1, 144, dim, device=dev, dtype=torch.bfloat16, requires_grad=True)
        assert ("PatchMergeFn" in type(m(xx).grad_fn).__name__) == fused_by_default


_STAGES = [dict(layers=1, Nv=144, Cv=128, Na=256, Ca=96), dict(layers=1, Nv=36, Cv=256, Na=64, Ca=192)]


def _stage0_grads_ok(tr):
    for name in ("audio_adapter_blocks_p1", "vis_adapter_blocks_p1", "audio_adapter_blocks_p2", "vis_adapter_blocks_p2"):
        for n, p in getattr(tr.stack, name)[0].named_parameters():
            if n == "gate_tk":                                # declared and never read by the reference forward either
                continue
            assert p.grad is not None and torch.isfinite(p.grad).all() and float(p.grad.abs().sum()) > 0, (name, n)
    for mod in (tr.blocks, tr.vis_merge, tr.aud_merge, tr.norm):
        assert all(p.grad is None for p in mod.parameters())


def test_trunk_fused_and_aten_merges_against_fp32():
    dev = torch.device("cuda:0")
    BT = 4

    def make(dtype):
        torch.manual_seed(0)
        tr = AVETrunk(_STAGES, dtype=dtype)
        with torch.no_grad():
            for n, p in tr.stack.named_parameters():
                if n.endswith("gate") or n.endswith("gate_av"):
                    p.fill_(0.5)
            for m in (tr.vis_merge, tr.aud_merge, tr.norm):
                for p in m.parameters():
                    p.add_((0.1 * torch.randn(p.shape)).to(p.dtype))
        return tr

    g = torch.Generator().manual_seed(1)
    f_v = torch.randn(BT, 144, 128, generator=g).bfloat16()
    f_a = torch.randn(BT, 256, 96, generator=g).bfloat16()
    cv, ca = torch.randn(BT, 1, 256, generator=g).bfloat16(), torch.randn(BT, 1, 192, generator=g).bfloat16()
    res = {}
    for tag, dtype in (("fp32", torch.float32), ("aten", torch.bfloat16), ("fused", torch.bfloat16)):
        tr = make(dtype).to(dev).train()
        if tag == "aten":
            for m in list(tr.vis_merge) + list(tr.aud_merge):
                m.fused = False
        if tag == "fused":
            for m in list(tr.vis_merge) + list(tr.aud_merge):
                m.fused = True                                # (raises instead of falling back)
        xv = f_v.clone().to(dev, dtype).requires_grad_(True)
        xa = f_a.clone().to(dev, dtype).requires_grad_(True)
        pv, pa, outs, maps = tr(xv, xa)
        torch.autograd.backward([pv, pa], [cv.to(dev, dtype), ca.to(dev, dtype)])
        torch.cuda.synchronize()
        assert pv.shape == (BT, 1, 256) and pa.shape == (BT, 1, 192)
        _stage0_grads_ok(tr)
        res[tag] = [t.detach().float().cpu() for t in (pv, pa, xv.grad, xa.grad)]
    for k, what in enumerate(("pooled_v", "pooled_a", "d f_v", "d f_a")):
        _rule(_L2(res["fused"][k], res["fp32"][k]), _L2(res["aten"][k], res["fp32"][k]), f"trunk {what}")


def test_front_ends_into_a_two_stage_trunk_at_the_real_geometry():
    """waveform / image -> stage-0 tokens (4096 x 96 / 2304 x 128) -> stage 0 -> merges -> stage 1 (1024 x 192 / 576 x 256), forward and backward"""
    dev = torch.device("cuda:0")
    torch.manual_seed(0)
    B = 2
    fe_a = HTSATFrontEnd(embed_dim=96, out_dtype=torch.bfloat16).to(dev).eval()
    fe_v = PatchEmbed(192, in_chans=3, embed_dim=128, out_dtype=torch.bfloat16).to(dev).eval()
    tr = AVETrunk(ave_stage_shapes("swinv2_base")[:2]).to(dev).train()
    for m in list(tr.vis_merge) + list(tr.aud_merge):
        m.fused = True                                        # the kernels, whatever the default dispatch says of these shapes
    with torch.no_grad():
        for n, p in tr.stack.named_parameters():
            if n.endswith("gate") or n.endswith("gate_av"):
                p.fill_(0.5)
    f_a = fe_a(0.1 * torch.randn(B, 160000, device=dev))
    f_v = fe_v(torch.randn(B, 3, 192, 192, device=dev))
    assert f_a.shape == (B, 4096, 96) and f_v.shape == (B, 2304, 128)
    pv, pa, outs, maps = tr(f_v, f_a)
    assert outs[1][0].shape == (B, 576, 256) and outs[1][1].shape == (B, 1024, 192)
    torch.autograd.backward([pv, pa], [torch.randn_like(pv), torch.randn_like(pa)])
    torch.cuda.synchronize()
    for t in (pv, pa, maps[0], maps[1]) + tuple(t for pr in outs for t in pr):
        assert torch.isfinite(t.float()).all()
    _stage0_grads_ok(tr)
