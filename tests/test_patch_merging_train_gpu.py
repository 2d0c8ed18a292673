"""GPU: the parameter gradients of the patch-merging kernels (csrc/pmerge.hip: pm_lnbwd_sums_k, pm_wgrad_k behind
dgsct_patch_merge_backward_params), `weight_grads=True` on the merge modules and `merge_weight_grads=True` on AVETrunk.

The accuracy criterion is the one of tests/test_patch_merging_gpu.py (`_rule`): against the fp32 evaluation of the SAME module the fused
path may be no further off than 1.5 x the bf16 ATen formulation is, + 2e-3, in relative L2 -- here for y, dx, dW, d ln_w and d ln_b.  The
exact-data test needs no tolerance: small integers as data, a 0/1 selection matrix as W and mu = 0, rstd = 1, ln_w = 1, ln_b = 0 make
every product and every sum exact (all below 2^24), so gather addressing, slab split and tile edges are compared bit for bit against
index arithmetic."""
import copy

import pytest
import torch
import torch.nn.functional as F

import dgsct_amd  # noqa: F401
from dgsct_amd import AVETrunk, merging
from dgsct_amd._lib import PMERGE_NORM_FIRST, PMERGE_NORM_LAST, default_lib
from dgsct_amd.train import make_optimizer

from test_patch_merging_gpu import FORMS, _L2, _STAGES, _ramp, _rule, _selection, _token_and_offset, _zero_mean_ints

pytestmark = pytest.mark.gpu
_NAMES = ("y", "dx", "dW", "d ln_w", "d ln_b")
# ragged row blocks, one-row frames, 4C no power of two, the 1- / 2- / 3-chunk row kernels; 45 rows = a ragged 64-row step; 512 rows =
# several row slabs adding into one tile of dW.  _LONG: 2700 rows = 43 steps of 64 rows, the last one ragged (12 rows) -> 2 steps per slab
# (the split stops at 40 slabs), 22 slabs, the last slab a single short step: the weight-gradient kernel's row loop runs twice (its
# accumulators carried, both LDS images re-staged behind the barrier), as it does at every training batch; C = 96 adds the ragged
# output tile (2C = 192).  85 workgroups of the column-sum kernel leave 85 partials, which part_reduce splits 7 ways.
_COMMON = [(3, 6, 4, 32), (1, 2, 2, 96), (2, 4, 8, 96), (5, 6, 6, 128), (2, 4, 4, 192), (1, 4, 4, 384), (8, 16, 16, 32)]
_LONG = [(3, 60, 60, 32), (3, 60, 60, 96)]
_SWEEP = ([("htsat", c) for c in _COMMON + _LONG] + [("swinv2", c) for c in _COMMON + _LONG] + [("swinv2", (1, 4, 4, 768))])


def _run(m, x, cot, dev, param_dtype, map_dtype):
    """forward + backward of a copy of m: (y, dx, dW, d ln_w, d ln_b) in fp32 on the CPU, and the dtypes of the three parameter gradients"""
    m = copy.deepcopy(m).to(dev, param_dtype)
    xi = x.clone().to(dev, map_dtype).requires_grad_(True)
    y = m(xi)
    y.backward(cot.to(dev, map_dtype))
    torch.cuda.synchronize()
    gs = (m.reduction.weight.grad, m.norm.weight.grad, m.norm.bias.grad)
    return [t.detach().float().cpu() for t in (y, xi.grad) + gs], [g.dtype for g in gs], y.grad_fn


@pytest.mark.parametrize("form,shape", _SWEEP, ids=[f"{f}-{'x'.join(map(str, s))}" for f, s in _SWEEP])
def test_trainable_fused_merge_against_fp32_on_the_same_module(form, shape):
    B, H, W, C = shape
    dev = torch.device("cuda:0")
    torch.manual_seed(7)
    ref = FORMS[form]((H, W), C, fused=False).eval()
    with torch.no_grad():
        for p in ref.parameters():
            p.add_(0.1 * torch.randn_like(p))
    fused = FORMS[form]((H, W), C, fused=True, weight_grads=True).eval()
    fused.load_state_dict(ref.state_dict())
    x = torch.randn(B, H * W, C).bfloat16()
    cot = torch.randn(B, (H // 2) * (W // 2), 2 * C).bfloat16()
    fp32, _, _ = _run(ref, x, cot, dev, torch.float32, torch.float32)
    aten, _, _ = _run(ref, x, cot, dev, torch.bfloat16, torch.bfloat16)
    got, dtypes, fn = _run(fused, x, cot, dev, torch.float32, torch.bfloat16)          # fp32 masters, a bf16 map
    assert "PatchMergeTrainFn" in type(fn).__name__
    assert dtypes == [torch.float32] * 3
    for k, what in enumerate(_NAMES):
        _rule(_L2(got[k], fp32[k]), _L2(aten[k], fp32[k]), f"{form} {shape} {what}")


def _functional(mode, B, H, W, C, x, w, lw, lb, cot, dtype):
    """the merge written out in ATen on the tensors of a raw library call: (y, dx, dW, d ln_w, d ln_b) in fp32 on the CPU"""
    x, w, lw, lb = (t.detach().to(dtype).requires_grad_(True) for t in (x, w, lw, lb))
    g = merging.gather_2x2(x, H, W)
    y = F.linear(F.layer_norm(g, (4 * C,), lw, lb, 1e-5), w) if mode == PMERGE_NORM_FIRST else F.layer_norm(F.linear(g, w), (2 * C,), lw, lb, 1e-5)
    y.backward(cot.to(dtype))
    return [t.detach().float().cpu() for t in (y, x.grad, w.grad, lw.grad, lb.grad)]


def _raw_case(mode, shape, seed=1):
    B, H, W, C = shape
    dev = torch.device("cuda:0")
    lib = default_lib()
    torch.manual_seed(seed)
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
    return dict(lib=lib, x=x, w=w, lw=lw, lb=lb, out=out, pre=pre, mu=mu, rstd=rstd, dout=dout, st=st, cn=cn)


def _backward_params(mode, shape, c, fill=float("nan")):
    B, H, W, C = shape
    dev, lib = c["x"].device, c["lib"]
    dx = torch.full_like(c["x"], float("nan"))
    dw = torch.full((2 * C, 4 * C), fill, device=dev)
    dlw, dlb = torch.full((c["cn"],), fill, device=dev), torch.full((c["cn"],), fill, device=dev)
    ws = torch.empty(lib.patch_merge_params_ws_bytes(mode, B, H, W, C), dtype=torch.uint8, device=dev)
    lib.patch_merge_backward_params(mode, B, H, W, C, c["dout"].data_ptr(), c["x"].data_ptr(), c["w"].data_ptr(), c["lw"].data_ptr(), c["lb"].data_ptr(),
                                    c["pre"].data_ptr() if mode == PMERGE_NORM_LAST else None, c["mu"].data_ptr(), c["rstd"].data_ptr(), 1e-5,
                                    dx.data_ptr(), dw.data_ptr(), dlw.data_ptr(), dlb.data_ptr(), ws.data_ptr(), c["st"])
    torch.cuda.synchronize()
    return dx, dw, dlw, dlb


_RAW = [(m, s) for m in (PMERGE_NORM_FIRST, PMERGE_NORM_LAST) for s in ((5, 6, 6, 128), (2, 4, 4, 192))]
# every instantiation of the row kernel, which the bit-identity rests on: 1 / 2 / 3 chunks of 512 channels per row in both modes
# (NORM_FIRST 4C = 512, 768, 1536; NORM_LAST 2C = 256, 384 above, 768 and 1536 here), and the multi-step shape
_RAW_DX = _RAW + [(PMERGE_NORM_FIRST, (1, 4, 4, 384)), (PMERGE_NORM_LAST, (2, 4, 4, 384)), (PMERGE_NORM_LAST, (1, 4, 4, 768)),
                  (PMERGE_NORM_FIRST, _LONG[1]), (PMERGE_NORM_LAST, _LONG[1])]


@pytest.mark.parametrize("mode,shape", _RAW_DX, ids=lambda v: str(v).replace(", ", "x"))
def test_dx_is_bit_identical_to_the_frozen_backward(mode, shape):
    B, H, W, C = shape
    c = _raw_case(mode, shape)
    lib = c["lib"]
    dx0 = torch.full_like(c["x"], float("nan"))
    ws = torch.empty(lib.patch_merge_ws_bytes(mode, B, H, W, C), dtype=torch.uint8, device=dx0.device)
    lib.patch_merge_backward(mode, B, H, W, C, c["dout"].data_ptr(), c["x"].data_ptr(), c["w"].data_ptr(), c["lw"].data_ptr(),
                             c["pre"].data_ptr() if mode == PMERGE_NORM_LAST else None, c["mu"].data_ptr(), c["rstd"].data_ptr(), 1e-5,
                             dx0.data_ptr(), ws.data_ptr(), c["st"])
    dx1 = _backward_params(mode, shape, c)[0]
    assert not torch.isnan(dx0.float()).any()
    assert torch.equal(dx0, dx1)


@pytest.mark.parametrize("mode,shape", _RAW, ids=lambda v: str(v).replace(", ", "x"))
def test_the_call_zeroes_its_gradient_buffers(mode, shape):
    """dw / dln_w / dln_b handed over full of NaN come back finite and inside the rule (dW is summed with atomics, so two calls may differ
    in its last bits: no bit-equality between runs is asked for)"""
    B, H, W, C = shape
    c = _raw_case(mode, shape)
    got = _backward_params(mode, shape, c)
    for t in got:
        assert torch.isfinite(t.float()).all()
    args = (mode, B, H, W, C, c["x"], c["w"], c["lw"], c["lb"], c["dout"])
    fp32, aten = _functional(*args, torch.float32), _functional(*args, torch.bfloat16)
    for k in (1, 2, 3, 4):
        _rule(_L2(got[k - 1], fp32[k]), _L2(aten[k], fp32[k]), f"mode {mode} {shape} {_NAMES[k]}")


def _exact_on_integer_data(shape):
    B, H, W, C = shape
    dev = torch.device("cuda:0")
    H2, W2, rows = H // 2, W // 2, B * (H // 2) * (W // 2)
    x = _ramp(B, H, W, C)
    w, sel = _selection(C)
    dh, dw_, ch = _token_and_offset(H, W, C)
    b_, i_, j_, k_ = torch.meshgrid(torch.arange(B), torch.arange(H2), torch.arange(W2), torch.arange(4 * C), indexing="ij")
    xg = x[b_, 2 * i_ + dh[k_], 2 * j_ + dw_[k_], ch[k_]].reshape(rows, 4 * C)          # the virtual rows, by index arithmetic
    dout = _zero_mean_ints(rows, 2 * C)
    g = dout @ w
    want_dw = dout.t() @ xg
    assert float(want_dw.abs().max()) < 2 ** 24 and float((g * xg).sum(0).abs().max()) < 2 ** 24
    for mode in (PMERGE_NORM_FIRST, PMERGE_NORM_LAST):
        cn = 4 * C if mode == PMERGE_NORM_FIRST else 2 * C
        c = dict(lib=default_lib(), x=x.reshape(B, H * W, C).to(dev, torch.bfloat16).contiguous(), w=w.to(dev, torch.bfloat16).contiguous(),
                 lw=torch.ones(cn, device=dev), lb=torch.zeros(cn, device=dev), pre=torch.zeros(B, H2 * W2, 2 * C, device=dev, dtype=torch.bfloat16),
                 mu=torch.zeros(rows, device=dev), rstd=torch.ones(rows, device=dev), dout=dout.reshape(B, H2 * W2, 2 * C).to(dev, torch.bfloat16).contiguous(),
                 st=torch.cuda.current_stream().cuda_stream, cn=cn)
        _, dw, dlw, dlb = _backward_params(mode, shape, c)
        assert torch.equal(dw.cpu(), want_dw), mode
        if mode == PMERGE_NORM_FIRST:                          # A = x exactly; x^ = x
            assert torch.equal(dlw.cpu(), (g * xg).sum(0))
            assert torch.equal(dlb.cpu(), g.sum(0))
        else:                                                  # zero `pre`: x^ = 0 and zero-mean rows make dpre = dout
            assert torch.equal(dlw.cpu(), torch.zeros(2 * C))
            assert torch.equal(dlb.cpu(), dout.sum(0))


@pytest.mark.parametrize("shape", [(2, 4, 6, 32), (3, 6, 10, 96), (8, 16, 16, 32)], ids=lambda s: "x".join(map(str, s)))
def test_parameter_gradients_are_exact_on_integer_data(shape):
    """|dout| <= 8, |x| <= 125, at most 512 rows: every sum stays below 2^24, so fp32 accumulation in any order is exact.  The last shape
    has 512 rows = 8 steps of 64 rows = 8 row slabs (one step each) adding into every tile of dW; (3,6,10,96) has 45 rows (one ragged
    step) and a ragged output tile (2C = 192 = 128 + 64)."""
    B, H, W, C = shape
    assert B * (H // 2) * (W // 2) <= 512
    _exact_on_integer_data(shape)


@pytest.mark.parametrize("shape", _LONG, ids=lambda s: "x".join(map(str, s)))
def test_parameter_gradients_are_exact_across_several_steps_of_a_slab(shape):
    """The same at 2700 rows (8 x 125 x 2700 = 2.7e6 < 2^24, asserted on the data): 43 steps of 64 rows in 22 slabs of 2 steps, the last
    slab one step of 12 rows.  A stale or half-staged LDS image in the second step, a lost accumulator or a wrong end of the last slab
    changes an integer, with no tolerance to hide in."""
    _exact_on_integer_data(shape)


def test_dispatch_of_a_trainable_merge():
    dev = torch.device("cuda:0")
    x = torch.randn(1, 16, 32, device=dev, dtype=torch.bfloat16, requires_grad=True)
    for cls in FORMS.values():
        m = cls((4, 4), 32, fused=True, weight_grads=True).to(dev)
        assert "PatchMergeTrainFn" in type(m(x).grad_fn).__name__
        m.weight_grads = False
        with pytest.raises(RuntimeError, match="requires grad"):
            m(x)
        m.weight_grads, m.fused = True, None
        listed = (m._MODE, 16, 32) in merging._KERNELS_FASTER_TRAIN
        assert ("PatchMerge" in type(m(x).grad_fn).__name__) == listed          # fused=None: by the table
        m.fused = False
        assert "PatchMerge" not in type(m(x).grad_fn).__name__
        # every listed shape takes the kernels under fused=None, a shape outside the table does not
        for mode, tokens, dim in merging._KERNELS_FASTER_TRAIN:
            if mode != m._MODE:
                continue
            side = int(round(tokens ** 0.5))
            mm = cls((side, side), dim, weight_grads=True).to(dev)
            xx = torch.randn(1, tokens, dim, device=dev, dtype=torch.bfloat16, requires_grad=True)
            assert "PatchMergeTrainFn" in type(mm(xx).grad_fn).__name__
        # frozen: the keyword changes nothing
        for wg in (False, True):
            f = cls((4, 4), 32, weight_grads=wg).to(dev, torch.bfloat16).requires_grad_(False)
            assert ("PatchMergeFn" in type(f(x).grad_fn).__name__) == ((f._MODE, 16, 32) in merging._KERNELS_FASTER)
            f.fused = True
            assert type(f(x).grad_fn).__name__.startswith("_PatchMergeFn")


def test_trunk_trains_the_audio_merges_through_the_kernels():
    dev = torch.device("cuda:0")
    BT = 4

    def make(dtype, **kw):
        torch.manual_seed(0)
        tr = AVETrunk(_STAGES, dtype=dtype, train_htsat=True, **kw)
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
    for tag, dtype, kw in (("fp32", torch.float32, {}), ("aten", torch.bfloat16, {}), ("fused", torch.bfloat16, dict(merge_weight_grads=True))):
        tr = make(dtype, **kw).to(dev).train()
        for m in tr.aud_merge:
            assert m.reduction.weight.dtype == torch.float32 and m.reduction.weight.requires_grad          # fp32 masters in every run
            m.fused = True if tag == "fused" else False       # (True raises instead of falling back)
        opt, _ = make_optimizer(tr, lr=1e-3, task="avs_s4")
        before = tr.aud_merge[0].reduction.weight.detach().clone()
        pv, pa, outs, maps = tr(f_v.clone().to(dev, dtype), f_a.clone().to(dev, dtype))
        torch.autograd.backward([pv, pa], [cv.to(dev, dtype), ca.to(dev, dtype)])
        torch.cuda.synchronize()
        m0 = tr.aud_merge[0]
        grads = [m0.reduction.weight.grad, m0.norm.weight.grad, m0.norm.bias.grad]
        for gr in grads:
            assert gr is not None and gr.dtype == torch.float32 and torch.isfinite(gr).all() and float(gr.abs().sum()) > 0
        res[tag] = [t.detach().float().cpu() for t in grads]
        if tag == "fused":
            opt.step()
            assert not torch.equal(before, tr.aud_merge[0].reduction.weight.detach())
    for k, what in enumerate(("dW", "d ln_w", "d ln_b")):
        _rule(_L2(res["fused"][k], res["fp32"][k]), _L2(res["aten"][k], res["fp32"][k]), f"trunk aud_merge[0] {what}")
