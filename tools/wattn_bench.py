"""Per-shape timing of the frozen blocks' kernels at the AVE stack's geometries (B = 160 frames, bf16): the fused window attention
(csrc/wattn.hip) forward / backward and the LayerNorm (+ residual) row kernels (dgsct_layer_norm_*), against their algorithmic bytes.
  window attention forward : qkv read once + O written          = B L (3C + C) 2 bytes
  window attention backward: qkv, O, dO read + dqkv written     = B L (3C + C + C + 3C) 2 bytes
  LayerNorm forward (+res) : x (+ residual) read, out written   = rows C (2 | 3) 2 bytes;   backward: dout, x read, dx written = rows C 3 x 2
usage: python tools/wattn_bench.py [swinv2_base|swinv2_large]
       python tools/wattn_bench.py --tables    trainable blocks: the frozen backward against the table-gradient backward
                                               (dgsct_window_attn_backward_tables) and the ATen path, B = 160 and 40"""
import math
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import dgsct_amd  # noqa: E402,F401
from dgsct_amd import ave_stage_shapes, ops  # noqa: E402
from dgsct_amd.backbone import _HTSAT_HEADS, _SWIN_HEADS  # noqa: E402

TABLES = "--tables" in sys.argv
sys.argv = [a for a in sys.argv if a != "--tables"]
backbone = sys.argv[1] if len(sys.argv) > 1 else "swinv2_base"
dev = torch.device("cuda:0")
B = 160


def timed(fn, reps=10):
    for _ in range(3):
        fn()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / reps * 1e3          # us


def aten_attention(qkv, bm, scale, R, ws, shift, heads, cosine):
    """the fused=False formulation of the blocks' attention (roll, window partition, [windows, heads, n, n] logits, reverse), what a trainable
    block had to use before the table-gradient backward"""
    from dgsct_amd.backbone import _from_windows, _to_windows
    B, L, C3 = qkv.shape
    hd, n, nW = C3 // (3 * heads), ws * ws, (R // ws) ** 2
    x = qkv.reshape(B, R, R, C3)
    if shift:
        x = torch.roll(x, (-shift, -shift), (1, 2))
    q, k, v = _to_windows(x, ws).reshape(B * nW, n, 3, heads, hd).permute(2, 0, 3, 1, 4)
    if cosine:
        q, k = torch.nn.functional.normalize(q, dim=-1), torch.nn.functional.normalize(k, dim=-1)
    logits = (q @ k.transpose(-2, -1)) * scale.to(q.dtype)[None, :, None, None]
    logits = (logits.reshape(B, nW, heads, n, n) + bm.to(q.dtype)[None]).reshape(B * nW, heads, n, n)
    o = _from_windows((logits.softmax(-1) @ v).transpose(1, 2).reshape(B * nW, n, heads * hd), ws, R, R)
    if shift:
        o = torch.roll(o, (shift, shift), (1, 2))
    return o.reshape(B, L, heads * hd)


def tables_table():
    """frozen backward vs table-gradient backward, alternating (each timed 10 x after 3 warm-up calls, the pair measured 3 times, best
    kept), and the ATen path fwd + bwd with trainable tables"""
    print(f"{'B':>4} {'block':>8} {'map':>5} {'C':>5} {'ws':>3} {'heads':>5} {'cos':>3} {'shift':>5}   {'bwd frozen':>11} {'bwd+tables':>11} "
          f"{'ratio':>6}   {'ATen fwd+bwd':>13} {'fused fwd+bwd+tab':>18} {'speed-up':>8}")
    for B_ in (160, 40):
        for s in ave_stage_shapes(backbone):
            for kind, N, C, ws0, heads in (("swin-v2", s["Nv"], s["Cv"], 12, _SWIN_HEADS[s["Cv"]]), ("hts-at", s["Na"], s["Ca"], 8, _HTSAT_HEADS[s["Ca"]])):
                R = int(round(math.sqrt(N)))
                ws = min(ws0, R)
                shift = ws // 2 if R > ws else 0
                n, nW = ws * ws, (R // ws) ** 2
                cosine = kind == "swin-v2"
                gen = torch.Generator().manual_seed(1)
                qkv = torch.randn(B_, N, 3 * C, generator=gen).to(dev, torch.bfloat16).requires_grad_(True)
                bm = torch.randn(nW if shift else 1, heads, n, n, generator=gen).to(dev).requires_grad_(True)
                scale = (torch.rand(heads, generator=gen) + 0.5).to(dev).requires_grad_(True)
                dout = torch.randn(B_, N, C, generator=gen).to(dev, torch.bfloat16)
                o_fz = ops.window_attention(qkv, bm.detach(), scale.detach(), R, R, ws, shift, heads, None, cosine)
                o_tb = ops.window_attention(qkv, bm, scale, R, R, ws, shift, heads, None, cosine)
                best = [1e30, 1e30]
                for _ in range(3):
                    best[0] = min(best[0], timed(lambda: torch.autograd.grad(o_fz, qkv, dout, retain_graph=True)))
                    best[1] = min(best[1], timed(lambda: torch.autograd.grad(o_tb, (qkv, bm, scale), dout, retain_graph=True)))

                def aten():
                    o = aten_attention(qkv, bm, scale, R, ws, shift, heads, cosine)
                    torch.autograd.grad(o, (qkv, bm, scale), dout)

                def fused():
                    o = ops.window_attention(qkv, bm, scale, R, R, ws, shift, heads, None, cosine)
                    torch.autograd.grad(o, (qkv, bm, scale), dout)
                t_a = timed(aten, reps=5)
                t_fu = timed(fused)
                print(f"{B_:4d} {kind:>8} {R:3d}^2 {C:5d} {ws:3d} {heads:5d} {int(cosine):3d} {shift:5d}   {best[0]:8.1f} us {best[1]:8.1f} us "
                      f"{best[1] / best[0]:6.2f}   {t_a:10.1f} us {t_fu:15.1f} us {t_a / t_fu:8.1f}", flush=True)
                del qkv, bm, o_fz, o_tb
                torch.cuda.empty_cache()


if TABLES:
    tables_table()
    sys.exit(0)

print(f"{'block':>8} {'map':>5} {'C':>5} {'ws':>3} {'heads':>5} {'cos':>3}   {'wattn fwd':>20}   {'wattn bwd':>20}   {'LN fwd (+res)':>20}   {'LN bwd':>20}")
tot = [0.0] * 4
for s in ave_stage_shapes(backbone):
    for kind, N, C, ws0, heads in (("swin-v2", s["Nv"], s["Cv"], 12, _SWIN_HEADS[s["Cv"]]), ("hts-at", s["Na"], s["Ca"], 8, _HTSAT_HEADS[s["Ca"]])):
        R = int(round(math.sqrt(N)))
        ws = min(ws0, R)
        shift = ws // 2 if (R > ws and os.environ.get("NOSHIFT") is None) else 0        # NOSHIFT=1: the un-shifted blocks (one bias table for all windows)
        n, nW = ws * ws, (R // ws) ** 2
        cosine = kind == "swin-v2"
        gen = torch.Generator().manual_seed(1)
        qkv = torch.randn(B, N, 3 * C, generator=gen).to(dev, torch.bfloat16).requires_grad_(True)
        bm = torch.randn(nW if shift else 1, heads, n, n, generator=gen).to(dev)
        scale = (torch.rand(heads, generator=gen) + 0.5).to(dev)
        dout = torch.randn(B, N, C, generator=gen).to(dev, torch.bfloat16)
        o = ops.window_attention(qkv, bm, scale, R, R, ws, shift, heads, None, cosine)
        t_f = timed(lambda: ops.window_attention(qkv.detach(), bm, scale, R, R, ws, shift, heads, None, cosine))
        t_b = timed(lambda: torch.autograd.grad(o, qkv, dout, retain_graph=True))
        x = torch.randn(B * N, C, generator=gen).to(dev, torch.bfloat16).requires_grad_(True)
        res = torch.randn(B * N, C, generator=gen).to(dev, torch.bfloat16) if cosine else None      # post-norm (Swin-V2): residual fused
        w, b_ = torch.ones(C, device=dev), torch.zeros(C, device=dev)
        y = ops.layer_norm(x, w, b_, 1e-5, res)
        g = torch.randn_like(y)
        t_lf = timed(lambda: ops.layer_norm(x.detach(), w, b_, 1e-5, res))
        t_lb = timed(lambda: torch.autograd.grad(y, x, g, retain_graph=True))
        by = [B * N * 4 * C * 2, B * N * 8 * C * 2, B * N * C * 2 * (3 if cosine else 2), B * N * C * 2 * 3]
        cells = [f"{t:8.1f} us {bb / t / 1e3:6.0f} GB/s" for t, bb in zip((t_f, t_b, t_lf, t_lb), by)]
        print(f"{kind:>8} {R:3d}^2 {C:5d} {ws:3d} {heads:5d} {int(cosine):3d}   " + "   ".join(f"{c:>20}" for c in cells))
        for i, t in enumerate((t_f, t_b, t_lf, t_lb)):
            tot[i] += t * s["layers"] * (1 if i < 2 else 2)           # one attention, two LayerNorms per block
print("per step (24 blocks), ms: wattn fwd %.2f  bwd %.2f   LayerNorm fwd %.2f  bwd %.2f   (HBM roof: 8000 GB/s; backward timings include one autograd node's "
      "host launch)" % tuple(t / 1e3 for t in tot))
