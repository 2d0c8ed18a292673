"""TEST INFRASTRUCTURE: parameter gradients of the backbone blocks, for training them (AVS-S4 trains the HTS-AT blocks:
DG-SCT/AVS/avs_scripts/avs_s4/train.py:145-163) -> tests/golden/htsat_block_grads.pt (HTS-AT) and
tests/golden/swinv2_block_grads.pt (Swin-V2).  Two files: together they would exceed the 1 MiB limit of a committed file.

* HTS-AT: ``WindowAttention`` / ``SwinTransformerBlock`` of ``avs_s4/model/htsat.py`` (the AVS-S4 copy, identical to the AVE one) and
  the helpers they need from ``avs_s4/model/layers.py``, taken with ``ast`` as oracle/make_golden_backbone.py does (its ``extract`` is
  reused; no reference text is stored), run in fp32 on the CPU: state, input, cotangent, output, input gradient and the gradient of
  EVERY parameter (``relative_position_bias_table`` included).  Cases: the three geometries of htsat_block.pt and one shifted case at
  HTS-AT's head width 24 (dim 48, 2 heads, MLP ratio 2; dim 96 / 4 heads / ratio 4 would not fit the file limit).
* Swin-V2: Hugging Face ``Swinv2Layer`` with its parameters renamed to timm's layout (oracle/make_golden_swinv2.py's route), fp32 and
  float64: the gradients of every parameter under timm names (``attn.cpb_mlp.*``, ``attn.logit_scale``, ``attn.q_bias``, ...).
* Asserted here: dg-sct_amd/backbone.py's ATen path (``fused=False``) reproduces the reference's parameter gradients in fp32 to 1e-5
  (HTS-AT: absolute; Swin-V2: relative to each gradient's largest element, and no further from the float64 result than 2 x HF's fp32).
Run where the reference tree exists:  python tools/make_golden_block_grads.py
"""
import importlib.util
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
REF_AVS = "/root/reference/DG-SCT/AVS/avs_scripts/avs_s4/model"

# name: (dim, map side, heads, window, shift, batch, mlp ratio)
HTSAT_CASES = {"plain": (32, 16, 4, 8, 0, 1, 4.0), "shifted": (32, 16, 4, 8, 4, 1, 4.0), "one_window": (32, 8, 4, 8, 4, 1, 4.0),
               "hw24_shifted": (48, 16, 2, 8, 4, 1, 2.0)}
SWIN_CASES = {"shifted": (32, 24, 2, 12, 6, 1), "small_plain": (32, 16, 4, 8, 0, 1)}


def _backbone():
    spec = importlib.util.spec_from_file_location("_bb", os.path.join(ROOT, "dg-sct_amd", "backbone.py"))
    bb = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(bb)
    return bb


def reference_htsat_block():
    import collections.abc
    import math
    import warnings
    from itertools import repeat
    import torch.nn as nn
    from oracle.make_golden_backbone import extract
    ns = dict(torch=torch, nn=nn, math=math, warnings=warnings, repeat=repeat, collections=collections)
    exec(extract(os.path.join(REF_AVS, "layers.py"), {"_ntuple", "drop_path", "DropPath", "Mlp", "_no_grad_trunc_normal_", "trunc_normal_"}), ns)
    ns["to_2tuple"] = ns["_ntuple"](2)
    exec(extract(os.path.join(REF_AVS, "htsat.py"), {"window_partition", "window_reverse", "WindowAttention", "SwinTransformerBlock"}), ns)
    return ns["SwinTransformerBlock"]


def _grads(named):
    return {k: p.grad.detach().clone() for k, p in named}


def htsat_cases(bb):
    Ref = reference_htsat_block()
    cases = {}
    for name, (dim, res, heads, ws, shift, B, mr) in HTSAT_CASES.items():
        torch.manual_seed(13)
        ref = Ref(dim, (res, res), heads, window_size=ws, shift_size=shift, mlp_ratio=mr).eval()
        with torch.no_grad():                                   # every parameter matters (biases / LayerNorm affine start at 0 / 1; a
            for n_, p in ref.named_parameters():                # trunc_normal(0.02) bias table would be invisible)
                p.add_((0.5 if "bias_table" in n_ else 0.1) * torch.randn_like(p))
        # the geometry-derived buffers (pair index, shift mask) are rebuilt by the constructor: not stored (load with strict=False)
        sd = {k: v.detach().clone() for k, v in ref.state_dict().items() if k.split(".")[-1] not in ("relative_position_index", "attn_mask")}
        g = torch.Generator().manual_seed(7)
        x = torch.randn(B, res * res, dim, generator=g)
        cot = torch.randn(B, res * res, dim, generator=g)
        xr = x.clone().requires_grad_(True)
        y, _ = ref(xr)
        y.backward(cot)
        gref = _grads(ref.named_parameters())
        mine = bb.HTSATBlock(dim, (res, res), heads, window_size=ws, shift_size=shift, mlp_ratio=mr, fused=False).eval()
        r_ = mine.load_state_dict(sd, strict=False)
        assert set(r_.missing_keys) <= {"attn_mask", "attn.relative_position_index"} and not r_.unexpected_keys, r_
        xm = x.clone().requires_grad_(True)
        ym, _ = mine(xm)
        ym.backward(cot)
        gm = _grads(mine.named_parameters())
        assert gm.keys() == gref.keys(), sorted(set(gm) ^ set(gref))
        err = max([(ym - y).abs().max().item(), (xm.grad - xr.grad).abs().max().item()] + [(gm[k] - gref[k]).abs().max().item() for k in gm])
        print(f"HTS-AT {name:13s} dim {dim} heads {heads} map {res}^2 window {ws} shift {shift}: max |aten - reference| over y, dx, "
              f"{len(gm)} parameter gradients = {err:.2e}")
        assert err < 1e-5, (name, err)
        cases[name] = dict(cfg=(dim, res, heads, ws, shift), mlp_ratio=mr, state=sd, x=x, cot=cot, y=y.detach(), dx=xr.grad.detach(),
                           grads=gref)
    return cases


def swin_cases(bb):
    from transformers import Swinv2Config
    from transformers.models.swinv2.modeling_swinv2 import Swinv2Layer
    from oracle.make_golden_swinv2 import to_timm_names

    def timm_grads(ref):
        return to_timm_names({k: p.grad for k, p in ref.named_parameters()})

    cases = {}
    for name, (dim, res, heads, ws, shift, B) in SWIN_CASES.items():
        torch.manual_seed(23)
        cfg = Swinv2Config(embed_dim=dim, depths=[1], num_heads=[heads], window_size=ws, mlp_ratio=4.0, hidden_dropout_prob=0.0,
                           attention_probs_dropout_prob=0.0, drop_path_rate=0.0, hidden_act="gelu", layer_norm_eps=1e-5)
        ref = Swinv2Layer(cfg, dim=dim, input_resolution=(res, res), num_heads=heads, shift_size=shift).eval()
        with torch.no_grad():
            for p in ref.parameters():
                p.add_(0.1 * torch.randn_like(p))
        sd = to_timm_names(ref.state_dict())
        g = torch.Generator().manual_seed(9)
        x = torch.randn(B, res * res, dim, generator=g)
        cot = torch.randn(B, res * res, dim, generator=g)
        res_ = {}
        for dt in (torch.float32, torch.float64):
            r = ref.to(dt)
            for p in r.parameters():
                p.grad = None
            xr = x.detach().to(dt).clone().requires_grad_(True)
            yr = r(xr, (res, res))[0]
            yr.backward(cot.to(dt))
            res_[dt] = (yr.detach(), xr.grad.detach(), timm_grads(r))
        ref = ref.float()
        mine = bb.SwinV2Block(dim, (res, res), heads, window_size=ws, shift_size=shift, fused=False).eval()
        r_ = mine.load_timm_state_dict(sd, strict=False)
        assert set(r_.missing_keys) <= {"attn_mask", "attn.relative_coords_table", "attn.relative_position_index"} and not r_.unexpected_keys
        xm = x.clone().requires_grad_(True)
        ym = mine(xm)
        ym.backward(cot)
        gm = _grads(mine.named_parameters())
        g32, g64 = res_[torch.float32][2], res_[torch.float64][2]
        assert gm.keys() == g32.keys(), sorted(set(gm) ^ set(g32))
        # fp32 rounding alone puts these sums ~1e-4 from exact (HF's own fp32 result against its float64 one), so the pin is relative and
        # anchored in float64, as tests/test_backbone.py does for dx: |aten - f64| <= 2 x |HF fp32 - f64| + 1e-5 max|g| per parameter
        rel = max(((gm[k] - g32[k]).abs().max() / g64[k].abs().max()).item() for k in gm)
        for k in gm:
            e_m, e_hf = (gm[k].double() - g64[k]).abs().max().item(), (g32[k].double() - g64[k]).abs().max().item()
            assert e_m <= 2 * e_hf + 1e-5 * g64[k].abs().max().item(), (name, k, e_m, e_hf)
        print(f"Swin-V2 {name:12s} dim {dim} heads {heads} map {res}^2 window {ws} shift {shift}: max |aten - HF| / max|g| over {len(gm)} "
              f"parameter gradients = {rel:.2e}")
        assert rel < 1e-5, (name, rel)
        cases[name] = dict(cfg=(dim, res, heads, ws, shift), state=sd, x=x, cot=cot, y=res_[torch.float32][0], dx=res_[torch.float32][1],
                           grads=g32, grads_f64=g64)
    return cases


def main():
    bb = _backbone()
    for fname, cases in (("htsat_block_grads.pt", htsat_cases(bb)), ("swinv2_block_grads.pt", swin_cases(bb))):
        path = os.path.join(ROOT, "tests", "golden", fname)
        torch.save(cases, path)
        print("wrote", path, os.path.getsize(path), "bytes")
        assert os.path.getsize(path) < 1 << 20


if __name__ == "__main__":
    main()
