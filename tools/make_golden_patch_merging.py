"""TEST INFRASTRUCTURE: golden vectors of the two patch-merging layers -> tests/golden/ref_patch_merging.pt   (SURVEY.md 8(f) row f4).

Runs where the reference tree and Hugging Face transformers exist:

* ``htsat``: the reference's ``PatchMerging`` (DG-SCT/AVE/nets/htsat.py:259-295), taken from the reference source with ``ast`` as
  oracle/make_golden_backbone.py does (no reference text is stored in this repo);
* ``swinv2``: transformers' ``Swinv2PatchMerging`` -- the INDEPENDENT pin of the Swin-V2 form (``norm(reduction(.))``).  timm==0.6.12's
  ``swin_transformer_v2.PatchMerging`` is what the AVE loop calls; timm is not installed here: parity against timm itself stays unpinned.

Every parameter is perturbed by 0.1 randn (LayerNorm affine starts at 1 / 0) and rounded to a bf16-representable value, so `state` is stored
in bf16 without loss (load_state_dict widens it).  Cases per form: (B, H, W, C) = (3, 6, 4, 32) and
(2, 8, 8, 96); each stores state, x, cot, y, dx (fp32, CPU).  The ATen formulation of dg-sct_amd/merging.py's modules, loaded with the same
state_dict, is asserted <= 1e-5 away on y and dx.  Data only, ~0.7 MB.
usage: python tools/make_golden_patch_merging.py <the reference's DG-SCT/AVE/nets directory>"""
import ast
import importlib
import os
import sys

import torch
import torch.nn as nn

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
REF = sys.argv[1] if len(sys.argv) > 1 else os.environ.get("DGSCT_REFERENCE_NETS", "")
if not os.path.isfile(os.path.join(REF, "htsat.py")):
    sys.exit("make_golden_patch_merging: give the reference's DG-SCT/AVE/nets directory (argument or $DGSCT_REFERENCE_NETS)")
CASES = [(3, 6, 4, 32), (2, 8, 8, 96)]


def extract(path, names):
    src = open(path).read()
    tree = ast.parse(src)
    return "\n\n".join(ast.get_source_segment(src, n) for n in tree.body
                       if isinstance(n, (ast.ClassDef, ast.FunctionDef)) and n.name in names)


def reference_htsat():
    ns = dict(torch=torch, nn=nn)
    exec(extract(os.path.join(REF, "htsat.py"), {"PatchMerging"}), ns)
    cls = ns["PatchMerging"]
    return lambda H, W, C: cls((H, W), C), lambda m, x, H, W: m(x)


def reference_swinv2():
    from transformers.models.swinv2.modeling_swinv2 import Swinv2PatchMerging
    return lambda H, W, C: Swinv2PatchMerging((H, W), C), lambda m, x, H, W: m(x, (H, W))


def main():
    mg = importlib.import_module("dgsct_amd.merging")
    forms = {"htsat": (reference_htsat(), mg.HTSATPatchMerging), "swinv2": (reference_swinv2(), mg.SwinV2PatchMerging)}
    out = {}
    for form, ((make, call), Mine) in forms.items():
        for B, H, W, C in CASES:
            torch.manual_seed(17)
            ref = make(H, W, C).eval()
            with torch.no_grad():
                for p in ref.parameters():
                    p.add_(0.1 * torch.randn_like(p))
                    p.copy_(p.bfloat16().float())                 # bf16-representable: the fixture stores the state in bf16 (half the file), exactly
            mine = Mine((H, W), C, fused=False).eval()
            sd = {k: v.clone() for k, v in ref.state_dict().items()}
            assert set(sd) == set(mine.state_dict()), sorted(set(sd) ^ set(mine.state_dict()))
            mine.load_state_dict(sd)
            g = torch.Generator().manual_seed(5)
            x = torch.randn(B, H * W, C, generator=g, requires_grad=True)
            cot = torch.randn(B, (H // 2) * (W // 2), 2 * C, generator=g)
            y = call(ref, x, H, W)
            y.backward(cot)
            x2 = x.detach().clone().requires_grad_(True)
            y2 = mine(x2)
            y2.backward(cot)
            err = max((y - y2).abs().max().item(), (x.grad - x2.grad).abs().max().item())
            assert err <= 1e-5, (form, (B, H, W, C), err)
            # the gather order, restated: view(B, H/2, 2, W/2, 2, C).permute(0, 1, 3, 4, 2, 5)
            v = x.detach().view(B, H // 2, 2, W // 2, 2, C).permute(0, 1, 3, 4, 2, 5).reshape(B, -1, 4 * C)
            assert torch.equal(v, mg.gather_2x2(x.detach(), H, W))
            out[f"{form}-{B}x{H}x{W}x{C}"] = dict(form=form, shape=(B, H, W, C), state={k: v.bfloat16() for k, v in sd.items()}, x=x.detach().clone(), cot=cot, y=y.detach().clone(),
                                                  dx=x.grad.clone())
            print(form, (B, H, W, C), "max |reference - restatement|", err)
    path = os.path.join(ROOT, "tests", "golden", "ref_patch_merging.pt")
    torch.save(out, path)
    print("wrote", path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
