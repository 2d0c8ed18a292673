"""TEST INFRASTRUCTURE: golden vectors of the CMBS event head -> tests/golden/ref_cmbs.pt   (SURVEY.md row 6).

Runs where the reference tree exists.  The reference's ``CMBS``, ``AudioVideoInter`` and ``SupvLocalizeModule``
(DG-SCT/AVE/nets/net_trans.py:254-292, :165-179, :116-138) are taken from the reference source with ``ast`` as
tools/make_golden_patch_merging.py does, with ``torch.nn.MultiheadAttention`` in the namespace (no reference text is stored in this
repo).  The module is built under ``torch.manual_seed(SEED)``, the inputs ``v``, ``a`` [T = 10, B = 3, 256] and the three cotangents are
``randn`` of a generator seeded 1; forward, then one backward of all three outputs.

Stored (fp32, CPU; data only, ~0.2 MB): ``seed``; ``keys`` (the 24 state_dict keys in order); ``state`` -- the EIGHT LIVE tensors in full;
``sha256`` -- the digest of every one of the 24 tensors' bytes (the 16 dead ones, 0.53 M parameters = 2.1 MB in fp32, would not fit a
committed file: a seeded construction is compared against their digests instead); ``v``, ``a``; ``cot_is``, ``cot_ev``, ``cot_av``; ``is_event``,
``event``, ``av``; ``d_v``, ``d_a``; ``grads`` (the eight live parameter gradients); ``no_grad`` (the parameters whose ``grad is None``);
``margins`` (top-4 / arg-max tie margins of the inputs).

Asserted before writing: the seeded construction of dg-sct_amd's ``CMBS`` reproduces every reference parameter bit for bit; its
``fused=False`` formulation is <= 1e-5 from the reference on outputs and input gradients; exactly the 16 dead parameters have no
gradient; the tie margins of the stored inputs -- min over (modality, b, k) of (4th - 5th largest score over t) and min over (b, d) of
(largest - second largest of f over t) -- are >= 1e-4, so no comparison against this fixture hinges on how a tie is broken.
(The file name carries the ``ref_`` prefix of the reference-generated fixtures: tests/helpers.golden_names() takes every other ``*.pt`` of
the directory for a single-adapter case.)
usage: python tools/make_golden_cmbs.py <the reference's DG-SCT/AVE/nets directory>"""
import ast
import hashlib
import importlib
import os
import sys

import torch
import torch.nn as nn
from torch.nn import MultiheadAttention

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
SEED, GEN_SEED, T, B = 3, 1, 10, 3
LIVE = ("localize_module.classifier.weight", "localize_module.classifier.bias", "localize_module.event_classifier.weight",
        "localize_module.event_classifier.bias", "audio_cas.weight", "audio_cas.bias", "video_cas.weight", "video_cas.bias")


def extract(path, names):
    src = open(path).read()
    tree = ast.parse(src)
    return "\n\n".join(ast.get_source_segment(src, n) for n in tree.body
                       if isinstance(n, (ast.ClassDef, ast.FunctionDef)) and n.name in names)


def digest(t: torch.Tensor) -> str:
    return hashlib.sha256(t.detach().contiguous().numpy().tobytes()).hexdigest()


def tie_margins(cas_v: torch.Tensor, cas_a: torch.Tensor, f: torch.Tensor):
    """cas_* [T, B, K], f [T, B, D] -> (min 4th - 5th largest over t, min largest - second largest of f over t); T = 4: no 5th, inf"""
    top = float("inf")
    for c in (cas_v, cas_a):
        s = c.sort(dim=0, descending=True)[0]
        if s.shape[0] > 4:
            top = min(top, (s[3] - s[4]).min().item())
    s = f.sort(dim=0, descending=True)[0]
    return top, (s[0] - s[1]).min().item()


def main():
    ref_dir = sys.argv[1] if len(sys.argv) > 1 else os.environ.get("DGSCT_REFERENCE_NETS", "")
    if not os.path.isfile(os.path.join(ref_dir, "net_trans.py")):
        sys.exit("make_golden_cmbs: give the reference's DG-SCT/AVE/nets directory (argument or $DGSCT_REFERENCE_NETS)")
    ns = dict(torch=torch, nn=nn, MultiheadAttention=MultiheadAttention)
    exec(extract(os.path.join(ref_dir, "net_trans.py"), {"CMBS", "AudioVideoInter", "SupvLocalizeModule"}), ns)
    cm = importlib.import_module("dgsct_amd.cmbs")

    torch.manual_seed(SEED)
    ref = ns["CMBS"](None).eval()
    torch.manual_seed(SEED)
    mine = cm.CMBS(None, fused=False).eval()
    sd, sd2 = ref.state_dict(), mine.state_dict()
    assert list(sd) == list(sd2), (list(sd), list(sd2))
    assert len(sd) == 24
    for k in sd:
        assert torch.equal(sd[k], sd2[k]), k

    g = torch.Generator().manual_seed(GEN_SEED)
    v = torch.randn(T, B, 256, generator=g)
    a = torch.randn(T, B, 256, generator=g)
    cots = [torch.randn(T, B, 1, generator=g), torch.randn(B, 28, generator=g), torch.randn(B, 28, generator=g)]

    def run(m):
        m.zero_grad(set_to_none=True)
        vv, aa = v.clone().requires_grad_(True), a.clone().requires_grad_(True)
        outs = m(vv, aa)
        torch.autograd.backward(list(outs), cots)
        return [o.detach().clone() for o in outs], vv.grad.clone(), aa.grad.clone()

    outs, d_v, d_a = run(ref)
    outs2, d_v2, d_a2 = run(mine)
    err = max(max((x - y).abs().max().item() for x, y in zip(outs, outs2)), (d_v - d_v2).abs().max().item(), (d_a - d_a2).abs().max().item())
    assert err <= 1e-5, err
    no_grad = [n for n, p in ref.named_parameters() if p.grad is None]
    assert sorted(no_grad) == sorted(k for k in sd if k not in LIVE) and len(no_grad) == 16, no_grad
    assert [n for n, p in mine.named_parameters() if p.grad is None] == no_grad
    grads = {n: p.grad.clone() for n, p in ref.named_parameters() if p.grad is not None}
    assert sorted(grads) == sorted(LIVE)

    with torch.no_grad():
        margins = tie_margins(ref.video_cas(v), ref.audio_cas(a), (v + a) / 2)
    assert margins[0] >= 1e-4 and margins[1] >= 1e-4, margins

    out = dict(seed=SEED, keys=list(sd), state={k: sd[k].clone() for k in LIVE}, sha256={k: digest(t) for k, t in sd.items()},
               v=v, a=a, cot_is=cots[0], cot_ev=cots[1], cot_av=cots[2], is_event=outs[0], event=outs[1], av=outs[2], d_v=d_v, d_a=d_a,
               grads=grads, no_grad=no_grad, margins=margins)
    path = os.path.join(ROOT, "tests", "golden", "ref_cmbs.pt")
    torch.save(out, path)
    print("max |reference - restatement|", err, "tie margins", margins)
    print("wrote", path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
