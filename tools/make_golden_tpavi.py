"""TEST INFRASTRUCTURE: golden vectors of the audio-visual TPAVI block -> tests/golden/ref_tpavi.pt, ref_tpavi_eval.pt.

Runs where the reference tree exists.  The reference's ``TPAVIModule`` is loaded from the file given on the command line
(DG-SCT/AVS/avs_scripts/avs_s4/model/TPAVI.py; it imports only torch) with importlib; no reference text is stored in this repo.  The
module is built at C = 64 under ``torch.manual_seed(SEED)``; what the constructor leaves at or near zero (the BatchNorm and LayerNorm
affine, the five biases) is set by ``tpavi_ref.set_nontrivial(state, SEED + 1)`` -- at the constructor's zeros z = LayerNorm(x) and nothing
would be tested.  ``x`` [2, 64, 5, 7, 7], ``audio`` [2, 5, 128] and the two cotangents are ``randn`` of a generator seeded GEN_SEED.  The
reference runs in float64, one forward and one backward of both outputs, in train mode and in eval mode.

Stored (data only; ref_tpavi.pt, 1.0 MB, holds everything but the ``eval`` record, ref_tpavi_eval.pt, 0.7 MB, holds that: together they
would pass the 1 MiB limit for a committed file): ``seed``, ``gen_seed``; ``keys`` (the 17 state_dict keys in order); ``state`` (fp32, after set_nontrivial);
``x``, ``audio``, ``cot_z``, ``cot_a`` (fp32); and per mode (``train`` / ``eval``) in float64: ``z``, ``audio_temp``, ``dx``, ``daudio``,
``grads`` (all 14 parameters), ``running_mean``, ``running_var``, ``num_batches_tracked`` after the call.

Asserted before writing: the seeded construction of dg-sct_amd's ``TPAVIModule`` reproduces every reference parameter bit for bit (keys,
order, values); tests/tpavi_ref.py is <= 1e-10 from the reference on every stored tensor.
(The file name carries the ``ref_`` prefix of the reference-generated fixtures: tests/helpers.golden_names() takes every other ``*.pt`` of
the directory for a single-adapter case.)
usage: python tools/make_golden_tpavi.py <the reference's DG-SCT/AVS/avs_scripts/avs_s4/model/TPAVI.py>"""
import importlib
import importlib.util
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
SEED, GEN_SEED, B, C, T, H, W = 5, 2, 2, 64, 5, 7, 7


def main():
    path = sys.argv[1] if len(sys.argv) > 1 else os.environ.get("DGSCT_REFERENCE_TPAVI", "")
    if not os.path.isfile(path):
        sys.exit("make_golden_tpavi: give the reference's avs_s4/model/TPAVI.py (argument or $DGSCT_REFERENCE_TPAVI)")
    spec = importlib.util.spec_from_file_location("reference_tpavi", path)
    refmod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(refmod)
    tp = importlib.import_module("dgsct_amd.tpavi")
    import tpavi_ref as R

    torch.manual_seed(SEED)
    ref = refmod.TPAVIModule(in_channels=C, mode='dot')
    torch.manual_seed(SEED)
    mine = tp.TPAVIModule(in_channels=C, mode='dot', fused=False)
    sd, sd2 = ref.state_dict(), mine.state_dict()
    assert list(sd) == list(sd2) == list(R.KEYS), (list(sd), list(sd2))
    for k in sd:
        assert torch.equal(sd[k], sd2[k]), k
    state = R.set_nontrivial({k: v.clone() for k, v in sd.items()}, SEED + 1)

    g = torch.Generator().manual_seed(GEN_SEED)
    x, audio = torch.randn(B, C, T, H, W, generator=g), torch.randn(B, T, 128, generator=g)
    cot_z, cot_a = torch.randn(B, C, T, H, W, generator=g), torch.randn(B, T, C, generator=g)

    out = dict(seed=SEED, gen_seed=GEN_SEED, keys=list(sd), state=state, x=x, audio=audio, cot_z=cot_z, cot_a=cot_a)
    worst = 0.0
    for mode in ("train", "eval"):
        m = refmod.TPAVIModule(in_channels=C, mode='dot')
        m.load_state_dict(state)
        m = m.double().train(mode == "train")
        xx, aa = x.double().requires_grad_(True), audio.double().requires_grad_(True)
        z, a_temp = m(xx, aa)
        torch.autograd.backward([z, a_temp], [cot_z.double(), cot_a.double()])
        sd_after = m.state_dict()
        rec = dict(z=z.detach(), audio_temp=a_temp.detach(), dx=xx.grad, daudio=aa.grad, grads={n: p.grad.clone() for n, p in m.named_parameters()},
                   running_mean=sd_after["W_z.1.running_mean"].clone(), running_var=sd_after["W_z.1.running_var"].clone(),
                   num_batches_tracked=int(sd_after["W_z.1.num_batches_tracked"]))
        assert sorted(rec["grads"]) == sorted(R.PARAMS)
        mine_ = R.tpavi_f64(state, x, audio, mode == "train", cot_z, cot_a)
        for k in ("z", "audio_temp", "dx", "daudio", "running_mean", "running_var"):
            worst = max(worst, (mine_[k] - rec[k]).abs().max().item())
        for k in R.PARAMS:
            worst = max(worst, (mine_["grads"][k] - rec["grads"][k]).abs().max().item())
        out[mode] = rec
    assert worst <= 1e-10, worst
    print("max |reference - tests/tpavi_ref.py|", worst)
    # two files: in float64 the two modes together are 1.3 MB, over the 1 MiB limit for a committed file
    for name, rec in (("ref_tpavi.pt", out), ("ref_tpavi_eval.pt", dict(eval=out.pop("eval")))):
        dst = os.path.join(ROOT, "tests", "golden", name)
        torch.save(rec, dst)
        assert os.path.getsize(dst) < 1_000_000, os.path.getsize(dst)
        print("wrote", dst, os.path.getsize(dst), "bytes")


if __name__ == "__main__":
    main()
