"""The audio / image front ends (dg-sct_amd/frontend.py) without a GPU: state_dict names, checkpoint loading (the derived STFT basis is
checked and dropped), the Slaney filterbank, the ATen formulation (fused=False, fp32, CPU) against the float64 reference of
tests/frontend_ref.py, the argument checks, and the optional binding of the C symbols (the host emulation has no front end)."""
import os
import sys

import pytest
import torch

import dgsct_amd
from dgsct_amd import HTSATFrontEnd, PatchEmbed
from dgsct_amd._lib import Lib

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import frontend_ref as R                    # noqa: E402
from helpers import fp32_err                # noqa: E402

AUDIO_KEYS = {"logmel_extractor.melW", "bn0.weight", "bn0.bias", "bn0.running_mean", "bn0.running_var", "bn0.num_batches_tracked",
              "patch_embed.proj.weight", "patch_embed.proj.bias", "patch_embed.norm.weight", "patch_embed.norm.bias"}


def test_exports():
    assert dgsct_amd.HTSATFrontEnd is HTSATFrontEnd and dgsct_amd.PatchEmbed is PatchEmbed


def test_state_dict_keys():
    m = HTSATFrontEnd()
    sd = m.state_dict()
    assert set(sd) == AUDIO_KEYS
    assert tuple(sd["logmel_extractor.melW"].shape) == (513, 64)
    assert tuple(sd["patch_embed.proj.weight"].shape) == (96, 1, 4, 4)
    p = PatchEmbed(192, in_chans=3, embed_dim=128)
    assert set(p.state_dict()) == {"proj.weight", "proj.bias", "norm.weight", "norm.bias"}
    assert tuple(p.state_dict()["proj.weight"].shape) == (128, 3, 4, 4)
    assert not any(q.requires_grad for q in list(m.parameters()) + list(p.parameters()))


def test_checkpoint_with_stft_basis_loads_and_other_basis_raises():
    src = R.randomise(HTSATFrontEnd(), 1)
    sd = dict(src.state_dict())
    real, imag = R.hann_basis()
    sd["spectrogram_extractor.stft.conv_real.weight"] = real.float()
    sd["spectrogram_extractor.stft.conv_imag.weight"] = imag.float()
    dst = HTSATFrontEnd()
    res = dst.load_state_dict(sd, strict=True)
    assert not res.missing_keys and not res.unexpected_keys
    assert set(dst.state_dict()) == AUDIO_KEYS
    for k, v in src.state_dict().items():
        assert torch.equal(v, dst.state_dict()[k]), k
    bad = dict(sd)
    bad["spectrogram_extractor.stft.conv_real.weight"] = real.float() * 1.01               # e.g. another window
    with pytest.raises(RuntimeError, match="DFT basis"):
        HTSATFrontEnd().load_state_dict(bad, strict=True)
    bad = dict(sd)
    bad["spectrogram_extractor.stft.conv_imag.weight"] = imag.float()[:, :, :512]          # another n_fft
    with pytest.raises(RuntimeError, match="DFT basis"):
        HTSATFrontEnd().load_state_dict(bad, strict=True)


def test_filterbank():
    W = HTSATFrontEnd().logmel_extractor.melW.double()
    ref = torch.from_numpy(R.slaney_melW())
    assert (W - ref).abs().max().item() < 1e-6
    assert (W >= 0).all()
    assert (W.sum(0) > 0).all()                                    # no empty filter
    assert ((W != 0).sum(1) <= 2).all()                            # a bin sits under at most two triangles


CASES = [(2, 3200), (3, 5000)]


@pytest.mark.parametrize("B,L", CASES)
def test_aten_logmel_against_float64(B, L):
    x = R.signal(B, L)
    m = HTSATFrontEnd(fused=False)
    lm = m.logmel_aten(x)
    ref = R.logmel(x)
    assert lm.shape == ref.shape == (B, L // 320 + 1, 64)
    assert (lm.double() - ref).abs().max().item() < 1e-4           # dB; an fp32 evaluation sits at 1.1e-5 .. 2.7e-5, and 8 x this error bounds the device


@pytest.mark.parametrize("training", [False, True])
@pytest.mark.parametrize("B,L", CASES)
def test_aten_tokens_against_float64(B, L, training):
    x = R.signal(B, L)
    m = R.randomise(HTSATFrontEnd(fused=False), 2).train(training)
    sd0 = {k: v.clone() for k, v in m.state_dict().items()}
    tok = m(x)
    ref, rm, rv = R.audio_tokens(R.logmel(x), sd0, training)
    assert tok.shape == (B, 4096, 96) and tok.dtype == torch.float32 and not tok.requires_grad
    assert fp32_err(tok, ref) < 1e-3
    sd1 = m.state_dict()
    if training:
        assert int(sd1["bn0.num_batches_tracked"]) == int(sd0["bn0.num_batches_tracked"]) + 1
        assert ((sd1["bn0.running_mean"].double() - rm).abs() / rm.abs().clamp_min(1e-3)).max().item() < 1e-4
        assert ((sd1["bn0.running_var"].double() - rv).abs() / rv.abs()).max().item() < 1e-4
    else:
        for k in sd0:
            assert torch.equal(sd0[k], sd1[k]), k


def test_patch_embed_aten_against_float64():
    g = torch.Generator().manual_seed(5)
    for shape, C in (((2, 3, 32, 48), 128), ((1, 1, 32, 32), 96)):
        m = R.randomise(PatchEmbed(shape[2:], in_chans=shape[1], embed_dim=C, fused=False), 6)
        img = torch.randn(shape, generator=g)
        tok = m(img)
        assert tok.shape == (shape[0], shape[2] * shape[3] // 16, C)
        assert fp32_err(tok, R.patch_tokens(img, m.state_dict())) < 1e-3
        assert m(img.bfloat16()).dtype == torch.bfloat16


def test_argument_checks():
    m = HTSATFrontEnd(fused=False)
    with pytest.raises(RuntimeError, match="frames"):
        m(torch.zeros(1, 320 * 1024))                              # 1025 frames
    with pytest.raises(RuntimeError, match="requires grad"):
        m(torch.zeros(1, 3200, requires_grad=True))
    with pytest.raises(RuntimeError, match="too few"):
        m(torch.zeros(1, 512))
    m(torch.zeros(1, 513))                                         # the shortest waveform the reflect padding admits
    with pytest.raises(RuntimeError, match="fp32 waveform"):
        m(torch.zeros(3200))
    with pytest.raises(RuntimeError, match="CUDA/HIP"):
        HTSATFrontEnd(fused=True)(torch.zeros(1, 3200))
    p = PatchEmbed(32, in_chans=3, embed_dim=96, fused=False)
    with pytest.raises(RuntimeError, match="does not match"):
        p(torch.zeros(1, 3, 32, 36))
    with pytest.raises(RuntimeError, match="requires grad"):
        p(torch.zeros(1, 3, 32, 32, requires_grad=True))
    with pytest.raises(ValueError):
        PatchEmbed(32, patch_size=8)
    with pytest.raises(ValueError):
        PatchEmbed(32, embed_dim=100)
    from dgsct_amd import ops
    with pytest.raises(RuntimeError, match="CUDA/HIP"):
        ops.logmel(torch.zeros(1, 3200), m.logmel_extractor.melW)
    with pytest.raises(RuntimeError, match="CUDA/HIP"):
        ops.patch_embed(torch.zeros(1, 3, 32, 32), p.proj.weight, p.proj.bias, p.norm.weight, p.norm.bias)


def test_mel_ranges_cover_the_nonzeros():
    from dgsct_amd import ops
    W = HTSATFrontEnd().logmel_extractor.melW
    r = ops.mel_ranges(W)
    assert r.dtype == torch.int32 and tuple(r.shape) == (64, 2)
    for mcol in range(64):
        lo, hi = int(r[mcol, 0]), int(r[mcol, 1])
        assert 0 <= lo < hi <= 513
        assert W[:lo, mcol].abs().sum() == 0 and W[hi:, mcol].abs().sum() == 0 and W[lo, mcol] != 0 and W[hi - 1, mcol] != 0
    dense = torch.ones(513, 64)
    dense[:, 3] = 0
    r = ops.mel_ranges(dense)
    assert r[0].tolist() == [0, 513] and r[3, 0] == r[3, 1]


def test_emulation_builds_and_has_no_front_end():
    sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "emu"))
    from build_emu import build_emu
    emu = Lib(build_emu())
    for call, name in ((lambda: emu.logmel_scratch_floats(1, 3200), "dgsct_logmel_scratch_floats"),
                       (lambda: emu.logmel_forward(1, 3200, None, None, None, None, None, None, None), "dgsct_logmel_forward"),
                       (lambda: emu.patch_embed_forward(0, 0, 0, 1, 3, 32, 32, 0, 96, None, None, None, None, None, None, None, 1e-5, None, None),
                        "dgsct_patch_embed_forward")):
        with pytest.raises(RuntimeError, match=name):
            call()


def test_product_library_exports_the_front_end_and_checks_arguments():
    lib = dgsct_amd.default_lib()
    assert lib.logmel_scratch_floats(2, 3200) == 2 * 6 * 384       # 11 frames = 6 frame pairs per clip, one workgroup each
    assert lib.logmel_scratch_floats(160, 320000) == 2048 * 384
    with pytest.raises(RuntimeError, match="n_fft = 1024"):
        lib.logmel_scratch_floats(2, 3200, n_fft=512)
    with pytest.raises(RuntimeError, match="n_fft = 1024"):
        lib.logmel_forward(2, 3200, 1, 1, None, 1, None, None, None, hop=160)
    with pytest.raises(RuntimeError, match="frames"):
        lib.logmel_scratch_floats(1, 320 * 1024)
    with pytest.raises(RuntimeError, match="frames"):
        lib.logmel_scratch_floats(1, 512)
