"""TEST INFRASTRUCTURE: the live part of the CMBS event head in plain torch at any (T, B, D, K), written like the reference (sort
descending over time, [:4], mean; DG-SCT/AVE/nets/net_trans.py:273-292), random inputs for it, and the tie margins of such inputs.
Shared by tests/test_cmbs_cpu.py and tests/test_cmbs_gpu.py."""
import math

import torch

PARAMS = ("Wvc", "bvc", "Wac", "bac", "wc", "bc", "We", "be")


def head_torch(v, a, Wvc, bvc, Wac, bac, wc, bc, We, be, gamma):
    """v, a [T, B, D]; Wvc, Wac, We [K, D]; bvc, bac, be [K]; wc [1, D]; bc [1] -> (is_event [T, B, 1], event [B, K], av [B, K])"""
    cas_v = (v @ Wvc.t() + bvc).permute(1, 0, 2)
    cas_a = (a @ Wac.t() + bac).permute(1, 0, 2)
    s_v = cas_v.sort(descending=True, dim=1)[0][:, :4, :].mean(dim=1)
    s_a = cas_a.sort(descending=True, dim=1)[0][:, :4, :].mean(dim=1)
    av = (s_v + s_a) / 2
    f = (v + a) / 2
    is_event = f @ wc.t() + bc
    event = f.max(dim=0)[0] @ We.t() + be + gamma * av
    return is_event, event, av


def make_case(T, B, D, K, seed):
    """inputs, nn.Linear-style parameters (uniform in +-1/sqrt(D)) and the three cotangents, from one seeded generator"""
    g = torch.Generator().manual_seed(seed)
    r = 1.0 / math.sqrt(D)
    u = lambda *s: (torch.rand(*s, generator=g) * 2 - 1) * r          # noqa: E731
    v, a = torch.randn(T, B, D, generator=g), torch.randn(T, B, D, generator=g)
    params = dict(Wvc=u(K, D), bvc=u(K), Wac=u(K, D), bac=u(K), wc=u(1, D), bc=u(1), We=u(K, D), be=u(K))
    cots = [torch.randn(T, B, 1, generator=g), torch.randn(B, K, generator=g), torch.randn(B, K, generator=g)]
    return v, a, params, cots


def tie_margins(v, a, Wvc, bvc, Wac, bac):
    """(min over (modality, b, k) of 4th - 5th largest score over t [inf at T = 4: there is no 5th],
        min over (b, d) of largest - second largest of f = (v + a) / 2 over t)"""
    top = float("inf")
    for c in (v @ Wvc.t() + bvc, a @ Wac.t() + bac):
        s = c.sort(dim=0, descending=True)[0]
        if s.shape[0] > 4:
            top = min(top, (s[3] - s[4]).min().item())
    s = ((v + a) / 2).sort(dim=0, descending=True)[0]
    return top, (s[0] - s[1]).min().item()
