"""Training-step plumbing around the adapter stack: what the reference's AVE script does between model and optimizer
(reference ``DG-SCT/AVE/main_trans.py``), restated for one-process-per-GPU data parallelism.

* ``trainable_by_name`` -- the freeze rule (``main_trans.py:211-256``): ``'ViT'``/``'swin'`` (optionally their norms) and
  ``'htsat'`` parameters are frozen; ``'adapter_blocks'``, ``'CMBS'``, ``'mlp_class'`` and ``'temporal_attn'`` train;
  ``'mlp_class'`` gets its own learning rate (``:257-260``).  ``task="avs_s4"``: AVS-S4's rule (``avs_s4/train.py:145-163``) --
  ``'ViT'``/``'swin'`` frozen, everything else (the HTS-AT blocks included) trains.
* ``make_optimizer`` -- ``optim.Adam(param_group)`` + ``StepLR(step_size=decay_epoch, gamma=decay)`` (``:276-278``) with the
  values of ``AVE/train.sh`` (lr 5e-4, lr_mlp 5e-6, decay 0.35 every 3 epochs).
* ``mix_lambda`` -- the reference's ``get_mix_lambda`` (``nets/utils.py:74-76``): the per-sample mix-up weights its launchers hand to the
  model, drawn one at a time from numpy's global generator.
* ``shard_clips`` / ``seed_everything`` -- per-rank sharding and seeding: the reference has one process (``--seed 43``,
  ``DataLoader(shuffle=True)``); with W ranks every rank draws the SAME epoch permutation (seed + epoch) and takes a strided
  slice of it, so the union over ranks is the single-process epoch order.
* ``StackTrainer`` -- one optimisation step of an ``AdapterStack``: forward, backward, gradient all-reduce
  (``GradAllReducer``), optimizer step.  ``bench.py`` times exactly this object; the gloo world-2 test drives the same code.

The ``accum_itr`` quirk (``main_trans.py:110,135-136``; ``train.sh`` uses ``--accum_itr=2``): the reference calls
``optimizer.zero_grad()`` EVERY iteration and ``optimizer.step()`` every ``accum_itr``-th, so the gradients of the other
iterations are discarded -- "accumulation" never accumulates; the effective schedule is "train on every 2nd batch with
batch size 8".  ``accum_mode="reference"`` reproduces that behaviour bit for bit (needed to re-trace the published
82.18 %); ``"accumulate"`` is the evident intent (gradients summed over ``accum_itr`` iterations, one step); default:
``"reference"``, because parity with the reference is the contract -- documented in DESIGN.md section 9.
"""
from __future__ import annotations

import random
from typing import Dict, Iterable, List, Optional, Sequence, Tuple

import numpy as np
import torch

TRAIN_KEYS = ("adapter_blocks", "CMBS", "mlp_class", "temporal_attn")      # main_trans.py:242-256


TASKS = ("ave", "avs_s4")


def trainable_by_name(named_parameters: Iterable[Tuple[str, torch.nn.Parameter]], is_vit_ln: bool = False, lr: float = 5e-4,
                      lr_mlp: float = 5e-6, task: str = "ave") -> List[Dict]:
    """Sets ``requires_grad`` by the reference's name rule and returns its ``param_group`` list (one entry per parameter,
    like the reference; frozen parameters are listed too -- Adam skips tensors without gradients).
    task "ave": main_trans.py:211-256 (is_vit_ln: the 'ViT'/'swin' norms train too); "avs_s4": avs_s4/train.py:145-163 ('ViT'/'swin'
    frozen, every other parameter trains; is_vit_ln does not apply)."""
    if task not in TASKS:
        raise ValueError(f"task must be one of {TASKS}, got {task!r}")
    groups = []
    for name, p in named_parameters:
        if task == "avs_s4":
            p.requires_grad = not ("ViT" in name or "swin" in name)
            groups.append({"params": p, "lr": lr})                  # (one learning rate: avs_s4/train.py builds Adam on all parameters)
            continue
        p.requires_grad = False
        if "ViT" in name or "swin" in name:
            p.requires_grad = bool(is_vit_ln) and "norm" in name
        elif "htsat" in name:
            p.requires_grad = False
        elif any(k in name for k in TRAIN_KEYS):
            p.requires_grad = True
        groups.append({"params": p, "lr": lr_mlp if "mlp_class" in name else lr})
    return groups


def ave_loss(is_event_scores: torch.Tensor, event_scores: torch.Tensor, audio_visual_gate: torch.Tensor, av_score: torch.Tensor,
             labels: torch.Tensor) -> torch.Tensor:
    """The four-term loss of the reference's AVE training loop (``main_trans.py:113-130``) on what ``AVENet`` / ``forward_swin`` return:
    ``is_event_scores`` / ``audio_visual_gate`` [T, B, 1], ``event_scores`` / ``av_score`` [B, 28], ``labels`` [B, T, 29] (one-hot per frame,
    the last class is background).

        labels_BCE [B, T]  = 1 where the frame carries a foreground class        labels_event [B] = the clip's foreground class
        loss = BCEWithLogits(is_event^T, labels_BCE) + BCEWithLogits(gate^T, labels_BCE)
             + CrossEntropy(event_scores, labels_event) + CrossEntropy(av_score, labels_event)              (all mean-reduced)

    ``audio_visual_gate`` is already a product of two sigmoids, and the reference feeds it to the LOGITS loss all the same
    (``criterion(audio_visual_gate, labels_BCE)`` with ``criterion = BCEWithLogitsLoss``): kept as it is, because parity with the
    reference's training signal is the contract.  A clip whose frames are all background gets ``labels_event`` 0, as the reference's
    ``max`` over an all-zero row gives it."""
    F = torch.nn.functional
    is_event = is_event_scores.transpose(1, 0).squeeze(-1).contiguous()
    gate = audio_visual_gate.transpose(1, 0).squeeze(-1).contiguous()
    labels_bce, labels_evn = labels[:, :, :-1].max(-1)
    labels_event, _ = labels_evn.max(-1)
    labels_bce = labels_bce.to(is_event.dtype)
    return (F.binary_cross_entropy_with_logits(is_event, labels_bce) + F.binary_cross_entropy_with_logits(gate, labels_bce)
            + F.cross_entropy(event_scores, labels_event) + F.cross_entropy(av_score, labels_event))


def mix_lambda(alpha: float, n: int) -> torch.Tensor:
    """``get_mix_lambda(alpha, n)`` (``nets/utils.py:74-76``; the launchers call it with alpha 0.5): n single ``np.random.beta(alpha, alpha, 1)``
    draws in order from numpy's global generator, as float32 ``[n]`` -- what ``HTSATFrontEnd`` / ``AVENet`` take as ``mixup_lambda``."""
    return torch.from_numpy(np.array([np.random.beta(alpha, alpha, 1)[0] for _ in range(n)]).astype(np.float32))


def make_optimizer(model: torch.nn.Module, lr: float = 5e-4, lr_mlp: float = 5e-6, decay: float = 0.35, decay_epoch: int = 3,
                   is_vit_ln: bool = False, fused: Optional[bool] = None, task: str = "ave"):
    groups = trainable_by_name(model.named_parameters(), is_vit_ln, lr, lr_mlp, task=task)
    kw = {}
    if fused is None:
        fused = all(g["params"].is_cuda for g in groups)
    if fused:
        kw["fused"] = True
    opt = torch.optim.Adam(groups, **kw)
    sched = torch.optim.lr_scheduler.StepLR(opt, step_size=decay_epoch, gamma=decay)
    return opt, sched


def seed_everything(seed: int = 43, rank: int = 0):
    """Model initialisation must be identical on every rank (same seed); data-side randomness is decorrelated by rank."""
    torch.manual_seed(seed)
    random.seed(seed * 1000 + rank)
    return torch.Generator().manual_seed(seed * 1000 + rank)


def shard_clips(n: int, rank: int, world: int, seed: int = 43, epoch: int = 0, shuffle: bool = True, drop_last: bool = False) -> List[int]:
    """Clip indices of `rank` for one epoch: every rank computes the same permutation (seed + epoch) and takes every
    world-th element; the tail is padded by wrapping around (or dropped) so that all ranks run the same number of steps."""
    g = torch.Generator().manual_seed(seed + epoch)
    order = torch.randperm(n, generator=g).tolist() if shuffle else list(range(n))
    if drop_last:
        order = order[: n - n % world]
    elif len(order) % world:
        order += order[: world - len(order) % world]
    return order[rank::world]


class StackTrainer:
    """forward + backward + (DP) all-reduce + optimizer step of an AdapterStack on fixed cotangents (the adapter-path
    benchmark of BASELINE.json) or on a loss callable."""

    def __init__(self, stack, optimizer=None, reducer=None, accum_itr: int = 1, accum_mode: str = "reference"):
        if accum_mode not in ("reference", "accumulate"):
            raise ValueError("accum_mode must be 'reference' or 'accumulate'")
        self.stack, self.opt, self.reducer = stack, optimizer, reducer
        self.accum_itr, self.accum_mode = max(1, int(accum_itr)), accum_mode
        self.params = [p for p in stack.parameters() if p.requires_grad]
        self.it = 0

    def fwd_bwd(self, feats, cots=None, mcots=None, loss_fn=None):
        outs, maps = self.stack(feats, **getattr(self, "block_kwargs", {}))      # (vis_block= / aud_block=: frozen backbone blocks, backbone.py)
        if loss_fn is not None:
            loss_fn(outs, maps).backward()
        else:
            tensors = [t for pair in outs for t in pair]
            grads = [g for pair in cots for g in pair]
            if mcots is not None:
                tensors += [maps[0], maps[1]]
                grads += [mcots[0], mcots[1]]
            torch.autograd.backward(tensors, grads)
        for fv, fa in feats:
            if fv.requires_grad:
                fv.grad = None
            if fa.requires_grad:
                fa.grad = None
        return outs, maps

    def zero_grad(self, set_to_none: bool = True):
        if self.opt is not None:
            self.opt.zero_grad(set_to_none=set_to_none)
        else:
            for p in self.params:
                if set_to_none:
                    p.grad = None
                elif p.grad is not None:
                    p.grad.zero_()

    def step(self, feats, cots=None, mcots=None, loss_fn=None, last: bool = False) -> bool:
        """One training iteration with the reference's control flow (main_trans.py:110-136).  Returns True when the
        optimizer stepped."""
        first_of_window = self.it % self.accum_itr == 0
        do_step = (self.it + 1) % self.accum_itr == 0 or last
        if self.accum_mode == "reference" or first_of_window:
            self.zero_grad()                                     # reference: every iteration (discards the previous one)
        if self.reducer is not None:
            # Only the stepping iteration communicates: its hooks (and finish()) see the gradients of the whole window in
            # "accumulate" mode, and in "reference" mode the iterations whose gradients are thrown away cost no all-reduce.
            self.reducer.paused = not do_step
        self.fwd_bwd(feats, cots, mcots, loss_fn)
        self.it += 1
        if do_step:
            if self.reducer is not None:
                self.reducer.finish()                            # mean over ranks of what this iteration (window) produced
            if self.opt is not None:
                self.opt.step()
        elif self.reducer is not None:
            self.reducer.discard()                               # (nothing was launched while paused)
        if last:
            self.it = 0                                          # the reference keys the window on batch_idx, which restarts every epoch (main_trans.py:135)
        return do_step
