"""TeacherKLLoss — drop-in for rl_algo_impls/loss/teacher_kl_loss.py:10-50.

PPO's teacher-KL term keeps a fine-tuned policy near a frozen checkpoint: after every rollout the
teacher's log-probability of each taken action joins the batch (add_to_batch ->
Batch.additional["teacher_logprobs"]), and every minibatch adds coef * mean(row) to the loss, with
d = teacher_logp - new_logp and row = (exp(d) - 1) - d (unbiased) or 0.5 d^2, times the
importance ratio when PPO passes it as weights.

On the device PPO computes the term inside its fused loss kernel (rai_ppo_loss_teacher, csrc/loss_body.h);
forward() below is the same expression in plain torch, for CPU use and as the in-repo reference.

ckpts_manager is any object with a `.latest_checkpoint` policy.  The reference's
PolicyCheckpointsManager is not part of this package: a one-attribute holder supplies the frozen
policy,

    class Holder:
        latest_checkpoint = teacher_policy
"""
from __future__ import annotations

from typing import Dict, Optional

import torch
from torch.nn.modules.loss import _Loss


class TeacherKLLoss(_Loss):
    def __init__(self, ckpts_manager, unbiased: bool = True, **kwargs) -> None:
        super().__init__(**kwargs)
        self.ckpts_manager = ckpts_manager
        self.unbiased = unbiased
        assert self.reduction == "mean", f"reduction must be 'mean', got {self.reduction}"

    def add_to_batch(self, batch) -> Dict[str, torch.Tensor]:
        teacher = self.ckpts_manager.latest_checkpoint
        assert teacher is not None, "No checkpoints available"
        with torch.no_grad():
            out = teacher(batch.obs, batch.actions, action_masks=batch.action_masks)
        # the reference's ACForward names the field; this package's policies return (logp, entropy, v)
        logp = out.logp_a if hasattr(out, "logp_a") else out[0]
        return {"teacher_logprobs": logp.detach()}

    def forward(self, training_logprobs: torch.Tensor, mb_additional: Dict[str, torch.Tensor],
                weights: Optional[torch.Tensor]) -> torch.Tensor:
        logratio = mb_additional["teacher_logprobs"] - training_logprobs
        if self.unbiased:
            loss = (torch.exp(logratio) - 1) - logratio
        else:
            loss = 0.5 * logratio**2
        if weights is not None:
            loss = loss * weights
        return loss.mean()
