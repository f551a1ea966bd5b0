"""rsl_rl's ``Distillation.update`` (feed-forward ``StudentTeacher``, one rank) restated in plain torch: the yardstick of
``learner.Distillation``.

Statement for statement what rsl_rl 3.x does: ``torch.optim.Adam(policy.parameters(), lr)`` (the teacher and ``std`` never get a
gradient, so Adam never steps them), per epoch and per stored time step ``actions = policy.act_inference(obs)``, ``behavior_loss =
loss_fn(actions, privileged_actions)`` (``mse_loss`` or ``huber_loss``), ``loss = loss + behavior_loss``, the ``.item()`` of the
logged loss, and every ``gradient_length`` steps — the counter runs across the epochs — ``zero_grad``, ``loss.backward()``,
``clip_grad_norm_`` over the student's parameters when ``max_grad_norm`` is set, ``optimizer.step()``, ``loss = 0``.  The loss that is
still accumulated when the update ends is discarded.  The time steps come from ``RolloutStorage.step_batches()``."""
from typing import Dict

import torch


class RslRlDistillation:
    def __init__(self, policy, storage, num_learning_epochs=1, gradient_length=15, learning_rate=1e-3, max_grad_norm=None, loss_type="mse",
                 class_name="Distillation"):
        self.policy, self.storage = policy, storage
        self.num_learning_epochs, self.gradient_length = num_learning_epochs, gradient_length
        self.learning_rate, self.max_grad_norm = learning_rate, max_grad_norm
        self.optimizer = torch.optim.Adam(policy.parameters(), lr=learning_rate)
        self.loss_fn = {"mse": torch.nn.functional.mse_loss, "huber": torch.nn.functional.huber_loss}[loss_type]
        self.num_steps = 0   # optimizer steps taken

    def update(self) -> Dict[str, float]:
        mean_behavior_loss = 0.0
        loss = 0
        cnt = 0
        for _epoch in range(self.num_learning_epochs):
            for obs, privileged_actions in self.storage.step_batches():
                actions = self.policy.act_mean(obs)   # rsl_rl's act_inference
                behavior_loss = self.loss_fn(actions, privileged_actions)
                loss = loss + behavior_loss
                mean_behavior_loss += behavior_loss.item()
                cnt += 1
                if cnt % self.gradient_length == 0:
                    self.optimizer.zero_grad()
                    loss.backward()
                    if self.max_grad_norm:
                        torch.nn.utils.clip_grad_norm_(self.policy.student.parameters(), self.max_grad_norm)
                    self.optimizer.step()
                    self.num_steps += 1
                    loss = 0
        return {"behavior": mean_behavior_loss / cnt}
