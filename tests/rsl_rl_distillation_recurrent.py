"""rsl_rl's ``StudentTeacherRecurrent`` and its ``Distillation.update`` (one rank) restated in plain torch: the yardstick of
``learner.StudentTeacherRecurrent`` and of ``learner.Distillation`` with a recurrent student.

The module is rsl_rl 3.x's statement for statement: ``Memory`` (tests/rsl_rl_recurrent.py) in front of the student MLP and, with
``teacher_recurrent``, in front of the teacher MLP; ``reset(dones, hidden_states)``, ``get_hidden_states`` and
``detach_hidden_states`` as rsl_rl's ``Memory`` has them.

The update is rsl_rl's loop — per epoch the student's state goes back to the one the rollout started from, detached; per stored step
``actions = policy.act_inference(obs)``, ``loss = loss + loss_fn(actions, privileged_actions)``, every ``gradient_length`` steps (the
counter runs across the epochs) ``zero_grad``, ONE ``loss.backward()`` over the window, ``clip_grad_norm_``, ``optimizer.step()``,
``detach_hidden_states()``, ``loss = 0``; then ``reset(dones)`` — with the two deviations ``learner.Distillation`` documents:

* the teacher's memory is never touched by the update (rsl_rl's ``reset(hidden_states=last_hidden_states)`` rewinds it);
* ``torch.optim.Adam`` is built over the student's and ``memory_s``'s parameters (what receives a gradient) and ``max_grad_norm``
  clips the norm over all of them (rsl_rl clips ``student.parameters()`` only).

The start state is ``storage.rnn_start["student"]``, which equals rsl_rl's ``last_hidden_states``: the state update k leaves behind
is the one collection k + 1 starts from.  The time steps come from ``RolloutStorage.step_batches(with_dones=True)``."""
from typing import Dict

import torch

from rsl_rl_recurrent import Memory, _mlp


def _detach(memory) -> None:
    hs = memory.hidden_states
    if hs is not None:
        memory.hidden_states = tuple(x.detach() for x in hs) if isinstance(hs, tuple) else hs.detach()


class RslRlStudentTeacherRecurrent(torch.nn.Module):
    """``normalizers``: ``(student, teacher)`` modules in front of the memories (``None``: ``nn.Identity``)."""

    is_recurrent = True

    def __init__(self, num_student_obs, num_teacher_obs, num_actions, student_hidden_dims, teacher_hidden_dims, init_noise_std=0.1,
                 noise_std_type="scalar", rnn_type="lstm", rnn_hidden_dim=256, rnn_num_layers=1, teacher_recurrent=False, normalizers=(None, None)):
        super().__init__()
        self.noise_std_type, self.teacher_recurrent, self.loaded_teacher = noise_std_type, teacher_recurrent, False
        self.memory_s = Memory(num_student_obs, rnn_type, rnn_num_layers, rnn_hidden_dim)
        self.student = _mlp([rnn_hidden_dim, *student_hidden_dims, num_actions])
        if teacher_recurrent:
            self.memory_t = Memory(num_teacher_obs, rnn_type, rnn_num_layers, rnn_hidden_dim)
        self.teacher = _mlp([rnn_hidden_dim if teacher_recurrent else num_teacher_obs, *teacher_hidden_dims, num_actions])
        self.teacher.eval()
        if noise_std_type == "scalar":
            self.std = torch.nn.Parameter(init_noise_std * torch.ones(num_actions))
        else:
            self.log_std = torch.nn.Parameter(torch.log(init_noise_std * torch.ones(num_actions)))
        self.student_obs_normalizer = normalizers[0] if normalizers[0] is not None else torch.nn.Identity()
        self.teacher_obs_normalizer = normalizers[1] if normalizers[1] is not None else torch.nn.Identity()

    def reset(self, dones=None, hidden_states=None):
        if hidden_states is None:
            hidden_states = (None, None)
        for memory, hs in ((self.memory_s, hidden_states[0]),) + (((self.memory_t, hidden_states[1]),) if self.teacher_recurrent else ()):
            if dones is None and hs is not None:   # rsl_rl Memory.reset(dones=None, hidden_states=…): install the given state
                memory.hidden_states = hs
            else:
                memory.reset(dones)

    def act_mean(self, obs):   # rsl_rl's act_inference
        obs = self.student_obs_normalizer(obs)
        return self.student(self.memory_s(obs).squeeze(0))

    def evaluate(self, teacher_obs):
        with torch.no_grad():
            obs = self.teacher_obs_normalizer(teacher_obs)
            if self.teacher_recurrent:
                obs = self.memory_t(obs).squeeze(0)
            return self.teacher(obs)

    def get_hidden_states(self):
        return self.memory_s.hidden_states, self.memory_t.hidden_states if self.teacher_recurrent else None

    def detach_hidden_states(self):
        _detach(self.memory_s)
        if self.teacher_recurrent:
            _detach(self.memory_t)


class RslRlRecurrentDistillation:
    def __init__(self, policy, storage, num_learning_epochs=1, gradient_length=15, learning_rate=1e-3, max_grad_norm=None, loss_type="mse",
                 class_name="Distillation"):
        self.policy, self.storage = policy, storage
        self.num_learning_epochs, self.gradient_length = num_learning_epochs, gradient_length
        self.learning_rate, self.max_grad_norm = learning_rate, max_grad_norm
        self.trained = list(policy.student.parameters()) + list(policy.memory_s.parameters())
        self.optimizer = torch.optim.Adam(self.trained, lr=learning_rate)
        self.loss_fn = {"mse": torch.nn.functional.mse_loss, "huber": torch.nn.functional.huber_loss}[loss_type]
        self.num_steps = 0   # optimizer steps taken

    def update(self) -> Dict[str, float]:
        mean_behavior_loss = 0.0
        loss = 0
        cnt = 0
        memory = self.policy.memory_s
        for _epoch in range(self.num_learning_epochs):
            start = tuple(x.detach().clone().unsqueeze(0) for x in self.storage.rnn_start["student"] if x is not None)
            memory.hidden_states = start if len(start) == 2 else start[0]
            for obs, privileged_actions, dones in self.storage.step_batches(with_dones=True):
                actions = self.policy.act_mean(obs)
                behavior_loss = self.loss_fn(actions, privileged_actions)
                loss = loss + behavior_loss
                mean_behavior_loss += behavior_loss.item()
                cnt += 1
                if cnt % self.gradient_length == 0:
                    self.optimizer.zero_grad()
                    loss.backward()   # once per window: back-propagation through time inside it
                    if self.max_grad_norm:
                        torch.nn.utils.clip_grad_norm_(self.trained, self.max_grad_norm)
                    self.optimizer.step()
                    self.num_steps += 1
                    _detach(memory)
                    loss = 0
                memory.reset(dones.view(-1))
        _detach(memory)
        return {"behavior": mean_behavior_loss / cnt}
