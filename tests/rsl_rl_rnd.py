"""rsl_rl's random network distillation restated in plain torch: the yardstick of ``learner.RandomNetworkDistillation``,
``learner.EmpiricalDiscountedVariationNormalization`` and ``learner.PPO(rnd_cfg=...)``.

* ``RslRlDiscountedVariationNormalization`` / ``RslRlRND``: the module — a frozen target and a trained predictor (Linear + ELU) on the
  normalised ``rnd_state``, the L2 distance of their outputs, the reward normaliser (a per-env discounted sum whose running std
  divides the reward, no eps, only when that std is positive), the weight schedules on ``update_counter``.
* ``RslRlRndPPO``: rsl_rl's ``PPO.update`` with RND, built on ``tests/rsl_rl_symmetry.py`` (and through it ``tests/rsl_rl_ppo.py``) by
  import.  The predictor has parameters and an Adam of its own and shares only the minibatch's ``indices`` with the policy's step,
  so the RND lines run as each minibatch is handed back to the generator: ``MSELoss(predictor(s), target(s).detach())`` on the
  ``rnd_state`` rows ``t`` of the batch's transitions through the state normaliser under ``no_grad``, ``zero_grad`` / ``backward`` /
  ``step`` with no clipping, and the ``.item()`` of the logged loss."""
from typing import Dict, Optional

import torch
from torch import nn

from rsl_rl_norm import RslRlEmpiricalNormalization
from rsl_rl_symmetry import RslRlSymmetryPPO


def _mlp(sizes):
    layers = []
    for i in range(len(sizes) - 1):
        layers.append(nn.Linear(sizes[i], sizes[i + 1]))
        if i < len(sizes) - 2:
            layers.append(nn.ELU())
    return nn.Sequential(*layers)


class RslRlDiscountedVariationNormalization(nn.Module):
    def __init__(self, eps=1e-2, gamma=0.99, until=None):
        super().__init__()
        self.emp_norm = RslRlEmpiricalNormalization(1, eps=eps, until=until)
        self.gamma = gamma
        self.avg = None

    def forward(self, rew):
        if self.training:
            self.avg = rew if self.avg is None else self.avg * self.gamma + rew
            self.emp_norm.update(self.avg.reshape(-1, 1))
        if self.emp_norm._std > 0:
            return rew / self.emp_norm._std.reshape(())
        return rew


class RslRlRND(nn.Module):
    def __init__(self, num_states, num_outputs, predictor_hidden_dims, target_hidden_dims, activation="elu", weight=0.0,
                 state_normalization=False, reward_normalization=False, weight_schedule=None):
        super().__init__()
        if activation != "elu":
            raise ValueError("only 'elu'")
        hidden = lambda dims: [num_states if h == -1 else h for h in dims]
        self.predictor = _mlp([num_states, *hidden(predictor_hidden_dims), num_outputs])
        self.target = _mlp([num_states, *hidden(target_hidden_dims), num_outputs])
        self.target.eval()
        for p in self.target.parameters():
            p.requires_grad = False
        self.initial_weight = self.weight = weight
        self.weight_schedule = weight_schedule
        self.state_normalizer = RslRlEmpiricalNormalization(num_states, until=10 ** 8) if state_normalization else nn.Identity()
        self.reward_normalizer = RslRlDiscountedVariationNormalization(eps=1e-2, gamma=0.99, until=10 ** 8) if reward_normalization else nn.Identity()
        self.update_counter = 0

    def update_normalization(self, rnd_state):
        if not isinstance(self.state_normalizer, nn.Identity):
            self.state_normalizer.update(rnd_state)

    def _weight(self):
        s, step = self.weight_schedule, self.update_counter
        if s is None or s["mode"] == "constant":
            return self.initial_weight
        if s["mode"] == "step":
            return self.initial_weight if step < s["final_step"] else s["final_value"]
        if s["mode"] == "linear":
            if step < s["initial_step"]:
                return self.initial_weight
            if step > s["final_step"]:
                return s["final_value"]
            return self.initial_weight + (s["final_value"] - self.initial_weight) * (step - s["initial_step"]) / (s["final_step"] - s["initial_step"])
        raise ValueError(f"unknown schedule {s!r}")

    @torch.no_grad()
    def get_intrinsic_reward(self, rnd_state):
        self.update_counter += 1
        x = self.state_normalizer(rnd_state)
        r = torch.linalg.norm(self.target(x) - self.predictor(x), dim=1)
        r = self.reward_normalizer(r)
        self.weight = self._weight()
        return r * self.weight


def rnd_state_rows(storage) -> torch.Tensor:
    """The ``rnd_state`` observation of every stored transition, ``[T·N, W]``: row ``t`` of each member, members side by side."""
    T, n = storage.num_steps, storage.env.num_envs
    parts = [storage.observation_rows(m)[:T].reshape(T * n, -1) for m in storage.obs_groups["rnd_state"]]
    return parts[0] if len(parts) == 1 else torch.cat(parts, dim=-1)


class _RndBatches:
    """The storage as the policy's loop sees it: every minibatch it hands out is followed by the RND step on that batch's rows."""

    def __init__(self, storage, owner):
        self._storage, self._owner = storage, owner

    def __getattr__(self, name):
        return getattr(self._storage, name)

    def mini_batch_generator(self, *args, **kwargs):
        for b in self._storage.mini_batch_generator(*args, **kwargs):
            yield b
            self._owner._rnd_minibatch(b)


class RslRlRndPPO(RslRlSymmetryPPO):
    def __init__(self, policy, storage, rnd, rnd_learning_rate=1e-3, symmetry_cfg=None, **algorithm):
        super().__init__(policy, _RndBatches(storage, self), symmetry_cfg=symmetry_cfg, **algorithm)
        self.rnd = rnd
        self.rnd_optimizer = torch.optim.Adam(rnd.predictor.parameters(), lr=rnd_learning_rate)
        self.mean_rnd_loss = 0.0

    def _rnd_minibatch(self, b):
        with torch.no_grad():
            rnd_state_batch = self.rnd.state_normalizer(rnd_state_rows(self.storage._storage)[b.indices])
        predicted_embedding = self.rnd.predictor(rnd_state_batch)
        target_embedding = self.rnd.target(rnd_state_batch).detach()
        rnd_loss = torch.nn.MSELoss()(predicted_embedding, target_embedding)
        self.rnd_optimizer.zero_grad()
        rnd_loss.backward()
        self.rnd_optimizer.step()
        self.mean_rnd_loss += rnd_loss.item()

    def update(self, generator: Optional[torch.Generator] = None) -> Dict[str, float]:
        self.mean_rnd_loss = 0.0
        out = super().update(generator)
        out["rnd"] = self.mean_rnd_loss / (self.num_learning_epochs * self.num_mini_batches)
        return out
