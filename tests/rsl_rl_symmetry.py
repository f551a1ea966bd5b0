"""rsl_rl's ``PPO.update`` with a ``symmetry_cfg`` (data augmentation and mirror loss) restated in plain torch: the yardstick of
``learner.PPO(symmetry_cfg=...)``, built on ``tests/rsl_rl_ppo.py``.

Statement for statement what rsl_rl does per minibatch when ``self.symmetry`` is set: with ``use_data_augmentation`` the
observations, critic observations and actions go through ``data_augmentation_func`` (originals first, then the mirrored copies)
and the four per-row scalars are repeated; the policy runs on the augmented batch; ``mu_batch`` / ``sigma_batch`` of the KL block
are the ORIGINAL rows; the symmetry loss is ``MSELoss(mean_actions[mb:], augmented(mean_actions[:mb]).detach()[mb:])`` — on the
mean of one more ``act_inference`` over the augmented observations (augmented here first when the batch was not) — and joins the
loss as ``mirror_loss_coeff * symmetry_loss`` only with ``use_mirror_loss`` (detached, so logged only, otherwise).  The function is
any callable with rsl_rl's signature ``f(obs=None, actions=None, env=None, obs_type="policy")``."""
from typing import Dict, Optional

import torch

from rsl_rl_ppo import RslRlPPO


class RslRlSymmetryPPO(RslRlPPO):
    def __init__(self, policy, storage, symmetry_cfg=None, **algorithm):
        super().__init__(policy, storage, **algorithm)
        if symmetry_cfg is not None:
            if not callable(symmetry_cfg.get("data_augmentation_func")):   # (rsl_rl resolves a string first; nothing to resolve here)
                raise ValueError(f"Symmetry configuration exists but the function is not callable: {symmetry_cfg.get('data_augmentation_func')}")
        self.symmetry = symmetry_cfg

    def update(self, generator: Optional[torch.Generator] = None) -> Dict[str, float]:
        if not self.symmetry:
            return super().update(generator)
        mean_value_loss = mean_surrogate_loss = mean_entropy = mean_symmetry_loss = 0.0
        env = getattr(self.storage, "env", None)
        for b in self.storage.mini_batch_generator(self.num_mini_batches, self.num_learning_epochs, generator=generator):
            obs_batch, critic_obs_batch, actions_batch = b.obs, b.critic_obs, b.actions
            old_actions_log_prob_batch, target_values_batch, advantages_batch, returns_batch = b.old_log_prob, b.values, b.advantages, b.returns
            original_batch_size = obs_batch.shape[0]
            if self.symmetry["use_data_augmentation"]:
                data_augmentation_func = self.symmetry["data_augmentation_func"]
                obs_batch, actions_batch = data_augmentation_func(obs=obs_batch, actions=actions_batch, env=env, obs_type="policy")
                critic_obs_batch, _ = data_augmentation_func(obs=critic_obs_batch, actions=None, env=env, obs_type="critic")
                num_aug = int(obs_batch.shape[0] / original_batch_size)
                old_actions_log_prob_batch = old_actions_log_prob_batch.repeat(num_aug)
                target_values_batch = target_values_batch.repeat(num_aug)
                advantages_batch = advantages_batch.repeat(num_aug)
                returns_batch = returns_batch.repeat(num_aug)
            mean_batch = self.policy.act_mean(obs_batch)
            std_batch = self.policy.std.expand_as(mean_batch)
            dist = torch.distributions.Normal(mean_batch, std_batch, validate_args=False)
            actions_log_prob_batch = dist.log_prob(actions_batch).sum(dim=-1)
            value_batch = self.policy.evaluate(critic_obs_batch)
            mu_batch, sigma_batch = mean_batch[:original_batch_size], std_batch[:original_batch_size]
            entropy_batch = dist.entropy().sum(dim=-1)[:original_batch_size]
            if self.desired_kl is not None and self.schedule == "adaptive":
                with torch.inference_mode():
                    kl = torch.sum(torch.log(sigma_batch / b.old_sigma + 1.0e-5)
                                   + (torch.square(b.old_sigma) + torch.square(b.old_mu - mu_batch)) / (2.0 * torch.square(sigma_batch))
                                   - 0.5, axis=-1)
                    kl_mean = torch.mean(kl)
                    if kl_mean > self.desired_kl * 2.0:
                        self.learning_rate = max(1e-5, self.learning_rate / 1.5)
                    elif kl_mean < self.desired_kl / 2.0 and kl_mean > 0.0:
                        self.learning_rate = min(1e-2, self.learning_rate * 1.5)
                    for param_group in self.optimizer.param_groups:
                        param_group["lr"] = self.learning_rate
            ratio = torch.exp(actions_log_prob_batch - torch.squeeze(old_actions_log_prob_batch))
            surrogate = -torch.squeeze(advantages_batch) * ratio
            surrogate_clipped = -torch.squeeze(advantages_batch) * torch.clamp(ratio, 1.0 - self.clip_param, 1.0 + self.clip_param)
            surrogate_loss = torch.max(surrogate, surrogate_clipped).mean()
            value_batch = value_batch.reshape(-1)
            if self.use_clipped_value_loss:
                value_clipped = target_values_batch + (value_batch - target_values_batch).clamp(-self.clip_param, self.clip_param)
                value_losses = (value_batch - returns_batch).pow(2)
                value_losses_clipped = (value_clipped - returns_batch).pow(2)
                value_loss = torch.max(value_losses, value_losses_clipped).mean()
            else:
                value_loss = (returns_batch - value_batch).pow(2).mean()
            loss = surrogate_loss + self.value_loss_coef * value_loss - self.entropy_coef * entropy_batch.mean()
            # the symmetry loss
            if not self.symmetry["use_data_augmentation"]:
                data_augmentation_func = self.symmetry["data_augmentation_func"]
                obs_batch, _ = data_augmentation_func(obs=obs_batch, actions=None, env=env, obs_type="policy")
                obs_batch = obs_batch.detach()
            mean_actions_batch = self.policy.act_mean(obs_batch.detach().clone())   # (act_inference: the actor's mean)
            action_mean_orig = mean_actions_batch[:original_batch_size]
            _, actions_mean_symm_batch = data_augmentation_func(obs=None, actions=action_mean_orig, env=env, obs_type="policy")
            mse_loss = torch.nn.MSELoss()
            symmetry_loss = mse_loss(mean_actions_batch[original_batch_size:], actions_mean_symm_batch.detach()[original_batch_size:])
            if self.symmetry["use_mirror_loss"]:
                loss += self.symmetry["mirror_loss_coeff"] * symmetry_loss
            else:
                symmetry_loss = symmetry_loss.detach()
            self.optimizer.zero_grad()
            loss.backward()
            torch.nn.utils.clip_grad_norm_(self.policy.parameters(), self.max_grad_norm)
            self.optimizer.step()
            mean_value_loss += value_loss.item()
            mean_surrogate_loss += surrogate_loss.item()
            mean_entropy += entropy_batch.mean().item()
            mean_symmetry_loss += symmetry_loss.item()
        k = self.num_learning_epochs * self.num_mini_batches
        return {"value_function": mean_value_loss / k, "surrogate": mean_surrogate_loss / k, "entropy": mean_entropy / k,
                "symmetry": mean_symmetry_loss / k}
