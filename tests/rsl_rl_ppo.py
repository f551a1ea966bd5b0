"""rsl_rl's ``PPO.update`` (non-recurrent path, no RND, no symmetry) restated in plain torch: the yardstick of ``learner.PPO``.

Statement for statement what rsl_rl 3.x does per minibatch — ``Normal(mu, std)`` (validation off, as rsl_rl's ActorCritic sets
it), the KL block with its ``kl_mean > desired_kl * 2.0`` test on the host, the surrogate and clipped value losses,
``loss.backward()``, ``clip_grad_norm_``, ``torch.optim.Adam(lr=…)`` with the lr written into the param group, and the three
``.item()`` of the logged losses — over the minibatches of ``RolloutStorage.mini_batch_generator``."""
from typing import Dict, Optional

import torch


class RslRlPPO:
    def __init__(self, policy, storage, clip_param=0.2, desired_kl=0.01, entropy_coef=0.01, gamma=0.99, lam=0.95, learning_rate=0.001,
                 max_grad_norm=1.0, num_learning_epochs=5, num_mini_batches=4, schedule="adaptive", use_clipped_value_loss=True,
                 value_loss_coef=1.0, class_name="PPO"):
        self.policy, self.storage = policy, storage
        self.clip_param, self.desired_kl, self.entropy_coef = clip_param, desired_kl, entropy_coef
        self.gamma, self.lam, self.learning_rate, self.max_grad_norm = gamma, lam, learning_rate, max_grad_norm
        self.num_learning_epochs, self.num_mini_batches, self.schedule = num_learning_epochs, num_mini_batches, schedule
        self.use_clipped_value_loss, self.value_loss_coef = use_clipped_value_loss, value_loss_coef
        self.optimizer = torch.optim.Adam(policy.parameters(), lr=learning_rate)

    def update(self, generator: Optional[torch.Generator] = None) -> Dict[str, float]:
        mean_value_loss = mean_surrogate_loss = mean_entropy = 0.0
        for b in self.storage.mini_batch_generator(self.num_mini_batches, self.num_learning_epochs, generator=generator):
            mu_batch = self.policy.act_mean(b.obs)
            sigma_batch = self.policy.std.expand_as(mu_batch)
            dist = torch.distributions.Normal(mu_batch, sigma_batch, validate_args=False)
            actions_log_prob_batch = dist.log_prob(b.actions).sum(dim=-1)
            value_batch = self.policy.evaluate(b.critic_obs)
            entropy_batch = dist.entropy().sum(dim=-1)
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
            ratio = torch.exp(actions_log_prob_batch - torch.squeeze(b.old_log_prob))
            surrogate = -torch.squeeze(b.advantages) * ratio
            surrogate_clipped = -torch.squeeze(b.advantages) * torch.clamp(ratio, 1.0 - self.clip_param, 1.0 + self.clip_param)
            surrogate_loss = torch.max(surrogate, surrogate_clipped).mean()
            value_batch = value_batch.reshape(-1)
            if self.use_clipped_value_loss:
                value_clipped = b.values + (value_batch - b.values).clamp(-self.clip_param, self.clip_param)
                value_losses = (value_batch - b.returns).pow(2)
                value_losses_clipped = (value_clipped - b.returns).pow(2)
                value_loss = torch.max(value_losses, value_losses_clipped).mean()
            else:
                value_loss = (b.returns - value_batch).pow(2).mean()
            loss = surrogate_loss + self.value_loss_coef * value_loss - self.entropy_coef * entropy_batch.mean()
            self.optimizer.zero_grad()
            loss.backward()
            torch.nn.utils.clip_grad_norm_(self.policy.parameters(), self.max_grad_norm)
            self.optimizer.step()
            mean_value_loss += value_loss.item()
            mean_surrogate_loss += surrogate_loss.item()
            mean_entropy += entropy_batch.mean().item()
        k = self.num_learning_epochs * self.num_mini_batches
        return {"value_function": mean_value_loss / k, "surrogate": mean_surrogate_loss / k, "entropy": mean_entropy / k}
