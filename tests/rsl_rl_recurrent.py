"""rsl_rl's recurrent policy restated in plain torch: the yardstick of ``learner.ActorCriticRecurrent``, of the trajectory
minibatches and of ``learner.PPO`` with a recurrent policy.

Statement for statement what rsl_rl 3.x does: ``Memory`` (a sequence-major one-layer ``nn.LSTM`` / ``nn.GRU``, its hidden state, the
masked reset), ``ActorCriticRecurrent`` (``obs -> normaliser -> memory -> MLP``), ``split_and_pad_trajectories`` /
``unpad_trajectories`` and ``RolloutStorage.recurrent_mini_batch_generator`` with its per-step ``saved_hidden_states``."""
from typing import Iterator, NamedTuple, Optional

import torch


def split_and_pad_trajectories(tensor: torch.Tensor, dones: torch.Tensor):
    """``tensor`` ``[T, N, ...]`` cut at the dones (``[T, N]``; the last step counts as one) into trajectories, env-major, padded with
    zeros to ``[T, ntraj, ...]``; and the masks ``[T, ntraj]`` of the real steps."""
    dones = dones.clone().to(torch.bool)
    dones[-1] = True
    flat_dones = dones.transpose(1, 0).reshape(-1, 1)
    done_indices = torch.cat((flat_dones.new_tensor([-1], dtype=torch.int64), flat_dones.nonzero()[:, 0]))
    trajectory_lengths = done_indices[1:] - done_indices[:-1]
    trajectories = torch.split(tensor.transpose(1, 0).flatten(0, 1), trajectory_lengths.tolist())
    trajectories = trajectories + (torch.zeros(tensor.shape[0], *tensor.shape[2:], device=tensor.device, dtype=tensor.dtype),)
    padded = torch.nn.utils.rnn.pad_sequence(trajectories)
    padded = padded[:, :-1]
    masks = trajectory_lengths > torch.arange(0, padded.shape[0], device=tensor.device).unsqueeze(1)
    return padded, masks


def unpad_trajectories(trajectories: torch.Tensor, masks: torch.Tensor) -> torch.Tensor:
    return trajectories.transpose(1, 0)[masks.transpose(1, 0)].view(-1, trajectories.shape[0], trajectories.shape[-1]).transpose(1, 0)


class Memory(torch.nn.Module):
    def __init__(self, input_size: int, type: str = "lstm", num_layers: int = 1, hidden_size: int = 256):
        super().__init__()
        rnn_cls = torch.nn.GRU if type.lower() == "gru" else torch.nn.LSTM
        self.rnn = rnn_cls(input_size=input_size, hidden_size=hidden_size, num_layers=num_layers)
        self.hidden_states = None

    def forward(self, input, masks=None, hidden_states=None):
        batch_mode = masks is not None
        if batch_mode:
            if hidden_states is None:
                raise ValueError("Hidden states not passed to memory module during policy update")
            out, _ = self.rnn(input, hidden_states)
            out = unpad_trajectories(out, masks)
        else:
            out, self.hidden_states = self.rnn(input.unsqueeze(0), self.hidden_states)
        return out

    def reset(self, dones=None):
        if dones is None:
            self.hidden_states = None
        elif self.hidden_states is not None:
            states = self.hidden_states if isinstance(self.hidden_states, tuple) else (self.hidden_states,)
            for hidden_state in states:
                hidden_state[..., dones == 1, :] = 0.0


def _mlp(sizes):
    layers = []
    for i in range(len(sizes) - 1):
        layers.append(torch.nn.Linear(sizes[i], sizes[i + 1]))
        if i < len(sizes) - 2:
            layers.append(torch.nn.ELU())
    return torch.nn.Sequential(*layers)


class RslRlActorCriticRecurrent(torch.nn.Module):
    """``normalizers``: ``(actor, critic)`` modules in front of the memories (``None``: ``nn.Identity``)."""

    is_recurrent = True

    def __init__(self, num_obs, num_actions, actor_hidden_dims, critic_hidden_dims, init_noise_std=1.0, num_critic_obs=None,
                 noise_std_type="scalar", rnn_type="lstm", rnn_hidden_dim=256, rnn_num_layers=1, normalizers=(None, None)):
        super().__init__()
        num_critic_obs = num_obs if num_critic_obs is None else num_critic_obs
        self.noise_std_type = noise_std_type
        self.memory_a = Memory(num_obs, rnn_type, rnn_num_layers, rnn_hidden_dim)
        self.memory_c = Memory(num_critic_obs, rnn_type, rnn_num_layers, rnn_hidden_dim)
        self.actor = _mlp([rnn_hidden_dim, *actor_hidden_dims, num_actions])
        self.critic = _mlp([rnn_hidden_dim, *critic_hidden_dims, 1])
        if noise_std_type == "scalar":
            self.std = torch.nn.Parameter(init_noise_std * torch.ones(num_actions))
        else:
            self.log_std = torch.nn.Parameter(torch.log(init_noise_std * torch.ones(num_actions)))
        self.actor_obs_normalizer = normalizers[0] if normalizers[0] is not None else torch.nn.Identity()
        self.critic_obs_normalizer = normalizers[1] if normalizers[1] is not None else torch.nn.Identity()

    def reset(self, dones=None):
        self.memory_a.reset(dones)
        self.memory_c.reset(dones)

    def act_mean(self, obs, masks=None, hidden_states=None):
        obs = self.actor_obs_normalizer(obs)
        out_mem = self.memory_a(obs, masks, hidden_states).squeeze(0)
        return self.actor(out_mem)

    def evaluate(self, obs, masks=None, hidden_states=None):
        obs = self.critic_obs_normalizer(obs)
        out_mem = self.memory_c(obs, masks, hidden_states).squeeze(0)
        return self.critic(out_mem)

    def get_hidden_states(self):
        return self.memory_a.hidden_states, self.memory_c.hidden_states


class RecurrentBatch(NamedTuple):
    obs: torch.Tensor                # [T, ntraj, W] padded
    critic_obs: torch.Tensor
    masks: torch.Tensor              # [T, ntraj] bool
    hid_a: tuple                     # per state tensor: [1, ntraj, H]
    hid_c: tuple
    env_start: int
    env_stop: int


def recurrent_mini_batches(obs: torch.Tensor, critic_obs: torch.Tensor, dones: torch.Tensor, saved_a: tuple, saved_c: tuple,
                           num_mini_batches: int, num_epochs: int = 1) -> Iterator[RecurrentBatch]:
    """rsl_rl's ``recurrent_mini_batch_generator`` on a rollout ``obs [T, N, W]``, ``dones [T, N]`` and the per-step saved hidden
    states ``saved_* = (h [T, 1, N, H], …)`` (the state each step started from).  Minibatch ``i`` is the envs
    ``[i·N // num_mini_batches, (i + 1)·N // num_mini_batches)``; the per-row fields of a batch are ``field[:, start:stop]``."""
    T, N = dones.shape
    padded_obs, masks = split_and_pad_trajectories(obs, dones)
    padded_critic, _ = split_and_pad_trajectories(critic_obs, dones)
    dones = dones.to(torch.bool)
    for _ep in range(num_epochs):
        first_traj = 0
        for i in range(num_mini_batches):
            start, stop = i * N // num_mini_batches, (i + 1) * N // num_mini_batches
            last_was_done = torch.zeros_like(dones, dtype=torch.bool)
            last_was_done[1:] = dones[:-1]
            last_was_done[0] = True
            last_traj = first_traj + int(torch.sum(last_was_done[:, start:stop]))
            lwd = last_was_done.permute(1, 0)
            hid_a = tuple(s.permute(2, 0, 1, 3)[lwd][first_traj:last_traj].transpose(1, 0).contiguous() for s in saved_a)
            hid_c = tuple(s.permute(2, 0, 1, 3)[lwd][first_traj:last_traj].transpose(1, 0).contiguous() for s in saved_c)
            yield RecurrentBatch(padded_obs[:, first_traj:last_traj], padded_critic[:, first_traj:last_traj], masks[:, first_traj:last_traj],
                                 hid_a, hid_c, start, stop)
            first_traj = last_traj


class RslRlRecurrentPPO:
    """rsl_rl's ``PPO.update`` for a recurrent policy: ``tests/rsl_rl_ppo.py``'s statements over ``recurrent_mini_batches`` — the
    policy in batch mode on the padded trajectories, the per-row fields ``field[:, start:stop]`` of the storage."""

    def __init__(self, policy, storage, clip_param=0.2, desired_kl=0.01, entropy_coef=0.01, gamma=0.99, lam=0.95, learning_rate=0.001,
                 max_grad_norm=1.0, num_learning_epochs=5, num_mini_batches=4, schedule="adaptive", use_clipped_value_loss=True,
                 value_loss_coef=1.0, class_name="PPO"):
        self.policy, self.storage = policy, storage
        self.clip_param, self.desired_kl, self.entropy_coef = clip_param, desired_kl, entropy_coef
        self.gamma, self.lam, self.learning_rate, self.max_grad_norm = gamma, lam, learning_rate, max_grad_norm
        self.num_learning_epochs, self.num_mini_batches, self.schedule = num_learning_epochs, num_mini_batches, schedule
        self.use_clipped_value_loss, self.value_loss_coef = use_clipped_value_loss, value_loss_coef
        self.optimizer = torch.optim.Adam(policy.parameters(), lr=learning_rate)

    def update(self, obs, critic_obs, saved_a, saved_c):
        """``obs`` / ``critic_obs`` ``[T, N, W]`` (already through the policy's normalisers, if it has any: the policy given here has
        none); ``saved_*``: the per-step hidden states rsl_rl's storage keeps."""
        st = self.storage
        mean_value_loss = mean_surrogate_loss = mean_entropy = 0.0
        for rb in recurrent_mini_batches(obs, critic_obs, st.dones, saved_a, saved_c, self.num_mini_batches, self.num_learning_epochs):
            cut = lambda x: x[:, rb.env_start:rb.env_stop]
            one = lambda h: h if len(h) == 2 else h[0]
            mu_batch = self.policy.act_mean(rb.obs, masks=rb.masks, hidden_states=one(rb.hid_a))
            sigma_batch = (self.policy.std if self.policy.noise_std_type == "scalar" else self.policy.log_std.exp()).expand_as(mu_batch)
            dist = torch.distributions.Normal(mu_batch, sigma_batch, validate_args=False)
            actions_log_prob_batch = dist.log_prob(cut(st.actions)).sum(dim=-1)
            value_batch = self.policy.evaluate(rb.critic_obs, masks=rb.masks, hidden_states=one(rb.hid_c)).squeeze(-1)
            entropy_batch = dist.entropy().sum(dim=-1)
            old_mu, old_sigma = cut(st.mu), cut(st.sigma)
            if self.desired_kl is not None and self.schedule == "adaptive":
                with torch.inference_mode():
                    kl = torch.sum(torch.log(sigma_batch / old_sigma + 1.0e-5)
                                   + (torch.square(old_sigma) + torch.square(old_mu - mu_batch)) / (2.0 * torch.square(sigma_batch)) - 0.5, axis=-1)
                    kl_mean = torch.mean(kl)
                    if kl_mean > self.desired_kl * 2.0:
                        self.learning_rate = max(1e-5, self.learning_rate / 1.5)
                    elif kl_mean < self.desired_kl / 2.0 and kl_mean > 0.0:
                        self.learning_rate = min(1e-2, self.learning_rate * 1.5)
                    for param_group in self.optimizer.param_groups:
                        param_group["lr"] = self.learning_rate
            advantages, returns, values = cut(st.advantages), cut(st.returns), cut(st.values)
            ratio = torch.exp(actions_log_prob_batch - cut(st.actions_log_prob))
            surrogate = -advantages * ratio
            surrogate_clipped = -advantages * torch.clamp(ratio, 1.0 - self.clip_param, 1.0 + self.clip_param)
            surrogate_loss = torch.max(surrogate, surrogate_clipped).mean()
            if self.use_clipped_value_loss:
                value_clipped = values + (value_batch - values).clamp(-self.clip_param, self.clip_param)
                value_loss = torch.max((value_batch - returns).pow(2), (value_clipped - returns).pow(2)).mean()
            else:
                value_loss = (returns - value_batch).pow(2).mean()
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
