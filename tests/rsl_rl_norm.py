"""rsl_rl's ``EmpiricalNormalization`` (rsl_rl/modules/normalizer.py) restated in plain torch: the yardstick of
``learner.EmpiricalNormalization``.  Statement for statement what rsl_rl does — the four buffers under its names, ``forward`` /
``inverse``, and ``update`` with its eval-mode and ``until`` tests."""
import torch
from torch import nn


class RslRlEmpiricalNormalization(nn.Module):
    def __init__(self, shape, eps=1e-2, until=None):
        super().__init__()
        self.eps = eps
        self.until = until
        self.register_buffer("_mean", torch.zeros(shape).unsqueeze(0))
        self.register_buffer("_var", torch.ones(shape).unsqueeze(0))
        self.register_buffer("_std", torch.ones(shape).unsqueeze(0))
        self.register_buffer("count", torch.tensor(0, dtype=torch.long))

    @property
    def mean(self):
        return self._mean.squeeze(0).clone()

    @property
    def std(self):
        return self._std.squeeze(0).clone()

    def forward(self, x):
        return (x - self._mean) / (self._std + self.eps)

    def update(self, x):
        if not self.training:
            return
        if self.until is not None and self.count >= self.until:
            return
        count_x = x.shape[0]
        self.count += count_x
        rate = count_x / self.count
        var_x = torch.var(x, dim=0, unbiased=False, keepdim=True)
        mean_x = torch.mean(x, dim=0, keepdim=True)
        delta_mean = mean_x - self._mean
        self._mean += rate * delta_mean
        self._var += rate * (var_x - self._var + delta_mean * (mean_x - self._mean))
        self._std = torch.sqrt(self._var)

    def inverse(self, y):
        return y * (self._std + self.eps) + self._mean
