"""Host cost of the four one-launch collection steps without a GPU: the Python that fills the descriptor, up to the launch.

usage: python tools/bench_act_stub.py [--calls 20000] [--envs 4096]

A stub backend whose entries return at once stands in for the library (as tests/test_act_descriptors.py), every tensor is a CPU
tensor; the policies are the reference's 512-256-128 MLPs with a 256-unit LSTM where recurrent.  Times ``--calls`` calls each of
``RolloutStorage.act_policy``, ``act_recurrent``, ``act_distill`` and ``act_distill_recurrent`` and prints one JSON line: µs per call
over all calls, and over the fastest batch of 200.
A proxy — the launch itself is left out — for comparing two trees: run it from each tree's own ``tools/``, alternating."""
import argparse
import json
import os
import sys
import time
from types import SimpleNamespace

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "genesis-forge_amd"))
os.environ.setdefault("GF_DEVICE", "cpu")

import torch  # noqa: E402

from genesis_forge_amd import _native as nat  # noqa: E402
from genesis_forge_amd import learner as L  # noqa: E402

OBS, COBS, A, HIDDEN, RNN_HIDDEN, T = 48, 235, 12, (512, 256, 128), 256, 24
BATCH = 200   # calls between two reads of the clock


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=20000)
    ap.add_argument("--envs", type=int, default=4096)
    a = ap.parse_args()
    n = a.envs
    stub = SimpleNamespace(**{name: (lambda args: None) for name in ("mlp_act", "mlp_recurrent_act", "mlp_distill_act", "mlp_recurrent_distill_act")})
    nat.set_backend(stub)
    om = SimpleNamespace(name="policy", observation_space=SimpleNamespace(shape=(OBS,)), _history_len=1, output="fresh")
    env = SimpleNamespace(num_envs=n, managers={"observation": [om]}, backend=stub, _rng_seed=1, env_offset=0)
    x, cx = torch.randn(n, OBS), torch.randn(n, COBS)
    paths = {
        "act_policy": (L.PolicyForward(L.ActorCriticMLP(OBS, A, HIDDEN, HIDDEN, num_critic_obs=COBS)), "act_policy"),
        "act_recurrent": (L.RecurrentForward(L.ActorCriticRecurrent(OBS, A, HIDDEN, HIDDEN, num_critic_obs=COBS, rnn_hidden_dim=RNN_HIDDEN)), "act_recurrent"),
        "act_distill": (L.DistillForward(L.StudentTeacherMLP(OBS, COBS, A, HIDDEN, HIDDEN)), "act_distill"),
        "act_distill_recurrent": (L.RecurrentDistillForward(L.StudentTeacherRecurrent(OBS, COBS, A, HIDDEN, HIDDEN, rnn_hidden_dim=RNN_HIDDEN)),
                                  "act_distill_recurrent"),
    }
    out = {"calls": a.calls, "envs": n}
    for name, (fwd, method) in paths.items():
        store = L.RolloutStorage(env, T)
        store.step = 1   # (a row in the middle of a rollout: the rollout-start state is saved once per T steps)
        step = getattr(store, method)
        for _ in range(200):
            step(fwd, x, cx)
        batches = []
        for _ in range(a.calls // BATCH):
            t0 = time.perf_counter()
            for _ in range(BATCH):
                step(fwd, x, cx)
            batches.append((time.perf_counter() - t0) / BATCH * 1e6)
        out[name + "_us"] = round(sum(batches) / len(batches), 3)
        out[name + "_best_us"] = round(min(batches), 3)   # the fastest batch: what a busy machine disturbs least
    print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
