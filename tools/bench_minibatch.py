"""PPO minibatches of a filled RolloutStorage: one gf_minibatch_gather launch per minibatch against rsl_rl's per-field torch indexing.

usage: python tools/bench_minibatch.py --num-envs 65536 --steps 24 --mini-batches 4 [--obs-width 48] [--critic-width 0]
                                       [--num-actions 12] [--epochs 5] [--repeats 20] [--history-len 1] [--history rows|frames]

The storage is filled with random rows; no env is stepped (only the buffers matter).  ``--critic-width W`` adds a second
observation-group member of W floats and the gait trainer's groups ({"policy": ["policy"], "critic": ["policy", "critic"]}).
``--history-len H --history frames``: the observations are histories of H frames (the widths are the rows': H·O, the gait trainer's
are 390 and 80 with H = 5) kept once per frame — ``RolloutStorage(history="frames")`` — and the gather rebuilds the rows from
synthetic frames; ``--history rows`` gathers the same minibatches from stored rows.  The torch path indexes materialised rows either way.
Both paths are timed with HIP events over ``--repeats`` generator calls of ``--epochs`` epochs (after one warm-up call) and
checked equal bit for bit.  Prints one JSON line: µs per minibatch of each path, the bytes one minibatch moves (the gathered
rows read + written, plus the indices) and that over each path's time as a fraction of 8 TB/s."""
import argparse
import json
import os
import sys
from types import SimpleNamespace

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "genesis-forge_amd"))

import torch  # noqa: E402

PEAK = 8.0e12   # B/s, MI355X HBM


class _Obs(SimpleNamespace):
    """What RolloutStorage reads of an ObservationManager when no step runs."""


def storage(n, T, obs_w, critic_w, A, history_len=1, history="rows"):
    from genesis_forge_amd import _native as nat
    from genesis_forge_amd.learner import RolloutStorage

    mk = lambda name, w: _Obs(name=name, observation_space=SimpleNamespace(shape=(w,)), output="fresh", _history_len=history_len, _unrolled=False)
    mgrs = [mk("policy", obs_w)] + ([mk("critic", critic_w)] if critic_w else [])
    env = SimpleNamespace(num_envs=n, managers={"observation": mgrs}, backend=nat.get_backend())
    groups = {"policy": ["policy"], "critic": ["policy", "critic"]} if critic_w else None
    st = RolloutStorage(env, T, obs_groups=groups, history=history)
    st._ensure_policy_rows(A)
    g = torch.Generator(device="cuda").manual_seed(0)
    obs = [] if st.observations is None else [st.observations]
    for t in [*obs, *st.group_rows.values(), *st.frames.values(), st.actions, st.values, st.advantages, st.returns, st.actions_log_prob, st.mu, st.sigma]:
        t.copy_(torch.randn(t.shape, device="cuda", generator=g))
    st._returns_ready = True
    return st


def torch_sources(st):
    """rsl_rl's flattened [T·N, …] arrays.  Its storage keeps the critic input as one buffer (privileged_observations), already
    concatenated when it was stored: built once here, outside the timed region, so the torch path pays one index per field."""
    T = st.num_steps
    names = {m for members in st.obs_groups.values() for m in members}
    flat = {k: st.observation_rows(k)[:T].flatten(0, 1) for k in names}   # (a frame-stored manager: its rows, materialised once)
    obs = flat["policy"]
    critic = torch.cat([flat[k] for k in st.obs_groups["critic"]], dim=-1) if st.obs_groups["critic"] != st.obs_groups["policy"] else None
    rest = [x.flatten(0, 1) for x in (st.actions, st.values, st.advantages, st.returns, st.actions_log_prob, st.mu, st.sigma)]
    return obs, critic, rest


def torch_batches(src, indices, num_mini_batches, num_epochs):
    obs, critic, rest = src
    mb = indices.numel() // num_mini_batches
    for _ in range(num_epochs):
        for i in range(num_mini_batches):
            b = indices[i * mb:(i + 1) * mb]
            o = obs[b]
            yield (o, o if critic is None else critic[b], *(x[b] for x in rest))


def timed(fn, repeats):
    fn()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(repeats):
        fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1) * 1e3 / repeats   # µs per call


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--num-envs", type=int, default=65536)
    ap.add_argument("--steps", type=int, default=24)
    ap.add_argument("--mini-batches", type=int, default=4)
    ap.add_argument("--epochs", type=int, default=5)
    ap.add_argument("--obs-width", type=int, default=48)
    ap.add_argument("--critic-width", type=int, default=0)
    ap.add_argument("--num-actions", type=int, default=12)
    ap.add_argument("--repeats", type=int, default=20)
    ap.add_argument("--history-len", type=int, default=1, help="H: the observation widths are H frames side by side")
    ap.add_argument("--history", default="rows", choices=["rows", "frames"], help="RolloutStorage(history=)")
    a = ap.parse_args()
    if a.history_len < 1 or a.obs_width % a.history_len or a.critic_width % a.history_len:
        raise SystemExit("--history-len must divide --obs-width and --critic-width")
    if not torch.cuda.is_available():
        raise SystemExit("bench_minibatch: no ROCm device (this tool measures the GPU only)")
    from genesis_forge_amd import gs

    gs.set_device("cuda:0")
    st = storage(a.num_envs, a.steps, a.obs_width, a.critic_width, a.num_actions, a.history_len, a.history)
    nmb, ep = a.mini_batches, a.epochs
    mb = a.num_envs * a.steps // nmb
    gen = torch.Generator(device="cuda").manual_seed(1)
    idx = torch.randperm(nmb * mb, device="cuda", generator=gen)
    src = torch_sources(st)
    # correctness first: every field of every minibatch of one epoch, HIP against torch
    for got, want in zip(st._mini_batches(idx, nmb, 1, mb), torch_batches(src, idx, nmb, 1)):
        for x, y in zip(got, want):
            assert torch.equal(x, y), "gf_minibatch_gather differs from torch indexing"

    def hip_call():
        for _b in st._mini_batches(idx, nmb, ep, mb):   # (a PPO update drops each batch before it draws the next)
            pass

    def torch_call():
        for _b in torch_batches(src, idx, nmb, ep):
            pass

    hip_us = timed(hip_call, a.repeats) / (nmb * ep)
    torch_us = timed(torch_call, a.repeats) / (nmb * ep)
    critic = a.obs_width + a.critic_width if a.critic_width else 0
    row_floats = a.obs_width + critic + 3 * a.num_actions + 4
    nbytes = mb * (row_floats * 4 * 2 + 8)
    print(json.dumps({"num_envs": a.num_envs, "steps": a.steps, "mini_batches": nmb, "epochs": ep, "rows_per_minibatch": mb,
                      "obs_width": a.obs_width, "critic_width": critic, "num_actions": a.num_actions,
                      "history_len": a.history_len, "history": a.history if st.frames else "rows",
                      "bytes_per_minibatch": nbytes, "hip_us_per_minibatch": round(hip_us, 2), "torch_us_per_minibatch": round(torch_us, 2),
                      "hip_frac_of_8TBps": round(nbytes / (hip_us * 1e-6) / PEAK, 3),
                      "torch_frac_of_8TBps": round(nbytes / (torch_us * 1e-6) / PEAK, 3),
                      "speedup": round(torch_us / hip_us, 2), "device": torch.cuda.get_device_name(0)}))


if __name__ == "__main__":
    main()
