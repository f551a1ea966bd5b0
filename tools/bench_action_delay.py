#!/usr/bin/env python3
"""Actuator latency — one gf_action_delay launch per step — against what it replaces, and what the env's step pays for it.

    python tools/bench_action_delay.py [--n 4096 16384 65536] [--out profiles/r32_action_delay.jsonl]
    python tools/bench_action_delay.py --step [--n …]

Without --step, per size, µs per call at D = 12 (median of `--batches` batches, fastest and slowest beside it), 0.3 % of the envs
fresh per call (a mask, as the step's done envs would be; episode_length is bound and says nothing):
  * kernel_lag_0_2 / kernel_lag_0_7: the dispatch's own begin / end timestamps (gf_profile_begin on GF_PHASE_TERRAIN), `--calls`
    launches per batch, rings of 3 and 8 slots;
  * all_fresh_kernel: the 8-slot ring with every env fresh in every call (8 slot stores per lane: the most a launch can do);
  * step_events: device events around a batch of back-to-back ActuatorDelay.step() calls (the launch and its host-side descriptor);
  * torch_events: the same with use_kernel = False and the draws handed in from torch.rand inside the timed call — the sequence as
    a torch user would write it (slot write, gather, where, draw, scatter);
  * torch_philox_events: use_kernel = False as the library's fallback runs it, the Philox draw restated in int64 tensor ops.
With --step, µs per step of Go2RoughTerrainEnv in the timed `rough_terrain` config of tools/bench_configs.py (wall clock over `--steps`
steps, synchronised per batch) with action_delay={} and without, the two envs alive together and their batches alternating.
One JSON line per row; needs a GPU."""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "genesis-forge_amd"))

DT = 0.02
DOFS = 12


def spread(xs):
    xs = sorted(xs)
    return {"median": xs[len(xs) // 2], "min": xs[0], "max": xs[-1]}


def event_batches(fn, calls, batches):
    import torch

    out = []
    for _ in range(batches):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(calls):
            fn()
        b.record()
        b.synchronize()
        out.append(a.elapsed_time(b) * 1e3 / calls)
    return spread(out)


def kernel_batches(backend, fn, calls, batches):
    import torch
    from genesis_forge_amd import _native as nat

    out = []
    for _ in range(batches):
        backend.profile_begin(nat.GF_PHASE_TERRAIN, calls)
        for _ in range(calls):
            fn()
        torch.cuda.synchronize()
        total_ms, count = backend.profile_end()
        assert count == calls, (count, calls)
        out.append(total_ms * 1e3 / count)
    return spread(out)


class Host:
    """What an ActuatorDelay reads off its env."""

    def __init__(self, n, backend, dev):
        import torch

        self.num_envs, self.backend, self.dt, self._rng_seed, self.env_offset = n, backend, DT, 1234, 0
        self.episode_length = torch.full((n,), 50, device=dev, dtype=torch.int32)


def bench_launch(args, emit):
    import torch
    from genesis_forge_amd import _native as nat
    from genesis_forge_amd import gs
    from genesis_forge_amd.managers import ActuatorDelay

    backend = nat.get_backend()
    for n in args.n:
        host = Host(n, backend, gs.device)
        g = torch.Generator().manual_seed(0)
        x = torch.randn(n, DOFS, generator=g).to(gs.device)
        done = torch.rand(n, device=gs.device) < 0.003
        every = torch.ones(n, device=gs.device, dtype=torch.bool)
        row = {"bench": "action_delay_launch", "num_envs": n, "num_dofs": DOFS, "fresh": int(done.sum()), "calls_per_batch": args.calls,
               "batches": args.batches}

        def warm(call, k=10):
            for _ in range(k):
                call()
            torch.cuda.synchronize()

        for lo, hi in ((0, 2), (0, 7)):
            pd = ActuatorDelay(host, DOFS, lag_steps=(lo, hi))
            call = lambda pd=pd: pd.step(x, done)
            warm(call)
            row[f"kernel_lag_{lo}_{hi}_us"] = kernel_batches(backend, call, args.calls, args.batches)
            row[f"mean_lag_{lo}_{hi}"] = float(pd.lag.float().mean())
        call = lambda: pd.step(x, every)                                  # (the 8-slot ring)
        warm(call)
        row["all_fresh_kernel_us"] = kernel_batches(backend, call, args.calls, args.batches)

        pd = ActuatorDelay(host, DOFS, lag_steps=(0, 2))
        call = lambda: pd.step(x, done)
        warm(call)
        row["step_events_us"] = event_batches(call, args.calls, args.batches)
        pd.use_kernel = False
        u = [None]

        def torch_form():
            u[0] = torch.rand(n, device=gs.device)                        # (a new tensor per call: bound again, as the kernel path's is not)
            pd.step(x, done, draws=u[0])

        warm(torch_form, 5)
        row["torch_events_us"] = event_batches(torch_form, max(1, args.calls // 5), args.batches)
        row["torch_over_step"] = row["torch_events_us"]["median"] / row["step_events_us"]["median"]
        warm(call, 3)
        row["torch_philox_events_us"] = event_batches(call, max(1, args.calls // 10), max(3, args.batches // 3))
        emit(row)


def make_env(n, delay):
    from genesis_forge_amd import tasks

    kw = {"action_delay": {}} if delay else {}
    env = tasks.BASELINE_CONFIGS["rough_terrain"][1](n, **kw)     # the timed rough_terrain config of tools/bench_configs.py
    env.trace_enabled = True
    env.build()
    env.seed(1234)
    env.reset()
    return env


def bench_step(args, emit):
    import torch
    from genesis_forge_amd import gs

    for n in args.n:
        row = {"bench": "action_delay_step", "num_envs": n, "steps_per_batch": args.steps, "batches": args.batches}
        envs = {"delay": make_env(n, True), "stock": make_env(n, False)}
        g = torch.Generator().manual_seed(0)
        acts = [torch.randn(n, 12, generator=g).to(gs.device) for _ in range(8)]
        for env in envs.values():
            for i in range(args.warmup):
                env.step(acts[i % 8])
        out = {k: [] for k in envs}
        for _ in range(args.batches):
            for arm, env in envs.items():          # alternating: both arms see the same machine
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                for i in range(args.steps):
                    env.step(acts[i % 8])
                torch.cuda.synchronize()
                out[arm].append((time.perf_counter() - t0) / args.steps * 1e6)
        for arm, env in envs.items():
            row[f"us_per_step_{arm}"] = spread(out[arm])
            row[f"recorded_{arm}"] = env._trace is not None
        row["mean_lag"] = float(envs["delay"].action_delay.lag.float().mean())
        row["delay_minus_stock_us"] = row["us_per_step_delay"]["median"] - row["us_per_step_stock"]["median"]
        emit(row)
        del envs


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, nargs="+", default=[4096, 16384, 65536])
    ap.add_argument("--calls", type=int, default=50)
    ap.add_argument("--batches", type=int, default=15)
    ap.add_argument("--steps", type=int, default=100)
    ap.add_argument("--warmup", type=int, default=100)
    ap.add_argument("--step", action="store_true", help="whole steps of Go2RoughTerrainEnv with and without action_delay=")
    ap.add_argument("--out", default="")
    args = ap.parse_args()
    os.environ.setdefault("GF_JIT", "sync")   # as tools/bench_configs.py: the config is timed on its compiled program
    import torch
    from genesis_forge_amd import gs

    if not torch.cuda.is_available():
        sys.exit("bench_action_delay needs a GPU: a CPU timing says nothing about the kernel")
    gs.set_device("cuda:0")
    sink = open(args.out, "a") if args.out else None

    def emit(row):
        line = json.dumps(row)
        print(line, flush=True)
        if sink:
            sink.write(line + "\n")
            sink.flush()

    (bench_step if args.step else bench_launch)(args, emit)


if __name__ == "__main__":
    main()
