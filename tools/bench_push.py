#!/usr/bin/env python3
"""The random pushes — one gf_push launch per step — against what they replace, and what the env's step pays for them.

    python tools/bench_push.py [--n 4096 16384 65536] [--out profiles/r31_push.jsonl]
    python tools/bench_push.py --step [--n …]

Without --step, per size, µs per call (median of `--batches` batches, fastest and slowest beside it), with the default 10-15 s interval
at 50 Hz (500-750 steps: about one env in 625 is due per step, the timers spread as they are in a long run) and 0.3 % of the envs done:
  * kernel: the dispatch's own begin / end timestamps (gf_profile_begin on GF_PHASE_TERRAIN), `--calls` launches per batch;
  * launch_events: device events around a batch of back-to-back PushDisturbance.step() calls (the launch and its host-side descriptor);
  * torch_events: the same event with use_kernel = False — the library's own float32 sequence as separate torch ops;
  * all_due_*: kernel and launch_events with an interval of one step (every env is pushed in every call: the most a launch can do);
  * global_events: PushDisturbance(per_env=False).step(), one timer for all envs;
  * legged_gym_push_events: legged_gym's global form in torch on a push step, `root_vel[:, :2] = rand` (torch.rand, scale, shift,
    assign), and legged_gym_idle_events: its other steps, `if step % k == 0` on the host and nothing on the device.
With --step, µs per step of Go2RoughTerrainEnv in the timed `rough_terrain` config of tools/bench_configs.py (wall clock over `--steps`
steps, synchronised per batch) with push={} and without, the two envs alive together and their batches alternating.
One JSON line per row; needs a GPU."""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "genesis-forge_amd"))

DT = 0.02


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


class Base:
    """Base velocities with masked setters: what the synthetic scene's entity hands to the launch."""

    def __init__(self, n, dev):
        import torch

        self.lin_vel, self.ang_vel = torch.zeros(n, 3, device=dev), torch.zeros(n, 3, device=dev)

    def gf_masked_base(self):
        return None, None, self.lin_vel, self.ang_vel


class Host:
    """What a PushDisturbance reads off its env."""

    def __init__(self, n, backend, dev):
        self.num_envs, self.backend, self.dt, self._rng_seed, self.env_offset = n, backend, DT, 1234, 0
        self.robot = Base(n, dev)


def spread_timers(pd):
    """Timers as a long run leaves them: uniform over the next mean interval."""
    import torch

    mean = (pd.interval_lo + pd.interval_hi) // 2
    pd.due.copy_((pd._step + 1 + torch.randint(0, mean, (pd.env.num_envs,))).to(torch.int32))


def bench_launch(args, emit):
    import torch
    from genesis_forge_amd import _native as nat
    from genesis_forge_amd import gs
    from genesis_forge_amd.managers import PushDisturbance

    backend = nat.get_backend()
    for n in args.n:
        host = Host(n, backend, gs.device)
        done = torch.rand(n, device=gs.device) < 0.003
        none = torch.zeros(n, device=gs.device, dtype=torch.bool)
        row = {"bench": "push_launch", "num_envs": n, "done": int(done.sum()), "calls_per_batch": args.calls, "batches": args.batches}

        pd = PushDisturbance(host)
        pd.build()
        row["interval_steps"] = [pd.interval_lo, pd.interval_hi]
        call = lambda: pd.step(done, none)
        spread_timers(pd)
        for _ in range(10):
            call()
        c0 = pd.read_counts()
        row["kernel_us"] = kernel_batches(backend, call, args.calls, args.batches)
        row["launch_events_us"] = event_batches(call, args.calls, args.batches)
        row["pushed_per_call"] = (pd.read_counts() - c0) / (2 * args.calls * args.batches)
        pd.use_kernel = False
        for _ in range(5):
            call()
        torch.cuda.synchronize()
        row["torch_events_us"] = event_batches(call, max(1, args.calls // 5), args.batches)
        row["torch_over_launch"] = row["torch_events_us"]["median"] / row["launch_events_us"]["median"]

        every = PushDisturbance(host, interval_s=(DT, DT))
        every.build()
        call = lambda: every.step(done, none)
        for _ in range(10):
            call()
        row["all_due_kernel_us"] = kernel_batches(backend, call, args.calls, args.batches)
        row["all_due_launch_events_us"] = event_batches(call, args.calls, args.batches)

        glob = PushDisturbance(host, per_env=False)
        glob.build()
        call = lambda: glob.step()
        for _ in range(10):
            call()
        row["global_events_us"] = event_batches(call, args.calls, args.batches)

        root_vel = torch.zeros(n, 6, device=gs.device)
        k = (pd.interval_lo + pd.interval_hi) // 2
        state = {"step": 0}

        def legged_gym(k):
            state["step"] += 1
            if state["step"] % k == 0:
                root_vel[:, :2] = torch.rand(n, 2, device=gs.device) * 1.0 - 0.5      # torch_rand_float(-max_vel, max_vel, (N, 2))

        for _ in range(10):
            legged_gym(1)
        torch.cuda.synchronize()
        row["legged_gym_push_events_us"] = event_batches(lambda: legged_gym(1), args.calls, args.batches)
        row["legged_gym_idle_events_us"] = event_batches(lambda: legged_gym(1 << 40), args.calls, args.batches)
        row["legged_gym_amortised_us"] = row["legged_gym_push_events_us"]["median"] / k
        emit(row)


def make_env(n, push):
    from genesis_forge_amd import tasks

    env = tasks.BASELINE_CONFIGS["rough_terrain"][1](n, push={} if push else None)     # the timed rough_terrain config of tools/bench_configs.py
    env.trace_enabled = True
    env.build()
    env.seed(1234)
    env.reset()
    if push:
        spread_timers(env.push)
    return env


def bench_step(args, emit):
    import torch
    from genesis_forge_amd import gs

    for n in args.n:
        row = {"bench": "push_step", "num_envs": n, "steps_per_batch": args.steps, "batches": args.batches}
        envs = {"push": make_env(n, True), "stock": make_env(n, False)}
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
        row["pushes"] = envs["push"].push.read_counts()
        row["push_minus_stock_us"] = row["us_per_step_push"]["median"] - row["us_per_step_stock"]["median"]
        emit(row)
        del envs


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, nargs="+", default=[4096, 16384, 65536])
    ap.add_argument("--calls", type=int, default=50)
    ap.add_argument("--batches", type=int, default=15)
    ap.add_argument("--steps", type=int, default=100)
    ap.add_argument("--warmup", type=int, default=100)
    ap.add_argument("--step", action="store_true", help="whole steps of Go2RoughTerrainEnv with and without push=")
    ap.add_argument("--out", default="")
    args = ap.parse_args()
    os.environ.setdefault("GF_JIT", "sync")   # as tools/bench_configs.py: the config is timed on its compiled program
    import torch
    from genesis_forge_amd import gs

    if not torch.cuda.is_available():
        sys.exit("bench_push needs a GPU: a CPU timing says nothing about the kernel")
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
