#!/usr/bin/env python3
"""HeightScanner.scan() — one gf_height_scan launch — against the scan composed from TerrainManager.get_terrain_height in torch.

    python tools/bench_height_scan.py [--n 4096 16384 65536] [--grid 17x11 11x11] [--out profiles/r28_height_scan.jsonl]
    python tools/bench_height_scan.py --step [--n …]        # Go2RoughTerrainEnv steps with the height_scan item off and on

Per size, µs per call, each the median of `--batches` batches with the fastest and slowest batch beside it:
  * kernel: the dispatch's own begin / end timestamps (gf_profile_begin on GF_PHASE_TERRAIN), `--calls` scans per batch;
  * scan_events / torch_events: device events around a batch of back-to-back calls, divided by the calls — what a caller waits for;
    the composition is about fifteen launches, so at small N this is its launch rate, not its traffic.
The output is N·P·4 bytes; `frac_hbm_peak` / `frac_copy_ceiling` are those bytes over the kernel time against 8 TB/s and against the
6.29 TB/s a float4 copy reaches on this GPU.  One JSON line per row; needs a GPU."""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "genesis-forge_amd"))

HBM_PEAK, COPY_CEILING = 8.0e12, 6.29e12


def torch_scan(tm, pattern, pos, quat, offset, lo, hi):
    """What a user writes today: broadcast the pattern, rotate it by the yaw in elementwise ops, one get_terrain_height over N·P
    points, subtract and clamp."""
    import torch

    qw, qx, qy, qz = quat[:, 0:1], quat[:, 1:2], quat[:, 2:3], quat[:, 3:4]
    c = 1.0 - 2.0 * (qy * qy + qz * qz)
    s = 2.0 * (qw * qz + qx * qy)
    nrm = torch.sqrt(c * c + s * s)
    flat = nrm < 1e-6
    cy = torch.where(flat, torch.ones_like(c), c / nrm)
    sy = torch.where(flat, torch.zeros_like(s), s / nrm)
    ox, oy = pattern[:, 0].unsqueeze(0), pattern[:, 1].unsqueeze(0)
    px = pos[:, 0:1] + (cy * ox - sy * oy)
    py = pos[:, 1:2] + (sy * ox + cy * oy)
    h = tm.get_terrain_height(px.reshape(-1), py.reshape(-1)).view(px.shape)
    return torch.clamp((pos[:, 2:3] - offset) - h, min=lo, max=hi)


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
    from genesis_forge_amd import _native as nat
    import torch

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


def make_env(n, grid, scan=True):
    from genesis_forge_amd import tasks

    nx, ny = grid
    hs = {"size": (0.1 * (nx - 1), 0.1 * (ny - 1)), "resolution": 0.1} if scan else None
    env = tasks.Go2RoughTerrainEnv(num_envs=n, height_reward=False, scene_kwargs=dict(ang_noise=0.05, seed=1234), height_scan=hs)
    env.trace_enabled = True   # the recorded step: what a training loop runs
    env.build()
    env.seed(1234)
    env.reset()
    return env


def bench_scan(args, emit):
    import torch
    from genesis_forge_amd import gs

    for grid in args.grid:
        for n in args.n:
            env = make_env(n, grid)
            acts = torch.zeros(n, 12, device=gs.device)
            for _ in range(5):
                env.step(acts)   # (poses off the spawn grid)
            sc, tm = env.height_scanner, env.terrain_manager
            v = env.entity_views(sc.entity)
            pos, quat = v.pos, v.quat
            ref = torch_scan(tm, sc.pattern, pos, quat, sc.offset, *sc.clip)
            got = sc.scan(pos, quat)
            torch.cuda.synchronize()
            worst = float((got - ref).abs().max())   # (the composition's device sqrt / divide may round differently: not bit for bit)
            for _ in range(20):
                sc.scan(pos, quat)
                torch_scan(tm, sc.pattern, pos, quat, sc.offset, *sc.clip)
            torch.cuda.synchronize()
            kern = kernel_batches(env.backend, lambda: sc.scan(pos, quat), args.calls, args.batches)
            ev_scan = event_batches(lambda: sc.scan(pos, quat), args.calls, args.batches)
            ev_torch = event_batches(lambda: torch_scan(tm, sc.pattern, pos, quat, sc.offset, *sc.clip), args.calls, args.batches)
            nbytes = n * sc.num_points * 4
            emit({"bench": "height_scan", "num_envs": n, "num_points": sc.num_points, "out_bytes": nbytes, "kernel_us": kern,
                  "scan_events_us": ev_scan, "torch_events_us": ev_torch, "torch_over_scan": ev_torch["median"] / ev_scan["median"],
                  "frac_hbm_peak": nbytes / (kern["median"] * 1e-6) / HBM_PEAK, "frac_copy_ceiling": nbytes / (kern["median"] * 1e-6) / COPY_CEILING,
                  "max_abs_diff_vs_torch": worst, "calls_per_batch": args.calls, "batches": args.batches})
            del env


def bench_step(args, emit):
    import torch
    from genesis_forge_amd import gs

    grid = args.grid[0]
    for n in args.n:
        row = {"bench": "height_scan_step", "num_envs": n, "num_points": grid[0] * grid[1], "steps_per_batch": args.steps, "batches": args.batches}
        for name, scan in (("off", False), ("on", True)):
            env = make_env(n, grid, scan)
            g = torch.Generator().manual_seed(0)
            acts = [torch.randn(n, 12, generator=g).to(gs.device) for _ in range(8)]
            for i in range(30):
                env.step(acts[i % 8])
            out = []
            for _ in range(args.batches):
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                for i in range(args.steps):
                    env.step(acts[i % 8])
                torch.cuda.synchronize()
                out.append((time.perf_counter() - t0) / args.steps * 1e6)
            row[f"us_per_step_{name}"] = spread(out)
            row[f"recorded_{name}"] = env._trace is not None
            del env
        row["item_cost_us"] = row["us_per_step_on"]["median"] - row["us_per_step_off"]["median"]
        emit(row)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, nargs="+", default=[4096, 16384, 65536])
    ap.add_argument("--grid", nargs="+", default=["17x11"], help="points along x and y at 0.1 m: 17x11 = the default 187, 11x11 = 121")
    ap.add_argument("--calls", type=int, default=50)
    ap.add_argument("--batches", type=int, default=15)
    ap.add_argument("--steps", type=int, default=100)
    ap.add_argument("--step", action="store_true", help="whole steps of Go2RoughTerrainEnv with the item off and on")
    ap.add_argument("--out", default="")
    args = ap.parse_args()
    args.grid = [tuple(int(v) for v in g.split("x")) for g in args.grid]
    import torch
    from genesis_forge_amd import gs

    if not torch.cuda.is_available():
        sys.exit("bench_height_scan needs a GPU: a CPU timing says nothing about the kernel")
    gs.set_device("cuda:0")
    sink = open(args.out, "a") if args.out else None

    def emit(row):
        line = json.dumps(row)
        print(line, flush=True)
        if sink:
            sink.write(line + "\n")
            sink.flush()

    (bench_step if args.step else bench_scan)(args, emit)


if __name__ == "__main__":
    main()
