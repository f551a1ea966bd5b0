#!/usr/bin/env python3
"""RayCaster.cast() — one gf_ray_cast launch — against the same float32 sequence composed from torch ops (the library's own fallback
for a backend without the entry, run on the GPU: every cell of the walk a round of masked tensor ops).

    python tools/bench_ray_cast.py [--n 4096 16384 65536] [--sensor cam16x12 cam32x24 lidar8x32] [--out profiles/r29_ray_cast.jsonl]
    python tools/bench_ray_cast.py --down [--n …]        # down_pattern 17 x 11 against gf_height_scan, for information
    python tools/bench_ray_cast.py --step [--n …]        # Go2RoughTerrainEnv steps with the depth item off and on

Per size, µs per call, each the median of `--batches` batches with the fastest and slowest batch beside it:
  * kernel: the dispatch's own begin / end timestamps (gf_profile_begin on GF_PHASE_TERRAIN), `--calls` casts per batch;
  * cast_events / torch_events: device events around a batch of back-to-back calls, divided by the calls — what a caller waits for
    (the composition syncs once per cell of the walk, so it gets `--torch-calls` calls per batch).
Alongside: rays per second, the mean and the largest number of cells a ray walks (the numpy restatement of tests/ray_cast_cases.py on
the first `--sample` envs), and the output's N·R·4 bytes over the kernel time against the 6.29 TB/s a float4 copy reaches on this GPU
(DESIGN.md).  One JSON line per row; needs a GPU."""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "genesis-forge_amd"))
sys.path.insert(0, os.path.join(ROOT, "tests"))

from bench_height_scan import event_batches, kernel_batches, spread   # noqa: E402

COPY_CEILING = 6.29e12


def sensor_kwargs(name):
    from genesis_forge_amd.managers.ray_caster import lidar_pattern, pinhole_pattern
    from genesis_forge_amd.tasks import Go2RoughTerrainEnv

    if name.startswith("cam"):
        w, h = (int(v) for v in name[3:].split("x"))
        return dict(Go2RoughTerrainEnv.DEPTH_CAMERA, pattern=pinhole_pattern(w, h, 87.0))
    if name.startswith("lidar"):
        c, a = (int(v) for v in name[5:].split("x"))
        return dict(pattern=lidar_pattern(c, (-25.0, 5.0), 360.0, 360.0 / a), offset_pos=(0.0, 0.0, 0.1), align="base", max_range=4.0)
    raise SystemExit(f"unknown sensor {name}")


def make_env(n, camera=None, scan=None):
    from genesis_forge_amd import tasks

    env = tasks.Go2RoughTerrainEnv(num_envs=n, height_reward=False, scene_kwargs=dict(ang_noise=0.05, seed=1234), depth_camera=camera,
                                   height_scan=scan)
    env.trace_enabled = True   # the recorded step: what a training loop runs
    env.build()
    env.seed(1234)
    env.reset()
    return env


def walk_stats(env, caster, pos, quat, sample):
    """(mean cells per ray that enters the field, largest, hit share) from the numpy restatement on the first `sample` envs."""
    import numpy as np
    import ray_cast_cases as rc

    tm = env.terrain_manager
    v = tm.gf_view()
    view = tuple(np.float32(x) for x in (v.x_min, v.x_span, v.y_min, v.y_span))
    res = rc.cast_f32(tm._height_field.cpu().numpy(), view, pos[:sample].cpu().numpy(), quat[:sample].cpu().numpy(),
                      caster.pattern.cpu().numpy(), rc.ALIGN[caster.align], caster.max_range)
    return float(res["cells"].mean()), int(res["cells"].max()), float(res["hit"].mean()), res


def bench_cast(args, emit):
    import torch
    from genesis_forge_amd import gs
    from genesis_forge_amd.managers import RayCaster

    for sensor in args.sensor:
        for n in args.n:
            env = make_env(n)
            acts = torch.zeros(n, 12, device=gs.device)
            for _ in range(5):
                env.step(acts)   # (poses off the spawn grid)
            # (a caster of its own, not an observation item: an observation frame holds at most 255 columns, a 32 x 24 image has 768)
            ca = RayCaster(env, env.terrain_manager, entity_manager=env.robot_manager, **sensor_kwargs(sensor))
            v = env.entity_views(ca.entity)
            pos, quat = v.pos, v.quat
            torch_out = torch.empty(n, ca.num_rays, device=gs.device)
            torch_cast = lambda: ca._cast_torch(pos, quat, torch_out, None)
            ref = torch_cast().clone()
            got = ca.cast(pos, quat)
            torch.cuda.synchronize()
            worst = float((got - ref).abs().max())   # (the composition's device sqrt / divide may round differently: not bit for bit)
            cells_mean, cells_max, hit_share, _ = walk_stats(env, ca, pos, quat, args.sample)
            for _ in range(20):
                ca.cast(pos, quat)
            torch.cuda.synchronize()
            kern = kernel_batches(env.backend, lambda: ca.cast(pos, quat), args.calls, args.batches)
            ev_cast = event_batches(lambda: ca.cast(pos, quat), args.calls, args.batches)
            ev_torch = event_batches(torch_cast, args.torch_calls, args.torch_batches) if args.torch_batches else {"median": float("nan")}
            nbytes = n * ca.num_rays * 4
            emit({"bench": "ray_cast", "sensor": sensor, "num_envs": n, "num_rays": ca.num_rays, "out_bytes": nbytes, "kernel_us": kern,
                  "cast_events_us": ev_cast, "torch_events_us": ev_torch, "torch_over_cast": ev_torch["median"] / ev_cast["median"],
                  "rays_per_s": n * ca.num_rays / (kern["median"] * 1e-6), "cells_per_ray_mean": cells_mean, "cells_per_ray_max": cells_max,
                  "hit_share": hit_share, "frac_copy_ceiling": nbytes / (kern["median"] * 1e-6) / COPY_CEILING,
                  "max_abs_diff_vs_torch": worst, "calls_per_batch": args.calls, "batches": args.batches,
                  "torch_calls_per_batch": args.torch_calls, "torch_batches": args.torch_batches, "label": args.label})
            del env


def bench_down(args, emit):
    """down_pattern 17 x 11 (align = yaw) against gf_height_scan on the same poses: the caster does more per point."""
    import torch
    from genesis_forge_amd import gs
    from genesis_forge_amd.managers import HeightScanner
    from genesis_forge_amd.managers.ray_caster import down_pattern

    for n in args.n:
        env = make_env(n, camera=dict(pattern=down_pattern((1.6, 1.0), 0.1, 0.5), offset_pos=(0.0, 0.0, 0.0), offset_euler=(0.0, 0.0, 0.0),
                                      align="yaw", max_range=2.0, output="distance"))
        acts = torch.zeros(n, 12, device=gs.device)
        for _ in range(5):
            env.step(acts)
        ca = env.depth_camera
        sc = HeightScanner(env, env.terrain_manager, entity_manager=env.robot_manager, offset=-0.5, clip=(-float("inf"), float("inf")))
        v = env.entity_views(ca.entity)
        pos, quat = v.pos, v.quat
        a, b = ca.cast(pos, quat), sc.scan(pos, quat)
        torch.cuda.synchronize()
        worst = float((a - b).abs()[(b >= 0) & (b < 2.0)].max())
        for _ in range(20):
            ca.cast(pos, quat)
            sc.scan(pos, quat)
        torch.cuda.synchronize()
        k_cast = kernel_batches(env.backend, lambda: ca.cast(pos, quat), args.calls, args.batches)
        k_scan = kernel_batches(env.backend, lambda: sc.scan(pos, quat), args.calls, args.batches)
        emit({"bench": "ray_cast_down_vs_height_scan", "num_envs": n, "num_rays": ca.num_rays, "ray_cast_kernel_us": k_cast,
              "height_scan_kernel_us": k_scan, "cast_over_scan": k_cast["median"] / k_scan["median"], "max_abs_diff_in_range": worst,
              "calls_per_batch": args.calls, "batches": args.batches})
        del env


def bench_step(args, emit):
    import torch
    from genesis_forge_amd import gs

    sensor = args.sensor[0]
    for n in args.n:
        row = {"bench": "ray_cast_step", "sensor": sensor, "num_envs": n, "steps_per_batch": args.steps, "batches": args.batches}
        for name, cam in (("off", None), ("on", sensor_kwargs(sensor))):
            env = make_env(n, camera=cam)
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
    ap.add_argument("--sensor", nargs="+", default=["cam16x12", "cam32x24", "lidar8x32"], help="camWxH (87 degrees, the env's default mount) or lidarCxA")
    ap.add_argument("--calls", type=int, default=50)
    ap.add_argument("--batches", type=int, default=15)
    ap.add_argument("--torch-calls", type=int, default=2)
    ap.add_argument("--torch-batches", type=int, default=5, help="0: do not time the composition")
    ap.add_argument("--sample", type=int, default=1024, help="envs the walk statistics are taken from")
    ap.add_argument("--steps", type=int, default=100)
    ap.add_argument("--down", action="store_true", help="down_pattern 17x11 against gf_height_scan")
    ap.add_argument("--step", action="store_true", help="whole steps of Go2RoughTerrainEnv with the depth item off and on")
    ap.add_argument("--label", default="", help="a note copied into every row (which build of the library was timed)")
    ap.add_argument("--out", default="")
    args = ap.parse_args()
    import torch
    from genesis_forge_amd import gs

    if not torch.cuda.is_available():
        sys.exit("bench_ray_cast needs a GPU: a CPU timing says nothing about the kernel")
    gs.set_device("cuda:0")
    sink = open(args.out, "a") if args.out else None

    def emit(row):
        line = json.dumps(row)
        print(line, flush=True)
        if sink:
            sink.write(line + "\n")
            sink.flush()

    (bench_step if args.step else bench_down if args.down else bench_cast)(args, emit)


if __name__ == "__main__":
    main()
