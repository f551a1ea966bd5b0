#!/usr/bin/env python3
"""DepthCamera.step() — one gf_depth_camera launch — against what it replaces, in one process on the same poses.

    python tools/bench_depth_camera.py [--n 4096 16384 65536] [--sensor cam16x12 cam32x24] [--out profiles/r36_depth_camera.jsonl]
    python tools/bench_depth_camera.py --step [--n …]     # Go2RoughTerrainEnv steps without and with depth_camera["model"]

Per sensor and size, µs per call, each the median of `--batches` batches with the fastest and slowest batch beside it:
  * cast_kernel: RayCaster.cast() on every env, the parent's path every step (the dispatch's own timestamps, gf_profile_begin on
    GF_PHASE_TERRAIN, `--calls` calls per batch);
  * camera_kernel[i<interval>_<phase>]: the new launch with stack 2 and latency (0, 2), interval 1 and 5, staggered and global — a
    batch of `--calls` calls covers whole intervals, so the global phase's empty launches are in the mean as often as they occur;
  * torch_events: the same model composed from torch ops around caster.cast() (DepthCamera.use_kernel = False on the GPU: gather the
    due rows, cast them, the pixel operations, the ring indexing), device events around `--torch-calls` back-to-back calls.
Every camera row carries its ratio to cast_kernel of the same process.  One JSON line per row; needs a GPU."""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "genesis-forge_amd"))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from bench_height_scan import event_batches, kernel_batches, spread   # noqa: E402
from bench_ray_cast import make_env, sensor_kwargs                    # noqa: E402

MODEL = dict(stack=2, latency=(0, 2), noise=0.02, dropout=0.01, normalize=True)
CONFIGS = [(1, "staggered"), (5, "staggered"), (5, "global")]


def bench_camera(args, emit):
    import torch
    from genesis_forge_amd import _native as nat
    from genesis_forge_amd import gs
    from genesis_forge_amd.managers import DepthCamera, RayCaster

    for sensor in args.sensor:
        for n in args.n:
            env = make_env(n)
            acts = torch.zeros(n, 12, device=gs.device)
            for _ in range(5):
                env.step(acts)   # (poses off the spawn grid; episode_length 5: nobody is fresh while the camera is timed)
            ca = RayCaster(env, env.terrain_manager, entity_manager=env.robot_manager, **sensor_kwargs(sensor))
            v = env.entity_views(ca.entity)
            pos, quat = v.pos, v.quat
            for _ in range(20):
                ca.cast(pos, quat)
            torch.cuda.synchronize()
            cast = kernel_batches(env.backend, lambda: ca.cast(pos, quat), args.calls, args.batches)
            row = {"bench": "depth_camera", "sensor": sensor, "num_envs": n, "num_rays": ca.num_rays, "model": repr(MODEL),
                   "span_envs": nat.GF_DEPTH_CAMERA_SPAN_ENVS, "cast_kernel_us": cast,
                   "calls_per_batch": args.calls, "batches": args.batches, "label": args.label}
            for interval, phase in CONFIGS:
                cam = DepthCamera(ca, interval=interval, phase=phase, **MODEL)
                step = lambda: cam.step(pos, quat)
                for _ in range(4 * interval):
                    step()
                torch.cuda.synchronize()
                kern = kernel_batches(env.backend, step, args.calls, args.batches)
                key = f"i{interval}_{phase}"
                row[f"camera_kernel_us_{key}"] = kern
                row[f"camera_over_cast_{key}"] = kern["median"] / cast["median"]
                if args.torch_batches:
                    cam.use_kernel = False
                    step()
                    torch.cuda.synchronize()
                    ev = event_batches(step, args.torch_calls, args.torch_batches)
                    row[f"torch_events_us_{key}"] = ev
                    row[f"torch_over_camera_{key}"] = ev["median"] / kern["median"]
                del cam
            emit(row)
            del env


def bench_step(args, emit):
    import torch
    from genesis_forge_amd import gs

    sensor = args.sensor[0]
    for n in args.n:
        row = {"bench": "depth_camera_step", "sensor": sensor, "num_envs": n, "steps_per_batch": args.steps, "batches": args.batches,
               "label": args.label}
        cam = sensor_kwargs(sensor)
        for name, dc in (("none", None), ("cast", cam), ("model", dict(cam, model=dict(interval=5, latency=(0, 2), noise=0.02, dropout=0.01)))):
            env = make_env(n, camera=dc)
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
        emit(row)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, nargs="+", default=[4096, 16384, 65536])
    ap.add_argument("--sensor", nargs="+", default=["cam16x12", "cam32x24"], help="camWxH: 87 degrees, the env's default mount")
    ap.add_argument("--calls", type=int, default=50, help="calls per batch: a multiple of the intervals timed")
    ap.add_argument("--batches", type=int, default=15)
    ap.add_argument("--torch-calls", type=int, default=10)
    ap.add_argument("--torch-batches", type=int, default=5, help="0: do not time the composition")
    ap.add_argument("--steps", type=int, default=100)
    ap.add_argument("--step", action="store_true", help="whole steps of Go2RoughTerrainEnv: no sensor, a cast per step, the camera model")
    ap.add_argument("--label", default="", help="a note copied into every row (which build of the library was timed)")
    ap.add_argument("--out", default="")
    args = ap.parse_args()
    import torch
    from genesis_forge_amd import gs

    if not torch.cuda.is_available():
        sys.exit("bench_depth_camera needs a GPU: a CPU timing says nothing about the kernel")
    gs.set_device("cuda:0")
    sink = open(args.out, "a") if args.out else None

    def emit(row):
        line = json.dumps(row)
        print(line, flush=True)
        if sink:
            sink.write(line + "\n")
            sink.flush()

    (bench_step if args.step else bench_camera)(args, emit)


if __name__ == "__main__":
    main()
