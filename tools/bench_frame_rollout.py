#!/usr/bin/env python3
"""Row-stored against frame-stored rollouts (``RolloutStorage(history=)``) on the gait trainer, the forms of one measurement built in
ONE process and alternated batch by batch (profiles/r17_frame_rollout.md).  One JSON line per (measurement, size, form): every
batch, their median and 3 x MAD.

* ``collect``: a collection step, ``bench_collect.collector(n, "fused_mlp", config="gait")`` with ``rows`` + ``fresh``, ``frames`` +
  ``fresh`` and ``frames`` + ``window``; µs per step over batches of ``--steps`` steps that end in a device synchronise.
* ``gather``: ``gf_minibatch_gather`` through ``RolloutStorage._mini_batches`` (4 minibatches x 5 epochs per call, HIP events) on
  ``bench_minibatch.storage`` stand-ins of ``--widths P,C`` (row widths of the policy and the critic manager, history_len 5) holding
  the same observations as rows and as frames; every minibatch is compared bit-equal first.
* ``storage``: ``torch.cuda.memory_allocated`` around the construction of each storage form alone.

    python tools/bench_frame_rollout.py [--measure collect,gather,storage] [--sizes 8192,65536] [--rounds 9] [--steps 120] [--widths 310,80]"""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "genesis-forge_amd"))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import torch  # noqa: E402

import bench_collect as bc  # noqa: E402
import bench_minibatch as bm  # noqa: E402
from genesis_forge_amd import gs  # noqa: E402

T, H = 24, 5
VARIANTS = (("rows", "fresh"), ("frames", "fresh"), ("frames", "window"))


def _spread(t):
    med = statistics.median(t)
    return {"batches": [round(x, 2) for x in t], "median_us": round(med, 2), "mad3_us": round(3 * statistics.median([abs(x - med) for x in t]), 2)}


def collect(n: int, rounds: int, steps: int):
    cs = [bc.collector(n, "fused_mlp", False, "gait", hist, outp) for hist, outp in VARIANTS]
    for c in cs:
        c.batch(72)
    times = [[] for _ in cs]
    for _ in range(rounds):
        for i, c in enumerate(cs):
            times[i].append(c.batch(steps))
    for (hist, outp), c, t in zip(VARIANTS, cs, times):
        st = c.store
        held = ([] if st.observations is None else [st.observations]) + [r for r in st.group_rows.values() if r is not st.observations] + list(st.frames.values())
        yield {"measure": "collect", "unit": "us per step", "config": "gait", "form": "fused_mlp", "num_envs": n, "history": hist, "output": outp,
               "steps_per_batch": steps, **_spread(t), "recorded_step": c.env._trace is not None,
               "fused_post": c.env._trace is not None and c.env._trace.post_refs is not None, "observation_bytes": sum(x.numel() * 4 for x in held)}
        st.detach()


def gather(n: int, rounds: int, widths):
    pw, cw = widths
    nmb, ep, repeats = 4, 5, 4
    mb = n * T // nmb
    idx = torch.randperm(nmb * mb, device="cuda", generator=torch.Generator(device="cuda").manual_seed(1))
    rows, frames = (bm.storage(n, T, pw, cw, 12, H, h) for h in ("rows", "frames"))
    for name in frames.frames:   # the same observations in both, the same policy rows
        rows.group_rows[name].copy_(frames.observation_rows(name))
    for k in ("actions", "values", "advantages", "returns", "actions_log_prob", "mu", "sigma"):
        getattr(frames, k).copy_(getattr(rows, k))
    for x, y in zip(rows._mini_batches(idx, nmb, 1, mb), frames._mini_batches(idx, nmb, 1, mb)):
        assert all(torch.equal(u, v) for u, v in zip(x, y)), "the frame gather differs from the row gather"
    sts = {"rows": rows, "frames": frames}
    times = {h: [] for h in sts}
    for _ in range(rounds):
        for h, st in sts.items():
            times[h].append(bm.timed(lambda st=st: [None for _b in st._mini_batches(idx, nmb, ep, mb)], repeats) / (nmb * ep))
    nbytes = mb * ((pw + pw + cw + 3 * 12 + 4) * 4 * 2 + 8)
    for h in sts:
        sp = _spread(times[h])
        yield {"measure": "gather", "unit": "us per minibatch", "num_envs": n, "steps": T, "policy_width": pw, "critic_width": cw, "history": h,
               "rows_per_minibatch": mb, "bytes_per_minibatch": nbytes, **sp, "TBps": round(nbytes / sp["median_us"] / 1e6, 2)}


def storage(n: int, widths):
    from types import SimpleNamespace

    from genesis_forge_amd import _native as nat
    from genesis_forge_amd.learner import RolloutStorage

    pw, cw = widths
    for hist in ("rows", "frames"):
        torch.cuda.synchronize()
        torch.cuda.empty_cache()
        m0 = torch.cuda.memory_allocated()
        mk = lambda name, w: bm._Obs(name=name, observation_space=SimpleNamespace(shape=(w,)), output="fresh", _history_len=H, _unrolled=False)
        env = SimpleNamespace(num_envs=n, managers={"observation": [mk("policy", pw), mk("critic", cw)]}, backend=nat.get_backend())
        st = RolloutStorage(env, T, obs_groups=bc.GAIT_GROUPS, history=hist)
        computed = (T + 1) * n * (pw + cw) * 4 if hist == "rows" else (T + H) * n * (pw + cw) // H * 4
        yield {"measure": "storage", "num_envs": n, "steps": T, "policy_width": pw, "critic_width": cw, "history": hist,
               "memory_allocated_bytes": torch.cuda.memory_allocated() - m0, "observation_bytes_computed": computed, "rewards_dones_bytes": T * n * 5}
        del st


def main() -> None:
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--measure", default="collect,gather,storage")
    ap.add_argument("--sizes", default="8192,65536")
    ap.add_argument("--rounds", type=int, default=9)
    ap.add_argument("--steps", type=int, default=120)
    ap.add_argument("--widths", default="310,80", help="row widths of the policy and the critic manager (gather, storage)")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_frame_rollout.py measures on a ROCm GPU: no device visible")
    gs.set_device("cuda:0")
    widths = tuple(int(x) for x in a.widths.split(","))
    for n in (int(x) for x in a.sizes.split(",")):
        for what in a.measure.split(","):
            recs = {"collect": lambda: collect(n, a.rounds, a.steps), "gather": lambda: gather(n, a.rounds, widths), "storage": lambda: storage(n, widths)}[what]()
            for rec in recs:
                print(json.dumps(rec), flush=True)
            torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
