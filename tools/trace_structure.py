#!/usr/bin/env python3
"""Address-free structure of the recorded step of many configs, on the CPU oracle backend (no GPU).

    python trace_structure.py <checkout> > structure.txt

Prints, per config, what a StepTrace hands to gf_replay_step: the op list, the patch table in order (kind, index, and every
address as "<ordinal of the recorded descriptor>:<its type>+<byte offset>"), the op each entry belongs to, where the Python
splits and afters sit, the per-piece tables of a split step and the two native tail segments.  Two checkouts whose recordings
are the same print the same bytes.  The ACCESS section is the only part that knows StepTrace's attribute names.
"""
import ctypes as C
import os
import re
import sys

ROOT = os.path.abspath(sys.argv[1])
sys.path.insert(0, os.path.join(ROOT, "genesis-forge_amd"))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import torch
from genesis_forge_amd import _native as nat, gs, tasks
from oracle_backend import OracleBackend
import test_fuzz_configs as fz
from genesis_like import GenesisLikeScene

gs.set_device("cpu")
nat.set_backend(OracleBackend(os.path.join(ROOT, "oracle", "libgf_oracle.so")))

STEPS = 48


# ---- ACCESS: the attribute names of the tree under test (these are the parent commit's) -------------------------------------------
def main_descriptors(tr): return tr.keep
def main_table(tr): return tr.replay_desc
def native_op(tr): return list(tr.native_op)
def pieces(tr): return [(s[0], s[1], s[3]) for s in tr.segments] if tr.splits else []      # (first op, count, GfReplay)
def tail(tr): return {k: (len(v["ops"]), v["ops"], v["desc"], v["keep"], len(v["patches"]), len(v["afters"])) for k, v in tr.tail_seg.items()}
# -------------------------------------------------------------------------------------------------------------------------------


def where(addr, regions):
    if not addr:
        return None
    for name, base, size in regions:
        if base <= addr < base + size:
            return f"{name}+{addr - base}"
    return "other"


def regions_of(descs, prefix, tr):
    r = [(f"{prefix}{i}:{type(a).__name__}", C.addressof(a), C.sizeof(a)) for i, a in enumerate(descs)]
    for name in ("post_refs", "_tail_refs"):
        x = getattr(tr, name, None)
        if x is not None:
            r.append((name, C.addressof(x), C.sizeof(x)))
    return r


def table(desc, regions):
    if not desc.num_patches:
        return []
    t = C.cast(desc.patches, C.POINTER(nat.GfReplayPatch))
    return [(t[i].kind, t[i].index, where(t[i].target, regions), where(t[i].target2, regions), where(t[i].aux, regions)) for i in range(desc.num_patches)]


def oplist(ops, n, regions):
    return [(ops[i].phase, where(ops[i].args, regions)) for i in range(n)]


def dump(tr):
    if tr is None:
        return None
    reg = regions_of(main_descriptors(tr), "d", tr)
    out = {"ops": oplist(tr.ops, tr.n_ops, reg), "table": table(main_table(tr), reg), "native_op": native_op(tr),
           "splits": [i for i, _ in tr.splits], "afters": [i for i, _ in tr.afters], "patches": len(tr.patches),
           "py_marks": [i for i, _ in tr.py_marks], "pieces": [(a0, cnt, table(d, reg)) for a0, cnt, d in pieces(tr)],
           "post_flags": None if tr.post_refs is None else tr.post_refs.flags, "tail_python": tr.tail_python,
           "graph": tr.graph is not None, "n_params": tr.n_params, "scene_plan": [re.sub(r"\b\d{9,}\b", "ID", str(k)) for k, _ in tr.scene_plan]}   # (keys carry an id())
    for part, (n, ops, desc, keep, n_patches, n_afters) in sorted(tail(tr).items()):
        treg = regions_of(keep, "t", tr)
        out["tail_" + part] = (oplist(ops, n, treg), table(desc, treg), n_patches, n_afters)
    return out


def drive(env, seed):
    env.build()
    env.seed(seed)
    env.reset()
    width = env.action_space.shape[0]
    g = torch.Generator().manual_seed(seed)
    for _ in range(STEPS):
        env.step(torch.randn(env.num_envs, width, generator=g))
    return env._trace


for scene_cls in (None, GenesisLikeScene):
    tag = "synthetic" if scene_cls is None else "genesis_like"
    for name, (_n, make) in tasks.BASELINE_CONFIGS.items():
        if scene_cls is None:
            env = make(70, max_episode_length_s=1)
        else:
            with tasks.use_scene(scene_cls):
                env = make(70, max_episode_length_s=1)
        print(tag, name, dump(drive(env, 5)))
    fz.SCENE_CLS[0] = scene_cls
    try:
        for seed in fz.SEEDS:
            print(tag, "fuzz", seed, dump(drive(fz.make_fuzz_env(seed), seed)))
    finally:
        fz.SCENE_CLS[0] = None
