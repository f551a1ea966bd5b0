#!/usr/bin/env python3
"""Where the fused post-physics launch of a CONFIG spends its time: per-wave wall-clock stamps at the phase boundaries of
`post_ws_kernel` (GF_WSTAMP in csrc/gf_post_ws.h), taken in a DIAGNOSTIC build of the library (-DGF_STAMPS, built into
tools/_stamps/; no product build contains a stamp) while the env steps on the recorded path.

    python tools/stamp_config.py build                    # here or on the GPU box: hipcc, ~1 min (again after any change under csrc/ or include/)
    python tools/stamp_config.py run gait_8192 [steps]    # on the GPU box

Up to 16 workgroups spread over the grid are stamped.  The phase table is the middle workgroup's; the placement report behind it says,
from the HW_ID / XCC_ID registers every stamped wave records, which role ran on which SIMD of which CU and how long each role was
busy and idle between the tick's barrier and the role barrier.  GF_ROLE_SHIFT=s (0 ... 15; this build only) rotates the roles of the
static programs the tick covers by (tile >> s) & 3 — profiles/r33_role_balance.md.
"""
import ctypes as C
import os
import subprocess
import sys
from concurrent.futures import ThreadPoolExecutor

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "genesis-forge_amd", "csrc")
OUT = os.path.join(ROOT, "tools", "_stamps")
LIB = os.path.join(OUT, "libgf_step_stamps.so")
SLOTS, STAMP_WORDS = 16, 16 * 4 * 16 + 16 * 4 * 2   # kStampSlots, kStampWords of csrc/gf_post_args.h
ROLES = ["control", "reward", "obs-rows", "obs-misc"]
NAMES = ["args staged", "pre-barrier done", "past barrier A", "role stores", "obs starts", "tile built", "past barrier B", "end"]


def build():
    os.makedirs(OUT, exist_ok=True)
    flags = "--offload-arch=gfx950 -O3 -ffp-contract=off -fPIC -std=c++17 -fvisibility=hidden -DGF_STAMPS".split()
    srcs = [f for f in sorted(os.listdir(CSRC)) if f.endswith(".hip")]
    with open(os.path.join(OUT, "stamps_var.cpp"), "w") as f:
        f.write('extern "C" __attribute__((visibility("default"))) unsigned long long* gf_debug_stamps = nullptr;\n')

    def cc(s):
        o = os.path.join(OUT, s[:-4] + ".o")
        subprocess.run(["hipcc", *flags, "-I", CSRC, "-c", os.path.join(CSRC, s), "-o", o], check=True)
        return o

    with ThreadPoolExecutor(6) as ex:
        objs = list(ex.map(cc, srcs))
    var = os.path.join(OUT, "stamps_var.o")
    subprocess.run(["g++", "-fPIC", "-c", os.path.join(OUT, "stamps_var.cpp"), "-o", var], check=True)
    subprocess.run(["hipcc", "--offload-arch=gfx950", "-shared", "-fPIC", "-o", LIB, *objs, var], check=True)
    print("built", LIB)


class Placement:
    """Where the hardware put the waves of the stamped workgroups (GF_WHERE: HW_ID and XCC_ID of every wave, read with s_getreg) and what
    each role did between the tick's barrier (stamp 13; a launch without a tick: its first stamp) and the role barrier (stamp 3):
    busy = up to the end of its pre-barrier block (stamp 2), idle = from there to the barrier's far side."""

    def __init__(self):
        self.cu = {}                                   # (xcc, se, sh, cu) -> {"n": launches, "simd": [role][simd] count, "busy": [role], "idle": [role]}
        self.wave_simd = [[0] * 4 for _ in range(4)]   # [index of the wave in its workgroup][SIMD]
        self.role_simd = [[0] * 4 for _ in range(4)]   # [role][SIMD]
        self.same_simd = [0] * 5                       # workgroups whose four waves sit on k distinct SIMDs
        self.tiles = {}                                # slot -> (tile, set of CUs it ran on)

    def add(self, h, slots, stride):
        base = SLOTS * 4 * 16
        for s in range(slots):
            simds = set()
            key = None
            for role in range(4):
                hw, x = h[base + (4 * s + role) * 2], h[base + (4 * s + role) * 2 + 1]
                simd, cu, sh, se, xcc, wave = (hw >> 4) & 3, (hw >> 8) & 15, (hw >> 12) & 1, (hw >> 13) & 7, x & 15, (x >> 32) & 3
                key = (xcc, se, sh, cu)
                c = self.cu.setdefault(key, {"n": 0, "simd": [[0] * 4 for _ in range(4)], "busy": [0.0] * 4, "idle": [0.0] * 4})
                c["simd"][role][simd] += 1
                st = h[64 * s + 16 * role: 64 * s + 16 * role + 16]
                start = st[13] if st[13] else st[1]
                c["busy"][role] += (st[2] - start) / 100.0
                c["idle"][role] += (st[3] - st[2]) / 100.0
                self.wave_simd[wave][simd] += 1
                self.role_simd[role][simd] += 1
                simds.add(simd)
            self.cu[key]["n"] += 1
            self.same_simd[len(simds)] += 1
            self.tiles.setdefault(s, (s * stride, set()))[1].add(key)

    def report(self):
        print("  placement of the stamped workgroups (tile: CUs it ran on, as XCC.SE.SH.CU)")
        for s, (tile, cus) in sorted(self.tiles.items()):
            print(f"    slot {s:2d} tile {tile:5d}: " + " ".join("%d.%d.%d.%d" % k for k in sorted(cus)))
        print("  waves of one workgroup on 1 / 2 / 3 / 4 distinct SIMDs: " + " / ".join(str(v) for v in self.same_simd[1:]))
        for title, m, names in (("index of the wave in its workgroup", self.wave_simd, ["wave %d" % i for i in range(4)]), ("role", self.role_simd, ROLES)):
            print(f"  {title} x SIMD 0 1 2 3 (counts over every stamped workgroup and launch)")
            for i in range(4):
                print(f"    {names[i]:>9s}: " + " ".join(f"{v:7d}" for v in m[i]))
        print("  per CU seen: launches | per role: SIMD counts 0/1/2/3, busy and idle us between the tick's barrier and the role barrier")
        for key, c in sorted(self.cu.items()):
            n = max(1, c["n"])
            cells = [f"{ROLES[r]} {'/'.join(str(v) for v in c['simd'][r])} busy {c['busy'][r] / n:.2f} idle {c['idle'][r] / n:.2f}" for r in range(4)]
            print("    %d.%d.%d.%d n=%d | " % (*key, c["n"]) + " | ".join(cells))
        nn = sum(c["n"] for c in self.cu.values())
        if nn:
            print("  all stamped workgroups, mean us: " + " | ".join(
                f"{ROLES[r]} busy {sum(c['busy'][r] for c in self.cu.values()) / nn:.2f} idle {sum(c['idle'][r] for c in self.cu.values()) / nn:.2f}" for r in range(4)))


def run(config, steps):
    os.environ["GF_JIT"] = "off"   # a plugin is compiled against the product GfPostArgs layout
    sys.path.insert(0, os.path.join(ROOT, "genesis-forge_amd"))
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import torch
    from genesis_forge_amd import _native, gs, tasks
    _native.lib_path = lambda: LIB
    gs.set_device("cuda:0")
    name, _, size = config.partition("@")   # "go2_cmd@1048576": the config at another size
    n, factory = tasks.BASELINE_CONFIGS[name]
    n = int(size) if size else n
    env = factory(n)
    env.build()
    env.seed(1)
    env.reset()
    lib = _native.get_backend().lib
    stamps = torch.zeros(STAMP_WORDS, dtype=torch.int64, device="cuda")
    D = env.action_space.shape[0]
    acts = [torch.randn(n, D, device="cuda") for _ in range(4)]
    for i in range(20):
        env.step(acts[i % 4])
    assert env._trace is not None, "not recorded"
    C.c_void_p.in_dll(lib, "gf_debug_stamps").value = stamps.data_ptr()
    tiles = (n + 63) // 64
    stride = max(1, tiles // SLOTS)
    slots = min(SLOTS, (tiles + stride - 1) // stride)
    mid = min(SLOTS - 1, tiles // 2 // stride)
    acc = torch.zeros(4, 16, dtype=torch.float64)
    where = Placement()
    for i in range(steps):
        env.step(acts[i % 4])
        torch.cuda.synchronize()
        h = stamps.cpu().tolist()
        t0 = min(h[64 * mid + 16 * w + 1] for w in range(4))
        for w in range(4):
            for k in range(1, 16):
                if h[64 * mid + 16 * w + k]:   # (a stamp this launch does not take stays 0)
                    acc[w, k] += (h[64 * mid + 16 * w + k] - t0) / 100.0
        where.add(h, slots, stride)
    acc /= steps
    print(f"{config}: {n} envs, fused={env._trace.post_refs is not None}, mean of {steps} launches, us since the first wave had its args (middle workgroup)")
    print("          " + " ".join(f"{s:>17s}" for s in NAMES))
    for w in range(4):
        print(f"  wave {w}: " + " ".join(f"{float(acc[w, k]):17.2f}" for k in range(1, 9)))
    print("  inside the pre-barrier block — wave 0: terminations evaluated | command draws | gait manager;  wave 1: rows reduced | (behind the barrier) fold starts | fold done;  wave 2: rows requested")
    for w in (0, 1, 2):
        print(f"  wave {w}: " + " ".join(f"{float(acc[w, k]):17.2f}" for k in range(9, 12 if w < 2 else 10)))
    print("  folded contact phase (0 when the launch has none): slot ids + masks in LDS | prefix done | contributions in LDS | links done")
    print("  (a step folded into one launch, post_ws_kernel_tick, has no contact phase: tick of the tile done | past the tick's barrier | 0 | 0)")
    for w in range(4):
        print(f"  wave {w}: " + " ".join(f"{float(acc[w, k]):17.2f}" for k in range(12, 16)))
    print(f"  (rows are ROLES: role = wave unless GF_ROLE_SHIFT rotates them; GF_ROLE_SHIFT={os.environ.get('GF_ROLE_SHIFT', 'unset')})")
    where.report()


if __name__ == "__main__":
    if sys.argv[1] == "build":
        build()
    else:
        run(sys.argv[2], int(sys.argv[3]) if len(sys.argv) > 3 else 200)
