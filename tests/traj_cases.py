"""Cases and a plain-loop reference for gf_traj_table / gf_traj_gather (tests/test_traj_edges.py).

The reference is written from the contract in include/gf_step.h.  The table is built per env: walk ``t``, close a trajectory at a done
or at ``T - 1``.  Every other output is built per trajectory: its rows copied side by side from the segments (row ``(t, n)`` of a
segment lies ``(t·N + n)·row_stride`` floats behind its pointer), zeros from ``len`` on, the masks, the un-pad index, and the initial
states from the rollout-start state where ``t0 == 0``.  The normaliser is torch's three float32 operations ``(v - mean) / (std + eps)``:
each is correctly rounded and the library is built without contraction, so every comparison is bit for bit.

``gather_plan`` restates the launch: grid x = ``min(ceil(most / 256), 4096)`` workgroups of 256 lanes, ``most`` the largest job; a job
with more elements than lanes strides."""
import functools
from types import SimpleNamespace as NS

import torch

LANES, CAP = 256, 4096                      # kTrajBlock, the cap on grid x
MAX_INPUTS, MAX_WIDTH, MAX_HIDDEN = 4, 1024, 512

# ---- the table ----------------------------------------------------------------------------------------------------------------------
TABLE_N = [1, 63, 64, 65, 127, 128, 129, 191, 192, 193, 255, 256, 257, 511, 512, 513, 1025]
TABLE_T = [1, 2, 3, 24]
HOT_ENVS = [63, 64, 255, 256]               # a wave's last lane, the next wave's first, a chunk's last, the next chunk's first
PATTERNS = ["none", "all", "last", "first", "random0.1", "random0.5", "ramp", "ramp7"] + [f"hot{k}" for k in HOT_ENVS]


def patterns_of(N):
    return [p for p in PATTERNS if not p.startswith("hot") or int(p[3:]) < N]


def make_dones(T, N, pattern, seed=0):
    """``[T, N]`` uint8."""
    d = torch.zeros(T, N, dtype=torch.uint8)
    if pattern == "all":
        d[:] = 1
    elif pattern == "last":
        d[T - 1] = 1
    elif pattern == "first":
        d[0] = 1
    elif pattern.startswith("random"):
        g = torch.Generator().manual_seed(seed * 7919 + T * 131 + N)
        d = (torch.rand(T, N, generator=g) < float(pattern[6:])).to(torch.uint8)
    elif pattern == "ramp":                 # env n has n % T dones: neighbouring counts differ
        for n in range(N):
            d[:n % T, n] = 1
    elif pattern == "ramp7":                # env n has min(n % 7, T) dones: at T >= 7 the four wave totals of a chunk differ as well (64 % 7 = 1)
        for n in range(N):
            d[:min(n % 7, T), n] = 1
    elif pattern.startswith("hot"):         # exactly one env has every step done
        d[:, int(pattern[3:])] = 1
    else:
        assert pattern == "none", pattern
    return d


def ref_table(dones):
    """counts ``[N]``, offsets ``[N + 1]``, table ``[J, 3]`` = (env, t0, len), int32, env-major."""
    T, N = dones.shape
    cols = dones.t().tolist()
    counts, offsets, table = [], [0], []
    for n in range(N):
        t0 = c = 0
        for t in range(T):
            if t == T - 1 or cols[n][t]:
                table.append((n, t0, t + 1 - t0))
                t0, c = t + 1, c + 1
        counts.append(c)
        offsets.append(offsets[-1] + c)
    i32 = lambda x, shape: torch.tensor(x, dtype=torch.int32).reshape(shape)
    return i32(counts, (N,)), i32(offsets, (N + 1,)), i32(table, (-1, 3))


@functools.lru_cache(maxsize=None)
def table_case(T, N, pattern):
    """(dones, counts, offsets, table): computed once, shared, never written."""
    dones = make_dones(T, N, pattern)
    return (dones,) + ref_table(dones)


# ---- the gather ---------------------------------------------------------------------------------------------------------------------
def G(widths, strides=None, norm=None):
    """A group: segment widths; per segment row_stride 0, "eq" (the width) or an int > width (a view into a wider NaN-filled buffer);
    ``norm`` None or ``(eps, sliced)`` — ``sliced``: mean and std are 4-byte-offset slices of a larger tensor."""
    return NS(widths=tuple(widths), strides=tuple(strides or [0] * len(widths)), norm=norm, W=sum(widths))


def S(H, kind):
    return NS(H=H, kind=kind)               # kind "lstm" (c0 given) or "gru" (c0 and c_start NULL)


def case(name, T, N, pattern, g0, g1=None, s0=None, s1=None, splits=(1,)):
    return NS(name=name, T=T, N=N, pattern=pattern, groups=(g0, g1), states=(s0, s1), splits=tuple(splits))


GATHER_CASES = [
    case("tiny", 1, 1, "none", G([1]), s0=S(1, "lstm")),
    case("split", 2, 7, "random0.5", G([3], ["eq"], norm=(0.0, False)), G([1, 3], [3, 4], norm=(1e-2, True)), S(6, "gru"), S(6, "lstm"),
         splits=(1, 2, 3, 7)),
    case("four-segments", 24, 65, "random0.1", G([1, 20, 26, 1], [3, 0, "eq", 2], norm=(1e-2, True)), G([4, 1], ["eq", 0]), S(64, "lstm"),
         splits=(3,)),
    case("wide", 2, 3, "random0.5", G([256, 1], [258, 0]), G([1, 511, 511, 1], [0, "eq", 513, 0], norm=(0.0, False)), None, S(512, "gru")),
    case("ramp", 24, 257, "ramp", G([5], norm=(1e-2, False)), None, S(6, "lstm"), S(4, "gru"), splits=(1, 2)),
    case("never-done", 24, 5, "none", G([3]), G([4]), S(6, "gru"), None, splits=(5,)),
    case("done-first", 24, 5, "first", G([3], [5]), None, None, S(6, "lstm"), splits=(2,)),
    case("done-last", 2, 64, "last", G([4], ["eq"]), None, S(1, "gru"), S(1, "lstm")),
    case("hot", 24, 65, "hot64", G([1, 4], [0, 6]), None, S(6, "lstm"), splits=(3,)),
    # the three grid-stride loops, each at the smallest shape that passes 1 048 576 elements of its job
    case("stride-observations", 8, 130, "random0.3", G([1024])),
    case("stride-rows", 24, 1821, "all", G([1])),
    case("stride-states", 1, 2100, "none", G([1]), None, S(512, "lstm"), S(512, "gru")),
]
STRIDE_CASES = {"stride-observations": "obs0", "stride-rows": "rows", "stride-states": "h0"}
CASES_BY_NAME = {c.name: c for c in GATHER_CASES}


def gather_plan(T, J, widths, hiddens):
    """The launch restated: the jobs' element counts, grid x, and the jobs whose loop strides."""
    jobs = {"obs0": T * J * widths[0], "obs1": T * J * widths[1], "rows": T * J, "h0": J * hiddens[0], "h1": J * hiddens[1]}
    most = max(jobs.values())
    blocks = min(-(-most // LANES), CAP)
    return jobs, blocks, {k for k, v in jobs.items() if v > blocks * LANES}


def bounds_of(N, M):
    """The generator's split: minibatch i is the envs [i·N // M, (i + 1)·N // M)."""
    return [i * N // M for i in range(M + 1)]


@functools.lru_cache(maxsize=4)
def build(name):
    """The inputs of a case on the CPU — computed once, shared, never written — with the reference table."""
    c = CASES_BY_NAME[name]
    T, N = c.T, c.N
    g = torch.Generator().manual_seed(sum(map(ord, name)))
    dones = make_dones(T, N, c.pattern, seed=1)
    counts, offsets, table = ref_table(dones)
    groups = []
    for spec in c.groups:
        if spec is None:
            groups.append(None)
            continue
        segs = []
        for w, st in zip(spec.widths, spec.strides):
            rs = w if st in (0, "eq") else int(st)
            assert rs >= w
            off = 1 if rs - w >= 2 else 0                              # gap columns on both sides where there is room
            wide = torch.full((T * N, rs), float("nan"))
            wide[:, off:off + w] = torch.randn(T * N, w, generator=g)
            segs.append(NS(wide=wide, off=off, width=w, rs=rs, row_stride=0 if st == 0 else rs))
        mean = std = store = None
        eps = 0.0
        if spec.norm is not None:
            eps, sliced = spec.norm
            k = 1 if sliced else 0
            store = (torch.randn(spec.W + k, generator=g), torch.rand(spec.W + k, generator=g) + 0.5)
            mean, std = store[0][k:], store[1][k:]
        groups.append(NS(segs=segs, W=spec.W, mean=mean, std=std, eps=eps, store=store, sliced=bool(spec.norm and spec.norm[1])))
    states = []
    for spec in c.states:
        if spec is None:
            states.append(None)
            continue
        nz = lambda: torch.randn(N, spec.H, generator=g).abs() + 0.25   # no zero element: a late trajectory's zeros are distinguishable
        states.append(NS(H=spec.H, kind=spec.kind, h_start=nz(), c_start=nz() if spec.kind == "lstm" else None))
    return NS(case=c, T=T, N=N, dones=dones, counts=counts, offsets=offsets, table=table, groups=groups, states=states)


def minibatches(inp):
    """(env_start, env_stop, first_traj, num_traj) of every minibatch of every split of the case, without repeats."""
    out, offs = [], inp.offsets.tolist()
    for M in inp.case.splits:
        b = bounds_of(inp.N, M)
        for i in range(M):
            mb = (b[i], b[i + 1], offs[b[i]], offs[b[i + 1]] - offs[b[i]])
            if mb not in out:
                out.append(mb)
    return out


def observations(inp, k):
    """Group ``k`` as the ``[T, N, W]`` tensor rsl_rl would store, through the normaliser: for the CPU twin."""
    gr = inp.groups[k]
    x = torch.cat([s.wide.view(inp.T, inp.N, s.rs)[:, :, s.off:s.off + s.width] for s in gr.segs], dim=-1)
    if gr.mean is not None:
        x = (x - gr.mean) / (gr.std + torch.tensor(gr.eps, dtype=torch.float32))
    return x


def ref_gather(inp, e0, e1, j0, J):
    """The outputs of one minibatch — the envs [e0, e1), the trajectories [j0, j0 + J) — by plain loops over the trajectories."""
    T, N = inp.T, inp.N
    table = inp.table[j0:j0 + J].tolist()
    out = {}
    for k, gr in enumerate(inp.groups):
        if gr is None:
            continue
        dst = torch.zeros(T, J, gr.W)
        eps = torch.tensor(gr.eps, dtype=torch.float32)
        for j, (env, t0, ln) in enumerate(table):
            c = 0
            for s in gr.segs:
                v = s.wide.view(T, N, s.rs)[t0:t0 + ln, env, s.off:s.off + s.width]
                if gr.mean is not None:
                    v = (v - gr.mean[c:c + s.width]) / (gr.std[c:c + s.width] + eps)
                dst[:ln, j, c:c + s.width] = v
                c += s.width
        out[f"dst{k}"] = dst
    masks = torch.zeros(T, J, dtype=torch.uint8)
    unpad = torch.full(((e1 - e0) * T,), -1, dtype=torch.int64)
    for j, (env, t0, ln) in enumerate(table):
        masks[:ln, j] = 1
        at = (env - e0) * T + t0
        unpad[at:at + ln] = torch.arange(j * T, j * T + ln)
    out["masks"], out["unpad_index"] = masks, unpad
    for k, st in enumerate(inp.states):
        if st is None:
            continue
        for name, start in (("h0", st.h_start), ("c0", st.c_start)):
            if start is None:
                continue
            x = torch.zeros(J, st.H)
            for j, (env, t0, ln) in enumerate(table):
                if t0 == 0:
                    x[j] = start[env]
            out[f"{name}_{k}"] = x
    return out


def paths_of(inp, e0, e1, j0, J):
    """The paths one launch takes, from the dispatch restated here."""
    c, T = inp.case, inp.T
    tags = set()
    for k, gr in enumerate(inp.groups):
        if gr is None:
            tags.add(f"group{k}-absent")
            continue
        tags |= {f"group{k}-{'normalised' if gr.mean is not None else 'raw'}", f"segments-{len(gr.segs)}", f"W-{gr.W}"}
        if gr.mean is not None:
            tags |= {f"eps-{gr.eps:g}", "norm-sliced" if gr.sliced else "norm-whole"}
        for s in gr.segs:
            tags.add("row_stride-0" if s.row_stride == 0 else "row_stride-width" if s.row_stride == s.width else "row_stride-larger")
        tags |= {"width-1-first"} if gr.segs[0].width == 1 and len(gr.segs) > 1 else set()
        tags |= {"width-1-last"} if gr.segs[-1].width == 1 and len(gr.segs) > 1 else set()
    if inp.groups[0].mean is not None and inp.groups[1] is not None and inp.groups[1].mean is not None:
        tags.add("both-normalised")
    if inp.groups[0].mean is not None and inp.groups[1] is not None and inp.groups[1].mean is None:
        tags.add("group0-only-normalised")
    for k, st in enumerate(inp.states):
        tags.add(f"state{k}-{'absent' if st is None else st.kind}")
        if st is not None:
            tags.add(f"H-{st.H}")
    if inp.states[0] is not None and inp.states[1] is not None and (inp.states[0].kind, inp.states[1].kind) == ("gru", "lstm"):
        tags.add("gru-then-lstm")
    tags.add(f"T-{T}")
    lens = inp.table[j0:j0 + J, 2]
    tags.add("padding" if bool((lens < T).any()) else "no-padding")
    if bool((inp.table[j0:j0 + J, 1] > 0).any()):
        tags.add("late-start")
    if e0 > 0 and j0 > 0:
        tags.add("env_start>0")
    if e1 - e0 == 1:
        tags.add("single-env")
    if e1 - e0 == inp.N:
        tags.add("whole-rollout")
    if inp.table.shape[0] > j0 + J:
        tags.add("table_rows-beyond")
    widths = [0 if gr is None else gr.W for gr in inp.groups]
    hiddens = [0 if st is None else st.H for st in inp.states]
    _jobs, blocks, strided = gather_plan(T, J, widths, hiddens)
    tags.add("grid-capped" if blocks == CAP else "grid-uncapped")
    tags |= {f"strides-{k}" for k in strided}
    return tags


REQUIRED_PATHS = (
    {f"W-{w}" for w in (1, 3, 4, 5, 48, 257, 1024)} | {f"segments-{k}" for k in (1, 2, MAX_INPUTS)} | {"width-1-first", "width-1-last"}
    | {"row_stride-0", "row_stride-width", "row_stride-larger"}
    | {"group0-raw", "group0-normalised", "group1-raw", "group1-normalised", "group1-absent", "both-normalised", "group0-only-normalised"}
    | {"eps-0", "eps-0.01", "norm-sliced", "norm-whole"}
    | {f"H-{h}" for h in (1, 6, 64, 512)} | {f"state{k}-{x}" for k in (0, 1) for x in ("absent", "lstm", "gru")} | {"gru-then-lstm"}
    | {"T-1", "T-2", "T-24", "padding", "no-padding", "late-start", "env_start>0", "single-env", "whole-rollout", "table_rows-beyond"}
    | {"grid-capped", "grid-uncapped", "strides-obs0", "strides-rows", "strides-h0"})
