"""gf_episode_step through the raw GfEpisodeArgs at the edges of its index arithmetic, and gf_done_compact's three paths on uint8 masks.

The kernel gives a lane four consecutive envs: 16-byte loads where the float arrays are 16-byte aligned, the masks 4-byte aligned and
the lane's four envs exist, element loads otherwise; the done envs in front of a workgroup are counted from the whole mask in 16-byte
units (up to 65 536 envs) or from a count launch (above).  Reference: the ``RunnerRef`` deque restatement of
tests/test_episode_stats.py and ``r + (gamma * v) * time_out`` in float32 torch on the CPU; everything is compared bit for bit, every
array is a slice of a guarded buffer (tests/guarded.py), and the masks are uint8 with set bytes drawn from {1, 2, 0x7f, 0x80, 0xff}
("nonzero = done").  The unmarked leg runs the same patterns and states through ``EpisodeStatistics._update_torch``."""
import pytest
import torch

from genesis_forge_amd import _native as nat
from guarded import Guarded, raw_call, sync
from test_episode_stats import RunnerRef

GAMMA = 0.99
G32 = torch.tensor(GAMMA, dtype=torch.float32)
SET_BYTES = torch.tensor([1, 2, 0x7F, 0x80, 0xFF], dtype=torch.uint8)
SENTINEL_STATE = (-77, -78)   # the slot a launch writes starts as this
SIZES = [1, 2, 3, 4, 5, 15, 16, 17, 63, 64, 65, 255, 256, 257, 1023, 1024, 1025, 2049, 4097, 65535, 65536, 65537, 66561]
PATTERNS = ["none", "all", "first", "last", "block_edge", "window", "window+1", "random"]
WINDOWS = [1, 2, 7, 100]
STATES = ["empty", "nearly_full", "full"]   # (head, fill) = (0, 0), (W-1, W-1), (3 % W, W)


def _state(kind, W):
    return {"empty": (0, 0), "nearly_full": (W - 1, W - 1), "full": (3 % W, W)}[kind]


def _plain(r, v, to):
    """PPO.process_env_step: one product, one product, one sum, each rounded to float32."""
    return r + (G32 * v) * to


def _fma(r, v, to):
    """What a fused multiply-add of gamma * v into the sum would give (the product unrounded)."""
    return (G32.double() * v.double() * to.double() + r.double()).float()


def _inputs(n, g):
    """Random-normal rewards and values on which a fused evaluation of the bootstrap differs from the reference in EVERY row."""
    r, v, one = torch.randn(n, generator=g), torch.randn(n, generator=g), torch.ones(n)
    same = _plain(r, v, one) == _fma(r, v, one)
    while bool(same.any()):
        k = int(same.sum())
        r[same], v[same] = torch.randn(k, generator=g), torch.randn(k, generator=g)
        same = _plain(r, v, one) == _fma(r, v, one)
    return r, v


def _pattern(kind, n, W, g):
    m = torch.zeros(n, dtype=torch.bool)
    if kind == "all":
        m[:] = True
    elif kind == "first":
        m[0] = True
    elif kind == "last":
        m[n - 1] = True
    elif kind == "block_edge":   # the last env of the first workgroup and the first of the second
        m[[i for i in (1023, 1024) if i < n]] = True
    elif kind in ("window", "window+1"):
        m[torch.randperm(n, generator=g)[:min(n, W + (kind == "window+1"))]] = True
    elif kind == "random":
        m = torch.rand(n, generator=g) < 0.3
    else:
        assert kind == "none"
    return m


def _bytes(mask, g):
    """A bool mask as uint8 with every set byte drawn from SET_BYTES."""
    vals = SET_BYTES[torch.randint(0, len(SET_BYTES), (mask.numel(),), generator=g)]
    return torch.where(mask, vals, torch.zeros_like(vals))


def _i32(x):
    return x.contiguous().view(torch.int32)


class Case:
    """A start state and its reference."""

    def __init__(self, n, W, head, fill, seed):
        self.n, self.W, self.head, self.fill = n, W, head, fill
        self.g = g = torch.Generator().manual_seed(seed)
        self.s0 = torch.randn(n, generator=g)
        self.l0 = torch.randint(0, 50, (n,), generator=g).to(torch.float32)
        self.ring_r0 = 1000.0 + 0.5 * torch.arange(W, dtype=torch.float32)
        self.ring_l0 = 500.0 + torch.arange(W, dtype=torch.float32)
        self.ref = RunnerRef(n, W, "cpu")
        self.ref.cur_reward_sum.copy_(self.s0)
        self.ref.cur_episode_length.copy_(self.l0)
        live = [(head - fill + i) % W for i in range(fill)]
        self.ref.rewbuffer.extend(self.ring_r0[live].tolist())
        self.ref.lenbuffer.extend(self.ring_l0[live].tolist())

    def draw(self, pattern, to_rate=0.1):
        """One step's inputs: rewards, values, dones and time_outs (uint8)."""
        r, v = _inputs(self.n, self.g)
        d = _bytes(_pattern(pattern, self.n, self.W, self.g), self.g)
        to = _bytes(torch.rand(self.n, generator=self.g) < to_rate, self.g)
        if not bool(to.any()):
            to[self.n // 2] = 0x80
        return r, v, d, to


class Device:
    """The kernel's arrays for a Case, guarded, and a CPU mirror of what they must hold."""

    def __init__(self, dev, case, parity=0, off_f32=0, off_u8=0, off_dones=None):
        n, W = case.n, case.W
        self.dev, self.case, self.parity = dev, case, parity
        F, U, I = torch.float32, torch.uint8, torch.int32
        self.r, self.v = Guarded(n, F, dev, off_f32), Guarded(n, F, dev, off_f32)
        self.s, self.l = Guarded(n, F, dev, off_f32, case.s0), Guarded(n, F, dev, off_f32, case.l0)
        self.d, self.to = Guarded(n, U, dev, off_u8 if off_dones is None else off_dones), Guarded(n, U, dev, off_u8)
        self.ring_r, self.ring_l = Guarded(W, F, dev, 0, case.ring_r0), Guarded(W, F, dev, 0, case.ring_l0)
        st = [0, 0, 0, 0]
        st[2 * parity:2 * parity + 2] = (case.head, case.fill)
        st[2 * (1 - parity):2 * (1 - parity) + 2] = SENTINEL_STATE
        self.state = Guarded(4, I, dev, 0, torch.tensor(st, dtype=I))
        self.blocks = -(-n // nat.GF_EPISODE_BLOCK_ENVS)
        self.counts = Guarded(self.blocks, I, dev)
        self.m_ring_r, self.m_ring_l, self.m_state = case.ring_r0.clone(), case.ring_l0.clone(), torch.tensor(st, dtype=I)
        self.m_s, self.m_l = case.s0.clone(), case.l0.clone()

    def step(self, backend, r, v, d, to, mode="both"):
        case, n, W, p = self.case, self.case.n, self.case.W, self.parity
        stats, boot = mode != "boot", mode != "stats"
        for g, x in ((self.r, r), (self.v, v), (self.d, d), (self.to, to)):
            g.t.copy_(x)
        a = nat.GfEpisodeArgs()
        a.num_envs, a.rewards, a.gamma = n, self.r.ptr, GAMMA
        if boot:
            a.time_outs, a.values = self.to.ptr, self.v.ptr
        if stats:
            a.dones, a.cur_reward_sum, a.cur_episode_length = self.d.ptr, self.s.ptr, self.l.ptr
            a.ring_reward, a.ring_length, a.ring_state, a.block_counts = self.ring_r.ptr, self.ring_l.ptr, self.state.ptr, self.counts.ptr
            a.window, a.parity = W, p
        assert raw_call(backend, "episode_step", a) == 0
        sync(self.dev)
        tag = (n, W, mode, p)
        for g in (self.r, self.v, self.s, self.l, self.d, self.to, self.ring_r, self.ring_l, self.state, self.counts):
            assert g.guards_ok(), ("wrote outside an array", tag)
        assert torch.equal(_i32(self.v.cpu()), _i32(v)) and torch.equal(self.d.cpu(), d) and torch.equal(self.to.cpu(), to), ("an input changed", tag)
        # the reward row
        hit = (to != 0).to(torch.float32)
        want_r = _plain(r, v, hit) if boot else r
        if boot:
            assert bool((_fma(r, v, hit) != want_r)[to != 0].any()), "a fused evaluation must differ on these inputs"
        assert torch.equal(_i32(self.r.cpu()), _i32(want_r)), ("rewards: r + (gamma * v) * time_out after the statistics read r", tag)
        # the statistics
        if stats:
            tot = int((d != 0).sum())
            case.ref.step(r, d)   # the RAW reward
            self.m_s, self.m_l = case.ref.cur_reward_sum.clone(), case.ref.cur_episode_length.clone()
            st = self.state.cpu()
            assert torch.equal(st[2 * p:2 * p + 2], self.m_state[2 * p:2 * p + 2]), ("the read slot of ring_state changed", tag)
            head0, fill0 = self.m_state[2 * p:2 * p + 2].tolist()
            head, fill = st[2 * (1 - p):2 * (1 - p) + 2].tolist()
            assert (head, fill) == ((head0 + tot) % W, min(W, fill0 + tot)) and fill == len(case.ref.rewbuffer), ("ring_state", tag, head, fill)
            live = [(head - fill + i) % W for i in range(fill)]
            ring_r, ring_l = self.ring_r.cpu(), self.ring_l.cpu()
            assert torch.equal(_i32(ring_r[live]), _i32(torch.tensor(list(case.ref.rewbuffer), dtype=torch.float32))), ("rewbuffer, oldest first", tag)
            assert torch.equal(_i32(ring_l[live]), _i32(torch.tensor(list(case.ref.lenbuffer), dtype=torch.float32))), ("lenbuffer, oldest first", tag)
            rest = sorted(set(range(W)) - set(live))
            assert torch.equal(_i32(ring_r[rest]), _i32(self.m_ring_r[rest])) and torch.equal(_i32(ring_l[rest]), _i32(self.m_ring_l[rest])), ("ring entries outside the window", tag)
            self.m_ring_r, self.m_ring_l, self.m_state = ring_r, ring_l, st
            if n > nat.GF_EPISODE_SINGLE_MAX:
                pad = torch.zeros(self.blocks * nat.GF_EPISODE_BLOCK_ENVS, dtype=torch.int32)
                pad[:n] = (d != 0).to(torch.int32)
                assert torch.equal(self.counts.cpu(), pad.reshape(self.blocks, -1).sum(1).to(torch.int32)), ("block_counts", tag)
            else:
                assert self.counts.untouched(), ("one launch needs no block counts", tag)
            self.parity = 1 - p
        else:
            assert torch.equal(self.state.cpu(), self.m_state) and self.counts.untouched()
            assert torch.equal(_i32(self.ring_r.cpu()), _i32(self.m_ring_r)) and torch.equal(_i32(self.ring_l.cpu()), _i32(self.m_ring_l))
        assert torch.equal(_i32(self.s.cpu()), _i32(self.m_s)) and torch.equal(_i32(self.l.cpu()), _i32(self.m_l)), ("cur_reward_sum / cur_episode_length", tag)


# ---- GPU ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("n", SIZES)
def test_sizes_hip(hip_backend, n):
    """Three steps (parity 0, 1, 0) at every size: the 4-env lane split, the partial last mask unit, the 1 024-env workgroup edge,
    the last one-launch and the first two-launch sizes."""
    case = Case(n, 7, 3, 7, seed=n)
    dev = Device("cuda", case)
    for pattern in ("random", "all", "last"):
        dev.step(hip_backend, *case.draw(pattern))


@pytest.mark.gpu
@pytest.mark.parametrize("state", STATES)
@pytest.mark.parametrize("W", WINDOWS)
@pytest.mark.parametrize("pattern", PATTERNS)
def test_patterns_hip(hip_backend, pattern, W, state):
    head, fill = _state(state, W)
    case = Case(2049, W, head, fill, seed=W * 10 + len(pattern))
    Device("cuda", case, parity=(W + fill) & 1).step(hip_backend, *case.draw(pattern))


@pytest.mark.gpu
@pytest.mark.parametrize("parity", [0, 1])
def test_parity_sequence_hip(hip_backend, parity):
    case = Case(1025, 7, 0, 0, seed=parity)
    dev = Device("cuda", case, parity=parity)
    for pattern in ("window+1", "first", "random"):
        dev.step(hip_backend, *case.draw(pattern))


@pytest.mark.gpu
@pytest.mark.parametrize("n", [5, 1025])
def test_modes_hip(hip_backend, n):
    """Statistics only, bootstrap only (dones NULL), both — one after the other on the same arrays."""
    case = Case(n, 7, 3, 7, seed=n)
    dev = Device("cuda", case)
    for mode in ("stats", "boot", "both", "boot", "stats"):
        dev.step(hip_backend, *case.draw("random", to_rate=0.5), mode=mode)


ALIGN = {"f32": dict(off_f32=1), "u8": dict(off_u8=1), "dones4": dict(off_dones=4), "all": dict(off_f32=1, off_u8=1, off_dones=5)}


@pytest.mark.gpu
@pytest.mark.parametrize("n", [17, 1025, 4097])
@pytest.mark.parametrize("kind", list(ALIGN))
def test_alignment_hip(hip_backend, kind, n):
    """The float arrays one float off (no 16-byte loads), the masks one byte off (no 4-byte loads), dones 4 bytes off (4-byte loads,
    no 16-byte mask units), and all of it at once."""
    case = Case(n, 7, 3, 7, seed=n + len(kind))
    dev = Device("cuda", case, **ALIGN[kind])
    for pattern in ("random", "all"):
        dev.step(hip_backend, *case.draw(pattern))


@pytest.mark.gpu
@pytest.mark.parametrize("head,fill", [(-1, 0), (7, 3), (2, 8), (1 << 30, -5)])
def test_out_of_range_ring_state_hip(hip_backend, head, fill):
    """A ring_state word outside its range never becomes an index outside the ring: only the W ring entries, cur_* and the written
    slot change, and the written head and fill are in range."""
    n, W = 1025, 7
    case = Case(n, W, 0, 0, seed=11)
    dev = Device("cuda", case)
    bad = torch.tensor([head, fill, *SENTINEL_STATE], dtype=torch.int32)
    dev.state.t.copy_(bad)
    r, v, d, _to = case.draw("random")
    dev.r.t.copy_(r)
    dev.d.t.copy_(d)
    a = nat.GfEpisodeArgs()
    a.num_envs, a.rewards, a.dones, a.gamma = n, dev.r.ptr, dev.d.ptr, GAMMA
    a.cur_reward_sum, a.cur_episode_length, a.ring_reward, a.ring_length = dev.s.ptr, dev.l.ptr, dev.ring_r.ptr, dev.ring_l.ptr
    a.ring_state, a.block_counts, a.window, a.parity = dev.state.ptr, dev.counts.ptr, W, 0
    assert raw_call(hip_backend, "episode_step", a) == 0
    sync("cuda")
    for g in (dev.r, dev.s, dev.l, dev.d, dev.ring_r, dev.ring_l, dev.state):
        assert g.guards_ok()
    assert dev.counts.untouched() and dev.v.untouched() and dev.to.untouched()
    assert torch.equal(_i32(dev.r.cpu()), _i32(r)) and torch.equal(dev.d.cpu(), d)
    st = dev.state.cpu()
    assert torch.equal(st[:2], bad[:2]), "the read slot"
    assert 0 <= int(st[2]) < W and 0 <= int(st[3]) <= W
    case.ref.step(r, d)
    assert torch.equal(_i32(dev.s.cpu()), _i32(case.ref.cur_reward_sum)) and torch.equal(_i32(dev.l.cpu()), _i32(case.ref.cur_episode_length))


# ---- CPU: the same patterns and states through EpisodeStatistics._update_torch ------------------------------------------------------
def _torch_leg(n, W, head, fill, parity, patterns, seed):
    from genesis_forge_amd.learner import EpisodeStatistics

    case = Case(n, W, head, fill, seed)
    st = EpisodeStatistics(n, W, device="cpu")
    st.cur_reward_sum.copy_(case.s0)
    st.cur_episode_length.copy_(case.l0)
    st.ring_reward.copy_(case.ring_r0)
    st.ring_length.copy_(case.ring_l0)
    st._calls = parity
    st.ring_state[2 * parity], st.ring_state[2 * parity + 1] = head, fill
    for pattern in patterns:
        r, v, d, to = case.draw(pattern)
        assert bool((_fma(r, v, (to != 0).float()) != _plain(r, v, (to != 0).float()))[to != 0].any())
        st._update_torch(r, d)
        case.ref.step(r, d)
        tag = (n, W, head, fill, pattern)
        assert _i32(torch.tensor(st.rewbuffer)).tolist() == _i32(torch.tensor(list(case.ref.rewbuffer), dtype=torch.float32)).tolist(), tag
        assert st.lenbuffer == list(case.ref.lenbuffer), tag
        assert torch.equal(_i32(st.cur_reward_sum), _i32(case.ref.cur_reward_sum)) and torch.equal(st.cur_episode_length, case.ref.cur_episode_length), tag


@pytest.mark.parametrize("n", [n for n in SIZES if n <= 4097])
def test_sizes_torch(n):
    _torch_leg(n, 7, 3, 7, 0, ("random", "all", "last"), seed=n)


@pytest.mark.parametrize("state", STATES)
@pytest.mark.parametrize("W", WINDOWS)
def test_patterns_torch(W, state):
    head, fill = _state(state, W)
    for pattern in PATTERNS:
        _torch_leg(2049, W, head, fill, (W + fill) & 1, (pattern,), seed=W * 10 + len(pattern))


# ---- gf_done_compact: one case per path, uint8 masks ------------------------------------------------------------------------------------
COMPACT = {   # path: (n, mask offset in bytes)
    "single": (3 * 4096 + 5, 0),          # one launch: a workgroup counts the masks in front of it with its own SWAR expression
    "two_launch": (131072 + 4096 + 3, 0),  # 34 workgroups of 4 096 envs: above the 32 of the one-launch path
    "unaligned": (3 * 4096 + 5, 3),        # masks 3 bytes off: the element path of both kernels' loads
    "unaligned_two_launch": (131072 + 4096 + 3, 3),
}


def _compact(backend, dev, n, off):
    g = torch.Generator().manual_seed(n + off)
    m1, m2 = _bytes(torch.rand(n, generator=g) < 0.3, g), _bytes(torch.rand(n, generator=g) < 0.1, g)
    for second in (None, m2):
        mask, mask2 = Guarded(n, torch.uint8, dev, off, m1), Guarded(n, torch.uint8, dev, off, m2)
        ids, count = Guarded(n, torch.int64, dev), Guarded(1, torch.int32, dev)
        scratch = Guarded((n + 4095) // 4096 + 1, torch.int32, dev)
        a = nat.GfCompactArgs()
        a.num_envs, a.mask, a.mask2 = n, mask.ptr, (None if second is None else mask2.ptr)
        a.ids_out, a.count_out, a.block_counts = ids.ptr, count.ptr, scratch.ptr
        assert raw_call(backend, "done_compact", a) == 0
        sync(dev)
        want = ((m1 != 0) if second is None else ((m1 != 0) | (m2 != 0))).nonzero().reshape(-1)
        k = int(count.cpu()[0])
        assert k == want.numel(), (n, off, k, want.numel())
        assert torch.equal(ids.cpu()[:k], want), "the ascending index list"
        tail = ids.raw[ids.start + 8 * k:]
        assert bool((tail == 0xA5).all()) and ids.guards_ok(), "wrote past the list"
        assert mask.guards_ok() and mask2.guards_ok() and count.guards_ok() and scratch.guards_ok()
        assert torch.equal(mask.cpu(), m1) and torch.equal(mask2.cpu(), m2)


@pytest.mark.parametrize("path", list(COMPACT))
def test_done_compact_bytes_oracle(oracle_backend, path):
    _compact(oracle_backend, "cpu", *COMPACT[path])


@pytest.mark.gpu
@pytest.mark.parametrize("path", list(COMPACT))
def test_done_compact_bytes_hip(hip_backend, path):
    _compact(hip_backend, "cuda", *COMPACT[path])
