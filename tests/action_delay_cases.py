"""Restatement and inputs for tests/test_action_delay.py: gf_action_delay's contract (include/gf_step.h) in numpy — values move as
int32 views (bits), the one float32 product of the lag draw is rounded once —, the Philox draws of the kernel's block layout, and the
sequences of calls the kernel is walked through.  Nothing here imports the HIP library.

A *case* names a shape, a ring size, a lag range and what makes envs fresh; ``script(case)`` turns it into a start state and
T = 2L + 3 calls, ``walk(case)`` runs the restatement over them, and ``conditions(case)`` asserts what the case is there to show:
every lag of a randomised range occurs, fresh and ordinary envs meet in one call, an env reads a slot written before ``head`` wrapped."""
import numpy as np

import philox

MAX_SLOTS = 64                  # GF_ACTION_DELAY_MAX_SLOTS (asserted against the binding in the tests)
SEED_TAG = 0xAC7DE1A7C0FFEE5D   # GF_ACTION_DELAY_SEED_TAG (asserted against the binding in the tests)
F = np.float32
M32 = 0xFFFFFFFF

#: N at 1, around the wave, around the workgroup's 256 lanes, and a size of several workgroups that is no multiple of a wave
SIZES = [1, 63, 64, 65, 255, 256, 257, 1000]
#: D = 1, 3 and 13 go element by element (N * D % 4 != 0 among them, and at D = 3 a 16-byte word that would straddle two envs),
#: D = 4 and 12 as 16-byte words
DOFS = [1, 3, 4, 12, 13]
SLOTS = [1, 2, 3, 8, 64]
#: what makes an env fresh in a sequence
SOURCES = ["episode_length", "mask", "mask2", "prime_all", "combined", "nobody", "everybody"]


def case(n=65, d=12, slots=3, lag=None, source="combined", philox_mode=True, env_offset=0, step0=100, head0=0, seed=0, key=0x1234_5678_9ABC):
    lag = (0, slots - 1) if lag is None else lag
    return dict(n=n, d=d, slots=slots, lag=tuple(lag), source=source, philox=philox_mode, env_offset=env_offset, step0=step0, head0=head0,
                seed=seed, key=key, calls=2 * slots + 3)


def case_id(c):
    return (f"N{c['n']}-D{c['d']}-L{c['slots']}-lag{c['lag'][0]}_{c['lag'][1]}-{c['source']}-{'philox' if c['philox'] else 'draws'}"
            f"-off{c['env_offset']}-step{c['step0']:#x}-head{c['head0']}")


def shape_cases():
    """Every N with every D at L = 3.  One env cannot show three lags: it gets a fixed one — and a seed at which it is fresh in some
    calls and not in others and reads across a wrap (``conditions``; seeds that did not give that were replaced by these)."""
    one = {1: 1000, 3: 1001, 4: 1000, 12: 1001, 13: 1000}
    return [case(n=n, d=d, slots=3, lag=(2, 2) if n == 1 else (0, 2), seed=one[d] if n == 1 else n * 16 + d) for n in SIZES for d in DOFS]


def slot_cases():
    """Every L with a 16-byte and an element-wise D, the whole range of lags, head starting in the middle of the ring."""
    return [case(n=65, d=d, slots=L, head0=L // 2, seed=L * 16 + d) for L in SLOTS for d in (12, 13)]


def source_cases():
    out = [case(n=257, d=12, slots=3, head0=1, source=s, seed=40 + i) for i, s in enumerate(SOURCES)]
    out += [case(n=257, d=13, slots=8, lag=(1, 5), source=s, seed=60 + i) for i, s in enumerate(SOURCES)]
    return out


def draw_cases():
    return [case(n=257, d=12, slots=8, philox_mode=False, seed=80),                        # parity draws
            case(n=257, d=12, slots=8, step0=(1 << 32) - 4, seed=81),                      # the call counter crosses 2^32
            case(n=257, d=3, slots=3, step0=(1 << 32) - 2, seed=82),
            case(n=257, d=12, slots=8, env_offset=17, seed=83),
            case(n=257, d=12, slots=8, env_offset=4_294_967_290, seed=84),                 # n + env_offset wraps
            case(n=257, d=12, slots=8, key=0xFEED_5EED_0123_4567, seed=85)]


def all_cases():
    return shape_cases() + slot_cases() + source_cases() + draw_cases()


# ---------------------------------------------------------------------------------------------------------------------------
# draws and the restatement
# ---------------------------------------------------------------------------------------------------------------------------
def philox_draws(seed, step, n, env_offset):
    """[n] u: the x word of the block with key seed ^ SEED_TAG and counter (n + env_offset modulo 2^32, 0, step, 0)."""
    key = (int(seed) ^ SEED_TAG) & 0xFFFFFFFFFFFFFFFF
    ids = ((np.arange(n, dtype=np.uint64) + np.uint64(env_offset)) & np.uint64(M32)).astype(np.uint32)
    return np.ascontiguousarray(philox.block_uniform(key, int(step) & M32, ids, 0)[:, 0])


def reference(st, call, cfg):
    """One launch.  ``st``: ring [L, N, D], lag [N], out [N, D]; ``call``: in [N, D], episode_length / mask / mask2 ([N] or None),
    prime_all, head, u ([N] draws); ``cfg``: lag_lo, lag_hi.  Returns (state after, fresh [N], slot read [N] or -1)."""
    x = np.ascontiguousarray(call["in"]).view(np.int32)
    ring, lag, out = st["ring"].view(np.int32).copy(), st["lag"].copy(), st["out"].view(np.int32).copy()
    L, n = ring.shape[0], lag.shape[0]
    head = int(call["head"])
    assert 0 <= head < L and 0 <= cfg["lag_lo"] <= cfg["lag_hi"] <= L - 1
    # 1
    fresh = np.full(n, bool(call["prime_all"]))
    if call["episode_length"] is not None:
        fresh = fresh | (call["episode_length"] <= 1)
    for k in ("mask", "mask2"):
        if call[k] is not None:
            fresh = fresh | call[k].astype(bool)
    # 2
    w = int(cfg["lag_hi"]) - int(cfg["lag_lo"]) + 1
    prod = call["u"] * F(w)
    assert prod.dtype == F
    new_lag = int(cfg["lag_lo"]) + np.minimum(np.where(fresh, prod, F(0)).astype(np.int32), w - 1)   # (an unused draw may hold anything)
    # 4
    old = ~fresh
    l = np.where((lag < 0) | (lag >= L), 0, lag)
    src = (head + L - l) % L
    lagged = ring[src, np.arange(n)]              # before the write: src != head wherever l != 0
    ring[head, old] = x[old]
    out[old] = np.where((l == 0)[:, None], x, lagged)[old]
    # 3
    ring[:, fresh] = x[fresh]
    out[fresh] = x[fresh]
    lag[fresh] = new_lag[fresh]
    read = np.where(old & (l != 0), src, -1)
    return {"ring": ring.view(F), "lag": lag.astype(np.int32), "out": out.view(F)}, fresh, read


SPECIALS = np.array([0x7FC12345, 0x7F800000, 0xFF800000, 0x80000000, 0x7F800001, 0x7FC00000, 0xFFC00001, 0x00000001, 0x807FFFFF],
                    dtype=np.uint32).view(F)   # a NaN with a payload, +-Inf, -0.0, a signalling NaN, more NaNs, subnormals


def script(c):
    """(start state, calls).  The start state is arbitrary but valid (lags in 0 … L-1), so that a sequence in which nobody is ever
    fresh still has a history; ``in`` is random with NaN / Inf / -0.0 / subnormal bit patterns planted in every call."""
    n, d, L = c["n"], c["d"], c["slots"]
    rng = np.random.default_rng(c["seed"])
    st = {"ring": rng.normal(size=(L, n, d)).astype(F), "lag": rng.integers(0, L, n).astype(np.int32), "out": rng.normal(size=(n, d)).astype(F)}
    calls = []
    for t in range(c["calls"]):
        x = rng.normal(size=(n, d)).astype(F)
        # a seventh of the values, walking through SPECIALS from call to call; below seven values, one in every other call (the
        # first five of SPECIALS within the shortest sequence, 5 calls of 9)
        k = n * d // 7
        if k:
            x.reshape(-1)[rng.choice(n * d, k, replace=False)] = SPECIALS[(t * k + np.arange(k)) % SPECIALS.size]
        elif t % 2 == 0:
            x.reshape(-1)[rng.integers(0, n * d)] = SPECIALS[(t // 2) % SPECIALS.size]
        src = c["source"]
        ep = mask = mask2 = None
        prime = 0
        some = lambda p=0.15: rng.random(n) < p
        if src == "episode_length":
            ep = rng.choice(np.array([0, 1, 2, 3, 500], dtype=np.int32), n, p=[0.05, 0.1, 0.35, 0.25, 0.25])
        elif src == "mask":
            mask = some()
        elif src == "mask2":
            mask2 = some()
        elif src == "prime_all":
            prime = int(t in (0, L + 1))
        elif src == "combined":
            ep = rng.choice(np.array([0, 1, 2, 7], dtype=np.int32), n, p=[0.03, 0.05, 0.42, 0.5])
            mask, mask2 = some(0.05), (some(0.05) if t % 2 else None)
        elif src == "nobody":              # every pointer null from the second call on, no prime: nobody is fresh
            if t == 0:
                ep, mask, mask2 = np.full(n, 2, dtype=np.int32), np.zeros(n, dtype=bool), np.zeros(n, dtype=bool)
        elif src == "everybody":           # each source alone makes everybody fresh, in turn
            which = t % 4
            ep = np.full(n, t % 2, dtype=np.int32) if which == 0 else (np.full(n, 9, dtype=np.int32) if which == 3 else None)
            mask = np.ones(n, dtype=bool) if which == 1 else None
            mask2 = np.ones(n, dtype=bool) if which == 2 else None
            prime = int(which == 3)
        else:
            raise KeyError(src)
        step = (c["step0"] + t) & M32
        u = philox_draws(c["key"], step, n, c["env_offset"]) if c["philox"] else rng.random(n).astype(F)
        u[u >= 1.0] = 0.5
        calls.append({"in": x, "episode_length": ep, "mask": mask, "mask2": mask2, "prime_all": prime, "head": (c["head0"] + t) % L,
                      "step": step, "u": u})
    return st, calls


def walk(c):
    """The restatement over the case's calls: [(state after, fresh, slot read)]."""
    st, calls = script(c)
    cfg = {"lag_lo": c["lag"][0], "lag_hi": c["lag"][1]}
    out = []
    for call in calls:
        st, fresh, read = reference(st, call, cfg)
        out.append((st, fresh, read))
    return out


def conditions(c, trail=None):
    """What the case must show, asserted on the restatement.  ``nobody`` / ``everybody`` are the two cases that are there to lack the
    mix; one env, or prime_all alone, cannot have fresh and ordinary envs in one call (both kinds of call must occur then); a ring of
    one slot is never read."""
    trail = walk(c) if trail is None else trail
    _st, calls = script(c)
    n, L, (lo, hi) = c["n"], c["slots"], c["lag"]
    fresh_any = [f for _s, f, _r in trail]
    if c["source"] == "nobody":
        assert not any(f.any() for f in fresh_any), "somebody is fresh"
    elif c["source"] == "everybody":
        assert all(f.all() for f in fresh_any), "somebody is not fresh"
    else:
        later = fresh_any[1:]
        if n > 1 and c["source"] != "prime_all":   # (prime_all alone: everybody or nobody, by construction)
            assert any(f.any() and not f.all() for f in later), "no call after the first has fresh and ordinary envs"
        else:
            assert any(f.all() for f in later) and any(not f.any() for f in later), "the env is never fresh, or always"
    if lo < hi and c["source"] != "nobody":
        drawn = set()
        for (st, f, _r) in trail:
            drawn |= set(st["lag"][f].tolist())
        assert drawn == set(range(lo, hi + 1)), f"lags drawn: {sorted(drawn)}"
    if L > 1 and c["source"] != "everybody":
        # the slot read in call t was written l = (head - slot) % L calls ago — by this sequence when t - l >= 0 —, and head has passed
        # L - 1 since then exactly when the slot's index is above head
        wrapped = False
        for t, ((_s, _f, read), call) in enumerate(zip(trail, calls)):
            got = read[read >= 0]
            wrapped = wrapped or bool(((got > call["head"]) & (t - (call["head"] - got) % L >= 0)).any())
        assert wrapped, "no env reads a slot written before head wrapped"
    for (st, _f, _r) in trail:
        assert ((st["lag"] >= 0) & (st["lag"] <= L - 1)).all()
