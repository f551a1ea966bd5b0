"""ContactManager.step restated in plain numpy, and the inputs of tests/test_contact_edges.py (helpers only, no tests).

``restate`` is the reference's contact/kernel.py:35-90 (which slots count for a tracked link, the reaction branch, the with-filter,
the mean position) plus contact_manager.py:399-403 (non-finite forces become 0) and :434-477 (air time) for ONE manager, in float64
by default.  It walks the slots in slot order and adds every matched slot's contribution as one step, so evaluated with
``dtype=np.float32`` it is the kernels' arithmetic (gf_contact_tile.h and the oracle both sum in slot order, one rounding per
operation): the self-check of the accuracy bounds uses that.  It is anchored to the reference twice on the CPU
(tests/golden/contact_kernel.npz and contact_edges.npz, tests/test_contact_edges.py).

``make_case`` builds inputs on which float32 arithmetic is EXACT, so that a kernel has to equal the restatement bit for value:
forces and positions are integers of magnitude <= 64, link quaternions are unit Hurwitz quaternions (rot_inv maps integer vectors to
integer vectors), dt = 1/64 and the air-time state is a multiple of it, at most ``MAX_OCCUPIED`` + 2 slots of an env hold a contact (a
summed component stays <= 64 * sqrt(3) * 14 < 2048, so even the sum of squares under the norm is exact) and the air-time thresholds
are k + 0.5.
"""
import itertools

import numpy as np

DT = 1.0 / 64.0
MAX_OCCUPIED = 12   # randomly occupied slots per env (make_case adds up to two)
MAX_ABS = 64        # |force component|, |position component|

# the 24 unit Hurwitz quaternions: (+-1, 0, 0, 0) and its permutations, and (+-1/2, +-1/2, +-1/2, +-1/2)
HURWITZ = np.array([[s if k == j else 0.0 for k in range(4)] for j in range(4) for s in (1.0, -1.0)] +
                   [list(p) for p in itertools.product((0.5, -0.5), repeat=4)], dtype=np.float32)


def rot_inv(q, v):
    """The inverse rotation of v by the quaternion q = (w, x, y, z), q not assumed to have unit length: the formula and the
    operation order of the reference's ti_inv_transform_by_quat as this project records it (tools/ref_stubs.py).  Works in the
    dtype of its arguments."""
    w, a, b, c = q[..., 0], -q[..., 1], -q[..., 2], -q[..., 3]
    two = q.dtype.type(2.0)
    t0 = (b * v[..., 2] - c * v[..., 1]) * two
    t1 = (c * v[..., 0] - a * v[..., 2]) * two
    t2 = (a * v[..., 1] - b * v[..., 0]) * two
    return np.stack([(v[..., 0] + w * t0) + (b * t2 - c * t1),
                     (v[..., 1] + w * t1) + (c * t0 - a * t2),
                     (v[..., 2] + w * t2) + (a * t1 - b * t0)], axis=-1)


def rot_inv_magnitude(q, v):
    """Per output component of rot_inv, the sum of the magnitudes of the terms that enter it: |v_x| + |w t0| + |b t2| + |c t1| with
    t0 bounded by 2 (|b v_z| + |c v_y|), and so on (float64)."""
    q, v = np.abs(q.astype(np.float64)), np.abs(v.astype(np.float64))
    w, a, b, c = q[..., 0], q[..., 1], q[..., 2], q[..., 3]
    t0 = (b * v[..., 2] + c * v[..., 1]) * 2.0
    t1 = (c * v[..., 0] + a * v[..., 2]) * 2.0
    t2 = (a * v[..., 1] + b * v[..., 0]) * 2.0
    return np.stack([v[..., 0] + w * t0 + b * t2 + c * t1, v[..., 1] + w * t1 + c * t0 + a * t2, v[..., 2] + w * t2 + a * t1 + b * t0], axis=-1)


def matched_slots(link_a, link_b, targets, withs):
    """For every slot in slot order that at least one (env, tracked link) pair includes: (slot, env indices, link indices, is_b).
    kernel.py:38-57: the slot involves the tracked link on either side, and with a filter the OTHER side is one of ``withs``."""
    targets = np.asarray(targets, dtype=np.int64)
    wl = None if withs is None else np.asarray(withs, dtype=np.int64)
    for c in np.flatnonzero(((link_a >= 0) | (link_b >= 0)).any(axis=0)):
        la, lb = link_a[:, c].astype(np.int64), link_b[:, c].astype(np.int64)
        is_a, is_b = la[:, None] == targets[None, :], lb[:, None] == targets[None, :]
        inc = is_a | is_b
        if wl is not None:
            inc = (is_a & np.isin(lb, wl)[:, None]) | (is_b & np.isin(la, wl)[:, None])
        n_idx, t_idx = np.nonzero(inc)
        if len(n_idx):
            yield int(c), n_idx, t_idx, is_b[n_idx, t_idx]


def restate(inp, targets, withs=None, threshold=None, air=None, dt=DT, dtype=np.float64):
    """One ContactManager.step.  ``inp``: force / position [N, C, 3], link_a / link_b [N, C], links_quat [N, NL, 4].  ``withs``: the
    with-filter's link ids, None = no filter.  ``air``: (last_air, current_air, last_contact, current_contact), each [N, L], with
    ``threshold`` — or None for a manager that tracks no air time.  Returns forces, pos_sum, counts, positions (the mean, or the
    zero sum where nothing matched), norm, air (the four arrays after the step), flag (a non-finite force component was replaced
    by 0 in a slot this manager includes) and, for error bounds, per output component the sums over the matched slots of |rotated
    force| (terms), of rot_inv_magnitude (mag) and of |position| (pabs)."""
    N, L = inp["link_a"].shape[0], len(targets)
    tg = np.asarray(targets, dtype=np.int64)
    quat = inp["links_quat"].astype(dtype)
    F, P, cnt = np.zeros((N, L, 3), dtype), np.zeros((N, L, 3), dtype), np.zeros((N, L), dtype)
    terms, mag, pabs = (np.zeros((N, L, 3), np.float64) for _ in range(3))
    flag = False
    for c, n_idx, t_idx, is_b in matched_slots(inp["link_a"], inp["link_b"], targets, withs):
        f = inp["force"][n_idx, c].astype(dtype)
        bad = ~np.isfinite(f)
        if bad.any():
            flag = True
            f = np.where(bad, dtype(0.0), f)
        q = quat[n_idx, tg[t_idx]]
        r = rot_inv(q, np.where(is_b[:, None], f, -f))   # the force is expressed on link_b; on link_a it is the reaction
        F[n_idx, t_idx] += r
        P[n_idx, t_idx] += inp["position"][n_idx, c].astype(dtype)
        cnt[n_idx, t_idx] += dtype(1.0)
        terms[n_idx, t_idx] += np.abs(r.astype(np.float64))
        mag[n_idx, t_idx] += rot_inv_magnitude(q, f)
        pabs[n_idx, t_idx] += np.abs(inp["position"][n_idx, c].astype(np.float64))
    with np.errstate(invalid="ignore", divide="ignore"):
        mean = np.where(cnt[..., None] > 0, P / np.where(cnt > 0, cnt, dtype(1.0))[..., None], P)
    norm = np.sqrt(F[..., 0] * F[..., 0] + F[..., 1] * F[..., 1] + F[..., 2] * F[..., 2])
    out = dict(forces=F, pos_sum=P, counts=cnt, positions=mean, norm=norm, flag=flag, terms=terms, mag=mag, pabs=pabs, air=None)
    if air is not None:
        last_air, cur_air, last_con, cur_con = (x.astype(dtype) for x in air)
        d = dtype(dt)
        is_contact = norm > dtype(np.float32(threshold))
        new_contact, new_detach = (cur_air > 0) & is_contact, (cur_con > 0) & ~is_contact
        out["air"] = (np.where(new_contact, cur_air + d, last_air), np.where(~is_contact, cur_air + d, dtype(0.0)),
                      np.where(new_detach, cur_con + d, last_con), np.where(is_contact, cur_con + d, dtype(0.0)))
        out["is_contact"] = is_contact
    return out


# ----------------------------------------------------------------------------------------------------
# inputs of the exact leg
# ----------------------------------------------------------------------------------------------------
def split_managers(T, rng, num_links, id_max=None, mode="auto"):
    """The managers of a case with T tracked links: ``mode`` 'auto' = one manager without a filter and one with (a single with-filter
    manager when T == 1), 'one' = one with-filter manager, 'four' = four managers of T / 4 links, a list = managers of these sizes.  Every manager tracks air time, with
    a threshold of the form k + 0.5.  Ids are distinct scene links; ``id_max`` (when given) is among them, and among the with ids."""
    ids = rng.permutation(num_links).astype(np.int64)
    if id_max is not None:
        ids = np.concatenate([[id_max], ids[ids != id_max]])
    ids = ids[:T + 6]
    tracked, others = ids[:T], ids[T:]
    if isinstance(mode, (list, tuple)):   # the managers' sizes
        cuts = np.cumsum([0] + list(mode))
        parts = [tracked[cuts[k]:cuts[k + 1]] for k in range(len(mode))]
    elif mode == "four":
        parts = [tracked[k * (T // 4):(k + 1) * (T // 4)] for k in range(4)]
    elif mode == "one" or T == 1:
        parts = [tracked]
    else:
        parts = [tracked[:(T + 1) // 2], tracked[(T + 1) // 2:]]
    mgrs = []
    for k, part in enumerate(parts):
        filtered = (k % 2 == 1) or len(parts) == 1
        withs = None
        if filtered:   # own links, links of the other managers and untracked ones (kernel.py:47-57)
            withs = [int(x) for x in np.concatenate([others[:3], tracked[::2][:8]])]
        mgrs.append(dict(targets=[int(x) for x in part], withs=withs, threshold=float(rng.randint(0, 60)) + 0.5))
    return mgrs, others


def make_case(N, C, T, seed, num_links=None, id_max=None, mode="auto"):
    """Exact inputs (module docstring) for N envs, C slots and T tracked links over the managers of ``split_managers``.  Every kind of
    slot occurs: the tracked link on side a, side b and both (a self-contact), one side -1, both sides -1 (an empty slot), pairs of
    untracked links, pairs of two tracked links; non-finite force components sit in slots that a manager includes."""
    rng = np.random.RandomState(seed)
    NL = num_links if num_links is not None else max(T + 8, 40)
    mgrs, others = split_managers(T, rng, NL, id_max, mode)
    tracked = np.concatenate([m["targets"] for m in mgrs])
    pool = np.concatenate([tracked, others]).astype(np.int32)
    la = np.full((N, C), -1, np.int32)
    lb = np.full((N, C), -1, np.int32)
    K = min(C, MAX_OCCUPIED)
    if C > 0:
        # occupied slots: random ones, and the first and the last slot of every env's row (the ends of the mask words and of the tail)
        occ = np.argsort(rng.uniform(size=(N, C)), axis=1)[:, :K]
        occ[::2, 0] = C - 1
        occ[1::3, K - 1] = 0
        rows = np.arange(N)[:, None]
        a = pool[rng.randint(0, len(pool), (N, K))]
        b = pool[rng.randint(0, len(pool), (N, K))]
        kind = rng.uniform(size=(N, K))
        b = np.where(kind < 0.12, a, b)                    # self-contact
        a = np.where((kind >= 0.12) & (kind < 0.24), -1, a)   # only side b
        b = np.where((kind >= 0.24) & (kind < 0.36), -1, b)   # only side a
        la[rows, occ], lb[rows, occ] = a, b                # (a slot drawn twice keeps its last pair)
        # the last slot of every env — the end of a workgroup's scalar tail — holds a contact that one of the managers includes
        for env in range(N):
            m = mgrs[env % len(mgrs)]
            pair = (m["targets"][env % len(m["targets"])], m["withs"][0] if m["withs"] is not None else -1)
            la[env, C - 1], lb[env, C - 1] = pair if (env // 2) % 2 == 0 else pair[::-1]
    force = rng.randint(-MAX_ABS, MAX_ABS + 1, (N, C, 3)).astype(np.float32)
    position = rng.randint(-MAX_ABS, MAX_ABS + 1, (N, C, 3)).astype(np.float32)
    if C > 0:   # non-finite components where manager 0 includes them whatever its filter: its own link against its first with link
        t0 = mgrs[0]["targets"][0]
        w0 = mgrs[0]["withs"][0] if mgrs[0]["withs"] is not None else -1
        for env, slot, comp, val in ((0, 0, 0, np.nan), (N // 2, C - 1, 1, np.inf), (N - 1, C // 2, 2, -np.inf)):
            la[env, slot], lb[env, slot] = (t0, w0) if comp != 1 else (w0, t0)
            force[env, slot, comp] = val
    inp = dict(force=force, position=position, link_a=la, link_b=lb,
               links_quat=HURWITZ[rng.randint(0, 24, (N, NL))],
               links_vel=rng.randint(-MAX_ABS, MAX_ABS + 1, (N, NL, 3)).astype(np.float32),
               links_pos=rng.randint(-MAX_ABS, MAX_ABS + 1, (N, NL, 3)).astype(np.float32))
    for m in mgrs:   # air-time state in multiples of dt, many of them 0 (both branches of `> 0`)
        L = len(m["targets"])
        m["air"] = tuple((rng.randint(0, 6, (N, L)) * (rng.uniform(size=(N, L)) < 0.6)).astype(np.float32) * np.float32(DT) for _ in range(4))
    return dict(N=N, C=C, T=T, NL=NL, inp=inp, mgrs=mgrs, dt=DT)


def expected_exact(case):
    """Per manager, what a kernel must leave on an exact case: float32 arrays.  Checks the conditions on the inputs that make the
    comparison an equality: summed components <= 2048, and every norm further than 2^-20 of itself from the threshold."""
    want = []
    for m in case["mgrs"]:
        r = restate(case["inp"], m["targets"], m["withs"], m["threshold"], m["air"], case["dt"])
        assert np.abs(r["forces"]).max(initial=0.0) <= 2048 and np.abs(r["pos_sum"]).max(initial=0.0) <= 2048, "contact density too high for exact sums"
        assert (np.abs(r["norm"] - m["threshold"]) > 2.0 ** -20 * r["norm"]).all(), "a norm sits on its threshold"
        f32 = lambda a: a.astype(np.float32)
        assert all(np.array_equal(f32(r[k]).astype(np.float64), r[k]) for k in ("forces", "pos_sum", "counts"))
        cnt = f32(r["counts"])
        with np.errstate(invalid="ignore", divide="ignore"):
            mean = np.where(cnt[..., None] > 0, f32(r["pos_sum"]) / np.where(cnt > 0, cnt, np.float32(1.0))[..., None], f32(r["pos_sum"]))
        tg = np.asarray(m["targets"])
        want.append(dict(contacts=f32(r["forces"]), contact_positions=mean.astype(np.float32), position_counts=cnt,
                         air=[f32(x) for x in r["air"]], link_vel=case["inp"]["links_vel"][:, tg], link_pos=case["inp"]["links_pos"][:, tg],
                         flag=r["flag"]))
    return want


# ----------------------------------------------------------------------------------------------------
# inputs and bounds of the accuracy leg
# ----------------------------------------------------------------------------------------------------
U32 = 2.0 ** -24   # unit roundoff of float32


def make_float_case(N, C, T, seed, num_links=None, id_max=None, mode="auto"):
    """The slots, ids and air-time state of make_case with random float data: Gaussian forces of O(30 N), Gaussian positions and link
    kinematics, random unit quaternions of which a third are scaled off unit length (as in the entity_obs fixture: the kernels do not
    normalise, neither does the reference)."""
    case = make_case(N, C, T, seed, num_links, id_max, mode)
    rng = np.random.RandomState(seed + 1000)
    inp, NL = case["inp"], case["NL"]
    bad = ~np.isfinite(inp["force"])
    inp["force"] = np.where(bad, inp["force"], (30.0 * rng.standard_normal((N, C, 3)))).astype(np.float32)
    inp["position"] = rng.standard_normal((N, C, 3)).astype(np.float32)
    q = rng.standard_normal((N, NL, 4))
    q /= np.linalg.norm(q, axis=-1, keepdims=True)
    q *= np.where(rng.uniform(size=(N, NL, 1)) < 1.0 / 3.0, rng.uniform(0.8, 1.25, (N, NL, 1)), 1.0)
    inp["links_quat"] = q.astype(np.float32)
    inp["links_vel"] = rng.standard_normal((N, NL, 3)).astype(np.float32)
    inp["links_pos"] = rng.standard_normal((N, NL, 3)).astype(np.float32)
    return case


def accuracy_bounds(r, threshold):
    """Bounds on |float32 kernel - float64 restatement ``r``| from counting roundings (u = 2^-24, first order, times 1.001 for the
    higher-order terms; the float64 side's own error is 2^-29 of that).

    rot_inv, component x = (v_x + w t0) + (b t2 - c t1), t0 = (b v_z - c v_y) 2: with T0 = 2 (|b v_z| + |c v_y|) >= |t0|, the two
    products and the difference leave |dt0| <= 2u T0 (the doubling is exact); w t0 adds its own rounding: 3u |w| T0; the sum with
    v_x: u |v_x| + 4u |w| T0; likewise b t2 - c t1: 4u (|b| T2 + |c| T1); the final addition rounds once more, at most u times the
    magnitudes: in all <= u (2 |v_x| + 5 |w| T0 + 5 |b| T2 + 5 |c| T1) <= 5u M_x, M = rot_inv_magnitude.  Negating v is exact.
    The float32 sum of the k matched slots' contributions in slot order adds at most (k - 1) u sum |term|.
    Mean position: the same sum bound on the position sum, (k - 1) u sum |p| — kept undivided, the division by k only shrinks it —
    plus the one rounding of the division, u |mean|.
    Norm (sqrt of two fused multiply-adds over a product): at most the Euclidean length of the force bound plus 3u of the norm.
    Returns (force bound [N, L, 3], position bound [N, L, 3], decided [N, L]: the float64 norm is further from the threshold than
    its bound, so is_contact is determined)."""
    k = r["counts"].astype(np.float64)[..., None]
    fb = 1.001 * U32 * (5.0 * r["mag"] + np.maximum(k - 1.0, 0.0) * r["terms"])
    pb = 1.001 * U32 * (np.maximum(k - 1.0, 0.0) * r["pabs"] + np.abs(r["positions"]))
    nb = np.linalg.norm(fb, axis=-1) + 3.0 * U32 * r["norm"]
    return fb, pb, np.abs(r["norm"] - threshold) > nb
