"""Mirror symmetry of the PPO update: ``MirrorSymmetry``, ``gf_mirror_rows``, ``gf_mirror_loss``, ``gf_ppo_loss``'s ``kl_rows`` and
``learner.PPO(symmetry_cfg=...)`` against rsl_rl's update restated in torch (tests/rsl_rl_symmetry.py).

* CPU: table validation, ``from_items`` / ``repeat_frames`` against hand-written tables, ``__call__`` against explicit indexing, every
  refusal of the two new entry points and of ``kl_rows`` through the raw ABI (never-dereferenced pointers), the ``PPO`` refusals, and
  the oracle-backend ``PPO.update`` with each flag combination against the restatement.
* GPU: ``gf_mirror_rows`` bit for bit against torch indexing; ``gf_mirror_loss`` against float64 within the derived bounds;
  ``kl_rows``; ``PPO.update`` end to end, its host reads, and a policy that is symmetric by construction."""
import copy
import ctypes as C

import pytest
import torch

import test_ppo_update as tpu
from rsl_rl_symmetry import RslRlSymmetryPPO
from test_log_std import _as_rsl_rl, _recorded_kl

ALGO = tpu.ALGO
U = 2.0 ** -24   # unit roundoff of float32
E_NULL, E_RANGE = -1, -2
FAKE = 1 << 20   # (16-byte aligned; never dereferenced)

# Go2: joints FL, FR, RL, RR x (hip, thigh, calf) — the legs swap sides, the hip (abduction) changes sign; under y -> -y a velocity
# and the gravity direction flip y, an angular velocity (a pseudo-vector) flips x and z, the command (vx, vy, yaw rate) vy and yaw
JOINTS = ([3, 4, 5, 0, 1, 2, 9, 10, 11, 6, 7, 8], [-1, 1, 1] * 4)
ITEMS = {"velocity_cmd": ([0, 1, 2], [1, -1, -1]), "angle_velocity": ([0, 1, 2], [-1, 1, -1]), "linear_velocity": ([0, 1, 2], [1, -1, 1]),
         "projected_gravity": ([0, 1, 2], [1, -1, 1]), "dof_position": JOINTS, "dof_velocity": JOINTS, "actions": JOINTS}


def _random_involution(w, seed):
    """A random signed involution of ``w`` columns: random 2-cycles (sign ±1, the same on both ends) and fixed points (sign ±1)."""
    g = torch.Generator().manual_seed(seed * 1009 + w)
    order = torch.randperm(w, generator=g).tolist()
    perm, sign = list(range(w)), [1.0] * w
    while len(order) >= 2 and len(order) > w // 5:
        a, b = order.pop(), order.pop()
        perm[a], perm[b] = b, a
        sign[a] = sign[b] = 1.0 if int(torch.randint(0, 2, (1,), generator=g)) else -1.0
    for a in order:
        sign[a] = 1.0 if int(torch.randint(0, 2, (1,), generator=g)) else -1.0
    return perm, sign


def _tables(kind, w, seed=0):
    if kind == "identity":
        return list(range(w)), [1.0] * w
    if kind == "reversal":
        return list(range(w - 1, -1, -1)), [1.0] * w
    return _random_involution(w, seed)


# ---- CPU: MirrorSymmetry -----------------------------------------------------------------------------------------------------------
def test_table_validation():
    from genesis_forge_amd import MirrorSymmetry

    ok = ([1, 0, 2], [1, 1, -1])
    MirrorSymmetry(*ok, *ok)
    for bad, word in ((([0, 0, 2], [1, 1, 1]), "permutation"), (([0, 1, 3], [1, 1, 1]), "permutation"), (([0, 1, -1], [1, 1, 1]), "permutation"),
                      (([1, 0, 2], [1, 1, 0]), "sign"), (([1, 0, 2], [1, 1, 2]), "sign"), (([1, 2, 0], [1, 1, 1]), "involution"),
                      (([1, 0, 2], [1, -1, 1]), "involution"), (([1, 0, 2], [1, 1]), "sign"), (([0.5, 1, 2], [1, 1, 1]), "integers"),
                      (([], []), "non-empty")):
        for slot, name in ((0, "obs"), (1, "act"), (2, "critic_obs")):
            args = [ok, ok, ok]
            args[slot] = bad
            with pytest.raises(ValueError, match=word) as e:
                MirrorSymmetry(*args[0], *args[1], *args[2])
            assert name + "_" in str(e.value), f"the message names the table: {e.value}"
    with pytest.raises(ValueError, match="critic_obs"):
        MirrorSymmetry(*ok, *ok, critic_obs_perm=[0, 1, 2])
    s = MirrorSymmetry(*ok, [0], [-1])
    assert (s.obs_width, s.critic_obs_width, s.num_actions) == (3, 3, 1)
    p, sg = s.tables("policy", "cpu")
    assert p.dtype == torch.int32 and sg.dtype == torch.float32 and p.tolist() == [1, 0, 2] and sg.tolist() == [1.0, 1.0, -1.0]
    assert s.tables("policy", "cpu")[0] is p, "uploaded once per device"
    assert s.tables("critic", "cpu")[0].tolist() == [1, 0, 2], "the critic uses the policy tables when it has none"
    with pytest.raises(ValueError, match="wide"):
        s.mirror(torch.zeros(2, 4))


def test_from_items_and_history_against_hand_written_tables():
    from genesis_forge_amd import MirrorSymmetry

    widths = [("cmd", 3), ("height", 1), ("dofs", 4)]
    items = {"cmd": ([0, 1, 2], [1, -1, -1]), "dofs": ([2, 3, 0, 1], [-1, 1, -1, 1])}
    perm, sign = MirrorSymmetry.item_tables(widths, items)
    assert perm.tolist() == [0, 1, 2, 3, 6, 7, 4, 5] and sign.tolist() == [1, -1, -1, 1, -1, 1, -1, 1]
    assert MirrorSymmetry.item_tables(dict(widths), items)[0].tolist() == perm.tolist()
    p3, s3 = MirrorSymmetry.repeat_frames(perm, sign, 3)
    assert p3.tolist() == [0, 1, 2, 3, 6, 7, 4, 5, 8, 9, 10, 11, 14, 15, 12, 13, 16, 17, 18, 19, 22, 23, 20, 21]
    assert s3.tolist() == [1, -1, -1, 1, -1, 1, -1, 1] * 3
    assert MirrorSymmetry.item_tables(widths, items, history_len=3)[0].tolist() == p3.tolist()
    group = MirrorSymmetry.item_tables([widths, [("extra", 2)]], dict(items, extra=([1, 0], [1, 1])))
    assert group[0].tolist() == [0, 1, 2, 3, 6, 7, 4, 5, 9, 8]
    with pytest.raises(ValueError, match="'dofs' is 3 wide"):
        MirrorSymmetry.item_tables(widths, {"dofs": ([0, 2, 1], [1, 1, 1])})
    with pytest.raises(ValueError, match="no item"):
        MirrorSymmetry.item_tables(widths, {"feet": ([0], [1])})
    with pytest.raises(ValueError, match="history_len"):
        MirrorSymmetry.repeat_frames(perm, sign, 0)
    sym = MirrorSymmetry.from_items(widths, items, [1, 0], [1, 1], critic_obs=[widths, [("extra", 2)]], critic_items=items)
    assert (sym.obs_width, sym.critic_obs_width, sym.num_actions) == (8, 10, 2)
    assert sym.host_tables("critic")[0].tolist() == [0, 1, 2, 3, 6, 7, 4, 5, 8, 9]


def test_from_items_reads_a_built_observation_manager(oracle_backend):
    """The Go2 task's manager, with history: the frame table repeated over the frames the manager keeps."""
    from genesis_forge_amd import MirrorSymmetry, tasks

    env = tasks.Go2CommandDirectionEnv(num_envs=4, history=3)
    env.build()
    om = env.managers["observation"][0]
    names = [n for n, *_ in om._plan]
    items = {k: v for k, v in ITEMS.items() if k in names}
    sym = MirrorSymmetry.from_items(om, items, *JOINTS)
    frame = sum(w for *_x, w in om._plan)
    assert sym.obs_width == 3 * frame == om.observation_space.shape[0]
    one = MirrorSymmetry.item_tables([(n, w) for n, _c, _s, w in om._plan], items)
    p, s = sym.host_tables("policy")
    for h in range(3):
        assert p[h * frame:(h + 1) * frame].tolist() == (one[0] + h * frame).tolist() and s[h * frame:(h + 1) * frame].tolist() == one[1].tolist()
    at = names.index("dof_position")
    col = sum(w for *_x, w in om._plan[:at])
    assert p[col:col + 12].tolist() == [col + j for j in JOINTS[0]] and s[col:col + 12].tolist() == [float(x) for x in JOINTS[1]]


def test_call_is_rsl_rls_augmentation_function():
    from genesis_forge_amd import MirrorSymmetry

    op, osg = _random_involution(7, 1)
    cp, csg = _random_involution(9, 2)
    ap, asg = _random_involution(4, 3)
    sym = MirrorSymmetry(op, osg, ap, asg, cp, csg)
    g = torch.Generator().manual_seed(0)
    obs, cobs, act = torch.randn(5, 7, generator=g), torch.randn(5, 9, generator=g), torch.randn(5, 4, generator=g)

    def explicit(x, perm, sign):
        out = torch.empty_like(x)
        for n in range(x.shape[0]):
            for j in range(x.shape[1]):
                out[n, j] = sign[j] * x[n, perm[j]]
        return out

    o, a = sym(obs=obs, actions=act, env=None, obs_type="policy")
    assert torch.equal(o, torch.cat([obs, explicit(obs, op, osg)])) and torch.equal(a, torch.cat([act, explicit(act, ap, asg)]))
    c, none = sym(obs=cobs, actions=None, obs_type="critic")
    assert none is None and torch.equal(c, torch.cat([cobs, explicit(cobs, cp, csg)]))
    none, a = sym(obs=None, actions=act)
    assert none is None and a.shape == (10, 4)
    assert torch.equal(sym.mirror(sym.mirror(obs)), obs), "an involution"
    assert sym(obs.double())[0].dtype == torch.float64


# ---- CPU: the raw ABI ------------------------------------------------------------------------------------------------------------------
def _lib():
    from genesis_forge_amd import _native as nat

    lib = C.CDLL(nat.lib_path())
    lib.gf_sizeof.restype = C.c_int
    for f, st in ((lib.gf_mirror_rows, nat.GfMirrorRowsArgs), (lib.gf_mirror_loss, nat.GfMirrorLossArgs), (lib.gf_ppo_loss, nat.GfPpoLossArgs)):
        f.restype, f.argtypes = C.c_int, [C.POINTER(st), C.c_void_p]
    return lib, nat


def test_abi_sizes_and_refusals():
    """ABI 11, gf_sizeof 31 / 32 / 26 against the binding, and every refusal returns its code before any launch (no device is
    touched: the non-NULL pointers are never dereferenced)."""
    lib, nat = _lib()
    lib.gf_abi_version.restype = C.c_int
    assert lib.gf_abi_version() == nat.GF_ABI_VERSION == 11
    assert (nat.GF_SIZEOF_MIRROR_ROWS, nat.GF_SIZEOF_MIRROR_LOSS) == (31, 32)
    assert lib.gf_sizeof(31) == C.sizeof(nat.GfMirrorRowsArgs) == 16 + 4 * 72 + 4 * 16
    assert lib.gf_sizeof(32) == C.sizeof(nat.GfMirrorLossArgs) == 88
    assert lib.gf_sizeof(nat.GF_SIZEOF_PPO_LOSS) == C.sizeof(nat.GfPpoLossArgs)
    assert nat.GfPpoLossArgs.kl_rows.offset == C.sizeof(nat.GfPpoLossArgs) - 8, "kl_rows is the trailing field"

    def rows_args(fields=1, scalars=1, **kw):
        a = nat.GfMirrorRowsArgs()
        a.num_rows, a.num_fields, a.num_scalars = 100, fields, scalars
        for f in a.fields:
            f.src = f.dst_copy = f.dst_mirror = f.perm = f.sign = f.in_mean = f.in_std = FAKE
            f.width, f.row_stride, f.in_eps = 48, 0, 0.01
        for s in a.scalars:
            s.src = s.dst = FAKE
        for k, v in kw.items():
            if k.startswith("f_"):
                setattr(a.fields[0], k[2:], v)
            elif k.startswith("s_"):
                setattr(a.scalars[0], k[2:], v)
            else:
                setattr(a, k, v)
        return a

    call = lambda a: lib.gf_mirror_rows(C.byref(a), None)
    assert lib.gf_mirror_rows(None, None) == E_NULL
    for k in ("src", "dst_mirror", "perm", "sign"):
        assert call(rows_args(**{"f_" + k: None})) == E_NULL, k
    assert call(rows_args(f_in_std=None)) == E_NULL, "a mean without a std"
    for k in ("src", "dst"):
        assert call(rows_args(**{"s_" + k: None})) == E_NULL, k
    assert call(rows_args(num_rows=-1)) == E_RANGE
    assert call(rows_args(fields=-1)) == E_RANGE and call(rows_args(fields=nat.GF_MIRROR_MAX_FIELDS + 1)) == E_RANGE
    assert call(rows_args(scalars=-1)) == E_RANGE and call(rows_args(scalars=nat.GF_MIRROR_MAX_SCALARS + 1)) == E_RANGE
    assert call(rows_args(fields=0, scalars=0)) == E_RANGE, "nothing to do"
    assert call(rows_args(f_width=0)) == E_RANGE and call(rows_args(f_width=nat.GF_MIRROR_MAX_WIDTH + 1)) == E_RANGE
    assert call(rows_args(f_row_stride=47)) == E_RANGE and call(rows_args(f_row_stride=-4)) == E_RANGE
    assert call(rows_args(num_rows=0)) == 0, "no rows: a no-op"
    assert call(rows_args(num_rows=0, f_dst_copy=None, f_in_mean=None, f_in_std=None, f_row_stride=64, fields=4, scalars=4)) == 0

    def loss_args(**kw):
        a = nat.GfMirrorLossArgs()
        a.num_rows, a.num_actions, a.coeff = 300, 12, 0.5
        a.mu_mirror = a.mu_orig = a.perm = a.sign = a.grad = a.out = a.sums = a.workspace = FAKE
        a.workspace_bytes = nat.mirror_loss_workspace_bytes(300)
        for k, v in kw.items():
            setattr(a, k, v)
        return a

    lcall = lambda a: lib.gf_mirror_loss(C.byref(a), None)
    assert lib.gf_mirror_loss(None, None) == E_NULL
    for k in ("mu_mirror", "mu_orig", "perm", "sign", "out", "workspace"):
        assert lcall(loss_args(**{k: None})) == E_NULL, k
    assert lcall(loss_args(num_rows=-1)) == E_RANGE and lcall(loss_args(num_actions=0)) == E_RANGE
    assert lcall(loss_args(workspace_bytes=nat.mirror_loss_workspace_bytes(300) - 8)) == E_RANGE
    assert lcall(loss_args(workspace=FAKE + 4)) == E_RANGE
    assert lcall(loss_args(num_rows=0, workspace_bytes=0, grad=None, sums=None)) == 0
    assert nat.mirror_loss_workspace_bytes(300) == 16 and nat.mirror_loss_workspace_bytes(256) == 8

    def ppo_args(**kw):
        a = nat.GfPpoLossArgs()
        a.num_rows, a.num_actions, a.use_clipped_value_loss = 300, 12, 1
        for k in ("mu", "sigma", "value", "actions", "old_log_prob", "advantages", "target_values", "returns", "old_mu", "old_sigma",
                  "grad_mu", "grad_value", "grad_sigma", "out", "workspace"):
            setattr(a, k, FAKE)
        a.workspace_bytes = nat.ppo_loss_workspace_bytes(300, 12)
        for k, v in kw.items():
            setattr(a, k, v)
        return a

    pcall = lambda a: lib.gf_ppo_loss(C.byref(a), None)
    assert pcall(ppo_args(kl_rows=-1)) == E_RANGE and pcall(ppo_args(kl_rows=301)) == E_RANGE
    assert pcall(ppo_args(kl_rows=1, num_rows=0)) == E_RANGE, "kl_rows past num_rows, even with no rows"
    assert pcall(ppo_args(kl_rows=0, num_rows=0)) == 0


# ---- CPU: PPO ----------------------------------------------------------------------------------------------------------------------------
def _go2_symmetry(env):
    from genesis_forge_amd import MirrorSymmetry

    om = env.managers["observation"][0]
    have = [n for n, *_ in om._plan]
    return MirrorSymmetry.from_items(om, {k: v for k, v in ITEMS.items() if k in have}, *JOINTS)


def test_ppo_symmetry_cfg_refusals(oracle_backend):
    from genesis_forge_amd import MirrorSymmetry
    from genesis_forge_amd.learner import PPO

    env, st, policy, _state = tpu._setup("go2", 16, 4, "cpu")
    sym = _go2_symmetry(env)
    ok = dict(use_data_augmentation=True, use_mirror_loss=True, mirror_loss_coeff=0.5, data_augmentation_func=sym)
    ppo = PPO(policy, st, **dict(ALGO, symmetry_cfg=ok))
    assert ppo.symmetry == {"func": sym, "augment": True, "mirror": True, "coeff": 0.5}
    assert PPO(policy, st, **dict(ALGO, symmetry_cfg=None)).symmetry is None
    logging_only = PPO(policy, st, **dict(ALGO, symmetry_cfg=dict(data_augmentation_func=sym))).symmetry
    assert (logging_only["augment"], logging_only["mirror"]) == (False, False)
    W = st.obs_width
    narrow = MirrorSymmetry(list(range(W - 1)), [1] * (W - 1), *JOINTS)
    few = MirrorSymmetry(*sym.host_tables("policy"), [1, 0], [1, 1])
    critic = MirrorSymmetry(*sym.host_tables("policy"), *JOINTS, critic_obs_perm=[0, 1], critic_obs_sign=[1, 1])
    for bad, word in (({"use_data_augmentation": True}, "data_augmentation_func"),               # the pinned dict: no function
                      (dict(ok, data_augmentation_func=None), "data_augmentation_func"),
                      (dict(ok, data_augmentation_func="my_module:mirror"), "string"),
                      (dict(ok, data_augmentation_func=lambda obs=None, actions=None, env=None, obs_type="policy": (obs, actions)), "Python callable"),
                      (dict(ok, data_augmentation_func=narrow), "policy observation"), (dict(ok, data_augmentation_func=few), "action"),
                      (dict(ok, data_augmentation_func=critic), "critic observation"), (dict(ok, _env=env), "_env"),
                      (dict(ok, use_mirror_los=True), "use_mirror_los"), ("mirror", "dict"), ([sym], "dict")):
        with pytest.raises(ValueError, match="symmetry_cfg") as e:
            PPO(policy, st, **dict(ALGO, symmetry_cfg=bad))
        assert word in str(e.value), f"{word!r} not in {e.value}"
    for bad, word in ((dict(rnd_cfg={"weight": 1.0}), "rnd_cfg"), (dict(normalize_advantage_per_mini_batch=True), "normalize_advantage_per_mini_batch")):
        with pytest.raises(ValueError, match=word):   # still refused
            PPO(policy, st, **dict(ALGO, symmetry_cfg=ok, **bad))


MODES = {"augment": (True, False), "mirror": (False, True), "both": (True, True), "logging": (False, False)}


def _rollout(dev, norm=False, log=False, n=70, T=5, hidden=(32, 16), seed=4):
    """A Go2 rollout of T steps x n envs collected by a fresh policy (given noise: the same on both backends), returns computed."""
    from genesis_forge_amd.learner import ActorCriticMLP, RolloutStorage

    env = tpu._env("go2", n)
    obs, extras = env.reset()
    st = RolloutStorage(env, T).attach()
    st.begin(obs, extras)
    A = env.action_space.shape[0]
    torch.manual_seed(0)
    policy = ActorCriticMLP(st.obs_width, A, hidden, hidden, init_noise_std=0.8, actor_obs_normalization=norm, critic_obs_normalization=norm,
                            noise_std_type="log" if log else "scalar").to(dev)
    g = torch.Generator().manual_seed(seed)
    if norm:
        policy.update_normalization(obs)
    for _ in range(T):
        with torch.no_grad():
            mean, values = policy.act_mean(obs), policy.evaluate(obs)
        std = (policy.log_std if log else policy.std).detach()
        actions = st.act(mean, std, values, noise=torch.randn(n, A, generator=g).to(dev), std_is_log=log)
        obs, _r, _te, tr, extras = env.step(actions)
        if norm:
            policy.update_normalization(obs)
        st.process_env_step(tr)
    with torch.no_grad():
        st.compute_returns(policy.evaluate(obs), gamma=ALGO["gamma"], lam=ALGO["lam"])
    st.detach()
    return env, st, policy


def _update_vs_restatement(dev, mode, norm=False, log=False):
    """``PPO.update`` with a symmetry_cfg against the restatement on the same rollout and the same minibatch stream: the comparisons
    and tolerances of test_ppo_update._end_to_end (losses to 1e-4 relative — the symmetry mean with them —, equal learning rates, the
    parameters' bulk and maximum), for the 20 minibatches of one update.  The minibatch stream's seed is one whose reference run keeps
    every KL clear of the schedule's thresholds (checked below): 12 for the augmented batches, 10 otherwise."""
    from genesis_forge_amd.learner import PPO

    env, st, policy = _rollout(dev, norm, log)
    sym = _go2_symmetry(env)
    aug, mir = MODES[mode]
    seed = 12 if aug else 10
    cfg = dict(use_data_augmentation=aug, use_mirror_loss=mir, mirror_loss_coeff=0.5, data_augmentation_func=sym)
    ref_policy = _as_rsl_rl(policy) if log else copy.deepcopy(policy)
    before = tpu._flat(policy).clone()
    ppo, ref = PPO(policy, st, **dict(ALGO, symmetry_cfg=cfg)), RslRlSymmetryPPO(ref_policy, st, **dict(ALGO, symmetry_cfg=cfg))
    kls = []
    with _recorded_kl(kls):
        want = ref.update(generator=torch.Generator(device=dev).manual_seed(seed))
    steps = ALGO["num_learning_epochs"] * ALGO["num_mini_batches"]
    assert len(kls) == steps
    for kl in kls:   # equal learning rates need every KL clear of the schedule's two thresholds
        for edge in (2.0 * ALGO["desired_kl"], ALGO["desired_kl"] / 2.0):
            assert abs(kl - edge) > 1e-3 * edge, f"a minibatch KL of the reference run ({kl}) within 1e-3 of {edge}: pick another seed"
    with tpu.host_reads() as c:
        got = ppo.update(generator=torch.Generator(device=dev).manual_seed(seed))
    assert c[0] == 1, f"PPO.update read the device {c[0]} times"
    print(f"    {mode} norm={norm} log={log}: got {got}\n    want {want}  lr {ppo.learning_rate} vs {ref.learning_rate}")
    assert set(got) == {"value_function", "surrogate", "entropy", "symmetry"}
    for k in ("value_function", "surrogate", "entropy", "symmetry"):
        assert abs(got[k] - want[k]) <= 1e-4 * max(abs(want[k]), 1e-6), f"{k} {got[k]} vs {want[k]}"
    assert got["symmetry"] > 1e-6, "a randomly initialised policy is not symmetric"
    assert ppo.learning_rate == ref.learning_rate, f"lr {ppo.learning_rate} vs {ref.learning_rate}"
    a, b = tpu._flat(policy), tpu._flat(ref_policy)
    d = (a - b).abs()
    bulk = float((d <= 1e-4 + 1e-3 * b.abs()).float().mean())
    print(f"    parameters: bulk {bulk:.4f}, max diff {float(d.max()):.3e}, moved {float((a - before).abs().max()):.3e}")
    assert bulk >= 0.995, f"only {bulk:.4f} of the parameters agree to 1e-4 + 1e-3|p| (max diff {float(d.max())})"
    assert float(d.max()) <= 2 * 3.2 * 1e-2 * steps
    assert float((a - before).abs().max()) > 1e-3, "the update moved the parameters"
    return got


@pytest.mark.parametrize("mode", list(MODES))
def test_update_matches_the_restatement_cpu(oracle_backend, mode):
    _update_vs_restatement("cpu", mode)


def test_update_with_normalizers_and_log_std_cpu(oracle_backend):
    _update_vs_restatement("cpu", "both", norm=True, log=True)


def test_the_mirror_loss_changes_the_update_and_logging_only_does_not(oracle_backend):
    """Logging-only trains exactly as no symmetry_cfg at all; the mirror loss does not."""
    from genesis_forge_amd.learner import PPO

    out = {}
    for name, cfg in (("none", None), ("logging", {}), ("mirror", dict(use_mirror_loss=True, mirror_loss_coeff=0.5))):
        env, st, policy = _rollout("cpu")
        if cfg is not None:
            cfg = dict(cfg, data_augmentation_func=_go2_symmetry(env))
        ppo = PPO(policy, st, **dict(ALGO, symmetry_cfg=cfg))
        losses = ppo.update(generator=torch.Generator().manual_seed(3))
        out[name] = (tpu._flat(policy).clone(), losses)
    assert "symmetry" not in out["none"][1] and "symmetry" in out["logging"][1]
    assert torch.equal(out["none"][0], out["logging"][0])
    assert {k: v for k, v in out["logging"][1].items() if k != "symmetry"} == out["none"][1]
    assert not torch.equal(out["none"][0], out["mirror"][0])


def test_runner_logs_the_symmetry_mean(oracle_backend):
    from genesis_forge_amd.runner import OnPolicyRunner

    def run(symmetric):
        env = tpu._env("go2", 16)
        env.reset()
        algo = dict(ALGO)
        if symmetric:
            algo["symmetry_cfg"] = dict(use_data_augmentation=True, use_mirror_loss=True, mirror_loss_coeff=0.5, data_augmentation_func=_go2_symmetry(env))
        cfg = {"algorithm": algo, "policy": {"activation": "elu", "actor_hidden_dims": [16], "critic_hidden_dims": [16], "init_noise_std": 0.8,
                                             "class_name": "ActorCritic"},
               "runner": {"experiment_name": "test", "max_iterations": 1}, "runner_class_name": "OnPolicyRunner",
               "seed": 1, "num_steps_per_env": 4, "save_interval": 100, "empirical_normalization": False}
        torch.manual_seed(0)
        runner = OnPolicyRunner(env, cfg, None, device="cpu", action_noise=torch.Generator().manual_seed(2))
        runner.learn(1)
        return runner.last_log

    plain, symm = run(False), run(True)
    assert "symmetry" not in plain and set(symm) == set(plain) | {"symmetry"} and symm["symmetry"] > 0.0


# ---- GPU: gf_mirror_rows -------------------------------------------------------------------------------------------------------------------
def _mirror_rows(backend, fields, scalars=(), rows=None):
    """One gf_mirror_rows.  ``fields``: dicts ``src`` ``[rows, w]`` (possibly a strided view), ``perm`` / ``sign`` (device int32 /
    float32), ``copy`` (bool), ``norm`` (mean, std, eps) or None, optional ``out`` (a [2·rows, w] tensor to write into).  Returns
    ``[(copy or None, mirror)]`` and the ``[2·rows]`` scalars."""
    from genesis_forge_amd import _native as nat

    a = nat.GfMirrorRowsArgs()
    rows = int(fields[0]["src"].shape[0]) if rows is None else rows
    a.num_rows, a.num_fields, a.num_scalars = rows, len(fields), len(scalars)
    outs, keep = [], []
    for f, d in zip(a.fields, fields):
        src = d["src"]
        w = int(src.shape[1])
        dst = d.get("out")
        if dst is None:
            dst = torch.full((2 * rows, w), 7.0, device=src.device)
        f.src, f.width, f.row_stride = src.data_ptr(), w, 0 if src.is_contiguous() else src.stride(0)
        f.dst_copy = dst.data_ptr() if d.get("copy", True) else None
        f.dst_mirror = dst.data_ptr() + rows * w * 4
        f.perm, f.sign = d["perm"].data_ptr(), d["sign"].data_ptr()
        if d.get("norm") is not None:
            f.in_mean, f.in_std, f.in_eps = d["norm"][0].data_ptr(), d["norm"][1].data_ptr(), d["norm"][2]
        outs.append((dst[:rows] if d.get("copy", True) else None, dst[rows:]))
        keep.append(dst)
    souts = []
    for s, src in zip(a.scalars, scalars):
        dst = torch.full((2 * rows,), 7.0, device=src.device)
        s.src, s.dst = src.data_ptr(), dst.data_ptr()
        souts.append(dst)
    backend.mirror_rows(a)
    return outs, souts


def _dev_tables(perm, sign):
    return torch.tensor(perm, dtype=torch.int32, device="cuda"), torch.tensor(sign, dtype=torch.float32, device="cuda")


ROWS = [1, 63, 64, 65, 257]
WIDTHS = [1, 3, 4, 5, 48, 235, 1024]


@pytest.mark.gpu
@pytest.mark.parametrize("w", WIDTHS)
def test_mirror_rows_is_torch_indexing_bit_for_bit(hip_backend, w):
    """Every row count x identity / reversal / random involution at this width: widths 4, 48 and 1 024 take the 16-byte path, the others
    the element path; 257 rows of width 1 024 are 33 workgroups of 8 rows, 65 rows of width 48 two of 64."""
    g = torch.Generator().manual_seed(w)
    for rows in ROWS:
        x = torch.randn(rows, w, generator=g).cuda()
        for kind in ("identity", "reversal", "random"):
            perm, sign = _tables(kind, w, seed=rows)
            p, s = _dev_tables(perm, sign)
            (out,), _ = _mirror_rows(hip_backend, [dict(src=x, perm=p, sign=s)])
            want = s * x[:, p.long()]
            assert torch.equal(out[0], x), f"copy: rows {rows} {kind}"
            assert torch.equal(out[1], want), f"mirror: rows {rows} {kind}"
            if kind == "identity":
                assert torch.equal(out[1], x)
    # the mirrored half alone (dst_copy NULL): the copy half keeps its filler
    (out,), _ = _mirror_rows(hip_backend, [dict(src=x, perm=p, sign=s, copy=False)])
    assert out[0] is None and torch.equal(out[1], want)


@pytest.mark.gpu
def test_mirror_rows_four_fields_strided_misaligned_and_scalars(hip_backend):
    """One launch: a strided window source, a field whose base is one float off 16-byte alignment (the element path at a width that
    would otherwise take 16-byte chunks), a 12-wide action field, a spare, and four replicated scalars — field widths whose tile
    counts differ, so the grid's widest row is not every field's."""
    rows = 300
    g = torch.Generator().manual_seed(5)
    big = torch.randn(rows, 3 * 48 + 8, generator=g).cuda()
    window = big[:, 8:8 + 96]                                  # row stride 152 floats, 16-byte aligned, not contiguous
    assert not window.is_contiguous() and window.data_ptr() % 16 == 0
    buf = torch.randn(rows * 48 + 4, generator=g).cuda()
    off = buf[1:1 + rows * 48].view(rows, 48)                   # one float off alignment
    assert off.data_ptr() % 16 == 4
    act = torch.randn(rows, 12, generator=g).cuda()
    spare = torch.randn(rows, 1000, generator=g).cuda()
    fields = []
    for x, seed in ((window, 1), (off, 2), (act, 3), (spare, 4)):
        p, s = _dev_tables(*_random_involution(x.shape[1], seed))
        fields.append(dict(src=x, perm=p, sign=s))
    misaligned_out = torch.full((2 * rows * 48 + 4,), 7.0, device="cuda")[1:1 + 2 * rows * 48].view(2 * rows, 48)
    fields[1]["out"] = misaligned_out
    scalars = [torch.randn(rows, generator=g).cuda() for _ in range(4)]
    outs, souts = _mirror_rows(hip_backend, fields, scalars)
    for d, (cp, mi) in zip(fields, outs):
        assert torch.equal(cp, d["src"]) and torch.equal(mi, d["sign"] * d["src"][:, d["perm"].long()]), d["src"].shape
    for src, dst in zip(scalars, souts):
        assert torch.equal(dst, src.repeat(2))
    # scalars alone, and more scalar rows than one workgroup's 1 024
    many = torch.randn(2500, generator=g).cuda()
    _, (dst,) = _mirror_rows(hip_backend, [], [many], rows=2500)
    assert torch.equal(dst, many.repeat(2))


@pytest.mark.gpu
@pytest.mark.parametrize("w", [5, 48, 235])
def test_mirror_rows_normalises_at_the_destination_column(hip_backend, w):
    """Both halves are the float32 expression ``(v - mean) / (std + eps)`` (CPU torch: one subtraction, one addition, one correctly
    rounded division) of the CPU-mirrored RAW input, and the copy half is gf_minibatch_gather's normalised rows bit for bit."""
    from genesis_forge_amd import _native as nat

    rows, eps = 257, 1e-2
    g = torch.Generator().manual_seed(w)
    x = torch.randn(rows, w, generator=g) * 3.0 + 1.0
    mean, std = torch.randn(w, generator=g), torch.rand(w, generator=g) + 0.1
    perm, sign = _random_involution(w, 9)
    p, s = _dev_tables(perm, sign)
    (out,), _ = _mirror_rows(hip_backend, [dict(src=x.cuda(), perm=p, sign=s, norm=(mean.cuda(), std.cuda(), eps))])
    mirrored = torch.tensor(sign) * x[:, torch.tensor(perm)]
    f = lambda v: (v - mean) / (std + eps)
    assert torch.equal(out[0].cpu(), f(x)) and torch.equal(out[1].cpu(), f(mirrored))
    assert not torch.equal(out[1].cpu(), torch.tensor(sign) * f(x)[:, torch.tensor(perm)]), "normalised at the destination, not the source, column"
    a = nat.GfMinibatchArgs()
    idx = torch.arange(rows, device="cuda")
    xs, ms, ss, dst = x.cuda(), mean.cuda(), std.cuda(), torch.empty(rows, w, device="cuda")
    a.num_rows, a.num_src_rows, a.indices, a.num_fields = rows, rows, idx.data_ptr(), 1
    fd = a.fields[0]
    fd.src, fd.dst, fd.src_width, fd.dst_width, fd.dst_col = xs.data_ptr(), dst.data_ptr(), w, w, 0
    fd.mean, fd.std, fd.eps = ms.data_ptr(), ss.data_ptr(), eps
    hip_backend.minibatch_gather(a)
    assert torch.equal(out[0], dst)


# ---- GPU: gf_mirror_loss -----------------------------------------------------------------------------------------------------------------
def _mirror_loss(backend, mu_mirror, mu_orig, perm, sign, coeff, grad, sums=None):
    from genesis_forge_amd import _native as nat

    mb, A = mu_mirror.shape
    out = torch.full((1,), 7.0, device="cuda")
    ws = torch.empty(max(1, nat.mirror_loss_workspace_bytes(mb) // 8), device="cuda", dtype=torch.float64)
    a = nat.GfMirrorLossArgs()
    a.num_rows, a.num_actions, a.coeff = mb, A, coeff
    a.mu_mirror, a.mu_orig, a.perm, a.sign = mu_mirror.data_ptr(), mu_orig.data_ptr(), perm.data_ptr(), sign.data_ptr()
    a.grad = None if grad is None else grad.data_ptr()
    a.out, a.sums = out.data_ptr(), None if sums is None else sums.data_ptr()
    a.workspace, a.workspace_bytes = ws.data_ptr(), ws.numel() * 8
    backend.mirror_loss(a)
    return out


@pytest.mark.gpu
@pytest.mark.parametrize("A", [3, 12, 64])
def test_mirror_loss_and_gradient_against_float64(hip_backend, A):
    """Rows around the workgroup (256) and around the finalize launch's width (256 partials = 65 536 rows).  Bounds, derived: d is one
    float32 rounding of the exact difference; the gradient adds three (1 / (mb·A), coeff times it, the product with 2·d): elementwise
    within 4·2^-24 relative.  The loss sums d² in double and rounds the mean once: within 2^-22 relative."""
    coeff = 0.75   # (exact in float32: the argument's conversion is not a rounding of the kernel's)
    p, s = _dev_tables(*_random_involution(A, 4))
    for mb in ([1, 255, 256, 257, 65535, 65537] if A != 64 else [1, 255, 257, 65537]):
        g = torch.Generator().manual_seed(mb + A)
        mm, mo = torch.randn(mb, A, generator=g).cuda(), torch.randn(mb, A, generator=g).cuda()
        d64 = mm.double() - s.double() * mo.double()[:, p.long()]
        loss64, grad64 = float((d64 * d64).mean()), coeff * 2.0 * d64 / (mb * A)
        zero = torch.zeros(mb, A, device="cuda")
        sums = torch.tensor([1.5], dtype=torch.float64, device="cuda")
        out = _mirror_loss(hip_backend, mm, mo, p, s, coeff, zero, sums)
        e_loss = abs(float(out[0]) - loss64) / loss64
        e_grad = float(((zero.double() - grad64).abs() / grad64.abs().clamp_min(1e-300)).max())
        print(f"    A={A} mb={mb}: loss rel err {e_loss:.3e} (bound {4 * U:.3e}), grad rel err {e_grad:.3e} (bound {4 * U:.3e})")
        assert e_loss <= 4 * U, f"loss {float(out[0])} vs {loss64}"
        assert bool(((zero.double() - grad64).abs() <= 4 * U * grad64.abs()).all()), f"gradient: max rel err {e_grad}"
        assert float(sums[0]) == 1.5 + float(out[0]), "the running sum takes the float32 loss"
        # added into a non-zero buffer, not stored: one float32 addition of the value the zeroed buffer received
        base = torch.randn(mb, A, generator=g).cuda()
        buf = base.clone()
        again = _mirror_loss(hip_backend, mm, mo, p, s, coeff, buf)
        assert torch.equal(buf, base + zero) and torch.equal(again, out), "bitwise reproducible, and an addition"
        # logging only: no gradient pointer, the same loss; coeff 0: the buffer keeps its bits
        assert torch.equal(_mirror_loss(hip_backend, mm, mo, p, s, coeff, None), out)
        keep = base.clone()
        keep[0, 0] = -0.0
        bits = keep.view(torch.int32).clone()
        assert torch.equal(_mirror_loss(hip_backend, mm, mo, p, s, 0.0, keep), out)
        assert torch.equal(keep.view(torch.int32), bits)


# ---- GPU: gf_ppo_loss kl_rows ----------------------------------------------------------------------------------------------------------------
def _raw_loss_kl(backend, inp, kl_rows, with_grads=True):
    from genesis_forge_amd import _native as nat

    mb, A = inp["mu"].shape
    out = {"grad_mu": torch.full((mb, A), 7.0, device="cuda"), "grad_value": torch.full((mb,), 7.0, device="cuda"),
           "grad_sigma": torch.full((A,), 7.0, device="cuda"), "out": torch.zeros(5, device="cuda")}
    ws = torch.empty(max(1, nat.ppo_loss_workspace_bytes(mb, A) // 8), device="cuda", dtype=torch.float64)
    a = nat.GfPpoLossArgs()
    a.num_rows, a.num_actions, a.use_clipped_value_loss = mb, A, 1
    for k in ("mu", "sigma", "value", "actions", "old_log_prob", "advantages", "target_values", "returns", "old_mu", "old_sigma"):
        setattr(a, k, inp[k].data_ptr())
    a.clip_param, a.value_loss_coef, a.entropy_coef = 0.2, 1.0, 0.01
    if with_grads:
        a.grad_mu, a.grad_value, a.grad_sigma = (out[k].data_ptr() for k in ("grad_mu", "grad_value", "grad_sigma"))
    a.out = out["out"].data_ptr()
    a.workspace, a.workspace_bytes = ws.data_ptr(), ws.numel() * 8
    a.kl_rows = kl_rows
    backend.ppo_loss(a)
    return out


@pytest.mark.gpu
@pytest.mark.parametrize("A", [12, 5])
@pytest.mark.parametrize("mb", [1, 87, 256, 300])
def test_kl_rows_takes_the_kl_from_the_first_rows_only(hip_backend, A, mb):
    full = tpu._synthetic(2 * mb, A, "cuda", seed=3)
    zero, same = _raw_loss_kl(hip_backend, full, 0), _raw_loss_kl(hip_backend, full, 2 * mb)
    for k in zero:
        assert torch.equal(zero[k], same[k]), f"kl_rows = num_rows is kl_rows = 0: {k}"
    # old_mu / old_sigma of the original rows only: exactly mb rows long (the rows behind them do not exist)
    half = dict(full, old_mu=full["old_mu"][:mb].clone(), old_sigma=full["old_sigma"][:mb].clone())
    got = _raw_loss_kl(hip_backend, half, mb)
    first = _raw_loss_kl(hip_backend, {k: (v if k == "sigma" else v[:mb].contiguous()) for k, v in full.items()}, 0, with_grads=False)
    assert torch.equal(got["out"][3], first["out"][3]), "the KL of the first mb rows alone"
    assert not torch.equal(got["out"][3], zero["out"][3])
    for k in ("grad_mu", "grad_value", "grad_sigma"):
        assert torch.equal(got[k], zero[k]), k
    assert torch.equal(got["out"][[0, 1, 2, 4]], zero["out"][[0, 1, 2, 4]])


# ---- GPU: PPO.update ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("variant", ["plain", "norm", "log"])
@pytest.mark.parametrize("mode", list(MODES))
def test_update_matches_the_restatement_hip(hip_backend, mode, variant):
    _update_vs_restatement("cuda", mode, norm=variant == "norm", log=variant == "log")


@pytest.mark.gpu
def test_symmetric_minibatches_never_synchronise(hip_backend):
    """The sync debug mode, if this build honours it (positive control first), over the minibatches of every flag combination."""
    from genesis_forge_amd.learner import PPO

    honoured = False
    torch.cuda.set_sync_debug_mode("error")
    try:
        torch.ones(1, device="cuda").item()
    except RuntimeError:
        honoured = True
    finally:
        torch.cuda.set_sync_debug_mode(0)
    env, st, policy = _rollout("cuda", norm=True)
    sym = _go2_symmetry(env)
    for mode, (aug, mir) in MODES.items():
        ppo = PPO(policy, st, **dict(ALGO, symmetry_cfg=dict(use_data_augmentation=aug, use_mirror_loss=mir, mirror_loss_coeff=0.5, data_augmentation_func=sym)))
        norms = ppo._normalizers()
        batches = ppo._symmetry_batches(torch.Generator(device="cuda").manual_seed(0), norms)
        if honoured:
            torch.cuda.set_sync_debug_mode("error")
        try:
            for b in batches:
                ppo._minibatch_symmetry(b, norms)
        finally:
            torch.cuda.set_sync_debug_mode(0)
        assert ppo._calls == ALGO["num_learning_epochs"] * ALGO["num_mini_batches"], mode


def _symmetrise(policy, sym):
    """Make the actor exactly equivariant — actor(mirror(obs)) = mirror(actor(obs)) in exact arithmetic — by averaging every layer
    with its mirrored self: hidden units mirror by reversal (a pure permutation: ELU is not odd).  fl(a + b) = fl(b + a), so the two
    ends of every mirrored pair of weights hold the same bits."""
    layers = [m for m in policy.actor if isinstance(m, torch.nn.Linear)]
    dev = layers[0].weight.device
    op, osg = (t.to(dev) for t in sym.host_tables("policy"))
    ap, asg = (t.to(dev) for t in sym.host_tables("actions"))
    maps = [(op, osg)] + [(torch.arange(l.out_features - 1, -1, -1, device=dev), torch.ones(l.out_features, device=dev)) for l in layers[:-1]] + [(ap, asg)]
    with torch.no_grad():
        for l, (pi, si), (po, so) in zip(layers, maps[:-1], maps[1:]):
            W = l.weight.data
            l.weight.data.copy_((W + so[:, None] * W[po][:, pi] * si[None, :]) / 2)
            l.bias.data.copy_((l.bias.data + so * l.bias.data[po]) / 2)
    return maps


@pytest.mark.gpu
def test_a_symmetric_policy_has_no_symmetry_loss_and_mirrored_gradients(hip_backend):
    """End-to-end sign check.  The loss of a policy that is symmetric by construction vanishes within float32: the two sides differ
    by the forward's rounding only — three layers of at most 48-term dot products, a few 1e-6 of the outputs' scale in the worst
    case — so the mean of d² is below (1e-5 · max|mu|)².  An augmented batch is its own mirror image, so the actor's gradient is
    invariant under the layer's mirror maps; the rows' rounding (sums of 174 products) stays below 1e-4 of the largest entry.  A
    table applied with a wrong sign or direction anywhere on the way breaks both by orders of magnitude."""
    from genesis_forge_amd.learner import PPO

    env, st, policy = _rollout("cuda")
    sym = _go2_symmetry(env)
    maps = _symmetrise(policy, sym)
    cfg = dict(use_data_augmentation=True, use_mirror_loss=True, mirror_loss_coeff=0.5, data_augmentation_func=sym)
    ppo = PPO(policy, st, **dict(ALGO, symmetry_cfg=cfg))
    b = next(iter(ppo._symmetry_batches(torch.Generator(device="cuda").manual_seed(0), (None, None))))
    with torch.no_grad():
        mu = policy.act_mean(b.obs)
        scale = float(mu.abs().max())
        assert float((policy.act_mean(sym.mirror(b.obs)) - sym.mirror(mu, "actions")).abs().max()) <= 1e-5 * scale, "the construction is equivariant"
    ppo._minibatch_symmetry(b, (None, None))
    loss = float(ppo._sym_out[0])
    print(f"    symmetric policy: symmetry loss {loss:.3e}, bound {(1e-5 * scale) ** 2:.3e} (max|mu| {scale:.3e})")
    assert 0.0 <= loss <= (1e-5 * scale) ** 2
    layers = [m for m in policy.actor if isinstance(m, torch.nn.Linear)]
    for i, (l, (pi, si), (po, so)) in enumerate(zip(layers, maps[:-1], maps[1:])):
        G = l.weight.grad
        top = float(G.abs().max())
        assert top > 0.0
        err = float((G - so[:, None] * G[po][:, pi] * si[None, :]).abs().max())
        print(f"    layer {i}: max|G| {top:.3e}, max|G - mirror(G)| {err:.3e}")
        assert err <= 1e-4 * top, f"layer {i}: the gradient is not its own mirror image ({err} vs {top})"
    # and the control: a generic policy's loss is nowhere near
    env2, st2, generic = _rollout("cuda")
    ppo2 = PPO(generic, st2, **dict(ALGO, symmetry_cfg=dict(cfg, data_augmentation_func=_go2_symmetry(env2))))
    ppo2._minibatch_symmetry(next(iter(ppo2._symmetry_batches(torch.Generator(device="cuda").manual_seed(0), (None, None)))), (None, None))
    assert float(ppo2._sym_out[0]) > 1e4 * (1e-5 * scale) ** 2
