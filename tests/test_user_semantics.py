"""Two user paths the recorded step must carry exactly as the ordinary step does (the reference's documented ways to run a
curriculum and to extend a manager):

* a term's ``params`` REPLACED (``cfg[name].params = {...}``): an opaque reward / termination function, a native catalogue term, a
  native term of a second entity (a Python-evaluated column), a class-style fn — every call after the edit sees the new params;
* what the ``step()`` of a user RewardManager / TerminationManager class RETURNS, a new tensor included: the env resets from it,
  writes it into the rollout rows and returns it (managed_env.py:303-315 of the reference).

Every case checks the ordinary step against an expectation recomputed here with torch, and the recorded step against the ordinary
step bit for bit (outputs, episode lengths, logs, rollout rows, the managers' own buffers)."""
import math

import pytest
import torch

from helpers import FLOAT_TOL
from envs import Go2CommandDirectionEnv

STEPS = 40
GPU_SIZES = (1000, 4096 + 37)   # (the second one leaves the fused program a partial last tile)


# -- replaced params ------------------------------------------------------------------------------------------------------------------
def _spy_reward(env, k=1.0):
    """Opaque reward term: ``k * base_z``.  Logs the params it was called with next to those the cfg holds at that moment."""
    z = env.robot_manager.base_pos[:, 2].clone()
    rm = env.reward_manager
    env.spy.append({"term": "r", "step": env.step_count, "got": {"k": k}, "want": dict(rm.cfg["spy"].params),
                    "cfg": {n: (c.weight, dict(c.params)) for n, c in rm.cfg.items()}, "z": z, "box_z": env.box.get_pos()[:, 2].clone()})
    return k * z


def _spy_termination(env, h=0.0):
    """Opaque termination term: ``base_z < h``.  Logs what the native terms of its manager read at the same point of the step."""
    z = env.robot_manager.base_pos[:, 2].clone()
    tm = env.termination_manager
    env.spy.append({"term": "t", "step": env.step_count, "got": {"h": h}, "want": dict(tm.term_cfg["spy"].params),
                    "cfg": {n: dict(c.params) for n, c in tm.term_cfg.items()}, "z": z,
                    "grav": env.robot_manager.get_projected_gravity().clone(), "ep": env.episode_length.clone(),
                    "max_ep": env.max_episode_length.clone()})
    return z < h


def _make_class_term():
    from genesis_forge_amd.managers import MdpFnClass

    class ScaledHeight(MdpFnClass):
        """Class-style term fn: ``scale * base_z**2``; the params reach it per call (config_item.py)."""

        def __init__(self, env, scale=1.0):
            super().__init__(env)

        def __call__(self, env, scale=1.0):
            z = env.robot_manager.base_pos[:, 2]
            out = scale * z * z
            env.spy.append({"term": "c", "step": env.step_count, "got": {"scale": scale}, "want": dict(env.reward_manager.cfg["cls"].params),
                            "out": out.clone()})
            return out

    return ScaledHeight


# what each kind edits: (manager, term, params A, params B); the native-term kind replaces a reward AND a termination term
def _edits(env, kind):
    em = env.robot_manager
    rm, tm = env.reward_manager.cfg, env.termination_manager.term_cfg
    return {
        "opaque_reward": [(rm, "spy", {"k": 3.0}, {"k": 10.0})],
        "opaque_termination": [(tm, "spy", {"h": 0.30}, {"h": 0.395})],
        "native": [(rm, "height", {"target_height": 0.30}, {"target_height": 0.45}),
                   (tm, "fall", {"limit_angle": 10.0, "entity_manager": em}, {"limit_angle": 4.0, "entity_manager": em})],
        "second_entity": [(rm, "box", {"target_height": 0.10, "entity_attr": "box"}, {"target_height": 0.60, "entity_attr": "box"})],
        "class": [(rm, "cls", {"scale": 1.0}, {"scale": -4.0})],
    }[kind]


def _param_env_cls(reset_edit=None):
    from genesis_forge_amd.managers import RewardManager, TerminationManager
    from genesis_forge_amd.mdp import rewards, terminations
    from genesis_forge_amd.scene import morphs

    Cls = _make_class_term()

    class ParamEnv(Go2CommandDirectionEnv):
        def __init__(self, **kw):
            super().__init__(**kw)
            self.spy = []
            # a second robot: a native term on it is evaluated through its own launch and fed to the reward kernel as a column
            self.box = self.scene.add_entity(morphs.URDF(file="urdf/go2/urdf/go2.urdf", pos=[1.0, 0.0, 0.25], quat=[1.0, 0.0, 0.0, 0.0]))

        def config(self):
            super().config()
            self.managers["reward"] = None
            self.reward_manager = RewardManager(self, logging_enabled=True, cfg={
                "spy": {"weight": 0.5, "fn": _spy_reward, "params": {"k": 3.0}},
                "height": {"weight": -2.0, "fn": rewards.base_height, "params": {"target_height": 0.30}},
                "box": {"weight": 0.7, "fn": rewards.base_height, "params": {"target_height": 0.10, "entity_attr": "box"}},
                "cls": {"weight": 0.3, "fn": Cls, "params": {"scale": 1.0}},
            })
            self.managers["termination"] = None
            self.termination_manager = TerminationManager(self, logging_enabled=True, term_cfg={
                "timeout": {"fn": terminations.timeout, "time_out": True},
                "fall": {"fn": terminations.bad_orientation, "params": {"limit_angle": 10.0, "entity_manager": self.robot_manager}},
                "spy": {"fn": _spy_termination, "params": {"h": 0.30}},
            })

    if reset_edit is None:
        return ParamEnv

    class ResetEditEnv(ParamEnv):
        """The edit made by user code INSIDE the step: a reset() override (the reference's curriculum hook)."""
        edit_from = None

        def reset(self, env_ids=None):
            out = super().reset(env_ids)
            if env_ids is not None and self.edit_from is not None and self.step_count >= self.edit_from:
                self.edit_from = None
                reset_edit(self)
            return out

    return ResetEditEnv


def _schedule(place):
    """{step index: which params (0 = A, 1 = B)} for the places an edit can be made between steps."""
    return {"before": {0: 1}, "between": {20: 1}, "aba": {12: 1, 24: 0}, "reset": {}}[place]


def _apply(env, kind, which):
    for cfg, name, a, b in _edits(env, kind):
        cfg[name].params = dict(b if which else a)


def _run_params(dev, trace, kind, place, n):
    Env = _param_env_cls(reset_edit=(lambda env: _apply(env, kind, 1)) if place == "reset" else None)
    env = Env(num_envs=n, max_episode_length_s=1, cmd_resample_s=0.3, scene_kwargs=dict(ang_noise=0.3, seed=3))
    env.trace_enabled = trace
    env.build()
    env.seed(5)
    env.reset()
    if place == "reset":
        env.edit_from = 20
    sched = _schedule(place)
    g = torch.Generator().manual_seed(0)
    outs = []
    for t in range(STEPS):
        if t in sched:
            _apply(env, kind, sched[t])
        o, r, te, tr, ex = env.step(torch.randn(n, 12, generator=g).to(dev))
        outs.append({"step": env.step_count, "obs": o.cpu().clone(), "rew": r.cpu().clone(), "term": te.cpu().clone(), "trunc": tr.cpu().clone(),
                     "ep": env.episode_length.cpu().clone(), "log": {k: float(v) for k, v in ex["episode"].items()}})
    if place == "reset":
        assert env.edit_from is None, "no env was reset after step 20: the reset() edit never ran"
    return outs, env


def _spy_by_step(env):
    out: dict = {}
    for e in env.spy:
        out.setdefault(e["step"], {})[e["term"]] = e
    return out


def _check_expectation(outs, env, kind):
    """The ordinary step against torch: every call sees the cfg's params, the reward is sum(weight * dt * term) in float64, the
    termination masks are the terms at the cfg's limits in the reference's float32 order (tests/golden/orientation_sweep.npz)."""
    spies = _spy_by_step(env)
    dt = env.dt
    edited = {name for _cfg, name, _a, _b in _edits(env, kind)}
    seen_b = False
    for row in outs:
        s = spies[row["step"]]
        for e in s.values():
            assert e["got"] == {k: v for k, v in e["want"].items()}, f"step {row['step']}: term '{e['term']}' called with {e['got']}, the cfg holds {e['want']}"
        r, t = s["r"], s["t"]
        z = r["z"].double()
        cfg = r["cfg"]
        want = torch.zeros_like(z)
        want += cfg["spy"][0] * dt * (cfg["spy"][1]["k"] * z)
        want += cfg["height"][0] * dt * (z - cfg["height"][1]["target_height"]) ** 2
        want += cfg["box"][0] * dt * (r["box_z"].double() - cfg["box"][1]["target_height"]) ** 2
        want += cfg["cls"][0] * dt * s["c"]["out"].double()
        got = row["rew"].double()
        err = (got - want.cpu()).abs().max().item()
        assert err <= FLOAT_TOL, f"step {row['step']}: reward differs from sum(w*dt*term) by {err}"
        # termination masks, float32 in the reference's order (terminations.py:52-71)
        tc = t["cfg"]
        tilt = torch.asin(torch.clamp(torch.norm(t["grav"][:, :2], dim=1), max=0.99))
        fall = (~(t["ep"] <= 0)) & (tilt > math.radians(tc["fall"]["limit_angle"]))
        low = t["z"] < tc["spy"]["h"]
        assert torch.equal(row["term"], (fall | low).cpu()), f"step {row['step']}: terminated differs in {int((row['term'] != (fall | low).cpu()).sum())} envs"
        assert torch.equal(row["trunc"], (t["ep"] > t["max_ep"]).cpu()), f"step {row['step']}: truncated differs"
        seen_b |= any(r["cfg"].get(nm, (None, None))[1] == b or t["cfg"].get(nm) == b for _c, nm, _a, b in _edits(env, kind))
    assert seen_b, f"the edit of {sorted(edited)} never took effect"


def _same_params(a, b, ea, eb):
    assert len(a) == len(b)
    for x, y in zip(a, b):
        for k in ("step", "obs", "rew", "term", "trunc", "ep"):
            assert (x[k] == y[k]) if k == "step" else torch.equal(x[k], y[k]), f"{k} differs at step {x['step']}"
        assert x["log"] == y["log"], f"log differs at step {x['step']}: {x['log']} vs {y['log']}"
    assert len(ea.spy) == len(eb.spy), "the terms were called a different number of times"
    for p, q in zip(ea.spy, eb.spy):
        assert p["term"] == q["term"] and p["step"] == q["step"] and p["got"] == q["got"]
        for k in ("z", "out", "grav", "ep"):
            if k in p:
                assert torch.equal(p[k], q[k]), f"term '{p['term']}' read a different {k} at step {p['step']}"


KINDS = ["opaque_reward", "opaque_termination", "native", "second_entity", "class"]
PLACES = ["before", "between", "reset", "aba"]


@pytest.mark.parametrize("place", PLACES)
@pytest.mark.parametrize("kind", KINDS)
def test_replaced_params_reach_every_step_cpu(oracle_backend, kind, place):
    a, ea = _run_params("cpu", False, kind, place, 70)
    _check_expectation(a, ea, kind)
    before = oracle_backend.replays
    b, eb = _run_params("cpu", True, kind, place, 70)
    assert oracle_backend.replays - before >= 15, "the step was not recorded"
    _same_params(a, b, ea, eb)
    _check_expectation(b, eb, kind)


@pytest.mark.gpu
@pytest.mark.parametrize("n", GPU_SIZES)
@pytest.mark.parametrize("place", PLACES)
@pytest.mark.parametrize("kind", KINDS)
def test_replaced_params_reach_every_step_hip(hip_backend, kind, place, n):
    a, ea = _run_params("cuda", False, kind, place, n)
    _check_expectation(a, ea, kind)
    b, eb = _run_params("cuda", True, kind, place, n)
    assert eb._trace is not None, f"not recorded: {eb._untraceable}"
    _same_params(a, b, ea, eb)


def _contact_swap_run(dev, trace, n, swap_at):
    """``has_contact`` pointed at the OTHER ContactManager by a params replacement: another structure — the recording must be
    dropped and made again, not patched."""
    from genesis_forge_amd.managers import RewardManager
    from genesis_forge_amd.mdp import rewards

    class Env(Go2CommandDirectionEnv):
        def config(self):
            super().config()
            rc = {k: {"weight": v.weight, "fn": v.fn, "params": dict(v.params)} for k, v in self.reward_manager.cfg.items()}
            self.managers["reward"] = None
            self.reward_manager = RewardManager(self, logging_enabled=True, cfg=rc)

    env = Env(num_envs=n, max_episode_length_s=1, cmd_resample_s=0.3, contacts=True, scene_kwargs=dict(ang_noise=0.3, seed=3))
    env.trace_enabled = trace
    env.build()
    env.seed(5)
    env.reset()
    g = torch.Generator().manual_seed(0)
    outs, traces = [], []
    for t in range(STEPS):
        if t == swap_at:
            env.reward_manager.cfg["undesired_contacts"].params = {"contact_manager": env.foot_contacts, "threshold": 5.0}
        o, r, te, tr, ex = env.step(torch.randn(n, 12, generator=g).to(dev))
        outs.append((o.cpu().clone(), r.cpu().clone(), te.cpu().clone(), tr.cpu().clone(), env.episode_length.cpu().clone(),
                     {k: float(v) for k, v in ex["episode"].items()}))
        traces.append(env._trace)
    return outs, env, traces


def _contact_swap_check(dev, n):
    a, _, _ = _contact_swap_run(dev, False, n, 20)
    b, env, traces = _contact_swap_run(dev, True, n, 20)
    for t, (x, y) in enumerate(zip(a, b)):
        for k in range(5):
            assert torch.equal(x[k], y[k]), f"output {k} differs at step {t}"
        assert x[5] == y[5], f"log differs at step {t}"
    assert traces[19] is not None and traces[20] is not traces[19], "the recording was patched instead of dropped"
    assert env._trace is not None and env._trace is not traces[19], "not recorded again after the new structure"
    prog = env.reward_manager._program
    assert any(c[0] is env.foot_contacts for c in prog.slots.contacts) and not any(c[0] is env.body_contacts for c in prog.slots.contacts)
    c, _, _ = _contact_swap_run(dev, False, n, None)
    assert any(not torch.equal(x[1], y[1]) for x, y in zip(a[21:], c[21:])), "the swap made no difference to the reward"


def test_params_naming_another_manager_drop_the_recording_cpu(oracle_backend):
    _contact_swap_check("cpu", 70)


@pytest.mark.gpu
@pytest.mark.parametrize("n", GPU_SIZES)
def test_params_naming_another_manager_drop_the_recording_hip(hip_backend, n):
    _contact_swap_check("cuda", n)


# -- what a user step() returns -------------------------------------------------------------------------------------------------------
def _returns_env(variant):
    """User RewardManager / TerminationManager classes whose step() returns what the step must carry on with.  Each logs a copy of
    what it returned, by step.  ``…+reset``: the env overrides reset() as well (a curriculum hook): the done envs are reset by index
    list through it, and ``super().reset(ids)`` must reset from the returned masks too."""
    variant, _, with_reset = variant.partition("+")
    from genesis_forge_amd.managers import RewardManager, TerminationManager

    class Rewards(RewardManager):
        def step(self):
            r = super().step()
            if variant == "reward_double":
                out = r * 2
            elif variant == "reward_where":
                out = torch.where(self.env.episode_length > 3, r, 0)
            else:   # control: in place on the manager's buffer
                out = r.clamp_(min=-0.5)
            self.env.returned.setdefault(self.env.step_count, {})["rew"] = out.clone()
            return out

    class Terminations(TerminationManager):
        def step(self):
            te, tr = super().step()
            env = self.env
            extra = (env.episode_length % 7) == 3   # envs terminated by the override alone
            if variant == "term_or":
                te = te | extra
            elif variant == "term_clone":
                te, tr = te.clone(), tr
            elif variant == "term_mixed":   # in place on some steps, a new tensor on others
                if env.step_count % 3 == 0:
                    te |= extra
                else:
                    te = te | extra
            else:   # control
                te &= env.episode_length > 2
            env.returned.setdefault(env.step_count, {}).update(term=te.clone(), trunc=tr.clone())
            return te, tr

    class Env(Go2CommandDirectionEnv):
        def config(self):
            super().config()
            self.returned = {}
            if variant.startswith("reward") or variant == "in_place":
                rc = {k: {"weight": v.weight, "fn": v.fn, "params": dict(v.params)} for k, v in self.reward_manager.cfg.items()}
                self.managers["reward"] = None
                self.reward_manager = Rewards(self, logging_enabled=True, cfg=rc)
            if variant.startswith("term") or variant == "in_place":
                tc = {k: {"fn": v.fn, "params": dict(v.params), "time_out": v.time_out} for k, v in self.termination_manager.term_cfg.items()}
                self.managers["termination"] = None
                self.termination_manager = Terminations(self, logging_enabled=True, term_cfg=tc)

    if not with_reset:
        return Env

    class ResetEnv(Env):
        def reset(self, env_ids=None):
            return super().reset(env_ids)

    return ResetEnv


def _run_returns(dev, trace, variant, n, horizon=8):
    from genesis_forge_amd.learner import RolloutStorage

    env = _returns_env(variant)(num_envs=n, max_episode_length_s=1, cmd_resample_s=0.3, contacts=True, history=2,
                                scene_kwargs=dict(ang_noise=0.3, seed=3))
    env.trace_enabled = trace
    env.build()
    env.seed(5)
    obs, _ = env.reset()
    store = RolloutStorage(env, horizon).attach()
    store.begin(obs)
    g = torch.Generator().manual_seed(0)
    outs = []
    for k in range(STEPS):
        ep0 = env.episode_length.cpu().clone()
        o, r, te, tr, ex = env.step(torch.randn(n, 12, generator=g).to(dev))
        log = {k: float(v) for k, v in ex["episode"].items()}
        t = k % horizon
        rm, tm = env.reward_manager, env.termination_manager
        outs.append({"step": env.step_count, "obs": o.cpu().clone(), "rew": r.cpu().clone(), "term": te.cpu().clone(), "trunc": tr.cpu().clone(),
                     "ep0": ep0, "ep": env.episode_length.cpu().clone(), "log": log, "resets": int(ex["episode"]._snap.wait().reset_count),
                     "ro_obs": store.observations[t + 1].cpu().clone(), "ro_rew": store.rewards[t].cpu().clone(), "ro_done": store.dones[t].cpu().clone(),
                     "bufs": (rm._reward_buf.cpu().clone(), tm._terminated_buf.cpu().clone(), tm._truncated_buf.cpu().clone())})
    return outs, env


def _check_returns(outs, env):
    """The step returns the values the user's step() returned, resets exactly the envs they mark done — episode lengths and the
    step's reset counter — and the rollout rows hold them."""
    n_done = 0
    for row in outs:
        ret = env.returned[row["step"]]
        if "rew" in ret:
            assert torch.equal(row["rew"], ret["rew"].cpu()), f"step {row['step']}: the reward is not what step() returned"
        if "term" in ret:
            assert torch.equal(row["term"], ret["term"].cpu()) and torch.equal(row["trunc"], ret["trunc"].cpu()), \
                f"step {row['step']}: the masks are not what step() returned"
        done = row["term"] | row["trunc"]
        n_done += int(done.sum())
        want_ep = torch.where(done, torch.zeros_like(row["ep0"]), row["ep0"] + 1)
        assert torch.equal(row["ep"], want_ep), f"step {row['step']}: reset {int((row['ep'] != want_ep).sum())} envs other than the returned done ones"
        assert row["resets"] == int(done.sum()), f"step {row['step']}: the reset counter says {row['resets']}, the returned masks {int(done.sum())}"
        assert torch.equal(row["ro_rew"], row["rew"]) and torch.equal(row["ro_done"], done) and torch.equal(row["ro_obs"], row["obs"]), \
            f"step {row['step']}: the rollout rows are not the step's"
    assert n_done > 0, "no env was reset: the case tests nothing"


def _same_returns(a, b):
    for x, y in zip(a, b):
        assert x["resets"] == y["resets"], f"reset counter differs at step {x['step']}"
        for k in ("obs", "rew", "term", "trunc", "ep", "ro_obs", "ro_rew", "ro_done"):
            assert torch.equal(x[k], y[k]), f"{k} differs at step {x['step']}"
        for i, (p, q) in enumerate(zip(x["bufs"], y["bufs"])):
            assert torch.equal(p, q), f"manager buffer {i} differs at step {x['step']}"
        assert x["log"] == y["log"], f"log differs at step {x['step']}: {x['log']} vs {y['log']}"


VARIANTS = ["reward_double", "reward_where", "term_or", "term_clone", "term_mixed", "in_place", "term_or+reset", "reward_double+reset"]


@pytest.mark.parametrize("variant", VARIANTS)
def test_user_step_returns_are_the_step_outputs_cpu(oracle_backend, variant):
    a, ea = _run_returns("cpu", False, variant, 70)
    _check_returns(a, ea)
    before = oracle_backend.replays
    b, eb = _run_returns("cpu", True, variant, 70)
    tr = eb._trace
    assert tr is not None, f"not recorded: {eb._untraceable}"
    assert len(tr.py_marks) == (2 if variant == "in_place" else 1) and tr.post_refs is None and tr.tail_python == variant.endswith("+reset")
    assert oracle_backend.replays - before >= 30
    _same_returns(a, b)
    _check_returns(b, eb)


@pytest.mark.gpu
@pytest.mark.parametrize("n", GPU_SIZES)
@pytest.mark.parametrize("variant", VARIANTS)
def test_user_step_returns_are_the_step_outputs_hip(hip_backend, variant, n):
    a, ea = _run_returns("cuda", False, variant, n)
    _check_returns(a, ea)
    b, eb = _run_returns("cuda", True, variant, n)
    assert eb._trace is not None and len(eb._trace.py_marks) == (2 if variant == "in_place" else 1)
    _same_returns(a, b)
    _check_returns(b, eb)


def _bad_return_env(what):
    from genesis_forge_amd.managers import RewardManager, TerminationManager

    class Rewards(RewardManager):
        def step(self):
            r = super().step()
            return r.double() if self.env.step_count >= 6 else r

    class Terminations(TerminationManager):
        def step(self):
            te, tr = super().step()
            return (te.float() if self.env.step_count >= 6 else te), tr

    class Env(Go2CommandDirectionEnv):
        def config(self):
            super().config()
            if what == "reward":
                rc = {k: {"weight": v.weight, "fn": v.fn, "params": dict(v.params)} for k, v in self.reward_manager.cfg.items()}
                self.managers["reward"] = None
                self.reward_manager = Rewards(self, logging_enabled=True, cfg=rc)
            else:
                tc = {k: {"fn": v.fn, "params": dict(v.params), "time_out": v.time_out} for k, v in self.termination_manager.term_cfg.items()}
                self.managers["termination"] = None
                self.termination_manager = Terminations(self, logging_enabled=True, term_cfg=tc)

    return Env


@pytest.mark.parametrize("what", ["reward", "termination"])
@pytest.mark.parametrize("trace", [False, True])
def test_user_step_returns_of_another_dtype_are_refused_cpu(oracle_backend, what, trace):
    """The returned tensors are read by address (masked reset, rollout rows, a recorded step's copies): a float mask or a float64
    reward is refused on both paths rather than reinterpreted or silently cast."""
    env = _bad_return_env(what)(num_envs=8, scene_kwargs=dict(seed=3))
    env.trace_enabled = trace
    env.build()
    env.seed(5)
    env.reset()
    for _ in range(5):
        env.step(torch.zeros(8, 12))
    assert (env._trace is not None) == trace   # (step 6 is a replayed step of the recording, or an ordinary step)
    with pytest.raises(TypeError, match="float32" if what == "reward" else "torch.bool"):
        env.step(torch.zeros(8, 12))
