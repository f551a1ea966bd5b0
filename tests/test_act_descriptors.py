"""The descriptors of the one-launch collection steps, field by field, without a GPU.

The HIP branch of ``RolloutStorage.act_policy`` / ``act_recurrent`` / ``act_distill`` / ``act_distill_recurrent`` and of the forwards'
``mean`` / ``value`` / ``act`` only fills a ctypes descriptor and hands it to ``backend.<entry>``.  A stub backend that records a copy
of what it was handed stands in for the library; every tensor is a CPU tensor.  Every field of the captured descriptor is compared with
the value ``include/gf_step.h`` gives it, written out here from the tensors — a field no case names must be zero / NULL (every case
starts from a fresh forward)."""
import ctypes as C
from types import SimpleNamespace

import pytest
import torch

N, T = 3, 4                      # envs, steps of the storage
OBS, COBS, HID, A, RH = 5, 7, 4, 2, 4   # obs -> (rnn RH ->) HID -> A actions; the critic / teacher may read COBS
SEED, ENV_OFFSET = 0x1234ABCD5, 64      # the stub env's Philox seed and the global id of its env 0
RNN_LSTM, RNN_GRU = 1, 2         # gf_step.h: GF_RNN_LSTM / GF_RNN_GRU (GF_RNN_NONE is 0)
KINDS = ("lstm", "gru")
ENTRIES = ("policy_act", "mlp_act", "mlp_recurrent_act", "mlp_distill_act", "mlp_recurrent_distill_act")


class _Stub:
    """A backend that captures descriptors and nothing else."""

    def __init__(self):
        self.calls = []

    def __getattr__(self, name):
        if name not in ENTRIES:
            raise AttributeError(name)
        return lambda args: self.calls.append((name, type(args).from_buffer_copy(bytes(args))))

    def last(self, entry):
        name, args = self.calls[-1]
        assert name == entry, f"the launch went to {name}, not {entry}"
        return args


@pytest.fixture()
def stub(monkeypatch):
    from genesis_forge_amd import _native as nat
    from genesis_forge_amd import gs

    b = _Stub()
    monkeypatch.setattr(gs, "device", torch.device("cpu"))
    monkeypatch.setattr(nat, "get_backend", lambda: b)
    torch.manual_seed(0)
    return b


def _store(stub, step=0):
    """A real RolloutStorage over a stub env; ``step`` transitions of the rollout are taken as written."""
    from genesis_forge_amd.learner import RolloutStorage

    om = SimpleNamespace(name="policy", observation_space=SimpleNamespace(shape=(OBS,)), _history_len=1, output="fresh")
    env = SimpleNamespace(num_envs=N, managers={"observation": [om]}, backend=stub, _rng_seed=SEED, env_offset=ENV_OFFSET)
    st = RolloutStorage(env, T)
    st.step = st._serial = step
    return st


def _obs(form, width):
    """``(what the caller passes, its segments, each segment's row_stride field)``."""
    if form == "one":
        x = torch.randn(N, width)
        return x, (x,), (0,)
    if form == "two":
        a, b = torch.randn(N, 2), torch.randn(N, width - 2)
        return (a, b), (a, b), (0, 0)
    buf = torch.randn(N, width + 3)   # "window": the strided view a window-mode ObservationManager hands out
    v = buf[:, :width]
    v._gf_window = True
    return v, (v,), (width + 3,)


# ---- a descriptor as {field path: value}, and what gf_step.h says the fields are ----------------------------------------------------
def _flat(s, prefix=""):
    out = {}
    for name, _ in s._fields_:
        v = getattr(s, name)
        if isinstance(v, C.Array):
            for i, e in enumerate(v):
                out.update(_flat(e, f"{prefix}{name}[{i}]."))
        elif isinstance(v, C.Structure):
            out.update(_flat(v, f"{prefix}{name}."))
        else:
            out[prefix + name] = 0 if v is None else v
    return out


def _same(got, want, skip=()):
    """Every field of ``got`` is ``want``'s, or zero / NULL where ``want`` does not name it; ``skip``: fields checked elsewhere."""
    got = _flat(got)
    assert set(want) <= set(got), sorted(set(want) - set(got))
    full = dict.fromkeys(got, 0)
    full.update(want)
    diff = {k: (got[k], full[k]) for k in got if k not in skip and got[k] != full[k]}
    assert not diff, f"(got, want): {diff}"


def _ptr(t, offset=0):
    return 0 if t is None else t.data_ptr() + offset


def _net(prefix, net, parts, strides, norm=None):
    """GfMlpNet: the segments side by side, the Linear layers in order, the normaliser's buffers."""
    linears = [m for m in net if isinstance(m, torch.nn.Linear)]
    d = {prefix + "num_layers": len(linears), prefix + "num_inputs": len(parts)}
    for i, (x, stride) in enumerate(zip(parts, strides)):
        d.update({f"{prefix}inputs[{i}].rows": x.data_ptr(), f"{prefix}inputs[{i}].width": x.shape[1], f"{prefix}inputs[{i}].row_stride": stride})
    for i, m in enumerate(linears):
        d.update({f"{prefix}layers[{i}].weight": m.weight.data_ptr(), f"{prefix}layers[{i}].bias": m.bias.data_ptr(),
                  f"{prefix}layers[{i}].out_width": m.out_features})
    if norm is not None:
        d.update({prefix + "in_mean": norm._mean.data_ptr(), prefix + "in_std": norm._std.data_ptr(), prefix + "in_eps": C.c_float(norm.eps).value})
    return d


def _cell(prefix, rnn, h, c=None, reset=None, h_save=None, c_save=None):
    """GfRnnCell: the rnn's four parameters read in place, the state, the reset flags and the two save rows."""
    return {prefix + "type": RNN_LSTM if isinstance(rnn, torch.nn.LSTM) else RNN_GRU, prefix + "hidden": rnn.hidden_size,
            prefix + "w_ih": rnn.weight_ih_l0.data_ptr(), prefix + "w_hh": rnn.weight_hh_l0.data_ptr(),
            prefix + "b_ih": rnn.bias_ih_l0.data_ptr(), prefix + "b_hh": rnn.bias_hh_l0.data_ptr(),
            prefix + "h": _ptr(h), prefix + "c": _ptr(c), prefix + "reset": _ptr(reset), prefix + "h_save": _ptr(h_save), prefix + "c_save": _ptr(c_save)}


def _hc(memory):
    """``(h, c)`` of a memory's state, ``c`` None for a GRU."""
    hs = memory.hidden_states
    return (hs[0], hs[1]) if isinstance(hs, tuple) else (hs, None)


def _std(policy):
    return policy.log_std if policy.noise_std_type == "log" else policy.std


def _ppo_sampling(prefix, store, policy, noise, out, t, stream, seed=SEED):
    """The sampling half of a GfMlpActArgs in a collection step: row ``t`` of the five policy rows."""
    return {prefix + "std": _std(policy).data_ptr(), prefix + "noise": _ptr(noise), prefix + "seed": seed, prefix + "stream": stream,
            prefix + "env_offset": ENV_OFFSET, prefix + "std_per_env": 0, prefix + "std_is_log": 1 if policy.noise_std_type == "log" else 0,
            prefix + "mean": 0, prefix + "values": 0, prefix + "actions": out.data_ptr(),
            prefix + "actions_out": store.actions.data_ptr() + t * N * A * 4, prefix + "mu_out": store.mu.data_ptr() + t * N * A * 4,
            prefix + "sigma_out": store.sigma.data_ptr() + t * N * A * 4, prefix + "values_out": store.values.data_ptr() + t * N * 4,
            prefix + "log_prob_out": store.actions_log_prob.data_ptr() + t * N * 4}


def _distill_sampling(prefix, policy, noise, out, stream, seed=SEED, env_offset=ENV_OFFSET, actions_out=0, teacher_actions_out=0):
    """The sampling half of a GfMlpDistillArgs (``teacher_actions``, a fresh tensor, is the caller's to check)."""
    return {prefix + "std": _std(policy).data_ptr(), prefix + "noise": _ptr(noise), prefix + "seed": seed, prefix + "stream": stream,
            prefix + "env_offset": env_offset, prefix + "std_is_log": 1 if policy.noise_std_type == "log" else 0, prefix + "mean": 0,
            prefix + "actions": out.data_ptr(), prefix + "actions_out": actions_out, prefix + "teacher_actions_out": teacher_actions_out}


def _storage_path(store, out, stream_before, serial):
    """What every storage path leaves behind."""
    assert store._act_stream == stream_before + 1, "the noise stream advances by exactly one per call"
    assert store._serial == serial and store._pol_serial == serial + 1
    assert tuple(out.shape) == (N, A) and out.dtype == torch.float32 and out.is_contiguous()
    rows = store.actions
    assert not rows.data_ptr() <= out.data_ptr() < rows.data_ptr() + rows.numel() * 4, "the returned tensor is fresh, not a storage row"


def _twice(stub, entry, call, fresh):
    """Two consecutive calls on one forward: the same descriptor but for ``stream`` and the ``fresh`` output pointers."""
    call()
    first = _flat(stub.last(entry))
    call()
    second = _flat(stub.last(entry))
    stream = [k for k in first if k.endswith("stream")]
    assert len(stream) == 1 and second[stream[0]] == first[stream[0]] + 1
    diff = {k for k in first if first[k] != second[k]} - set(fresh) - set(stream)
    assert not diff, {k: (first[k], second[k]) for k in diff}


# ---- act_policy, PolicyForward.mean / .value ------------------------------------------------------------------------------------------
def _mlp_policy(critic="shared", norm=False, std_type="scalar"):
    from genesis_forge_amd.learner import ActorCriticMLP, PolicyForward

    policy = ActorCriticMLP(OBS, A, (HID,), (HID,), 0.6, num_critic_obs=None if critic == "shared" else COBS,
                            actor_obs_normalization=norm, critic_obs_normalization=norm, noise_std_type=std_type)
    return policy, PolicyForward(policy)


@pytest.mark.parametrize("with_noise", [False, True])
@pytest.mark.parametrize("std_type", ["scalar", "log"])
@pytest.mark.parametrize("norm", [False, True])
@pytest.mark.parametrize("form", ["one", "two", "window"])
@pytest.mark.parametrize("critic", ["shared", "separate"])
def test_act_policy(stub, critic, form, norm, std_type, with_noise):
    policy, fwd = _mlp_policy(critic, norm, std_type)
    store = _store(stub, step=1)
    obs, parts, strides = _obs(form, OBS)
    cobs, cparts, cstrides = (None, parts, strides) if critic == "shared" else _obs("one", COBS)
    noise = torch.randn(N, A) if with_noise else None
    out = store.act_policy(fwd, obs, cobs, noise=noise)
    assert len(stub.calls) == 1
    want = {"num_envs": N}
    want.update(_net("actor.", policy.actor, parts, strides, policy.actor_obs_normalizer if norm else None))
    want.update(_net("critic.", policy.critic, cparts, cstrides, policy.critic_obs_normalizer if norm else None))
    want.update(_ppo_sampling("", store, policy, noise, out, t=1, stream=0))
    _same(stub.last("mlp_act"), want)
    _storage_path(store, out, stream_before=0, serial=1)


def test_act_policy_rows_seed_and_stream(stub):
    """Row 0 at the start of a rollout and once the storage is full, row ``step`` between; ``seed()`` replaces the env's seed and
    restarts the stream."""
    policy, fwd = _mlp_policy()
    store = _store(stub)
    x = torch.randn(N, OBS)
    for call, (step, t) in enumerate(((0, 0), (3, 3), (T, 0))):
        store.step = store._serial = step
        out = store.act_policy(fwd, x)
        got = _flat(stub.last("mlp_act"))
        want = _ppo_sampling("", store, policy, None, out, t=t, stream=call)
        assert {k: got[k] for k in want} == want
    store.seed(7 - (1 << 64))   # (taken modulo 2^64)
    out = store.act_policy(fwd, x)
    got = _flat(stub.last("mlp_act"))
    assert (got["seed"], got["stream"], store._act_stream) == (7, 0, 1)


def test_act_policy_twice(stub):
    policy, fwd = _mlp_policy("separate", norm=True)
    store = _store(stub, step=2)
    x, cx, noise = torch.randn(N, OBS), torch.randn(N, COBS), torch.randn(N, A)
    keep = []
    _twice(stub, "mlp_act", lambda: keep.append(store.act_policy(fwd, x, cx, noise=noise)), fresh=("actions",))


@pytest.mark.parametrize("norm", [False, True])
@pytest.mark.parametrize("form", ["one", "two", "window"])
def test_policy_forward_mean_and_value(stub, form, norm):
    policy, fwd = _mlp_policy("separate", norm)
    obs, parts, strides = _obs(form, OBS)
    out = fwd.mean(obs)
    assert tuple(out.shape) == (N, A) and out.dtype == torch.float32
    want = {"num_envs": N, "mean": out.data_ptr()}   # critic.num_layers == 0; every sampling and row pointer NULL
    want.update(_net("actor.", policy.actor, parts, strides, policy.actor_obs_normalizer if norm else None))
    _same(stub.last("mlp_act"), want)

    policy, fwd = _mlp_policy("separate", norm)
    cobs, cparts, cstrides = _obs(form, COBS)
    out = fwd.value(cobs)
    assert tuple(out.shape) == (N, 1) and out.dtype == torch.float32
    want = {"num_envs": N, "values": out.data_ptr()}
    want.update(_net("critic.", policy.critic, cparts, cstrides, policy.critic_obs_normalizer if norm else None))
    _same(stub.last("mlp_act"), want)


# ---- act_recurrent, RecurrentForward.mean / .value --------------------------------------------------------------------------------------
def _recurrent_policy(kind, norm=False, std_type="scalar", own_state=False):
    from genesis_forge_amd.learner import ActorCriticRecurrent, RecurrentForward

    policy = ActorCriticRecurrent(OBS, A, (HID,), (HID,), 0.6, num_critic_obs=COBS, actor_obs_normalization=norm,
                                  critic_obs_normalization=norm, noise_std_type=std_type, rnn_type=kind, rnn_hidden_dim=RH)
    return policy, RecurrentForward(policy, own_state=own_state)


def _recurrent_want(store, policy, fwd, parts, strides, cparts, cstrides, noise, out, t, stream, norm=False, reset=(None, None), save=None,
                    memories=None):
    ma, mc = memories or (policy.memory_a, policy.memory_c)
    want = {"act.num_envs": N}
    want.update(_net("act.actor.", policy.actor, parts, strides, policy.actor_obs_normalizer if norm else None))
    want.update(_net("act.critic.", policy.critic, cparts, cstrides, policy.critic_obs_normalizer if norm else None))
    want.update(_ppo_sampling("act.", store, policy, noise, out, t=t, stream=stream))
    sa, sc = ((None, None), (None, None)) if save is None else (save["actor"], save["critic"])
    want.update(_cell("actor_cell.", ma.rnn, *_hc(ma), reset=reset[0], h_save=sa[0], c_save=sa[1]))
    want.update(_cell("critic_cell.", mc.rnn, *_hc(mc), reset=reset[1], h_save=sc[0], c_save=sc[1]))
    return want


@pytest.mark.parametrize("with_noise", [False, True])
@pytest.mark.parametrize("norm", [False, True])
@pytest.mark.parametrize("row", [0, 1])
@pytest.mark.parametrize("kind", KINDS)
def test_act_recurrent(stub, kind, row, norm, with_noise):
    policy, fwd = _recurrent_policy(kind, norm, "log" if norm else "scalar")
    store = _store(stub, step=row)
    obs, parts, strides = _obs("two" if row else "window", OBS)
    cobs, cparts, cstrides = _obs("one", COBS)
    noise = torch.randn(N, A) if with_noise else None
    out = store.act_recurrent(fwd, obs, cobs, noise=noise)
    assert len(stub.calls) == 1
    save = None
    if row == 0:   # the launch writes the state the rollout starts from
        save = store.rnn_start
        assert set(save) == {"actor", "critic"}
        for h, c in save.values():
            assert tuple(h.shape) == (N, RH) and h.dtype == torch.float32 and (c is None) == (kind == "gru")
            assert c is None or (tuple(c.shape) == (N, RH) and c.dtype == torch.float32)
    for m in (policy.memory_a, policy.memory_c):   # the policy's own state, created as zeros
        h, c = _hc(m)
        assert tuple(h.shape) == (1, N, RH) and (c is None) == (kind == "gru")
    got = stub.last("mlp_recurrent_act")
    _same(got, _recurrent_want(store, policy, fwd, parts, strides, cparts, cstrides, noise, out, row, 0, norm, save=save))
    if kind == "gru":
        assert got.actor_cell.c is None and got.actor_cell.c_save is None and got.critic_cell.c is None and got.critic_cell.c_save is None
    if row == 1:
        assert got.actor_cell.h_save is None and got.critic_cell.h_save is None and not hasattr(store, "rnn_start")
    _storage_path(store, out, stream_before=0, serial=row)


@pytest.mark.parametrize("kind", KINDS)
def test_act_recurrent_pending_resets(stub, kind):
    policy, fwd = _recurrent_policy(kind)
    store = _store(stub, step=1)
    x, cx = torch.randn(N, OBS), torch.randn(N, COBS)
    parts, cparts = (x,), (cx,)
    dones = torch.tensor([True, False, True])
    # reset(dones), then a step: both cells carry the flags, and both are consumed
    fwd.reset(dones)
    assert all(p is not None for p in fwd._pending.values())
    out = store.act_recurrent(fwd, x, cx)
    want = _recurrent_want(store, policy, fwd, parts, (0,), cparts, (0,), None, out, 1, 0, reset=(dones, dones))
    _same(stub.last("mlp_recurrent_act"), want)
    assert fwd._pending == {"actor": None, "critic": None}
    # the next step carries none
    out = store.act_recurrent(fwd, x, cx)
    _same(stub.last("mlp_recurrent_act"), _recurrent_want(store, policy, fwd, parts, (0,), cparts, (0,), None, out, 1, 1))
    # reset(dones), then value() alone: only the critic's flag is consumed; the actor's waits for the next step
    dones2 = torch.tensor([0, 1, 0], dtype=torch.uint8)
    fwd.reset(dones2)
    v = fwd.value(cx)
    assert fwd._pending["critic"] is None and fwd._pending["actor"] is not None
    want = {"act.num_envs": N, "act.values": v.data_ptr()}
    want.update(_net("act.critic.", policy.critic, cparts, (0,)))
    want.update(_cell("critic_cell.", policy.memory_c.rnn, *_hc(policy.memory_c), reset=dones2))
    # what the kernel does not read of a net that is left out, and of a launch that samples nothing, is left as the last step's
    live = ("act.actor.num_layers", "actor_cell.type", "actor_cell.reset", "actor_cell.h_save", "actor_cell.c_save")
    skip = [k for k in _flat(stub.last("mlp_recurrent_act")) if k.startswith(("act.actor.", "actor_cell.")) and k not in live]
    _same(stub.last("mlp_recurrent_act"), want, skip=skip + ["act.seed", "act.stream", "act.env_offset"])
    out = store.act_recurrent(fwd, x, cx)
    _same(stub.last("mlp_recurrent_act"), _recurrent_want(store, policy, fwd, parts, (0,), cparts, (0,), None, out, 1, 2, reset=(dones2, None)))
    assert fwd._pending == {"actor": None, "critic": None}


@pytest.mark.parametrize("kind", KINDS)
def test_act_recurrent_own_state(stub, kind):
    policy, fwd = _recurrent_policy(kind, own_state=True)
    store = _store(stub, step=0)
    x, cx = torch.randn(N, OBS), torch.randn(N, COBS)
    out = store.act_recurrent(fwd, x, cx)
    assert policy.get_hidden_states() == (None, None), "the policy's own memories are left alone"
    holders = (fwd._memory["actor"], fwd._memory["critic"])
    assert holders[0].rnn is policy.memory_a.rnn and holders[1].rnn is policy.memory_c.rnn
    want = _recurrent_want(store, policy, fwd, (x,), (0,), (cx,), (0,), None, out, 0, 0, save=store.rnn_start, memories=holders)
    _same(stub.last("mlp_recurrent_act"), want)


@pytest.mark.parametrize("kind", KINDS)
def test_act_recurrent_twice(stub, kind):
    policy, fwd = _recurrent_policy(kind, norm=True)
    store = _store(stub, step=1)
    x, cx, noise = torch.randn(N, OBS), torch.randn(N, COBS), torch.randn(N, A)
    keep = []
    _twice(stub, "mlp_recurrent_act", lambda: keep.append(store.act_recurrent(fwd, x, cx, noise=noise)), fresh=("act.actions",))


@pytest.mark.parametrize("norm", [False, True])
@pytest.mark.parametrize("kind", KINDS)
def test_recurrent_forward_mean_and_value(stub, kind, norm):
    policy, fwd = _recurrent_policy(kind, norm)
    obs, parts, strides = _obs("two", OBS)
    out = fwd.mean(obs)
    assert tuple(out.shape) == (N, A) and out.dtype == torch.float32
    want = {"act.num_envs": N, "act.mean": out.data_ptr()}   # the critic: num_layers == 0 and GF_RNN_NONE
    want.update(_net("act.actor.", policy.actor, parts, strides, policy.actor_obs_normalizer if norm else None))
    want.update(_cell("actor_cell.", policy.memory_a.rnn, *_hc(policy.memory_a)))
    got = stub.last("mlp_recurrent_act")
    _same(got, want)
    assert got.critic_cell.type == 0 and got.act.critic.num_layers == 0 and policy.memory_c.hidden_states is None

    policy, fwd = _recurrent_policy(kind, norm)
    cobs, cparts, cstrides = _obs("window", COBS)
    out = fwd.value(cobs)
    assert tuple(out.shape) == (N, 1) and out.dtype == torch.float32
    want = {"act.num_envs": N, "act.values": out.data_ptr()}
    want.update(_net("act.critic.", policy.critic, cparts, cstrides, policy.critic_obs_normalizer if norm else None))
    want.update(_cell("critic_cell.", policy.memory_c.rnn, *_hc(policy.memory_c)))
    got = stub.last("mlp_recurrent_act")
    _same(got, want)
    assert got.actor_cell.type == 0 and got.act.actor.num_layers == 0 and policy.memory_a.hidden_states is None


# ---- act_distill, DistillForward.act / .mean -------------------------------------------------------------------------------------------
def _distill_policy(norm=False, std_type="scalar"):
    from genesis_forge_amd.learner import DistillForward, StudentTeacherMLP

    policy = StudentTeacherMLP(OBS, COBS, A, (HID,), (HID, HID), 0.2, student_obs_normalization=norm, teacher_obs_normalization=norm,
                               noise_std_type=std_type)
    return policy, DistillForward(policy)


@pytest.mark.parametrize("with_noise", [False, True])
@pytest.mark.parametrize("std_type", ["scalar", "log"])
@pytest.mark.parametrize("norm", [False, True])
@pytest.mark.parametrize("form", ["one", "two", "window"])
@pytest.mark.parametrize("row", [0, 1])
def test_act_distill(stub, row, form, norm, std_type, with_noise):
    policy, fwd = _distill_policy(norm, std_type)
    store = _store(stub, step=row)
    obs, parts, strides = _obs(form, OBS)
    tobs, tparts, tstrides = _obs("one", COBS)
    noise = torch.randn(N, A) if with_noise else None
    out = store.act_distill(fwd, obs, tobs, noise=noise)
    assert len(stub.calls) == 1
    want = {"num_envs": N}
    want.update(_net("student.", policy.student, parts, strides, policy.student_obs_normalizer if norm else None))
    want.update(_net("teacher.", policy.teacher, tparts, tstrides, policy.teacher_obs_normalizer if norm else None))
    want.update(_distill_sampling("", policy, noise, out, stream=0, actions_out=store.actions.data_ptr() + row * N * A * 4,
                                  teacher_actions_out=store.privileged_actions.data_ptr() + row * N * A * 4))
    got = stub.last("mlp_distill_act")
    _same(got, want, skip=("teacher_actions",))
    assert got.teacher_actions not in (None, got.actions, got.teacher_actions_out), "the teacher's actions go to a tensor of their own too"
    assert store.values is None and tuple(store.privileged_actions.shape) == (T, N, A)
    _storage_path(store, out, stream_before=0, serial=row)


def test_act_distill_teacher_reads_obs_and_twice(stub):
    from genesis_forge_amd.learner import DistillForward, StudentTeacherMLP

    policy = StudentTeacherMLP(OBS, OBS, A, (HID,), (HID,), 0.2)
    fwd = DistillForward(policy)
    store = _store(stub, step=2)
    obs, parts, strides = _obs("two", OBS)
    out = store.act_distill(fwd, obs)
    want = {"num_envs": N}
    want.update(_net("student.", policy.student, parts, strides))
    want.update(_net("teacher.", policy.teacher, parts, strides))
    want.update(_distill_sampling("", policy, None, out, stream=0, actions_out=store.actions.data_ptr() + 2 * N * A * 4,
                                  teacher_actions_out=store.privileged_actions.data_ptr() + 2 * N * A * 4))
    _same(stub.last("mlp_distill_act"), want, skip=("teacher_actions",))
    keep = []
    _twice(stub, "mlp_distill_act", lambda: keep.append(store.act_distill(fwd, obs)), fresh=("actions", "teacher_actions"))


@pytest.mark.parametrize("norm", [False, True])
def test_distill_forward_act_and_mean(stub, norm):
    policy, fwd = _distill_policy(norm, "log")
    obs, parts, strides = _obs("window", OBS)
    tobs, tparts, tstrides = _obs("two", COBS)
    noise, rows, trows = torch.randn(N, A), torch.zeros(N, A), torch.zeros(N, A)
    actions, teacher = fwd.act(obs, tobs, noise, seed=5 - (1 << 64), stream=9, env_offset=32, actions_out=rows, teacher_actions_out=trows, backend=stub)
    for t in (actions, teacher):
        assert tuple(t.shape) == (N, A) and t.dtype == torch.float32
    want = {"num_envs": N, "teacher_actions": teacher.data_ptr()}
    want.update(_net("student.", policy.student, parts, strides, policy.student_obs_normalizer if norm else None))
    want.update(_net("teacher.", policy.teacher, tparts, tstrides, policy.teacher_obs_normalizer if norm else None))
    want.update(_distill_sampling("", policy, noise, actions, stream=9, seed=5, env_offset=32, actions_out=rows.data_ptr(),
                                  teacher_actions_out=trows.data_ptr()))
    _same(stub.last("mlp_distill_act"), want)
    # no second destinations, no noise, the process-wide backend
    actions, teacher = fwd.act(obs, tobs)
    want.update(_distill_sampling("", policy, None, actions, stream=0, seed=0, env_offset=0))
    want["teacher_actions"] = teacher.data_ptr()
    _same(stub.last("mlp_distill_act"), want)

    policy, fwd = _distill_policy(norm)
    out = fwd.mean(obs)
    assert tuple(out.shape) == (N, A) and out.dtype == torch.float32
    want = {"num_envs": N, "mean": out.data_ptr()}   # a gf_mlp_act descriptor: the student as its actor, no critic, nothing sampled
    want.update(_net("actor.", policy.student, parts, strides, policy.student_obs_normalizer if norm else None))
    _same(stub.last("mlp_act"), want)


# ---- act_distill_recurrent, RecurrentDistillForward.act / .mean -------------------------------------------------------------------------
def _recurrent_distill_policy(kind, teacher_recurrent, norm=False, std_type="scalar", own_state=False):
    from genesis_forge_amd.learner import RecurrentDistillForward, StudentTeacherRecurrent

    policy = StudentTeacherRecurrent(OBS, COBS, A, (HID,), (HID, HID), 0.2, student_obs_normalization=norm, teacher_obs_normalization=norm,
                                     noise_std_type=std_type, rnn_type=kind, rnn_hidden_dim=RH, teacher_recurrent=teacher_recurrent)
    return policy, RecurrentDistillForward(policy, own_state=own_state)


def _recurrent_distill_want(policy, parts, strides, tparts, tstrides, norm, sampling, save=None, reset=(None, None), memories=None):
    ms, mt = memories or (policy.memory_s, getattr(policy, "memory_t", None))
    want = {"act.num_envs": N}
    want.update(_net("act.student.", policy.student, parts, strides, policy.student_obs_normalizer if norm else None))
    want.update(_net("act.teacher.", policy.teacher, tparts, tstrides, policy.teacher_obs_normalizer if norm else None))
    want.update(sampling)
    ss = (None, None) if save is None else save["student"]
    want.update(_cell("student_cell.", ms.rnn, *_hc(ms), reset=reset[0], h_save=ss[0], c_save=ss[1]))
    if mt is not None:   # (without a memory the teacher's cell is GF_RNN_NONE: all zero)
        want.update(_cell("teacher_cell.", mt.rnn, *_hc(mt), reset=reset[1]))
    return want


@pytest.mark.parametrize("norm", [False, True])
@pytest.mark.parametrize("row", [0, 1])
@pytest.mark.parametrize("teacher_recurrent", [False, True])
@pytest.mark.parametrize("kind", KINDS)
def test_act_distill_recurrent(stub, kind, teacher_recurrent, row, norm):
    policy, fwd = _recurrent_distill_policy(kind, teacher_recurrent, norm, "log" if norm else "scalar")
    store = _store(stub, step=row)
    obs, parts, strides = _obs("window" if row else "two", OBS)
    tobs, tparts, tstrides = _obs("one", COBS)
    noise = torch.randn(N, A) if norm else None
    dones = torch.tensor([False, True, True])
    fwd.reset(dones)
    assert set(fwd._pending) == ({"student", "teacher"} if teacher_recurrent else {"student"})
    out = store.act_distill_recurrent(fwd, obs, tobs, noise=noise)
    assert len(stub.calls) == 1
    save = None
    if row == 0:
        save = store.rnn_start
        assert set(save) == {"student"}, "the teacher's start state is not kept"
        h, c = save["student"]
        assert tuple(h.shape) == (N, RH) and h.dtype == torch.float32 and (c is None) == (kind == "gru")
        assert c is None or (tuple(c.shape) == (N, RH) and c.dtype == torch.float32)
    sampling = _distill_sampling("act.", policy, noise, out, stream=0, actions_out=store.actions.data_ptr() + row * N * A * 4,
                                 teacher_actions_out=store.privileged_actions.data_ptr() + row * N * A * 4)
    got = stub.last("mlp_recurrent_distill_act")
    _same(got, _recurrent_distill_want(policy, parts, strides, tparts, tstrides, norm, sampling, save, reset=(dones, dones)), skip=("act.teacher_actions",))
    assert got.act.teacher_actions not in (None, got.act.actions, got.act.teacher_actions_out)
    if not teacher_recurrent:
        tc = got.teacher_cell
        assert tc.type == 0 and tc.reset is None and tc.h_save is None and tc.c_save is None
    assert got.teacher_cell.h_save is None and got.teacher_cell.c_save is None
    if kind == "gru":
        assert got.student_cell.c is None and got.student_cell.c_save is None and got.teacher_cell.c is None
    if row == 1:
        assert got.student_cell.h_save is None and got.student_cell.c_save is None and not hasattr(store, "rnn_start")
    assert all(p is None for p in fwd._pending.values()), "the launch consumed the pending resets"
    _storage_path(store, out, stream_before=0, serial=row)


@pytest.mark.parametrize("teacher_recurrent", [False, True])
@pytest.mark.parametrize("kind", KINDS)
def test_act_distill_recurrent_twice(stub, kind, teacher_recurrent):
    policy, fwd = _recurrent_distill_policy(kind, teacher_recurrent, norm=True)
    store = _store(stub, step=1)
    x, tx, noise = torch.randn(N, OBS), torch.randn(N, COBS), torch.randn(N, A)
    keep = []
    _twice(stub, "mlp_recurrent_distill_act", lambda: keep.append(store.act_distill_recurrent(fwd, x, tx, noise=noise)),
           fresh=("act.actions", "act.teacher_actions"))


@pytest.mark.parametrize("own_state", [False, True])
@pytest.mark.parametrize("teacher_recurrent", [False, True])
@pytest.mark.parametrize("kind", KINDS)
def test_recurrent_distill_forward_act_and_mean(stub, kind, teacher_recurrent, own_state):
    policy, fwd = _recurrent_distill_policy(kind, teacher_recurrent, norm=True, own_state=own_state)
    obs, parts, strides = _obs("two", OBS)
    tobs, tparts, tstrides = _obs("window", COBS)
    noise, rows, trows = torch.randn(N, A), torch.zeros(N, A), torch.zeros(N, A)
    save = {"student": (torch.empty(N, RH), torch.empty(N, RH) if kind == "lstm" else None)}
    actions, teacher = fwd.act(obs, tobs, noise, seed=11, stream=3, env_offset=96, actions_out=rows, teacher_actions_out=trows, backend=stub, save=save)
    for t in (actions, teacher):
        assert tuple(t.shape) == (N, A) and t.dtype == torch.float32
    memories = (fwd._memory["student"], fwd._memory.get("teacher")) if own_state else None
    if own_state:
        assert policy.get_hidden_states() == (None, None)
    sampling = _distill_sampling("act.", policy, noise, actions, stream=3, seed=11, env_offset=96, actions_out=rows.data_ptr(),
                                 teacher_actions_out=trows.data_ptr())
    sampling["act.teacher_actions"] = teacher.data_ptr()
    _same(stub.last("mlp_recurrent_distill_act"), _recurrent_distill_want(policy, parts, strides, tparts, tstrides, True, sampling, save, memories=memories))

    policy, fwd = _recurrent_distill_policy(kind, teacher_recurrent, norm=True, own_state=own_state)
    out = fwd.mean(obs)
    assert tuple(out.shape) == (N, A) and out.dtype == torch.float32
    ms = fwd._memory["student"] if own_state else policy.memory_s
    want = {"act.num_envs": N, "act.mean": out.data_ptr()}   # a gf_mlp_recurrent_act descriptor: the student as its actor, no critic
    want.update(_net("act.actor.", policy.student, parts, strides, policy.student_obs_normalizer))
    want.update(_cell("actor_cell.", ms.rnn, *_hc(ms)))
    got = stub.last("mlp_recurrent_act")
    _same(got, want)
    assert got.critic_cell.type == 0 and got.act.critic.num_layers == 0
