"""learner.ConvEncoder and gf_conv_encode: the conv depth encoder in front of a distillation student.

Reference: torch.nn.functional.conv2d / elu / linear in float64 on the CPU, composed here (_ref).
* on the GPU: ConvEncoder.encode exact on integer data at every tile, block, chunk and tail edge; against torch's own float32 error on
  Gaussian data; the 1-D prefix of the row bit for bit; act_distill, one Distillation.update and a state-dict round trip end to end;
* without one: the constructor's and from_train_cfg's limits, the refusals, act_mean's composition, the state-dict keys, the tile plan."""
import pytest
import torch
import torch.nn.functional as F

from genesis_forge_amd import ConvEncoder
from genesis_forge_amd import _native as nat
from genesis_forge_amd.learner import (ActorCriticMLP, DistillForward, Distillation, EmpiricalNormalization, PPO, RecurrentDistillForward,
                                       RolloutStorage, StudentTeacherMLP, StudentTeacherRecurrent)

U = 2.0 ** -24
# (image_shape, channels, kernel, stride, padding, latent): K = 9, 75, 27 | 32, 25 | 9 | 288 (the 16-byte weight path); Cout 31, 33, 32, 1;
# strides whose output size floors; flat = 620, 396 (vector head rows), 6, 198 (by element; none a multiple of the head's 128-column
# chunk); case 1 has T = 25 and 12 positions: T·Ho·Wo = 300 is no multiple of 32
CASES = [((1, 5, 4), (31,), 3, 1, 1, 1),
         ((3, 7, 6), (33,), 5, 2, 2, 32),
         ((3, 7, 6), (32, 1), (3, 1), (3, 1), (1, 0), 33),
         ((1, 7, 6), (1, 32, 33), (5, 3, 3), (1, 2, 1), (2, 0, 1), 33)]


def _ref(enc, image, dtype=torch.float64):
    x = image.detach().cpu().to(dtype).reshape(-1, *enc.image_shape)
    for m in enc.conv[0::2]:
        x = F.elu(F.conv2d(x, m.weight.detach().cpu().to(dtype), m.bias.detach().cpu().to(dtype), stride=m.stride, padding=m.padding))
    return F.linear(x.flatten(1), enc.head.weight.detach().cpu().to(dtype), enc.head.bias.detach().cpu().to(dtype))


def _encoder(case, integer=False, seed=0):
    shape, ch, k, s, p, latent = case
    torch.manual_seed(seed)
    enc = ConvEncoder(shape, ch, k, s, p, latent)
    if integer:   # 0 / 1 everywhere: ELU is the identity and every sum stays below 2^24
        with torch.no_grad():
            for q in enc.parameters():
                q.copy_(torch.randint(0, 2, q.shape).float())
    return enc


@pytest.mark.gpu
@pytest.mark.parametrize("case", range(len(CASES)))
@pytest.mark.parametrize("n_of", [lambda T: 1, lambda T: T - 1, lambda T: T, lambda T: T + 1, lambda T: 2 * T + 1], ids=["1", "T-1", "T", "T+1", "2T+1"])
def test_encode_is_exact_on_integer_data(hip_backend, case, n_of):
    enc = _encoder(CASES[case], integer=True).cuda()
    n = n_of(enc.plan.tile_envs)
    image = torch.randint(0, 2, (n, enc.image_size), generator=torch.Generator().manual_seed(n)).float()
    want = _ref(enc, image)
    assert float(want.max()) < 2 ** 24 and float(want.min()) >= 0.0
    assert torch.equal(enc.encode(image.cuda()).cpu(), want.float())


@pytest.mark.gpu
@pytest.mark.parametrize("case", CASES + [((1, 12, 16), (16, 32), 3, 2, 0, 64), ((1, 24, 32), (16, 32), 3, 2, 0, 64)], ids=str)
def test_encode_is_as_accurate_as_torch_float32(hip_backend, case):
    """Both are float32 chains of the same lengths in different orders: the kernel may be 4 x as far from float64 as torch's own CPU
    float32 forward, plus 4 ulps of the output's scale."""
    enc = _encoder(case, seed=1)
    image = torch.randn(2 * enc.plan.tile_envs + 1, enc.image_size, generator=torch.Generator().manual_seed(2))
    want = _ref(enc, image)
    torch_err = float((enc(image).detach().double() - want).abs().max())
    err = float((enc.cuda().encode(image.cuda()).cpu().double() - want).abs().max())
    floor = 4 * U * float(want.abs().max())
    print(f"conv_encode accuracy {case}: kernel {err:.3e} torch {torch_err:.3e} ratio {err / max(torch_err, 1e-30):.2f} floor {floor:.3e}")
    assert err <= 4 * torch_err + floor


@pytest.mark.gpu
@pytest.mark.parametrize("w1,norm,layout", [(0, False, "own"), (1, True, "own"), (1, False, "block"), (45, True, "own"), (45, False, "two"),
                                            (45, True, "two"), (45, True, "block")])
def test_the_row_is_the_normalised_columns_then_the_latent(hip_backend, w1, norm, layout):
    enc = _encoder(CASES[1], seed=3).cuda()
    n, S, L = enc.plan.tile_envs + 3, enc.image_size, enc.latent_dim
    block = torch.randn(n, w1 + 7 + S, generator=torch.Generator().manual_seed(4)).cuda()
    if layout == "block":   # the 1-D columns lead a wider block, the image trails it: row strides above the widths
        obs, image = block[:, :w1], block[:, -S:]
    else:
        obs, image = block[:, :w1].contiguous(), block[:, -S:].contiguous()
    if layout == "two":
        obs = (obs[:, :20].contiguous(), obs[:, 20:].contiguous())
    normalizer = None
    want = block[:, :w1].cpu()
    if norm:
        normalizer = EmpiricalNormalization(w1).cuda()
        normalizer._mean.copy_(torch.randn(1, w1))
        normalizer._std.copy_(torch.rand(1, w1) + 0.1)
        want = (want - normalizer._mean.cpu()) / (normalizer._std.cpu() + normalizer.eps)   # gf_mlp_act's staging arithmetic, float32
    out = enc.encode(image, obs if w1 else None, normalizer)
    assert out.shape == (n, w1 + L)
    assert torch.equal(out[:, :w1].cpu(), want)
    assert torch.equal(out[:, w1:], enc.encode(block[:, -S:].contiguous()))


# ---- end to end, tiny: 64 envs, 4 steps, the trailing 8 x 6 columns of the gait env's observation as the image ----------------------
def _tiny(dev, seed=0):
    from test_ppo_update import _env

    env = _env("gait", 64)
    obs, extras = env.reset()
    for t in range(6):   # fill the 5-frame history: the image is the oldest frame's trailing columns
        obs, _r, _te, _tr, extras = env.step(torch.randn(64, env.action_space.shape[0], generator=torch.Generator().manual_seed(t)).to(dev))
    st = RolloutStorage(env, 4, obs_groups={"policy": ["policy"], "teacher": ["policy", "critic"]}).attach()
    st.begin(obs, extras)
    st.seed(5)
    width = lambda g: sum(st._widths[m] for m in st.obs_groups[g])
    torch.manual_seed(seed)
    enc = ConvEncoder((1, 6, 8), (4, 8), 3, 1, 1, latent_dim=16)
    policy = StudentTeacherMLP(width("policy") - 48, width("teacher"), env.action_space.shape[0], (32, 16), (32, 16), init_noise_std=0.3,
                               student_obs_normalization=True, student_encoder=enc).to(dev)
    return env, st, policy, obs, extras


@pytest.mark.gpu
def test_act_distill_update_and_checkpoint_end_to_end(hip_backend):
    env, st, policy, obs, extras = _tiny("cuda")
    fwd = DistillForward(policy)
    policy.student_obs_normalizer._mean.normal_()
    A = env.action_space.shape[0]
    for t in range(st.num_steps):
        tobs = (obs, extras["observations"]["critic"])
        noise = torch.randn(64, A, generator=torch.Generator().manual_seed(t)).cuda()
        actions = st.act_distill(fwd, obs, tobs, noise=noise)
        # encode, then the existing student / teacher launch on the row
        parts, image = policy.split_student_obs(obs)
        assert float(image.abs().max()) > 0.0
        row = policy.student_encoder.encode(image, parts, policy.student_obs_normalizer)
        plain = StudentTeacherMLP(row.shape[1], sum(x.shape[1] for x in tobs), A, (32, 16), (32, 16)).cuda()
        plain.student, plain.teacher, plain.std = policy.student, policy.teacher, policy.std
        want, want_teacher = DistillForward(plain).act(row, tobs, noise)
        assert torch.equal(actions, want) and torch.equal(st.actions[t], want) and torch.equal(st.privileged_actions[t], want_teacher)
        obs, _r, _te, _tr, extras = env.step(actions)
        st.process_env_step(None)

    fresh = _tiny("cuda", seed=9)[2]
    fresh.load_state_dict(policy.state_dict())
    assert torch.equal(DistillForward(fresh).mean(obs), fwd.mean(obs))

    def bc_loss():
        with torch.no_grad():
            return sum(float(F.mse_loss(policy.act_mean(o), target)) for o, target in st.step_batches())

    alg = Distillation(policy, st, num_learning_epochs=3, gradient_length=2, learning_rate=1e-3, max_grad_norm=1.0)   # six small Adam steps
    before, w0 = bc_loss(), policy.student_encoder.conv[0].weight.detach().clone()
    with torch.backends.cudnn.flags(enabled=False):   # (no first-use kernel search for a two-second test)
        alg.update()
    assert not torch.equal(policy.student_encoder.conv[0].weight, w0)
    assert bc_loss() < before


# ---- without a GPU -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kwargs,name", [(dict(channels=(4, 4, 4, 4)), "channels"), (dict(channels=()), "channels"), (dict(channels=(65,)), "channels"),
                                         (dict(image_shape=(65, 8, 8)), "image_shape"), (dict(image_shape=(8, 8)), "image_shape"),
                                         (dict(kernel_size=8), "kernel_size"), (dict(kernel_size=0), "kernel_size"), (dict(kernel_size=(3,)), "kernel_size"),
                                         (dict(stride=4), "stride"), (dict(stride=0), "stride"), (dict(padding=3), "padding"), (dict(padding=-1), "padding"),
                                         (dict(image_shape=(1, 2, 8)), "kernel_size"), (dict(latent_dim=0), "latent_dim"), (dict(latent_dim=513), "latent_dim"),
                                         (dict(image_shape=(1, 128, 128), channels=(64,), padding=1), "image_shape")])
def test_constructor_limits_name_their_argument(kwargs, name):
    with pytest.raises(ValueError, match=name):
        ConvEncoder(**dict(dict(image_shape=(1, 8, 8), channels=(4, 4), kernel_size=3, stride=1, padding=0, latent_dim=8), **kwargs))


def test_from_train_cfg_and_the_refusals():
    enc_cfg = dict(image_shape=(1, 6, 8), channels=(4,), kernel_size=3, stride=2, padding=1, latent_dim=16)
    policy = StudentTeacherMLP.from_train_cfg({"policy": {"student_encoder": enc_cfg, "student_hidden_dims": (8,), "teacher_hidden_dims": (8,)}}, 5, 9, 3)
    assert policy.student[0].in_features == 5 + 16 and policy.student_encoder.plan.flat == 4 * 3 * 4
    keys = set(policy.state_dict())
    assert {"student_encoder.conv.0.weight", "student_encoder.conv.0.bias", "student_encoder.head.weight", "student_encoder.head.bias"} <= keys
    assert not any(k.startswith("student_encoder") for k in StudentTeacherMLP(5, 9, 3, (8,), (8,)).state_dict())
    ppo_teacher = ActorCriticMLP(9, 3, (8,), (8,))
    assert policy.load_state_dict(ppo_teacher.state_dict()) is False and torch.equal(policy.teacher[0].weight, ppo_teacher.actor[0].weight)
    with pytest.raises(ValueError, match="student_encoder"):
        StudentTeacherMLP.from_train_cfg({"policy": {"student_encoder": dict(enc_cfg, dilation=2)}}, 5, 9, 3)
    with pytest.raises(ValueError, match="student_encoder"):
        StudentTeacherRecurrent.from_train_cfg({"policy": {"class_name": "StudentTeacherRecurrent", "student_encoder": enc_cfg}}, 5, 9, 3)
    with pytest.raises(ValueError, match="student_encoder"):
        StudentTeacherRecurrent(5, 9, 3, student_encoder=policy.student_encoder)
    with pytest.raises(ValueError, match="student_encoder"):
        ActorCriticMLP.from_train_cfg({"policy": {"student_encoder": enc_cfg}}, 5, 3)
    with pytest.raises(ValueError, match="student_encoder"):
        PPO(policy, None)
    recurrent = StudentTeacherRecurrent(5, 9, 3, (8,), (8,), rnn_hidden_dim=8)
    recurrent.student_encoder = policy.student_encoder
    with pytest.raises(ValueError, match="student_encoder"):
        RecurrentDistillForward(recurrent)
    with pytest.raises(ValueError, match="split across segments"):   # the image must lie whole inside the last segment
        policy.split_student_obs((torch.zeros(2, 5 + 20), torch.zeros(2, 28)))
    parts, image = policy.split_student_obs((torch.zeros(2, 3), torch.zeros(2, 2 + 48)))
    assert [tuple(x.shape) for x in parts] == [(2, 3), (2, 2)] and image.shape == (2, 48)


def test_act_mean_is_the_torch_composition():
    torch.manual_seed(0)
    enc = ConvEncoder((2, 5, 4), (3, 5), (3, 2), (1, 2), (1, 0), latent_dim=7)
    policy = StudentTeacherMLP(6, 9, 3, (8,), (8,), student_obs_normalization=True, student_encoder=enc)
    policy.student_obs_normalizer._mean.normal_()
    policy.student_obs_normalizer._std.uniform_(0.5, 2.0)
    obs = torch.randn(11, 6 + 40, requires_grad=True)
    norm, d = policy.student_obs_normalizer, torch.float64
    x = torch.cat(((obs[:, :6].double() - norm._mean.double()) / (norm._std.double() + norm.eps), _ref(enc, obs[:, 6:])), dim=1)
    want = F.linear(F.elu(F.linear(x, policy.student[0].weight.to(d), policy.student[0].bias.to(d))), policy.student[2].weight.to(d), policy.student[2].bias.to(d))
    got = policy.act_mean(obs)
    assert float((got.double() - want).abs().max()) <= 64 * U * float(want.abs().max())
    got.sum().backward()
    assert enc.conv[0].weight.grad is not None and obs.grad is not None


# LDS bytes = 4 · (table: the longest K rounded up to 16, + 128 address words) + T · 4 · (the two buffers' env strides): a buffer's stride
# is its largest activation — the head's input rounded up to the head's chunk (128 columns for a latent of up to 128, 32 for 512) — made odd
@pytest.mark.parametrize("kwargs,plan", [
    (dict(image_shape=(1, 12, 16)), (19, 63256, 192)),       # 576 + 19 · 4 · (257 + 561)
    (dict(image_shape=(1, 24, 32)), (4, 61792, 1120)),       # 704 + 4 · 4 · (1153 + 2641)
    (dict(image_shape=(1, 2, 2), channels=(1,), kernel_size=1, stride=1, latent_dim=1), (32, 17728, 4)),   # 576 + 32 · 4 · (5 + 129): the tile's cap
    (dict(image_shape=(1, 8, 8), channels=(64,), kernel_size=7, stride=1, padding=3, latent_dim=512), (3, 50712, 4096)),   # 768 + 3 · 4 · (65 + 4097)
    (dict(image_shape=(1, 64, 126), channels=(1,), kernel_size=1, stride=1), (1, 65096, 8064)),   # 576 + 4 · (8065 + 8065): the last size that fits
    (dict(image_shape=(1, 5, 1613), channels=(1,), kernel_size=1, stride=1), None)])   # 8 065 columns: 576 + 4 · (8065 + 8193) = 65 608 > 65 536
def test_the_tile_plan_at_its_limits(kwargs, plan):
    kwargs = dict(dict(channels=(16, 32), kernel_size=3, stride=2, padding=0, latent_dim=64), **kwargs)
    if plan is None:
        with pytest.raises(ValueError, match="image_shape"):
            ConvEncoder(**kwargs)
        return
    enc = ConvEncoder(**kwargs)
    assert tuple(enc.plan) == plan
    assert enc.plan.lds_bytes <= nat.GF_CONV_LDS_BYTES and 1 <= enc.plan.tile_envs <= nat.GF_CONV_MAX_TILE_ENVS
