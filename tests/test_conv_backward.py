"""learner.ConvEncoder(backward="hip") and gf_conv_encode_backward: the conv depth encoder's parameter gradients in HIP.

Reference: torch autograd in float64 on the CPU over F.conv2d / F.elu / F.linear, composed here (_ref).
* on the GPU: exact on 0/1 data at every tile edge, with a forced tile, forced groups (a workgroup walks three tiles, the last one
  partial) and a strided grad_latent; against torch's own float32 autograd on Gaussian data; the same bits on a second launch; one
  Distillation.update end to end;
* without one: the constructor's refusals, from_train_cfg's key, the backward plan's arithmetic, act_mean with backward="torch"."""
import copy

import pytest
import torch
import torch.nn.functional as F

from genesis_forge_amd import ConvEncoder
from genesis_forge_amd import _native as nat
from genesis_forge_amd.learner import DistillForward, Distillation, RolloutStorage, StudentTeacherMLP
from test_conv_encoder import CASES as FORWARD_CASES

U = 2.0 ** -24
# test_conv_encoder's four, and one with two column blocks in both layers, Cin > 32 in the dgrad and a latent above 128
CASES = FORWARD_CASES + [((2, 9, 8), (64, 64), 3, (2, 1), 1, 130)]
CAMERA = ((1, 12, 16), (16, 32), 3, 2, 0, 64)


def _ref(enc, image, g, dtype=torch.float64):
    """(the parameters' gradients, every layer's pre-activation with its .grad) of latent.backward(g) on the CPU in ``dtype``."""
    params = [q.detach().cpu().to(dtype).requires_grad_() for q in enc.parameters()]   # conv weight, bias, …, head weight, bias
    x, pres = image.cpu().to(dtype).reshape(-1, *enc.image_shape), []
    for i, m in enumerate(enc.conv[0::2]):
        pres.append(F.conv2d(x, params[2 * i], params[2 * i + 1], stride=m.stride, padding=m.padding))
        pres[-1].retain_grad()
        x = F.elu(pres[-1])
    F.linear(x.flatten(1), params[-2], params[-1]).backward(g.cpu().to(dtype))
    return [q.grad for q in params], pres


def _encoder(case, integer=False, seed=0):
    shape, ch, k, s, p, latent = case
    torch.manual_seed(seed)
    enc = ConvEncoder(shape, ch, k, s, p, latent, backward="hip")
    if integer:   # weights 0/1 with density 1/4, biases 0/1, head bias 0: ELU is the identity, its derivative 1
        with torch.no_grad():
            for q in enc.parameters():
                q.copy_((torch.rand(q.shape) < (0.25 if q.dim() > 1 else 0.5)).float())
            enc.head.bias.zero_()
    return enc


# (name, N from the plan's tile T, W1, forced tile_envs, forced groups)
RUNS = [("1", lambda T: 1, 0, 0, 0), ("T-1", lambda T: T - 1, 0, 0, 0), ("T", lambda T: T, 0, 0, 0), ("T+1,strided", lambda T: T + 1, 5, 0, 0),
        ("2T+1", lambda T: 2 * T + 1, 0, 0, 0), ("5T+1,groups=2", lambda T: 5 * T + 1, 0, 0, 2), ("tile_envs=1", lambda T: 3, 5, 1, 2)]


@pytest.mark.gpu
@pytest.mark.parametrize("case", range(len(CASES)))
@pytest.mark.parametrize("run", RUNS, ids=[r[0] for r in RUNS])
def test_backward_is_exact_on_integer_data(hip_backend, case, run):
    _name, n_of, w1, tile_envs, groups = run
    enc = _encoder(CASES[case], integer=True)
    n, L = max(n_of(enc.backward_plan.tile_envs), 1), enc.latent_dim
    gen = torch.Generator().manual_seed(n)
    image = torch.randint(0, 2, (n, enc.image_size), generator=gen).float()
    row = torch.full((n, w1 + L), 7.0)   # (the 1-D columns' gradient: never read)
    row[:, w1:] = F.one_hot(torch.randint(0, L, (n,), generator=gen), L).float()
    want, pres = _ref(enc, image, row[:, w1:])
    for t in want + [p.grad for p in pres]:
        assert float(t.min()) >= 0.0 and float(t.max()) < 2 ** 24
    got = enc.cuda()._backward_hip(image.cuda(), row.cuda(), w1, tile_envs, groups)
    for name, a, b in zip("w0 b0 w1 b1 w2 b2".split()[:len(want) - 2] + ["head_w", "head_b"], got, want):
        assert torch.equal(a.cpu(), b.float()), name


@pytest.mark.gpu
@pytest.mark.parametrize("case", CASES + [CAMERA], ids=str)
def test_backward_is_as_accurate_as_torch_float32(hip_backend, case):
    """Both are float32 sums of the same lengths in different orders: per gradient tensor the kernel may be 4 x as far from float64 as
    torch's own CPU float32 autograd, plus 4 ulps of the tensor's scale.  The row is encode()'s, bit for bit."""
    enc = _encoder(case, seed=1)
    n = 2 * enc.backward_plan.tile_envs + 1
    gen = torch.Generator().manual_seed(2)
    image, g = torch.randn(n, enc.image_size, generator=gen), torch.randn(n, enc.latent_dim, generator=gen)
    want, pres = _ref(enc, image, g)
    assert all(bool((p > 0).any()) and bool((p < 0).any()) for p in pres)   # both ELU branches, in every layer
    torch32, _ = _ref(enc, image, g, torch.float32)
    enc.cuda()
    row = enc.encode_train(image.cuda())
    assert row.grad_fn is not None and torch.equal(row, enc.encode(image.cuda()))
    row.backward(g.cuda())
    for i, (q, w, t) in enumerate(zip(enc.parameters(), want, torch32)):
        err, torch_err = float((q.grad.cpu().double() - w).abs().max()), float((t.double() - w).abs().max())
        floor = 4 * U * float(w.abs().max())
        print(f"conv_backward accuracy {case} tensor {i}: kernel {err:.3e} torch {torch_err:.3e} ratio {err / max(torch_err, 1e-30):.2f} floor {floor:.3e}")
        assert err <= 4 * torch_err + floor, i


@pytest.mark.gpu
@pytest.mark.parametrize("case", [CASES[1], CASES[3]], ids=str)
def test_one_backward_over_two_rows_sums_their_gradients(hip_backend, case):
    """Two encode_train rows of one encoder under a single backward (a loss summed over steps): each node's gradients are tensors of
    their own, so the engine's sum is the reference's — within the Gaussian bound, for the sum."""
    enc = _encoder(case, seed=5)
    n, gen = enc.backward_plan.tile_envs + 1, torch.Generator().manual_seed(6)
    images, gs = torch.randn(2, n, enc.image_size, generator=gen), torch.randn(2, n, enc.latent_dim, generator=gen)
    want = [a + b for a, b in zip(*(_ref(enc, im, g)[0] for im, g in zip(images, gs)))]
    torch32 = [a + b for a, b in zip(*(_ref(enc, im, g, torch.float32)[0] for im, g in zip(images, gs)))]
    enc.cuda()
    torch.autograd.backward([enc.encode_train(im.cuda()) for im in images], [g.cuda() for g in gs])
    for i, (q, w, t) in enumerate(zip(enc.parameters(), want, torch32)):
        err, torch_err = float((q.grad.cpu().double() - w).abs().max()), float((t.double() - w).abs().max())
        assert err <= 4 * torch_err + 4 * U * float(w.abs().max()), i


@pytest.mark.gpu
def test_two_launches_give_the_same_bits(hip_backend):
    enc = _encoder(CASES[3], seed=3).cuda()
    n = 5 * enc.backward_plan.tile_envs + 1
    gen = torch.Generator().manual_seed(4)
    image, g = torch.randn(n, enc.image_size, generator=gen).cuda(), torch.randn(n, enc.latent_dim, generator=gen).cuda()
    first = [t.clone() for t in enc._backward_hip(image, g, 0, 0, 2)]
    assert all(torch.equal(a, b) for a, b in zip(first, enc._backward_hip(image, g, 0, 0, 2)))


# ---- end to end, tiny: test_conv_encoder's setup — 64 envs, 4 steps, the trailing 8 x 6 columns of the gait env's observation as the image
def _tiny():
    from test_ppo_update import _env

    env = _env("gait", 64)
    obs, extras = env.reset()
    for t in range(6):   # fill the 5-frame history: the image is the oldest frame's trailing columns
        obs, _r, _te, _tr, extras = env.step(torch.randn(64, env.action_space.shape[0], generator=torch.Generator().manual_seed(t)).cuda())
    st = RolloutStorage(env, 4, obs_groups={"policy": ["policy"], "teacher": ["policy", "critic"]}).attach()
    st.begin(obs, extras)
    st.seed(5)
    width = lambda g: sum(st._widths[m] for m in st.obs_groups[g])
    enc = dict(image_shape=(1, 6, 8), channels=(4, 8), kernel_size=3, stride=1, padding=1, latent_dim=16)
    cfg = lambda backward: {"policy": {"student_encoder": dict(enc, backward=backward), "student_hidden_dims": (32, 16), "teacher_hidden_dims": (32, 16),
                                       "init_noise_std": 0.3, "student_obs_normalization": True}}
    make = lambda backward: StudentTeacherMLP.from_train_cfg(cfg(backward), width("policy") - 48, width("teacher"), env.action_space.shape[0])
    return env, st, make, obs, extras


@pytest.mark.gpu
def test_update_trains_the_encoder_end_to_end(hip_backend):
    env, st, make, obs, extras = _tiny()
    torch.manual_seed(0)
    policy, torch_policy = make("hip").cuda(), make("torch")   # (torch's own float32 autograd on the CPU, as in the Gaussian test)
    policy.student_obs_normalizer._mean.fill_(0.25)
    torch_policy.load_state_dict(policy.state_dict())
    A, fwd = env.action_space.shape[0], DistillForward(policy)
    for t in range(st.num_steps):
        noise = torch.randn(64, A, generator=torch.Generator().manual_seed(t)).cuda()
        obs, _r, _te, _tr, extras = env.step(st.act_distill(fwd, obs, (obs, extras["observations"]["critic"]), noise=noise))
        st.process_env_step(None)

    # one backward on the same minibatch: the hip encoder's gradients against the torch encoder's, float64 the reference
    o, _target = next(iter(st.step_batches()))
    g = torch.randn(64, A, generator=torch.Generator().manual_seed(9))
    ref = copy.deepcopy(torch_policy).double()
    for p, x, gg in ((policy, o, g.cuda()), (torch_policy, o.cpu(), g), (ref, o.cpu().double(), g.double())):
        mu = p.act_mean(x)
        assert mu.grad_fn is not None
        mu.backward(gg)
    for q, t, w in zip(*(p.student_encoder.parameters() for p in (policy, torch_policy, ref))):
        err, torch_err = float((q.grad.cpu().double() - w.grad).abs().max()), float((t.grad.double() - w.grad).abs().max())
        assert err <= 4 * torch_err + 4 * U * float(w.grad.abs().max())

    def bc_loss():
        with torch.no_grad():
            return sum(float(F.mse_loss(policy.act_mean(o), target)) for o, target in st.step_batches())

    policy.zero_grad(set_to_none=True)
    alg = Distillation(policy, st, num_learning_epochs=3, gradient_length=2, learning_rate=1e-3, max_grad_norm=1.0)   # six small Adam steps
    before, w0 = bc_loss(), policy.student_encoder.conv[0].weight.detach().clone()
    alg.update()
    assert not torch.equal(policy.student_encoder.conv[0].weight, w0)
    assert bc_loss() < before


# ---- without a GPU -------------------------------------------------------------------------------------------------------------------
def test_constructor_refusals_and_the_train_cfg_key():
    base = dict(image_shape=(1, 6, 8), channels=(4,), kernel_size=3, stride=2, padding=1, latent_dim=16)
    with pytest.raises(ValueError, match="backward"):
        ConvEncoder(**base, backward="cuda")
    with pytest.raises(ValueError, match="image_shape.*channels.*no banded backward"):   # the 87 x 58 depth camera: the forward bands it
        ConvEncoder((1, 58, 87), (16, 32), (5, 3), 2, 0, 64, form="banded", backward="hip")
    assert ConvEncoder(**base).backward == "torch" and ConvEncoder(**base).backward_plan is None
    for form in ("tile", "banded"):
        assert ConvEncoder(**base, form=form, backward="hip").backward_plan.tile_envs == 32
    pol = lambda enc: {"policy": {"student_encoder": enc, "student_hidden_dims": (8,), "teacher_hidden_dims": (8,)}}
    policy = StudentTeacherMLP.from_train_cfg(pol(dict(base, backward="hip")), 5, 9, 3)
    assert policy.student_encoder.backward == "hip" and not any("scratch" in k or "workspace" in k for k in policy.state_dict())
    assert copy.deepcopy(policy).student_encoder._scratch is not policy.student_encoder._scratch
    with pytest.raises(ValueError, match="student_encoder"):
        StudentTeacherMLP.from_train_cfg(pol(dict(base, backwards="hip")), 5, 9, 3)


# LDS bytes = 4 · (two tables of max(K + 1, layer 2's Cout · k²) rounded up to 32 words, + 128 address words)
#           + T · 4 · (every activation's size made odd, + the latent made odd)
@pytest.mark.parametrize("image_shape,plan", [
    ((1, 12, 16), (15, 4 * (2 * 288 + 128) + 15 * 4 * (193 + 561 + 193 + 65))),      # T = (65536 - 2816) // 4048
    ((1, 24, 32), (3, 4 * (2 * 288 + 128) + 3 * 4 * (769 + 2641 + 1121 + 65)))])     # T = (65536 - 2816) // 18384
def test_the_backward_plan(image_shape, plan):
    enc = ConvEncoder(image_shape, (16, 32), 3, 2, 0, 64, backward="hip")
    assert tuple(enc.backward_plan) == (plan[0], nat.GF_CONV_BWD_GROUPS, plan[1]) and plan[1] <= nat.GF_CONV_BWD_LDS_BYTES
    a = nat.GfConvBackwardArgs()
    enc._shapes(a.enc).num_envs = 100   # fewer tiles than the persistent grid: one workgroup each
    assert nat.conv_backward_plan(a)[1] == -(-100 // plan[0])
    a.tile_envs = plan[0] + 1
    assert nat.conv_backward_plan(a) is None and nat.conv_backward_workspace_bytes(a) == -2   # GF_E_RANGE: a forced tile that does not fit


def test_act_mean_with_the_torch_backward_is_unchanged():
    torch.manual_seed(0)
    enc = ConvEncoder((2, 5, 4), (3, 5), (3, 2), (1, 2), (1, 0), latent_dim=7, backward="torch")
    policy = StudentTeacherMLP(6, 9, 3, (8,), (8,), student_obs_normalization=True, student_encoder=enc)
    policy.student_obs_normalizer._mean.normal_()
    obs = torch.randn(11, 6 + 40)
    want = policy.student(torch.cat((policy.student_obs_normalizer(obs[:, :6]), enc(obs[:, 6:])), dim=-1))
    assert torch.equal(policy.act_mean(obs), want)
