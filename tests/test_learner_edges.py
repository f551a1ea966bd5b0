"""gf_ppo_loss, gf_adam_step and gf_gae through the raw ABI at the sizes where their loops wrap, their vector / scalar paths meet
and their optional pointers are NULL.

* gf_ppo_loss against torch autograd of rsl_rl's expression evaluated in FLOAT64, with first-order forward-error bounds of the
  float32 arithmetic computed from that reference (``_loss_bounds``); torch's own float32 evaluation has to stay below half of
  every bound (the CPU self-check: it guards the bounds and the inputs, not the kernel).  A in {13 … 64}: the finalize kernel's
  16 waves wrap over the 3 + A record columns from A = 14 on; mb = 16 385: 65 workgroup records, the finalize lanes stride twice.
  Then the loss-only mode, the running sums, and the scalar kernel forced onto A % 4 == 0 by misaligned buffers.
* gf_adam_step against clip_grad_norm_ + torch.optim.Adam(foreach=True) on one flat parameter, two steps, at the chunk edges, at
  257 norm partials and past 2^20 elements, where the norm kernel's workgroups read a second chunk each.
* gf_gae against rsl_rl's compute_returns loop (bit for bit) on T around its 12-step load batches and N around the workgroup
  size, with rows that are never / always / sometimes done; the same grid on the CPU oracle's twin.
* gf_bc_loss and gf_mirror_loss at 256, 257 and 513 workgroup records, where the lanes of finalize_mean_loss stride, and at A = 1,
  with the assertions and float64 bounds of tests/test_distillation.py and tests/test_symmetry.py."""
import functools
import math

import pytest
import torch

from test_learner import _torch_compute_returns
from test_ppo_update import _adam_args, _raw_loss, _synthetic, _torch_loss

U = 2.0 ** -24   # unit roundoff of float32
CLIP, CV, CE = 0.2, 1.0, 0.01   # _torch_loss's / _raw_loss's defaults
SCALARS = ("surrogate", "value_loss", "entropy", "kl_mean", "loss")
GRADS = ("grad_mu", "grad_value", "grad_sigma")
LOSS_A = [13, 14, 16, 28, 37, 64]
LOSS_MB = [256, 257, 16385]


# ---- gf_ppo_loss: the float64 reference and the bounds of a float32 evaluation -------------------------------------------------
def _loss_bounds(inp, ref, clipped):
    """First-order forward-error bounds of a float32 evaluation of the loss, in float64 from the float64 reference ``ref`` of
    the float64 inputs ``inp``.  Per row i: L_i bounds the sum of the magnitudes that enter log ratio_i, gamma_i the relative
    error of ratio_i, E_i the magnitude under the value loss's square."""
    mu, sd, x = inp["mu"], inp["sigma"], inp["actions"]
    mb, A = mu.shape
    d2 = (x - mu) ** 2
    L = (d2 / (2 * sd ** 2) + sd.log().abs() + 0.9189385).sum(-1) + inp["old_log_prob"].abs()
    gamma = U * ((A + 8) * L + 8)
    ar = inp["advantages"].abs() * ref["ratio"]
    if clipped:
        E = torch.maximum((inp["value"] - inp["returns"]).abs(), (inp["target_values"] - inp["returns"]).abs() + CLIP)
    else:
        E = (inp["value"] - inp["returns"]).abs()
    b = {"surrogate": (ar * gamma).mean() + 4 * U * ar.mean(),
         "value_loss": 8 * U * (E ** 2).mean(),
         "entropy": U * (A + 8) * (1.4189385 + sd.log()).abs().sum()}
    kl_terms = (sd / inp["old_sigma"] + 1e-5).log().abs() + (inp["old_sigma"] ** 2 + (inp["old_mu"] - mu) ** 2) / (2 * sd ** 2) + 0.5
    b["kl_mean"] = U * (A + 8) * kl_terms.sum(-1).mean()
    b["loss"] = (b["surrogate"] + CV * b["value_loss"] + CE * b["entropy"]
                 + 2 * U * (ref["surrogate"].abs() + CV * ref["value_loss"] + CE * ref["entropy"].abs()))
    b["grad_mu"] = ref["grad_mu"].abs() * (gamma + 8 * U)[:, None]
    b["grad_value"] = 16 * U * (2 * CV / mb) * E
    b["grad_sigma"] = ((ar / mb * (gamma + 8 * U))[:, None] * (d2 / sd ** 3 + 1 / sd)).sum(0) + 4 * U * CE / sd
    return b


@functools.lru_cache(maxsize=2)   # (the largest case holds some 30 MB)
def _loss_case(mb, A, clipped):
    """The float32 inputs of one shape (on the CPU), their float64 reference and its bounds: computed once, shared, never written."""
    inp = _synthetic(mb, A, "cpu", seed=1)
    inp64 = {k: v.double() for k, v in inp.items()}
    ref = _torch_loss(inp64, clipped)
    assert all(ref[k].dtype == torch.float64 for k in SCALARS + GRADS)
    # no row is left out of any check: no row lies where the two precisions could take different sides of a clamp
    r = ref["ratio"]
    assert float(torch.minimum((r - (1 - CLIP)).abs(), (r - (1 + CLIP)).abs()).min()) > 1e-4, "a ratio within 1e-4 of 1 ± clip"
    assert float(((inp64["value"] - inp64["target_values"]).abs() - CLIP).abs().min()) > 1e-4, "a |v - tv| within 1e-4 of clip"
    assert bool((r < 1 - CLIP).any()) and bool((r > 1 + CLIP).any()) and bool(((r > 1 - CLIP) & (r < 1 + CLIP)).any())
    return inp, ref, _loss_bounds(inp64, ref, clipped)


def _error_over_bound(got, ref, bounds):
    """The worst |got - ref| / bound of each output (0 where both are 0: a clipped row's gradient is exactly zero in both)."""
    out = {}
    for k in SCALARS + GRADS:
        err = (got[k].detach().double().cpu().reshape(ref[k].shape) - ref[k]).abs()
        assert bool(torch.isfinite(err).all()), f"{k}: not finite"
        q = torch.where(err == 0, torch.zeros_like(err), err / bounds[k])
        out[k] = float(q.max())
    return out


def _report(tag, mb, A, clipped, worst):
    print(f"\n{tag} A={A} mb={mb} clipped={int(clipped)} " + " ".join(f"{k}={v:.4f}" for k, v in worst.items()))


@pytest.mark.parametrize("A", LOSS_A)
@pytest.mark.parametrize("mb", LOSS_MB)
@pytest.mark.parametrize("clipped", [True, False])
def test_loss_bounds_hold_torch_f32_cpu(A, mb, clipped):
    """The self-check of the bounds and the inputs (no kernel runs): torch's float32 evaluation of the same expression stays at
    or below half of every bound."""
    inp, ref, bounds = _loss_case(mb, A, clipped)
    worst = _error_over_bound(_torch_loss(inp, clipped), ref, bounds)
    _report("loss_edges torch_f32", mb, A, clipped, worst)
    for k, v in worst.items():
        assert v <= 0.5, f"A={A} mb={mb} clipped={clipped}: torch f32 {k} at {v:.3f} of its bound"


@pytest.mark.gpu
@pytest.mark.parametrize("A", LOSS_A)
@pytest.mark.parametrize("mb", LOSS_MB)
@pytest.mark.parametrize("clipped", [True, False])
def test_loss_kernel_within_f32_bounds(hip_backend, A, mb, clipped):
    inp, ref, bounds = _loss_case(mb, A, clipped)
    dev = {k: v.cuda() for k, v in inp.items()}
    got = _raw_loss(hip_backend, dev, clipped)
    worst = _error_over_bound(got, ref, bounds)
    _report("loss_edges kernel", mb, A, clipped, worst)
    for k, v in worst.items():
        assert v <= 1.0, f"A={A} mb={mb} clipped={clipped}: {k} at {v:.3f} of its bound"
    again = _raw_loss(hip_backend, dev, clipped)   # the workspace is only scratch: a second call gives the same bits
    for k in SCALARS + GRADS:
        assert torch.equal(got[k], again[k]), k


def _launch_loss(backend, t, mb, A, clipped=True):
    """gf_ppo_loss on the tensors of ``t`` as they lie (views at any offset; grad_* / sums may be missing: NULL)."""
    from genesis_forge_amd import _native as nat

    ws = torch.empty(max(1, nat.ppo_loss_workspace_bytes(mb, A) // 8), device=t["mu"].device, dtype=torch.float64)
    a = nat.GfPpoLossArgs()
    a.num_rows, a.num_actions, a.use_clipped_value_loss = mb, A, int(clipped)
    for k in ("mu", "sigma", "value", "actions", "old_log_prob", "advantages", "target_values", "returns", "old_mu", "old_sigma", "out"):
        setattr(a, k, t[k].data_ptr())
    for k in GRADS + ("sums",):
        setattr(a, k, t[k].data_ptr() if k in t else None)
    a.clip_param, a.value_loss_coef, a.entropy_coef = CLIP, CV, CE
    a.workspace, a.workspace_bytes = ws.data_ptr(), ws.numel() * 8
    backend.ppo_loss(a)


def _loss_outputs(mb, A, grads=True):
    t = {"out": torch.full((5,), 7.0, device="cuda")}
    if grads:
        t.update(grad_mu=torch.full((mb, A), 7.0, device="cuda"), grad_value=torch.full((mb,), 7.0, device="cuda"),
                 grad_sigma=torch.full((A,), 7.0, device="cuda"))
    return t


@pytest.mark.gpu
@pytest.mark.parametrize("A", [12, 37])
@pytest.mark.parametrize("mb", [257, 16385])
def test_loss_only_mode_equals_the_call_with_gradients(hip_backend, A, mb):
    """All three gradient pointers NULL: the rows kernel returns before its second pass and the finalize kernel sums three
    record columns; the five scalars are those of the full call, bit for bit."""
    inp = {k: v.cuda() for k, v in _synthetic(mb, A, "cpu", seed=1).items()}
    full, only = _loss_outputs(mb, A), _loss_outputs(mb, A, grads=False)
    _launch_loss(hip_backend, {**inp, **full}, mb, A)
    _launch_loss(hip_backend, {**inp, **only}, mb, A)
    assert bool(torch.isfinite(full["out"]).all()) and bool((full["out"] != 7.0).all())
    assert torch.equal(full["out"], only["out"])


@pytest.mark.gpu
def test_loss_running_sums(hip_backend):
    """sums[] += value_loss, surrogate, entropy (rsl_rl's loss-dict order) in double: zeroed, then two calls."""
    mb, A = 257, 37
    inp = {k: v.cuda() for k, v in _synthetic(mb, A, "cpu", seed=1).items()}
    t = {**inp, **_loss_outputs(mb, A), "sums": torch.zeros(3, device="cuda", dtype=torch.float64)}
    _launch_loss(hip_backend, t, mb, A)
    _launch_loss(hip_backend, t, mb, A)
    out = t["out"].double()
    assert bool((out[:3] != 0).all())
    assert torch.equal(t["sums"], 2.0 * torch.stack([out[1], out[0], out[2]]))


def _offset_view(x, guard=7.0):
    """``x`` one float into a larger buffer (the base of a fresh allocation is 16-byte aligned, so the view is not), one guard
    float before it and three behind."""
    buf = torch.full((x.numel() + 4,), guard, device=x.device, dtype=x.dtype)
    view = buf[1:1 + x.numel()].view(x.shape)
    view.copy_(x)
    assert view.data_ptr() % 16 == 4
    return buf, view


@pytest.mark.gpu
@pytest.mark.parametrize("A", [12, 16])
@pytest.mark.parametrize("which", ["rows", "sigma"])
def test_loss_scalar_path_forced_by_misalignment(hip_backend, A, which):
    """A % 4 == 0 with [mb, A] buffers (or sigma alone) that are not 16-byte aligned: the scalar kernel runs on a shape the vector
    kernel normally takes, with the same arithmetic — every output bit for bit — and writes nothing around grad_mu."""
    mb = 257
    inp = {k: v.cuda() for k, v in _synthetic(mb, A, "cpu", seed=1).items()}
    want = _loss_outputs(mb, A)
    assert all(inp[k].data_ptr() % 16 == 0 for k in ("mu", "actions", "old_mu", "old_sigma", "sigma")) and want["grad_mu"].data_ptr() % 16 == 0
    _launch_loss(hip_backend, {**inp, **want}, mb, A)
    got = _loss_outputs(mb, A)
    t = {**inp, **got}
    keep = []   # (the buffers behind the views)
    for k in (("mu", "actions", "old_mu", "old_sigma", "grad_mu") if which == "rows" else ("sigma",)):
        buf, t[k] = _offset_view(t[k])
        keep.append(buf)
        if k == "grad_mu":
            gbuf, got["grad_mu"] = buf, t[k]
    _launch_loss(hip_backend, t, mb, A)
    for k in ("out",) + GRADS:
        assert bool((want[k] != 7.0).any()) and torch.equal(want[k], got[k]), k
    if which == "rows":
        assert float(gbuf[0]) == 7.0 and bool((gbuf[1 + mb * A:] == 7.0).all()), "a write outside the offset grad_mu view"


# ---- gf_adam_step ---------------------------------------------------------------------------------------------------------------
ADAM_TAIL = 1029   # the elements with large gradients: at 2^20 + 1029 exactly the two chunks the norm kernel's second pass reads


@pytest.mark.gpu
@pytest.mark.parametrize("numel", [1, 3, 4, 5, 1023, 1024, 1025, 262144 + 5, 2 ** 20 + ADAM_TAIL])
@pytest.mark.parametrize("offset", [0, 1])
def test_adam_step_sizes(hip_backend, numel, offset):
    """Two steps (both parities; the bias correction changes) against clip_grad_norm_ + Adam(foreach=True) on one flat parameter.
    The gradient is 1e-4·randn — alone far below max_grad_norm = 1 — plus 0.5·randn on the last 1 029 elements: a norm partial
    that is dropped or counted twice (257 partials: the update kernel's sum wraps by one; 1 026 chunks on 1 024 workgroups: the
    norm kernel's loop wraps) moves the clip coefficient of every element.  Offset 1: views one float into their buffers (the
    scalar kernels), 8 guard floats behind each."""
    from genesis_forge_amd import _native as nat

    g = torch.Generator().manual_seed(numel * 2 + offset)
    bufs = [torch.full((offset + numel + 8,), 7.0, device="cuda") for _ in range(4)]
    params, grads, m, v = (b[offset:offset + numel] for b in bufs)
    assert all(t.data_ptr() % 16 == 4 * offset for t in (params, grads, m, v))
    params.copy_(torch.randn(numel, generator=g))
    m.zero_()
    v.zero_()
    ref = params.detach().clone().requires_grad_(True)
    opt = torch.optim.Adam([ref], lr=1e-3, foreach=True)
    state = torch.zeros(4, device="cuda", dtype=torch.int64)
    state.view(torch.float64)[0] = 1e-3
    ws = torch.zeros(max(1, nat.adam_workspace_bytes(numel) // 8), device="cuda", dtype=torch.float64)
    tail = min(numel, ADAM_TAIL)
    for it in range(2):
        small = 1e-4 * torch.randn(numel, generator=g)
        assert float(small.double().norm()) < 1.0
        gr = small.clone()
        gr[numel - tail:] += 0.5 * torch.randn(tail, generator=g)
        grads.copy_(gr)
        ref.grad = gr.cuda()
        norm = torch.nn.utils.clip_grad_norm_([ref], 1.0)
        if numel >= 1023:
            assert float(norm) > 1.0
        opt.step()
        hip_backend.adam_step(_adam_args(params, grads, m, v, state, ws, it & 1))
        what = f"numel={numel} offset={offset} step {it + 1}: "
        torch.testing.assert_close(grads, ref.grad, rtol=1e-6, atol=1e-7, msg=lambda s: what + "grads: " + s)
        torch.testing.assert_close(params, ref.detach(), rtol=1e-6, atol=1e-7, msg=lambda s: what + "params: " + s)
        torch.testing.assert_close(m, opt.state[ref]["exp_avg"], rtol=1e-6, atol=1e-7, msg=lambda s: what + "exp_avg: " + s)
        torch.testing.assert_close(v, opt.state[ref]["exp_avg_sq"], rtol=1e-6, atol=1e-7, msg=lambda s: what + "exp_avg_sq: " + s)
    assert int(state[1]) == 2 and float(state.view(torch.float64)[0]) == 1e-3
    for b in bufs:
        assert bool((b[:offset] == 7.0).all()) and bool((b[offset + numel:] == 7.0).all()), "a write outside the view"


# ---- gf_gae ---------------------------------------------------------------------------------------------------------------------
GAE_T = [1, 11, 12, 13, 25]
GAE_N = [1, 63, 255, 256, 257, 1000]
GAMMA, LAM = 0.99, 0.95


@functools.lru_cache(maxsize=None)
def _gae_case(T, N, pattern):
    """Inputs of one shape and done pattern (on the CPU) and rsl_rl's loop on them: computed once, shared, never written."""
    gen = torch.Generator().manual_seed(1000 * T + N)
    rew, val, last = torch.randn(T, N, generator=gen), torch.randn(T, N, generator=gen), torch.randn(N, generator=gen)
    dones = {"random": torch.rand(T, N, generator=gen) < 0.3, "never": torch.zeros(T, N, dtype=torch.bool),
             "always": torch.ones(T, N, dtype=torch.bool)}[pattern]
    return rew, val, last, dones


def _gae_call(backend, inputs, normalize, moments=True, offset=0):
    """gf_gae on ``inputs``; ``offset``: the advantages start that many floats into a buffer with guard floats on both sides."""
    from genesis_forge_amd import _native as nat

    rew, val, last, dones = inputs
    T, N = rew.shape
    ret = torch.full((T, N), 7.0, device=rew.device)
    abuf = torch.full((offset + T * N + 4,), 7.0, device=rew.device)
    adv = abuf[offset:offset + T * N].view(T, N)
    assert adv.data_ptr() % 16 == 4 * offset
    mom = torch.full((2,), 7.0, dtype=torch.float64, device=rew.device)
    g = nat.GfGaeArgs()
    g.num_envs, g.num_steps, g.gamma, g.lam, g.normalize = N, T, GAMMA, LAM, int(normalize)
    g.rewards, g.values, g.dones, g.last_values = rew.data_ptr(), val.data_ptr(), dones.data_ptr(), last.data_ptr()
    g.returns, g.advantages = ret.data_ptr(), adv.data_ptr()
    g.moments = mom.data_ptr() if moments else None
    backend.call("gae", g)
    assert bool((abuf[:offset] == 7.0).all()) and bool((abuf[offset + T * N:] == 7.0).all()), "a write outside the advantages"
    return ret, adv, mom


def _check_gae(backend, dev, T, N, pattern, offset=0):
    """returns bit for bit; unnormalised advantages bit for bit, with and without the moments; the moments against exact sums;
    normalised advantages to the existing tests' 1e-5.  The normalising call is left out at N·T = 1: torch's unbiased std of one
    element is NaN, the kernel's variance there is 0 and it writes 0."""
    what = f"T={T} N={N} dones={pattern} offset={offset}: "
    n = T * N
    inputs = tuple(t.to(dev) for t in _gae_case(T, N, pattern))
    rew, val, last, dones = inputs
    want_ret, want_adv, raw = _torch_compute_returns(rew, val, dones, last, GAMMA, LAM, normalize=n > 1)
    assert torch.equal(raw, want_ret - val)
    x = raw.double().flatten().tolist()
    s1, s2, sabs = math.fsum(x), math.fsum(e * e for e in x), math.fsum(abs(e) for e in x)   # (a float32 squared is exact in double)

    def check_moments(mom, call):
        assert abs(float(mom[0]) - s1) <= n * 2.0 ** -53 * sabs, what + f"{call}: moments[0] {float(mom[0])!r} vs {s1!r}"
        assert abs(float(mom[1]) - s2) <= n * 2.0 ** -53 * s2, what + f"{call}: moments[1] {float(mom[1])!r} vs {s2!r}"

    ret, adv, mom = _gae_call(backend, inputs, False, offset=offset)
    assert torch.equal(ret, want_ret), what + f"returns differ from the torch loop by {float((ret - want_ret).abs().max())}"
    assert torch.equal(adv, raw), what + "advantages != returns - values"
    check_moments(mom, "normalize = 0")
    ret, adv, mom = _gae_call(backend, inputs, False, moments=False, offset=offset)
    assert torch.equal(ret, want_ret) and torch.equal(adv, raw), what + "normalize = 0 without the moments"
    assert bool((mom == 7.0).all())
    if n == 1:
        return
    ret, adv, mom = _gae_call(backend, inputs, True, offset=offset)
    assert torch.equal(ret, want_ret), what + "returns of the normalising call"
    assert torch.allclose(adv, want_adv, atol=1e-5, rtol=1e-5), what + f"normalised advantages: {float((adv - want_adv).abs().max())}"
    check_moments(mom, "normalize = 1")


@pytest.mark.gpu
@pytest.mark.parametrize("T", GAE_T)
@pytest.mark.parametrize("N", GAE_N)
def test_gae_kernel_shapes(hip_backend, T, N):
    """gf_gae alone: T around the 12 steps the kernel loads per batch, N around its workgroup size, rows that are sometimes / never
    / always done.  Normalisation at N·T = 1 is left out (see _check_gae)."""
    for pattern in ("random", "never", "always"):
        _check_gae(hip_backend, "cuda", T, N, pattern)


@pytest.mark.parametrize("T", GAE_T)
@pytest.mark.parametrize("N", GAE_N)
def test_gae_oracle_shapes(oracle_backend, T, N):
    """The CPU oracle's twin of gf_gae on the grid of test_gae_kernel_shapes."""
    for pattern in ("random", "never", "always"):
        _check_gae(oracle_backend, "cpu", T, N, pattern)


# N·T % 4 of 1, 2, 3 and 0 (an aligned buffer: 16-byte lanes and a scalar last lane), each also 4 bytes into its buffer (the scalar
# branch of the normalising kernel on every lane); more than one workgroup of that kernel at 13 x 258 and 12 x 256
GAE_TAILS = [(13, 257), (13, 258), (11, 257), (12, 256), (1, 2), (1, 3)]


@pytest.mark.gpu
@pytest.mark.parametrize("T,N", GAE_TAILS)
@pytest.mark.parametrize("offset", [0, 1])
def test_gae_normalize_tails_and_misaligned_advantages(hip_backend, T, N, offset):
    assert sorted({t * n % 4 for t, n in GAE_TAILS}) == [0, 1, 2, 3]
    _check_gae(hip_backend, "cuda", T, N, "random", offset=offset)


@pytest.mark.parametrize("T,N", GAE_TAILS)
@pytest.mark.parametrize("offset", [0, 1])
def test_gae_oracle_tails_and_misaligned_advantages(oracle_backend, T, N, offset):
    _check_gae(oracle_backend, "cpu", T, N, "random", offset=offset)


# ---- finalize_mean_loss (gf_reduce.h): the record stride of gf_bc_loss and gf_mirror_loss ------------------------------------------------
# One workgroup of 256 lanes sums ceil(rows / 256) records with a lane stride: 256 records — every lane one; 257 — lane 0 two;
# 513 — lane 0 three, every other lane two.
MEAN_LOSS_ROWS = [65536, 65537, 131073]
MEAN_LOSS_LANES = 256


def _records_per_lane(rows):
    nb = -(-rows // MEAN_LOSS_LANES)
    return nb, [len(range(lane, nb, MEAN_LOSS_LANES)) for lane in (0, 1, MEAN_LOSS_LANES - 1)]


def test_mean_loss_rows_reach_the_record_stride():
    assert [_records_per_lane(r) for r in MEAN_LOSS_ROWS] == [(256, [1, 1, 1]), (257, [2, 1, 1]), (513, [3, 2, 2])]
    assert _records_per_lane(513) == (3, [1, 1, 0]), "where the suite stopped before: three records, no lane strides"


@functools.lru_cache(maxsize=1)
def _mean_loss_inputs(rows, A):
    """mu, target (CPU float32) with |d| exactly 1, just inside and just outside in the first elements, as test_bc_loss_and_gradient."""
    g = torch.Generator().manual_seed(rows + A)
    mu, target = torch.randn(rows, A, generator=g), torch.randn(rows, A, generator=g) * 1.5
    one = torch.tensor(1.0)
    edge = [1.0, -1.0, float(torch.nextafter(one, one * 0)), -float(torch.nextafter(one, one * 0)), float(torch.nextafter(one, one * 2)),
            -float(torch.nextafter(one, one * 2))]
    target.view(-1)[:len(edge)] = 0.0
    mu.view(-1)[:len(edge)] = torch.tensor(edge)
    assert (mu - target).view(-1)[:len(edge)].tolist() == edge
    return mu, target


@pytest.mark.gpu
@pytest.mark.parametrize("A", [1, 3])
@pytest.mark.parametrize("rows", MEAN_LOSS_ROWS)
def test_bc_loss_record_stride(hip_backend, rows, A):
    """test_bc_loss_and_gradient's assertions and bounds (neither derivation depends on the row count: the sum is double) where the
    finalize lanes stride; every row is in every check."""
    from test_distillation import _bc_loss
    from test_symmetry import _mirror_loss

    perm, sign = torch.arange(A, dtype=torch.int32, device="cuda"), torch.ones(A, device="cuda")
    mu, target = (x.cuda() for x in _mean_loss_inputs(rows, A))
    d64 = mu.double() - target.double()
    for loss_type in (0, 1):
        if loss_type == 0:
            loss64, grad64 = float((d64 * d64).mean()), 2.0 * d64 / (rows * A)
        else:
            e = torch.where(d64.abs() < 1, 0.5 * d64 * d64, d64.abs() - 0.5)
            loss64, grad64 = float(e.mean()), d64.clamp(-1, 1) / (rows * A)
            ref = torch.nn.functional.huber_loss(mu.double(), target.double())
            assert abs(float(ref) - loss64) <= 1e-13 * loss64, "the float64 reference is torch's huber_loss"
        grad = torch.full((rows, A), 7.0, device="cuda")
        sums = torch.tensor([1.5], dtype=torch.float64, device="cuda")
        out = _bc_loss(hip_backend, mu, target, loss_type, grad, sums)
        e_loss = abs(float(out[0]) - loss64) / loss64
        e_grad = float(((grad.double() - grad64).abs() / grad64.abs().clamp_min(1e-300)).max())
        print(f"    A={A} rows={rows} type={loss_type}: loss rel err {e_loss:.3e}, grad rel err {e_grad:.3e} (bounds {4 * U:.3e})")
        assert e_loss <= 4 * U, f"loss {float(out[0])} vs {loss64}"
        assert bool(((grad.double() - grad64).abs() <= 4 * U * grad64.abs()).all()), f"gradient: max rel err {e_grad}"
        assert float(sums[0]) == 1.5 + float(out[0]), "the running sum takes the float32 loss"
        if loss_type == 0:
            zero = torch.zeros(rows, A, device="cuda")
            mir = _mirror_loss(hip_backend, mu, target, perm, sign, 1.0, zero)
            assert torch.equal(mir, out) and torch.equal(zero, grad), "mse is gf_mirror_loss's operation order"
        again = torch.full((rows, A), -3.0, device="cuda")   # written, not added; bitwise reproducible; loss only writes out / sums
        assert torch.equal(_bc_loss(hip_backend, mu, target, loss_type, again), out) and torch.equal(again, grad)
        assert torch.equal(_bc_loss(hip_backend, mu, target, loss_type, None, sums), out)
        assert float(sums[0]) == (1.5 + float(out[0])) + float(out[0])


@pytest.mark.gpu
@pytest.mark.parametrize("A", [1, 3])
@pytest.mark.parametrize("rows", MEAN_LOSS_ROWS)
def test_mirror_loss_record_stride(hip_backend, rows, A):
    """test_mirror_loss_and_gradient_against_float64's assertions and bounds where the finalize lanes stride.  A = 3: a 2-cycle, a fixed
    point and both signs; A = 1 has the one permutation, with sign -1."""
    from test_symmetry import _mirror_loss

    perm, sign = ([1, 0, 2], [-1.0, -1.0, 1.0]) if A == 3 else ([0], [-1.0])
    assert (perm != list(range(A)) or A == 1) and (len(set(sign)) == 2 or A == 1)
    p, s = torch.tensor(perm, dtype=torch.int32, device="cuda"), torch.tensor(sign, dtype=torch.float32, device="cuda")
    coeff = 0.75   # (exact in float32)
    g = torch.Generator().manual_seed(rows + A)
    mm, mo = torch.randn(rows, A, generator=g).cuda(), torch.randn(rows, A, generator=g).cuda()
    d64 = mm.double() - s.double() * mo.double()[:, p.long()]
    loss64, grad64 = float((d64 * d64).mean()), coeff * 2.0 * d64 / (rows * A)
    zero = torch.zeros(rows, A, device="cuda")
    sums = torch.tensor([1.5], dtype=torch.float64, device="cuda")
    out = _mirror_loss(hip_backend, mm, mo, p, s, coeff, zero, sums)
    e_loss = abs(float(out[0]) - loss64) / loss64
    e_grad = float(((zero.double() - grad64).abs() / grad64.abs().clamp_min(1e-300)).max())
    print(f"    A={A} rows={rows}: loss rel err {e_loss:.3e} (bound {4 * U:.3e}), grad rel err {e_grad:.3e} (bound {4 * U:.3e})")
    assert e_loss <= 4 * U, f"loss {float(out[0])} vs {loss64}"
    assert bool(((zero.double() - grad64).abs() <= 4 * U * grad64.abs()).all()), f"gradient: max rel err {e_grad}"
    assert float(sums[0]) == 1.5 + float(out[0]), "the running sum takes the float32 loss"
    base = torch.randn(rows, A, generator=g).cuda()   # added into a non-zero buffer, not stored
    buf = base.clone()
    again = _mirror_loss(hip_backend, mm, mo, p, s, coeff, buf)
    assert torch.equal(buf, base + zero) and torch.equal(again, out), "bitwise reproducible, and an addition"
    assert torch.equal(_mirror_loss(hip_backend, mm, mo, p, s, coeff, None), out)
    keep = base.clone()
    keep[0, 0] = -0.0
    bits = keep.view(torch.int32).clone()
    assert torch.equal(_mirror_loss(hip_backend, mm, mo, p, s, 0.0, keep), out)
    assert torch.equal(keep.view(torch.int32), bits)
