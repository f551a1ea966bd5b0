"""gf_masked_reset through its raw descriptor, at its edges (cases and numpy restatement: tests/reset_cases.py).

Every case of the table runs twice against the restatement, bit for bit on integer views of EVERY buffer the descriptor names: on
the CPU oracle (``gfo_masked_reset``, unmarked: this is what the restatement is held to before a GPU is touched) and on the GPU
(``gf_masked_reset``).  Buffers are slices of sentinel-filled allocations with 64 sentinel rows behind them (where a lane past
``num_envs`` would store) and guards around them; a buffer whose pointer a case leaves NULL is allocated all the same and must not
change.  The integer statistics are compared as sums over the 64 shards; ``reward_episode_sum`` with ``==`` where the quotients
are dyadic and under the derived bound of ``reset_cases.sums_close`` in the random-quotients cases.

The chain: the ops [reset, command(masked), command(masked), gait(masked)] through ``gf_run_ops`` with GF_OPT_CHAIN on fold into
``chain_b_kernel`` (the same bodies in their second build, one body per wave of a 256-lane workgroup) and with the option off run
as four launches; both must equal the restatement.  The library has no counter or hook that says which of the two ran (a profiled
phase keeps its own launch, so the profile hooks switch the chain off)."""
import numpy as np
import pytest

import reset_cases as rc
from genesis_forge_amd import _native as nat

FN = "masked_reset"
NAMES = sorted(rc.RESET)
CHAIN_SIZES = (65, 130, 4097)


def test_restatement_pins():
    """The restatement itself at the values the issue names, and against what it does not share with the oracle."""
    _s, want, _st = rc.case(FN, "episode_length_ties")
    assert want["max_episode_length"][:5].tolist() == [100, 100, 102, 98, 102]     # 99.5, 100.5, 101.5 to even; -2; 2 - 2^-22 rounds up
    x = np.linspace(-7.0, 7.0, 4001).astype(np.float32)
    s, c = rc.sincos_det(x)
    assert np.abs(s - np.sin(x.astype(np.float64))).max() < 2.5e-7 and np.abs(c - np.cos(x.astype(np.float64))).max() < 2.5e-7   # 2 ulp of 1
    import helpers
    fix = helpers.load("terrain")   # heights recorded from the reference's get_terrain_height
    tv = dict(height_field=rc.terrain_fixture(), x_min=-3.0, x_span=12.0, y_min=1.5, y_span=10.0, origin_z=0.25)
    assert np.abs(rc.terrain_height(tv, fix["x"], fix["y"]) - fix["heights"]).max() < 1e-6
    _s, want, st = rc.case(FN, "poison_bystander")
    assert all(np.isfinite(st["reward_episode_sum"]))
    _s, want, st = rc.case(FN, "poison_reset_env")
    assert st["reward_episode_sum"][0] == np.inf and st["reward_episode_sum"][1] == -np.inf and np.isnan(st["reward_episode_sum"][2])
    for name in NAMES:   # no case lets a NaN the arithmetic generated reach a float32 buffer (its sign is the platform's)
        spec, want, _st = rc.case(FN, name)
        for k, w in want.items():
            if w is not None and w.dtype == np.float32:
                assert not (np.isnan(w) & ~np.isnan(spec.arr[k])).any(), (name, k)


def _chain_specs(n):
    return [rc.reset_spec(n, D=12, T=5, mask="three_groups", spawn=True), rc.command_spec(n, R=3, mode=rc.CMD_MASKED, mask="three_groups"),
            rc.command_spec(n, R=5, mode=rc.CMD_MASKED, mask="three_groups", key=1), rc.gait_spec(n, mode=rc.CMD_MASKED, mask="three_groups")]


def _chain(backend, dev, n):
    specs = _chain_specs(n)
    wants = [rc.restate(s, flags_all=backend.name != "hip") for s in specs]   # (the oracle rewrites every block's swing / stance byte)
    for chain in (1, 0):
        if backend.name == "hip":
            backend.set_option(nat.GF_OPT_CHAIN, chain)
        try:
            ls = [rc.Launch(dev, s) for s in specs]
            assert rc.run_ops(backend, ls) == (0, -1)
        finally:
            if backend.name == "hip":
                backend.set_option(nat.GF_OPT_CHAIN, 1)
        for i, (l, (w, st)) in enumerate(zip(ls, wants)):
            l.check(w, st, f"op {i} of the run, chain option {chain}, {n} envs")
        if backend.name != "hip":
            break


# ---- CPU: the oracle against the restatement ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", NAMES)
def test_oracle_equals_the_restatement(oracle_backend, name):
    rc.run_case(oracle_backend, "cpu", FN, name)


def test_oracle_sharding_identity(oracle_backend):
    rc.sharding_identity(oracle_backend, "cpu", FN)


@pytest.mark.parametrize("n", CHAIN_SIZES)
def test_oracle_runs_the_four_ops_like_the_restatement(oracle_backend, n):
    _chain(oracle_backend, "cpu", n)


@pytest.mark.parametrize("which", ["scene_quat", "quat_stash"])
def test_oracle_refuses_a_misaligned_quaternion(oracle_backend, which):
    rc.refusal(oracle_backend, "cpu", rc.reset_spec(130, mask="all"), which)


# ---- GPU ----------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("name", NAMES)
def test_kernel_equals_the_restatement(hip_backend, name):
    rc.run_case(hip_backend, "cuda", FN, name)


@pytest.mark.gpu
def test_kernel_sharding_identity(hip_backend):
    rc.sharding_identity(hip_backend, "cuda", FN)


@pytest.mark.gpu
@pytest.mark.parametrize("n", CHAIN_SIZES)
def test_chain_and_four_launches_equal_the_restatement(hip_backend, n):
    _chain(hip_backend, "cuda", n)


@pytest.mark.gpu
@pytest.mark.parametrize("which", ["scene_quat", "quat_stash"])
def test_library_refuses_a_misaligned_quaternion(hip_backend, which):
    rc.refusal(hip_backend, "cuda", rc.reset_spec(130, mask="all"), which)
