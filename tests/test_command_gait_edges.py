"""gf_command_step and gf_gait_step through their raw descriptors, at their edges (cases and restatement: tests/reset_cases.py).

As in tests/test_reset_edges.py every case runs on the CPU oracle (unmarked) and on the GPU against the numpy restatement, bit for
bit on integer views of every buffer, with sentinel rows behind the arrays and the NULL-pointer buffers checked for silence.
``resample_count`` moves in STEP mode only; ``gait_count`` is the count per gait after the step's resample.  The swing / stance
bytes start from the sentinel 0xA5: a masked gait launch of the library rewrites only the blocks that hold a reset env (the oracle
rewrites every block, which the header also allows — ``flags_all`` in the restatement)."""
import numpy as np
import pytest

import reset_cases as rc

CMD, GAIT = "command_step", "gait_step"
CMD_NAMES, GAIT_NAMES = sorted(rc.COMMAND), sorted(rc.GAIT)


def test_restatement_pins():
    _s, want, _st = rc.case(GAIT, "trot_after_reset")
    assert want["wave_flags"][:2].tolist() == [rc.TROT_BYTE] * 2 == [0x69, 0x69]      # feet 0, 3 swing; feet 1, 2 on phi == π: stance
    spec, want, _st = rc.case(GAIT, "masked_65_last_block")
    assert want["wave_flags"][0] == 0xA5 and want["wave_flags"][1] == rc.foot_flags(want["state"][64:, 15], want["state"][64:, 0:4], rc.TWO_PI)[0]
    spec, want, _st = rc.case(GAIT, "inverse_cdf_edges")
    assert want["selected"][:9].tolist() == [1, 2, 3, 0, 1, 2, 1, 2, 3]                 # on the weight: the next gait; one ulp below: this one
    spec, want, st = rc.case(GAIT, "clock_edges")
    t = want["state"][:12, 14]
    assert t[0] == np.float32(0.1) + rc.DT and t[1] == 0 and t[3] == rc.DT and np.isnan(t[7]) and t[5] < np.float32(0.3)
    assert sum(st["gait_count"]) == 128                                               # selected -1 and 7 are no gait
    spec, want, _st = rc.case(CMD, "ranges_degenerate")
    c = want["command"]
    assert (c[:, 0] == 0.75).all() and (np.abs(c[:, 1]) <= 2).all() and (np.abs(c[:, 2:4]) <= np.float32(1e30)).all()
    assert np.isposinf(c[:, 4]).all() and np.isneginf(c[:, 5]).all() and (c[:, 6] == 0).all()   # hi - lo = ±inf; u > 0
    for fn, names in ((CMD, CMD_NAMES), (GAIT, GAIT_NAMES)):   # a NaN reaches a buffer only from a NaN input (the NaN period row)
        for name in names:
            spec, want, _st = rc.case(fn, name)
            for k, w in want.items():
                if w is not None and w.dtype == np.float32 and np.isnan(w).any():
                    assert name == "clock_edges" and k == "state" and np.isnan(spec.arr[k][np.isnan(w).any(axis=1)]).any(axis=1).all(), (name, k)


# ---- CPU: the oracle against the restatement ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", CMD_NAMES)
def test_oracle_command_equals_the_restatement(oracle_backend, name):
    rc.run_case(oracle_backend, "cpu", CMD, name)


@pytest.mark.parametrize("name", GAIT_NAMES)
def test_oracle_gait_equals_the_restatement(oracle_backend, name):
    rc.run_case(oracle_backend, "cpu", GAIT, name, flags_all=True)


@pytest.mark.parametrize("fn", [CMD, GAIT])
def test_oracle_sharding_identity(oracle_backend, fn):
    rc.sharding_identity(oracle_backend, "cpu", fn)


def test_oracle_refuses_misaligned_gait_rows(oracle_backend):
    rc.refusal(oracle_backend, "cpu", rc.gait_spec(130, mode=rc.CMD_ALL), "state")


# ---- GPU ----------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("name", CMD_NAMES)
def test_command_kernel_equals_the_restatement(hip_backend, name):
    rc.run_case(hip_backend, "cuda", CMD, name)


@pytest.mark.gpu
@pytest.mark.parametrize("name", GAIT_NAMES)
def test_gait_kernel_equals_the_restatement(hip_backend, name):
    rc.run_case(hip_backend, "cuda", GAIT, name)


@pytest.mark.gpu
@pytest.mark.parametrize("fn", [CMD, GAIT])
def test_kernel_sharding_identity(hip_backend, fn):
    rc.sharding_identity(hip_backend, "cuda", fn)


@pytest.mark.gpu
def test_library_refuses_misaligned_gait_rows(hip_backend):
    rc.refusal(hip_backend, "cuda", rc.gait_spec(130, mode=rc.CMD_ALL), "state")
