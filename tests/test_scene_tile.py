"""The 64-env tile tick of gf_synth_scene_step against the lane-per-env tick it replaced (GF_SCENE_LEGACY=1), bit for bit,
through the raw C ABI: partial last tiles, the float4 (D = 12, 28) and scalar (D = 5, unaligned rows) joint paths, a non-zero
env_offset, and the per-link / contact tile kernel."""
import ctypes as C
import os

import pytest

from genesis_forge_amd import _native as nat

pytestmark = pytest.mark.gpu


def _lib():
    lib = C.CDLL(nat.lib_path())
    lib.gf_synth_scene_step.restype = C.c_int
    lib.gf_synth_scene_step.argtypes = [C.POINTER(nat.GfSynthSceneArgs), C.c_void_p]
    return lib


def _state(torch, n, d, links, contacts, misalign):
    g = torch.Generator().manual_seed(1000 * n + 10 * d + links + 2 * contacts)
    q = torch.randn(n, 4, generator=g)
    q = q / q.norm(dim=1, keepdim=True)

    def rows(k):   # misalign = 1: the joint rows start 4 B past a 16-byte boundary
        return torch.randn(n * k + misalign, generator=g)
    st = {"pos": torch.randn(n, 3, generator=g) + torch.tensor([0.0, 0.0, 0.3]), "quat": q,
          "lin_vel": torch.randn(n, 3, generator=g), "ang_vel": torch.randn(n, 3, generator=g),
          "targets": rows(d), "dof_pos": rows(d), "dof_vel": torch.zeros(n * d + misalign)}
    L, Cn = 14, 6
    if links:
        st["links_quat_out"] = torch.zeros(n, L, 4)
        st["links_vel_out"] = torch.zeros(n, L, 3)
        st["links_pos_out"] = torch.zeros(n, L, 3)
    if contacts:
        st["contact_force_out"] = torch.zeros(n, Cn, 3)
        st["contact_pos_out"] = torch.zeros(n, Cn, 3)
        st["link_a_out"] = torch.zeros(n, Cn, dtype=torch.int32)
        st["link_b_out"] = torch.zeros(n, Cn, dtype=torch.int32)
    return {k: v.to("cuda") for k, v in st.items()}, L, Cn


def _tick(torch, lib, st, n, d, links, contacts, misalign, legacy, steps=3):
    a = nat.GfSynthSceneArgs()
    a.num_envs, a.num_dofs = n, d
    a.num_contacts = 6 if contacts else 0
    a.num_scene_links = 14
    a.dt, a.joint_rate, a.ang_noise, a.lin_noise, a.height_target = 0.02, 8.0, 0.3, 0.05, 0.3
    a.contact_prob, a.contact_force, a.foot_contact_prob = 0.3, 40.0, 0.5
    a.seed, a.env_offset = 0x1234_5678_9ABC, 777
    a.foot_link_mask = (1 << 5) | (1 << 9) if contacts else 0
    for k, v in st.items():
        base = v.data_ptr()
        if k in ("targets", "dof_pos", "dof_vel"):
            base += 4 * misalign
        setattr(a, k, base)
    os.environ["GF_SCENE_LEGACY"] = "1" if legacy else "0"
    try:
        for t in range(steps):
            a.tick = (5 << 32) + t
            assert lib.gf_synth_scene_step(C.byref(a), None) == 0
        torch.cuda.synchronize()
    finally:
        os.environ.pop("GF_SCENE_LEGACY", None)


@pytest.mark.parametrize("n", [1, 63, 64, 65, 4103, 65536])
@pytest.mark.parametrize("d,misalign", [(12, 0), (28, 0), (5, 0), (12, 1)])
@pytest.mark.parametrize("links,contacts", [(False, False), (True, False), (False, True), (True, True)])
def test_tile_tick_matches_lane_per_env(n, d, misalign, links, contacts):
    torch = pytest.importorskip("torch")
    if not torch.cuda.is_available():
        pytest.fail("no GPU")
    lib = _lib()
    new, _, _ = _state(torch, n, d, links, contacts, misalign)
    old = {k: v.clone() for k, v in new.items()}
    _tick(torch, lib, new, n, d, links, contacts, misalign, legacy=False)
    _tick(torch, lib, old, n, d, links, contacts, misalign, legacy=True)
    for k in new:
        a, b = new[k].cpu(), old[k].cpu()
        assert torch.equal(a.view(torch.int32), b.view(torch.int32)), f"{k}: tile tick differs from the lane-per-env tick"
