"""learner.ConvEncoder(form="banded") and gf_conv_encode_banded: the conv depth encoder in row bands, the head as a launch of its own.

* on the GPU: bit-equal to the tile form (the same k-ascending chains) at every band, tile, block and slab edge, the 1-D prefix included;
  a camera only this form serves against torch in float64; DistillationRunner end to end;
* without one: the plan of the cameras the tile form refuses, and the refusals."""
import pytest
import torch

from genesis_forge_amd import ConvEncoder
from genesis_forge_amd import _native as nat
from genesis_forge_amd.learner import EmpiricalNormalization
from test_conv_encoder import U, _ref

DEPTH = dict(image_shape=(1, 58, 87), channels=(16, 32), kernel_size=(5, 3), stride=2, padding=0, latent_dim=64)   # the parkour depth camera
# (image_shape, channels, kernel, stride, padding, latent): K = 9 (the by-element weight path) | a two-layer halo, a flooring stride, two
# latent column blocks | three layers, stride 3 | two conv column blocks.  The last layer's output is 7, 5, 2 and 4 rows high.
CASES = [((1, 7, 6), (3,), 3, 1, 1, 5),
         ((2, 9, 8), (4, 5), (3, 3), (2, 1), (1, 1), 33),
         ((1, 11, 7), (3, 4, 2), (5, 3, 3), (3, 1, 1), (2, 0, 1), 7),
         ((3, 7, 6), (33,), 5, 2, 2, 32)]
BANDS = {"1": lambda h: 1, "2": lambda h: min(2, h), "short-last": lambda h: max(h - 1, 1), "full": lambda h: h}


def _pair(case, seed=0, **banded):
    """The same weights in both forms, on the GPU."""
    encs = []
    for kwargs in (dict(form="banded", **banded), {}):
        torch.manual_seed(seed)
        encs.append(ConvEncoder(*case, **kwargs).cuda())
    return encs


def _images(enc, n):
    return torch.randn(n, enc.image_size, generator=torch.Generator().manual_seed(n)).cuda()


@pytest.mark.gpu
@pytest.mark.parametrize("rows", list(BANDS))
@pytest.mark.parametrize("case", range(len(CASES)))
def test_banded_equals_the_tile_form_bit_for_bit(hip_backend, case, rows):
    height = ConvEncoder(*CASES[case], form="banded").plan.band_rows   # (whole images fit: the plan's band is the last layer's height)
    banded, tile = _pair(CASES[case], band_rows=BANDS[rows](height))
    T = banded.plan.tile_envs
    assert banded.plan.num_bands == -(-height // banded.plan.band_rows)
    for n in sorted({1, T - 1, T + 1, 33}):   # (33: one row in the head's second block)
        image = _images(banded, n)
        assert torch.equal(banded.encode(image), tile.encode(image)), n


@pytest.mark.gpu
def test_a_forced_tile_straddles_a_row_block(hip_backend):
    banded, tile = _pair(CASES[1], band_rows=2, tile_envs=5)   # 5 envs x 2 rows x 4 columns = 40 rows of the last layer's GEMM
    assert banded.plan.tile_envs == 5 and banded.plan.num_bands == 3
    for n in (1, 4, 6, 33):
        image = _images(banded, n)
        assert torch.equal(banded.encode(image), tile.encode(image)), n


@pytest.mark.gpu
@pytest.mark.parametrize("flat,latent", [(300, 5), (301, 130), (516, 512)])
def test_the_head_walks_its_slabs(hip_backend, flat, latent):
    """A 1 x 1 conv on a flat image: `flat` is one or two slabs of 256 plus a tail that is no multiple of the chunk; 16-byte rows (300,
    516) and rows read by element (301); one, two and four column blocks per wave."""
    banded, tile = _pair(((1, 1, flat), (1,), 1, 1, 0, latent), seed=5)
    assert banded.plan.flat == flat
    image = _images(banded, 33)
    assert torch.equal(banded.encode(image), tile.encode(image))


@pytest.mark.gpu
def test_the_depth_camera_is_as_accurate_as_torch_float32(hip_backend):
    """test_conv_encoder's rule on a shape only this form serves: 4 x torch's own float32 error plus 4 ulps of the output's scale."""
    torch.manual_seed(1)
    enc = ConvEncoder(**DEPTH, form="banded")
    image = torch.randn(3, enc.image_size, generator=torch.Generator().manual_seed(2))
    want = _ref(enc, image)
    torch_err = float((enc(image).detach().double() - want).abs().max())
    err = float((enc.cuda().encode(image.cuda()).cpu().double() - want).abs().max())
    floor = 4 * U * float(want.abs().max())
    print(f"conv_encode_banded accuracy {enc.plan}: kernel {err:.3e} torch {torch_err:.3e} ratio {err / max(torch_err, 1e-30):.2f} floor {floor:.3e}")
    assert err <= 4 * torch_err + floor


@pytest.mark.gpu
@pytest.mark.parametrize("w1", [0, 45])
def test_the_row_is_the_tile_forms(hip_backend, w1):
    banded, tile = _pair(CASES[3], seed=3, band_rows=2, tile_envs=3)
    n = 7
    obs = torch.randn(n, max(w1, 1), generator=torch.Generator().manual_seed(4)).cuda() if w1 else None
    normalizer = None
    if w1:
        normalizer = EmpiricalNormalization(w1).cuda()
        normalizer._mean.copy_(torch.randn(1, w1))
        normalizer._std.copy_(torch.rand(1, w1) + 0.1)
    image = _images(banded, n)
    got, want = banded.encode(image, obs, normalizer), tile.encode(image, obs, normalizer)
    assert got.shape == (n, w1 + banded.latent_dim)
    assert torch.equal(got[:, :w1], want[:, :w1]) and torch.equal(got, want)


@pytest.mark.gpu
def test_the_runner_collects_and_updates_with_a_banded_encoder(hip_backend):
    """student_encoder.form = "banded" through DistillationRunner: one iteration collects and updates, and from the same seed, noise and
    weights as form = "tile" it stores the same actions.  (The update is torch's conv backward, whose sums are not ordered.)"""
    from test_distillation import _built, _cfg, _runner

    runs = []
    for form in ("banded", "tile"):
        cfg = _cfg()
        cfg["policy"]["student_encoder"] = dict(image_shape=(1, 6, 8), channels=(4, 8), kernel_size=3, stride=1, padding=1, latent_dim=16, form=form,
                                                **({"band_rows": 4} if form == "banded" else {}))
        r = _runner(_built(), "cuda", noise_seed=11, cfg=cfg)
        assert r.alg.policy.student_encoder.form == form
        r.alg.policy.loaded_teacher = True   # (the randomly initialised teacher will do)
        w0 = r.alg.policy.student_encoder.conv[0].weight.detach().clone()
        r.learn(1)
        assert not torch.equal(r.alg.policy.student_encoder.conv[0].weight, w0)
        runs.append(r.storage.actions.clone())
    assert float(runs[0].abs().max()) > 0.0 and torch.equal(runs[0], runs[1])


# ---- without a GPU -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kwargs", [DEPTH, dict(image_shape=(1, 64, 64), channels=(16, 32), kernel_size=3, stride=2),
                                    dict(image_shape=(1, 5, 1613), channels=(1,), kernel_size=1, stride=1)])   # (the tile plan's first refusal)
def test_cameras_the_tile_form_refuses_plan_banded(kwargs):
    enc = ConvEncoder(**kwargs, form="banded")
    height = enc.conv(torch.zeros(1, *enc.image_shape)).shape[2]
    plan = enc.plan
    assert plan.lds_bytes <= nat.GF_CONV_LDS_BYTES and 1 <= plan.tile_envs <= nat.GF_CONV_MAX_TILE_ENVS
    assert plan.num_bands * plan.band_rows >= height > (plan.num_bands - 1) * plan.band_rows and plan.flat == enc.head.in_features
    with pytest.raises(ValueError, match="image_shape"):
        ConvEncoder(**kwargs, form="tile")


def test_the_refusals_name_their_argument():
    with pytest.raises(ValueError, match="image_shape"):   # a one-row band: 3 x 4 096 image floats and 64 x 4 096 outputs
        ConvEncoder((1, 8, 4096), (64,), 3, 1, 1, form="banded")
    for forced in (dict(band_rows=8), dict(band_rows=14), dict(band_rows=-1), dict(tile_envs=33)):
        with pytest.raises(ValueError, match=next(iter(forced))):   # 7 rows is the tallest band of the depth camera that fits, 13 its height
            ConvEncoder(**DEPTH, form="banded", **forced)
    assert ConvEncoder(**DEPTH, form="banded", band_rows=3, tile_envs=2).plan[3:] == (3, 5)
    with pytest.raises(ValueError, match="form"):
        ConvEncoder((1, 8, 8), form="rows")
    with pytest.raises(ValueError, match="band_rows"):
        ConvEncoder((1, 8, 8), band_rows=2)
