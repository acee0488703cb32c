"""CPU: the LPIPS drop-in (gcd_amd/lpips.py) and its library (libgcd_amd_lpips.so; gcd_amd.csrc.build.LIBRARIES,
gcd_amd/_lib_lpips.py).  The oracle of the GPU tests (tests/lpips_util.py) is pinned to the executed reference recorded
in tests/golden/lpips_tiny.pt; the module has the reference's 33 names and loads the way the reference does; operands
that the HIP path cannot take raise GcdError; and the library's limits fit the tower (the rules every library is held to
are tests/test_libraries_host.py's)."""
import pytest
import torch

import lpips_util as U
from gcd_amd import _lib_lpips
from gcd_amd._lib import GcdError
from gcd_amd.lpips import LPIPS

CASES = ("tiny_40x56", "tiny_37x51", "full_64x96")


# ------------------------------------------------------------------------------------------------------------ the oracle
@pytest.mark.parametrize("name", CASES)
def test_restatement_equals_the_recorded_reference(name):
    rec, sd, x0, x1 = U.golden_case(name)
    y64 = U.lpips_oracle(sd, x0, x1, torch.float64)
    assert y64.shape == rec["y64"].shape == (rec["n"], 1, 1, 1)
    assert float((y64 - rec["y64"]).abs().max()) <= 1e-12
    y32 = U.lpips_oracle(sd, x0, x1, torch.float32)
    live = rec["y64"].reshape(-1) != 0
    gap = ((y32.double() - rec["y64"]).abs().reshape(-1)[live] / rec["y64"].abs().reshape(-1)[live]).max()
    # the reference's own float32 run is rec["y32_gap"] away from its float64 run; a second float32 evaluation of the
    # same chain (other summation order in the convolutions) gets twice that, and never less than a few ulp
    assert float(gap) <= max(2.0 * rec["y32_gap"], 1e-6), (float(gap), rec["y32_gap"])
    assert float(y64.reshape(-1)[0]) == float(y32.reshape(-1)[0]) == 0.0 == float(rec["y16emu"].reshape(-1)[0])
    assert bool((rec["y64"].reshape(-1)[1:] > 0).all())


def test_fp16_emulation_of_the_oracle_tracks_the_recorded_one():
    """round16=True places the storage points where the generator's hooks on the reference did."""
    rec, sd, x0, x1 = U.golden_case("tiny_40x56")
    y = U.lpips_oracle(sd, x0, x1, torch.float64, round16=True)
    assert float((y - rec["y16emu"]).abs().max()) <= 0.25 * U.case_bar(rec) * float(rec["y64"].abs().max())


# ------------------------------------------------------------------------------------------------------------ the module
@pytest.mark.parametrize("name", CASES)
def test_state_dict_has_the_reference_names_and_shapes(name):
    rec = U.load_golden()["cases"][name]
    m = LPIPS(chns=tuple(rec["chns"]))
    got = [(k, list(v.shape)) for k, v in m.state_dict().items()]
    assert got == list(zip(rec["names"], rec["shapes"])) and len(got) == 33
    assert not [n for n, p in m.named_parameters() if p.requires_grad] and not m.training
    assert [n for n, _ in m.named_buffers()] == ["scaling_layer.shift", "scaling_layer.scale"]
    assert torch.equal(m.scaling_layer.shift.reshape(-1), torch.tensor(U.SHIFT))
    assert torch.equal(m.scaling_layer.scale.reshape(-1), torch.tensor(U.SCALE))


def test_default_widths_are_vgg16_and_dropout_decides_the_lin_index():
    assert LPIPS().chns == [64, 128, 256, 512, 512]
    assert "lin0.model.0.weight" in LPIPS(use_dropout=False, chns=U.TINY).state_dict()
    for bad in ((32, 32, 64, 64), (32, 32, 64, 64, 48), (32, 32, 64, 64, 1024)):
        with pytest.raises(GcdError):
            LPIPS(chns=bad)


def test_lin_only_checkpoint_loads_by_name_and_torchvision_mapping():
    sd = U.seeded_state_dict(U.TINY, 7)
    m = LPIPS(chns=U.TINY)
    before = {k: v.clone() for k, v in m.state_dict().items()}
    lin_only = {k: v for k, v in sd.items() if k.startswith("lin")}
    missing, unexpected = m.load_state_dict(lin_only, strict=False)
    assert not unexpected and set(missing) == set(sd) - set(lin_only)
    after = m.state_dict()
    for k in sd:
        assert torch.equal(after[k], sd[k] if k in lin_only else before[k]), k
    # torchvision's vgg16().state_dict(): features.{i}.* (and classifier.*, ignored)
    tv = {f"features.{k.split('.')[2]}.{k.split('.')[3]}": v for k, v in sd.items() if k.startswith("net.")}
    tv["classifier.0.weight"] = torch.zeros(4, 4)
    m.load_torchvision_vgg16(tv)
    after = m.state_dict()
    for k in sd:
        assert torch.equal(after[k], sd[k]), k
    del tv["features.28.bias"]
    with pytest.raises(GcdError):
        m.load_torchvision_vgg16(tv)
    assert not [n for n, p in m.named_parameters() if p.requires_grad]


def test_operands_the_hip_path_cannot_take_raise():
    m = LPIPS(chns=U.TINY)
    x = torch.zeros(1, 3, 16, 16)
    with pytest.raises(GcdError):
        m(x, x)                                     # CPU operands: there is no CPU path
    with pytest.raises(GcdError):
        m(x, x, value_range="bytes")
    with pytest.raises(GcdError):
        m(x.numpy(), x.numpy())
    from gcd_amd.validation import validation_metrics
    with pytest.raises(GcdError):
        validation_metrics(x, x, m)
    with pytest.raises(GcdError):
        validation_metrics(x, x, object())


def test_chunking_keeps_every_activation_inside_the_limits():
    from gcd_amd import lpips as L
    m = LPIPS()
    # 576 x 1024: the 64-channel tap of one image is 75.5 MB of fp16; 28 images (14 pairs) are 2.11 GB, 32 MiB short
    # of 2^31 bytes, and 15 pairs are past it
    per_pair = 2 * 576 * 1024 * 64 * 2
    assert m._image_bytes(576, 1024) * 2 == per_pair and 14 * per_pair < 2 ** 31 < 15 * per_pair
    n = m.pairs_per_chunk(576, 1024)
    assert 1 <= n < 14 and n * per_pair <= L.MAX_ACTIVATION_BYTES < 2 ** 31 and (n + 1) * per_pair > L.MAX_ACTIVATION_BYTES
    assert m.pairs_per_chunk(256, 384) >= 14
    with pytest.raises(GcdError):
        m.pairs_per_chunk(576, 1024, pairs_at_a_time=15)
    assert m.pairs_per_chunk(576, 1024, pairs_at_a_time=14) == 14
    with pytest.raises(GcdError):
        m.pairs_per_chunk(576, 1024, pairs_at_a_time=0)
    with pytest.raises(GcdError):
        m.pairs_per_chunk(4096, 4096)               # one pair alone is past a gcd_gemm_f16 operand
    # a wide late tap can be the largest activation of a test-sized tower
    assert LPIPS(chns=(32, 512, 512, 512, 512))._image_bytes(64, 64) == 32 * 32 * 512 * 2


def test_training_loss_type_lpips_keeps_raising():
    from gcd_amd import training
    with pytest.raises(NotImplementedError):
        training.StandardDiffusionLoss(sigma_sampler_config={}, loss_weighting_config={}, loss_type="lpips")


# ----------------------------------------------------------------------------------------------------------- the library
def test_limits_fit_the_vgg16_tower():
    assert _lib_lpips.LPIPS_MAX_C >= 512 and _lib_lpips.LPIPS_MAX_C % _lib_lpips.LPIPS_C_MULTIPLE == 0
