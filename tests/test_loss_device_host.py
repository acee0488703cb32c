"""CPU: the loss library (libgcd_amd_loss.so; gcd_amd.csrc.build.LIBRARIES, gcd_amd/_lib_loss.py) and the loss engine
switch of gcd_amd/training.py.  The library's limits fit what the fine-tune step gives it and it refuses bad arguments (the
rules every library is held to are tests/test_libraries_host.py's).  The switch takes two names, defaults to torch, and
under `hip` operands that are not on a GPU raise GcdError."""
import ctypes
from pathlib import Path

import pytest
import torch

from gcd_amd import _lib_loss
from gcd_amd._lib import GcdError
from gcd_amd.csrc import build as b

ROOT = Path(__file__).resolve().parent.parent
GOLD = Path(__file__).resolve().parent / "golden" / "loss_kat.pt"
CFG = dict(
    harmonize_sigmas=True, focus_top=0.1, focus_steps=5000,
    batch2model_keys=["image_only_indicator", "num_video_frames"],
    loss_weighting_config={"target": "gcd_amd.training.EDMWeighting", "params": {"sigma_data": 1.0}},
    sigma_sampler_config={"target": "gcd_amd.training.EDMSampling", "params": {"p_mean": 1.0, "p_std": 1.6}})


# ----------------------------------------------------------------------------------------------------------- the library
def test_limits_fit_the_fine_tune_step():
    assert _lib_loss.LOSS_MAX_N >= 4 * 128 * 128 and _lib_loss.LOSS_MAX_CLASSES == 16     # full-resolution latents fit
    from gcd_amd import training as TR
    assert len(TR.PD_PERSON_RGB) + len(TR.PD_VEHICLE_RGB) <= _lib_loss.LOSS_MAX_CLASSES


def test_bad_arguments_return_a_status_and_a_message():
    """Every argument is checked before anything is launched (no device is needed to be refused)."""
    b.build(verbose=False)
    lib = _lib_loss.load()
    one = ctypes.c_void_p(16)                   # never dereferenced: every call below fails its checks first
    tab = (ctypes.c_float * 4)()
    bad = [lambda: lib.gcd_loss_class_map(None, 1, 8, 8, tab, 1, one, 1, 1, None),
           lambda: lib.gcd_loss_class_map(one, 1, 8, 8, tab, _lib_loss.LOSS_MAX_CLASSES + 1, one, 1, 1, None),
           lambda: lib.gcd_loss_class_map(one, 1, 8, 8, tab, 1, one, 9, 1, None),           # a map taller than the frame
           lambda: lib.gcd_loss_class_map(one, 1, 8, 1024, tab, 1, one, 1, _lib_loss.LOSS_MAX_MAP_W + 1, None),
           lambda: lib.gcd_loss_class_map(one, _lib_loss.LOSS_MAX_BT + 1, 8, 8, tab, 1, one, 1, 1, None),
           lambda: lib.gcd_loss_focal_fwd(one, one, one, None, 1, 12, 6, 0, 13, one, one, None),            # keep > n
           lambda: lib.gcd_loss_focal_fwd(one, one, one, None, 1, 12, 5, 0, 1, one, one, None),             # HW does not divide n
           lambda: lib.gcd_loss_focal_fwd(one, one, one, None, 1, 12, 6, 2, 1, one, one, None),             # loss_type
           lambda: lib.gcd_loss_focal_fwd(one, one, one, None, 1, _lib_loss.LOSS_MAX_N + 1, 1, 0, 1, one, one, None),
           lambda: lib.gcd_loss_focal_fwd(one, one, one, None, 1, 12, 6, 0, 1, one, None, None),            # no state
           lambda: lib.gcd_loss_focal_bwd(one, one, one, None, one, one, 1, 12, 6, 0, -1, one, None),
           lambda: lib.gcd_loss_focal_bwd(one, one, one, None, one, one, 1, 12, 6, 0, 1, None, None),
           lambda: lib.gcd_loss_focal_bwd(one, one, one, None, one, one, 1, 12, 6, 0, 1, one, None)]        # dout aliases out
    for k, call in enumerate(bad):
        assert call() == 2, k
        assert lib.gcd_loss_last_error().decode().startswith("gcd_loss_"), k
        with pytest.raises(GcdError):
            _lib_loss.check(2, "gcd_loss")


# ------------------------------------------------------------------------------------------------------------ the switch
def test_loss_engine_switch_takes_two_names_and_defaults_to_torch():
    import os
    import subprocess
    import sys
    from gcd_amd import training as TR
    assert TR.LOSS_ENGINE == os.environ.get("GCD_TRAIN_LOSS", "torch")
    # the environment variable is read at import: one child process (the variable's value goes through set_loss_engine,
    # so a typo raises there as it does below)
    code = "from gcd_amd import training as TR; print(TR.LOSS_ENGINE)"
    run = subprocess.run([sys.executable, "-c", code], cwd=ROOT, env=dict(os.environ, GCD_TRAIN_LOSS="hip"), capture_output=True,
                         text=True)
    assert run.stdout.strip() == "hip", run.stderr
    old = TR.LOSS_ENGINE
    try:
        for name in ("hip", "torch"):
            TR.set_loss_engine(name)
            assert TR.LOSS_ENGINE == name
        for bad in ("HIP", "triton", "", None):
            with pytest.raises(ValueError):
                TR.set_loss_engine(bad)
        assert TR.LOSS_ENGINE == "torch"
    finally:
        TR.set_loss_engine(old)


def test_hip_engine_refuses_cpu_operands_and_torch_engine_is_untouched():
    from gcd_amd import loss_device, training as TR
    g = torch.load(GOLD)
    w = g["weights"][:, None, None, None]
    case = next(c for c in g["cases"] if c["step"] > 0 and c["loss_type"] == "l2")
    loss = TR.StandardDiffusionLoss(**CFG)
    old = TR.LOSS_ENGINE
    try:
        TR.set_loss_engine("hip")
        with pytest.raises(GcdError):
            loss.get_loss(g["out"], g["tgt"], w, {"global_step": case["step"]})
        with pytest.raises(GcdError):          # also without a focal selection (step 0: cur_top = 1)
            loss.get_loss(g["out"], g["tgt"], w, {"global_step": 0})
        pd = TR.StandardDiffusionLoss(**dict(CFG, pd_person_weight=7.0))
        with pytest.raises(GcdError):
            pd.get_loss(g["out"], g["tgt"], w, {"global_step": 1, "jpg": torch.zeros(g["out"].shape[0], 3, 8, 8)})
        with pytest.raises(NotImplementedError):
            TR.StandardDiffusionLoss(**dict(CFG, loss_type="lpips"))
        TR.set_loss_engine("torch")
        got = loss.get_loss(g["out"], g["tgt"], w, {"global_step": case["step"]})
        assert torch.allclose(got, case["loss"], rtol=1e-6, atol=0)
    finally:
        TR.set_loss_engine(old)
    x = torch.zeros(2, 4, 3, 5)
    with pytest.raises(GcdError):
        loss_device.focal_loss(x, x, torch.ones(2), 1)
    with pytest.raises(GcdError):
        loss_device.class_weight_map(torch.zeros(2, 3, 8, 8), (1, 1), [((0, 0, 142), 3.0)])
    with pytest.raises(GcdError):
        loss_device.class_table([((0, 0, 0), 2.0)] * (_lib_loss.LOSS_MAX_CLASSES + 1))
    tab = loss_device.class_table([((0, 0, 142), 3.0), ((220, 20, 60), 7.0)])
    assert tab.dtype == torch.float32 and tab.shape == (2, 4) and tab[:, 3].tolist() == [2.0, 6.0]
    assert torch.equal(tab[0, :3], torch.tensor((0, 0, 142), dtype=torch.float32) / 127.5 - 1.0)


def test_class_list_is_the_reference_order():
    from gcd_amd import training as TR
    from oracle import loss_ref as R
    both = TR.StandardDiffusionLoss(**dict(CFG, pd_person_weight=7.0, pd_vehicle_weight=3.0))._pd_classes()
    assert [list(rgb) for rgb, _ in both] == R.PD_PERSON + R.PD_VEHICLE
    assert [wt for _, wt in both] == [7.0] * len(R.PD_PERSON) + [3.0] * len(R.PD_VEHICLE)
    assert TR.StandardDiffusionLoss(**CFG)._pd_classes() == []
    assert [list(rgb) for rgb, _ in TR.StandardDiffusionLoss(**dict(CFG, pd_vehicle_weight=3.0))._pd_classes()] == R.PD_VEHICLE
