"""CPU: the device-resident optimizer step — the C-ABI surface of include/gcd_amd_train_optim.h (symbols, struct layouts,
argument validation: observable without a GPU), LitEma's buffer names, and AdamHIP's checkpoints in torch.optim.Adam's
format."""
import copy
import ctypes
import io
import re
from pathlib import Path

import pytest
import torch

ROOT = Path(__file__).resolve().parent.parent
_DECL = r"^\s*(?:int|int64_t|const char\*)\s+(gcd_\w+)\s*\("


def test_optim_header_signatures():
    from gcd_amd import _lib
    header = (ROOT / "include" / "gcd_amd_train_optim.h").read_text()
    declared = set(re.findall(_DECL, header, flags=re.M))
    assert declared == set(_lib.TRAIN_OPTIM_SIGNATURES), (declared ^ set(_lib.TRAIN_OPTIM_SIGNATURES))
    assert len(declared) == 5
    # exported, bound and apart from every other table: tests/test_libraries_host.py
    from gcd_amd.csrc import build
    train = build.LIBRARIES["gcd_amd_train"]
    assert "train_optim.hip" in train.sources and "train_optim.hip" not in build.SOURCES
    assert ROOT / "include" / "gcd_amd_train_optim.h" in train.headers
    assert f"#define GCD_OPTIM_CHUNK {_lib.OPTIM_CHUNK}" in header


def test_optim_state_block_is_64_bytes_of_4_byte_fields():
    """(The layouts of the three structs against gcc's: tests/test_libraries_host.py.)"""
    from gcd_amd import _lib
    cls = _lib.OptimState
    assert ctypes.sizeof(cls) == 64
    assert all(ctypes.sizeof(t) % 4 == 0 and (ctypes.sizeof(t) == 4 or n == "reserved") for n, t in cls._fields_)


def _cfg(**kw):
    from gcd_amd import _lib
    c = _lib.OptimConfig()
    c.beta1, c.beta2, c.eps, c.weight_decay, c.grad_scale = 0.9, 0.999, 1e-8, 0.0, 1.0
    c.growth_factor, c.backoff_factor, c.growth_interval, c.ema_decay = 2.0, 0.5, 2000, 0.9999
    for k, v in kw.items():
        setattr(c, k, v)
    return c


def test_entries_refuse_bad_arguments_without_a_gpu():
    """Argument validation happens before any launch.  Pointers are fake (16 = aligned, non-null): nothing is launched."""
    from gcd_amd import _lib
    lib = _lib.load_train()
    P, BIG = 16, 1 << 29

    def refused(rc, *words):
        assert rc != 0
        msg = lib.gcd_train_last_error()
        for w in words:
            assert w in msg, (w, msg)

    ok = ctypes.byref(_cfg())
    assert lib.gcd_optim_gradstat_scratch_floats(7) == 7
    assert lib.gcd_optim_gradstat_scratch_floats(0) == 0
    refused(lib.gcd_optim_gradstat(P, 3, 7, ok, P, P, 6, None), b"scratch", b"gcd_optim_gradstat_scratch_floats")
    refused(lib.gcd_optim_gradstat(P, 3, 7, ok, P, 20, BIG, None), b"16-byte aligned")
    refused(lib.gcd_optim_gradstat(P, 0, 7, ok, P, P, BIG, None), b"empty table")
    refused(lib.gcd_optim_gradstat(P, 3, 2, ok, P, P, BIG, None), b"total_chunks")
    refused(lib.gcd_optim_gradstat(None, 3, 7, ok, P, P, BIG, None), b"null")
    refused(lib.gcd_optim_apply(P, 3, 7, ok, 20, None), b"16-byte aligned")
    refused(lib.gcd_optim_apply(P, 3, 7, None, P, None), b"null")
    refused(lib.gcd_optim_apply(P, 3, 7, ctypes.byref(_cfg(beta1=1.0)), P, None), b"betas")
    refused(lib.gcd_optim_apply(P, 3, 7, ctypes.byref(_cfg(weight_decay=-0.1)), P, None), b"weight_decay")
    refused(lib.gcd_optim_apply(P, 3, 7, ctypes.byref(_cfg(grad_scale=0.0)), P, None), b"grad_scale")
    refused(lib.gcd_optim_advance(ctypes.byref(_cfg(dynamic_scale=1, growth_interval=0)), P, None), b"growth_interval")
    refused(lib.gcd_optim_advance(ok, None, None), b"null")
    refused(lib.gcd_ema_update(P, 3, 7, ok, P, None), b"use_ema")
    refused(lib.gcd_ema_update(P, 3, 7, ctypes.byref(_cfg(use_ema=1, ema_decay=1.5)), P, None), b"ema_decay")


def test_new_source_holds_no_read_modify_write_reduction():
    src = (ROOT / "gcd_amd" / "csrc" / "train_optim.hip").read_text()
    assert "atomic" not in src.lower()
    assert "ordered fold" in src


def test_adamhip_keyword_validation_and_default_mode():
    from gcd_amd.training import AdamHIP
    p = [torch.nn.Parameter(torch.zeros(3))]
    assert AdamHIP(p).device_state is False                          # nothing given: the gcd_adam_step_multi path
    assert AdamHIP(p, device_state=True).device_state is True
    for kw in (dict(decoupled_weight_decay=True), dict(max_grad_norm=1.0), dict(loss_scale=128.0),
               dict(loss_scale="dynamic")):
        assert AdamHIP(p, **kw).device_state is True
    for bad in (dict(max_grad_norm=0.0), dict(max_grad_norm=-1.0), dict(loss_scale="static"), dict(loss_scale=0.0),
                dict(loss_scale="dynamic", growth_factor=1.0), dict(loss_scale="dynamic", backoff_factor=1.0),
                dict(loss_scale="dynamic", growth_interval=0), dict(ema=object()),
                dict(max_grad_norm=1.0, device_state=False)):
        with pytest.raises(ValueError):
            AdamHIP(p, **bad)
    opt = AdamHIP(p, loss_scale="dynamic", init_scale=1024.0, growth_interval=7)
    st = opt.stats()
    assert st["loss_scale"] == 1024.0 and st["step"] == 0 and st["skipped_steps"] == 0
    opt.set_lr(3e-4)
    assert abs(opt.stats()["lr"] - 3e-4) < 1e-10
    assert float(opt.scale(torch.tensor(2.0))) == 2048.0
    from gcd_amd import _lib
    with pytest.raises(_lib.GcdError, match="no CPU fallback"):
        p[0].grad = torch.zeros(3)
        opt.step()


def _tiny_unet():
    from gcd_amd.video_model import VideoUNet
    from oracle import svd_unet_ref as O
    torch.manual_seed(0)
    return VideoUNet(**O.TINY.as_reference_kwargs())


def test_litema_buffer_names_and_state_dict_keys():
    from gcd_amd.ema import LitEma
    net = _tiny_unet()
    frozen = next(iter(net.parameters()))
    frozen.requires_grad_(False)
    ema = LitEma(net, decay=0.999)
    names = {n for n, p in net.named_parameters() if p.requires_grad}
    want = {n.replace(".", "") for n in names} | {"decay", "num_updates"}
    assert set(ema.state_dict().keys()) == want
    assert {n for n, _ in ema.named_buffers()} == want
    assert ema.m_name2s_name == {n: n.replace(".", "") for n in names}
    assert ema.num_updates.dtype == torch.int32 and int(ema.num_updates) == 0 and ema.decay.dtype == torch.float32
    assert int(LitEma(net, use_num_upates=False).num_updates) == -1
    with pytest.raises(ValueError):
        LitEma(net, decay=1.5)
    # keys prefixed the way DiffusionEngine registers the module (model_ema.*) load unchanged
    ck = {"model_ema." + k: torch.full_like(v, 3) for k, v in ema.state_dict().items()}
    holder = torch.nn.Module()
    holder.model_ema = LitEma(net)
    holder.load_state_dict(ck)
    assert int(holder.model_ema.num_updates) == 3
    # identity matching; parameters outside the module have no shadow
    some = [p for p in net.parameters() if p.requires_grad][5]
    assert ema.shadow_of(some) is ema._buffers[[s for n, s in ema.m_name2s_name.items()
                                               if dict(net.named_parameters())[n] is some][0]]
    assert ema.shadow_of(torch.nn.Parameter(torch.zeros(1))) is None and ema.shadow_of(frozen) is None
    ema.reset_num_updates()
    assert int(ema.num_updates) == 0
    # store / copy_to / restore: the reference's semantics on the CPU
    from gcd_amd.ema import ema_scope
    before = some.detach().clone()
    with torch.no_grad():
        ema.shadow_of(some).add_(1.0)
    with ema_scope(net, ema):
        assert torch.equal(some.detach(), before + 1.0)
    assert torch.equal(some.detach(), before)


@pytest.mark.parametrize("device_state", [False, True])
def test_adamhip_state_dict_round_trips_and_loads_into_torch_adam(device_state):
    from gcd_amd import _lib
    from gcd_amd.training import AdamHIP
    g = torch.Generator().manual_seed(4)
    ps = [torch.nn.Parameter(torch.randn(s, generator=g)) for s in [(5, 3), (7,), (2, 2, 2)]]
    kw = dict(loss_scale="dynamic", max_grad_norm=1.0) if device_state else {}
    opt = AdamHIP(ps, lr=1e-3, betas=(0.8, 0.99), eps=1e-7, weight_decay=0.01, **kw)
    # a state as three steps would have left it (the step itself needs a GPU)
    for p, (m, v) in zip(ps, opt.state):
        m.copy_(torch.randn(m.shape, generator=g))
        v.copy_(torch.rand(v.shape, generator=g))
        opt._touched[id(p)] = True
    ref = torch.optim.Adam(ps, lr=1e-3, betas=(0.8, 0.99), eps=1e-7, weight_decay=0.01)
    for p in ps:
        p.grad = torch.zeros_like(p)
    for _ in range(3):
        ref.step()
    opt.load_state_dict({"state": {i: dict(step=torch.tensor(3.0), exp_avg=m, exp_avg_sq=v)
                                   for i, (m, v) in enumerate(opt.state)},
                         "param_groups": ref.state_dict()["param_groups"]})
    assert opt.stats()["step"] == 3
    buf = io.BytesIO()
    torch.save(opt.state_dict(), buf)
    buf.seek(0)
    sd = torch.load(buf)
    assert set(sd["state"][0]) == {"step", "exp_avg", "exp_avg_sq"} and float(sd["state"][0]["step"]) == 3.0
    assert (AdamHIP.SCALER_KEY in sd) == device_state
    if device_state:
        assert set(torch.amp.GradScaler("cpu").state_dict()) <= set(sd[AdamHIP.SCALER_KEY])
    for cls in (torch.optim.Adam, torch.optim.AdamW):
        t = cls(ps, lr=0.5)
        t.load_state_dict(copy.deepcopy(sd))      # (torch keeps the loaded tensors: its step would write into `sd`)
        assert t.param_groups[0]["lr"] == 1e-3 and t.param_groups[0]["betas"] == (0.8, 0.99)
        for i, (m, v) in enumerate(opt.state):
            assert torch.equal(t.state[ps[i]]["exp_avg"], m) and torch.equal(t.state[ps[i]]["exp_avg_sq"], v)
            assert float(t.state[ps[i]]["step"]) == 3.0
        t.step()                                 # torch continues from it
        assert float(t.state[ps[0]]["step"]) == 4.0
    # and back: a fresh optimizer takes torch's state
    opt2 = AdamHIP(ps, **kw)
    opt2.load_state_dict(sd)
    assert opt2.stats()["step"] == 3 and opt2.lr == 1e-3 and opt2.betas == (0.8, 0.99) and opt2._tables is None
    for (m, v), (m2, v2) in zip(opt.state, opt2.state):
        assert torch.equal(m, m2) and torch.equal(v, v2) and m.data_ptr() != m2.data_ptr()
    # per-parameter step counts that differ are refused
    sd["state"][1]["step"] = torch.tensor(5.0)
    with pytest.raises(_lib.GcdError, match="step counts differ"):
        opt2.load_state_dict(sd)
    with pytest.raises(_lib.GcdError, match="parameters"):
        AdamHIP(ps[:2], **kw).load_state_dict(opt.state_dict())
