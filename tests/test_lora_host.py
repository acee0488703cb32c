"""CPU: LoRA by merged weights (gcd_amd/lora.py) and its library (libgcd_amd_lora.so; gcd_amd.csrc.build.LIBRARIES,
gcd_amd/_lib_lora.py).  The layer selection is the reference's: tests/golden/lora_layers.json was written by
tools/make_golden_lora.py from the reference's own VideoUNet.  The library's limits fit the adapted layers, its table entry
mirrors every member of the C struct, and it refuses bad arguments (the rules every library is held to, the entry's layout
under gcc among them, are tests/test_libraries_host.py's)."""
import ctypes
import json
import re
from pathlib import Path

import pytest
import torch

from gcd_amd import _lib_lora, lora as L
from gcd_amd._lib import GcdError
from gcd_amd.csrc import build as b
from oracle import svd_unet_ref as O

ROOT = Path(__file__).resolve().parent.parent
GOLD = json.loads((Path(__file__).resolve().parent / "golden" / "lora_layers.json").read_text())
CONFIGS = {"TINY": O.TINY, "KUBRIC": O.KUBRIC}


def _meta(cfg):
    from gcd_amd.video_model import VideoUNet
    with torch.device("meta"):
        return VideoUNet(**cfg.as_reference_kwargs())


def _tiny_cpu(salt=3):
    from gcd_amd.video_model import VideoUNet
    from oracle import weights
    net = _meta(O.TINY)
    sd = weights.synth_state_dict({k: tuple(v.shape) for k, v in net.state_dict().items()}, salt)
    net = VideoUNet(**O.TINY.as_reference_kwargs())
    net.load_state_dict(sd)
    return net


# ------------------------------------------------------------------------------------------------------- the selection
@pytest.mark.parametrize("label", list(CONFIGS))
def test_time_lora_selects_the_reference_layers(label):
    gold = GOLD[label]
    net = _meta(CONFIGS[label])
    got = [[n, m.out_features, m.in_features] for n, m in L.adaptable_layers(net)]
    assert got == gold["time_lora"] and len(got) == 248
    assert sum(N * K for _, N, K in got) == gold["adapted_parameters"]
    assert sum(p.numel() for p in net.parameters()) == gold["parameters"]
    before = list(net.state_dict())
    lora = L.apply_ft_strategy(net, "time_lora")
    assert isinstance(lora, L.TimeLora) and lora.names == [n for n, _, _ in got] and (lora.r, lora.scale) == (16, 1.0 / 16)
    # the network keeps its modules, names and parameters; the adapters are the other module's
    assert list(net.state_dict()) == before and not any(m is lora for m in net.modules())
    assert all(m is not net for m in lora.modules()) and len(list(lora.parameters())) == 2 * 248
    assert sum(p.numel() for p in lora.parameters()) == sum(16 * (N + K) for _, N, K in got)
    trainable = [n for n, p in net.named_parameters() if p.requires_grad]
    assert set(trainable) == {n + ".weight" for n in lora.names} and len(trainable) == 248
    for a, bb, (_, N, K) in zip(lora.lora_A, lora.lora_B, got):
        assert tuple(a.shape) == (16, K) and tuple(bb.shape) == (N, 16) and a.requires_grad and bb.requires_grad
    if label == "KUBRIC":
        assert (gold["adapted_parameters"], gold["parameters"]) == (524247040, 1526427882)
        assert sum(p.numel() for p in lora.parameters()) == 11747328


@pytest.mark.parametrize("label", list(CONFIGS))
def test_time_dummy_and_everything_follow_the_reference_rules(label):
    gold = GOLD[label]
    net = _meta(CONFIGS[label])
    assert L.apply_ft_strategy(net, "everything") is None and all(p.requires_grad for p in net.parameters())
    assert L.apply_ft_strategy(net, "time") is None
    flags = {n: p.requires_grad for n, p in net.named_parameters()}
    assert len(flags) == gold["time"]["tensors"] and sum(flags.values()) == gold["time"]["trainable"] == 742
    assert all(v == ("time" in n) for n, v in flags.items())
    net = _meta(CONFIGS[label])
    assert L.apply_ft_strategy(net, "dummy") is None
    assert [n for n, p in net.named_parameters() if p.requires_grad] == gold["dummy"] == [L.DUMMY_PARAM]
    with pytest.raises(NotImplementedError):
        L.apply_ft_strategy(net, "lora")
    with pytest.raises(TypeError):
        L.apply_ft_strategy(net, "time", r=4)


def test_attach_initialises_like_peft_and_drops_a_cached_plan():
    net = _tiny_cpu()
    object.__setattr__(net, "_gcd_train_plan", object())
    net.out[2].bias.requires_grad_(False)
    before = {k: v.clone() for k, v in net.state_dict().items()}
    lora = L.TimeLora(net, generator=torch.Generator().manual_seed(4))
    assert "_gcd_train_plan" not in net.__dict__
    again = L.TimeLora(_tiny_cpu(), generator=torch.Generator().manual_seed(4))
    for a, a2, bb, m in zip(lora.lora_A, again.lora_A, lora.lora_B, lora._layers):
        K = m.in_features
        a, bb = a.detach(), bb.detach()
        assert torch.equal(a, a2) and float(a.abs().max()) <= K ** -0.5 and not bool(bb.any())
        assert float(a.abs().max()) > 0.8 * K ** -0.5 and abs(float(a.mean())) < 0.1 * K ** -0.5      # U(-1/sqrt K, 1/sqrt K)
    # B == 0: the weights are untouched bit for bit, W0 is a copy (not a view) of them
    for k, v in net.state_dict().items():
        assert torch.equal(v.view(torch.int32) if v.dtype == torch.float32 else v, before[k].view(torch.int32)
                           if v.dtype == torch.float32 else before[k]), k
    for w, w0 in zip(lora.weights(), lora.w0()):
        assert torch.equal(w, w0) and w.data_ptr() != w0.data_ptr()
    assert not any(k.startswith("w0_") for k in lora.state_dict()) and len(lora.state_dict()) == 2 * 248
    # without a GPU there is no kernel and no stand-in for one
    with pytest.raises(GcdError):
        lora.merge()
    with pytest.raises(GcdError):
        lora.project_grads()
    with pytest.raises(GcdError):
        lora.attach()
    with pytest.raises(ValueError):
        L.TimeLora(_meta(O.TINY), r=_lib_lora.LORA_MAX_RANK + 1)
    # unmerge: W0 back, the flags as they were (one had been frozen by the user)
    lora.weights()[0].data.add_(1.0)
    object.__setattr__(net, "_gcd_train_plan", object())
    lora.unmerge()
    assert "_gcd_train_plan" not in net.__dict__ and not lora.attached
    assert all(torch.equal(v, before[k]) for k, v in net.state_dict().items())
    assert [n for n, p in net.named_parameters() if not p.requires_grad] == ["out.2.bias"]
    with pytest.raises(GcdError):
        lora.unmerge()


def test_reference_state_dict_names_round_trip():
    net = _tiny_cpu(salt=5)
    lora = L.TimeLora(net, generator=torch.Generator().manual_seed(8))
    plain = net.state_dict()
    sd = lora.reference_state_dict()
    adapted = set(lora.names)
    assert len(sd) == len(plain) + 2 * 248
    for n in lora.names:
        assert {f"{n}.base_layer.weight", f"{n}.lora_A.default.weight", f"{n}.lora_B.default.weight"} <= set(sd)
        assert (f"{n}.base_layer.bias" in sd) == (f"{n}.bias" in plain) and f"{n}.weight" not in sd and f"{n}.bias" not in sd
    assert {k for k in sd if ".base_layer." not in k and ".lora_" not in k} == \
        {k for k in plain if k.rpartition(".")[0] not in adapted}
    # a checkpoint with other values, loaded into a second network: every tensor arrives under its own name
    g = torch.Generator().manual_seed(9)
    other = {k: torch.randn(v.shape, generator=g) for k, v in sd.items()}
    net2 = _tiny_cpu(salt=6)
    lora2 = L.TimeLora(net2)
    flags = {n: p.requires_grad for n, p in net2.named_parameters()}
    lora2.load_reference_state_dict(other, merge=False)
    back = lora2.reference_state_dict()
    assert list(back) == list(sd) and all(torch.equal(back[k], other[k]) for k in sd)
    assert {n: p.requires_grad for n, p in net2.named_parameters()} == flags
    for n, w, w0 in zip(lora2.names, lora2.weights(), lora2.w0()):
        assert torch.equal(w0, other[f"{n}.base_layer.weight"]) and torch.equal(w, w0)      # unmerged: merge() is the device's
    with pytest.raises(GcdError):
        lora2.load_reference_state_dict(other)                       # merge=True needs the GPU
    with pytest.raises(KeyError):
        lora2.load_reference_state_dict({k: v for k, v in other.items() if not k.endswith("lora_B.default.weight")}, merge=False)
    with pytest.raises(KeyError):
        lora2.load_reference_state_dict(dict(plain), merge=False)


# ----------------------------------------------------------------------------------------------------------- the library
def test_limits_fit_the_adapted_layers():
    assert _lib_lora.LORA_MAX_RANK == 64 and _lib_lora.LORA_MAX_ENTRIES >= 248
    assert _lib_lora.LORA_MAX_DIM >= max(max(N, K) for _, N, K in GOLD["KUBRIC"]["time_lora"])


def test_entry_mirrors_every_member_of_the_struct():
    """(Offsets and size against gcc: tests/test_libraries_host.py test_struct_layout_matches_header[LoraEntry].)"""
    cls = _lib_lora.LoraEntry
    fields = [f[0] for f in cls._fields_]
    assert ctypes.sizeof(cls) == 88
    # every member of the C struct is mirrored (names between the braces of the typedef)
    body = re.search(r"typedef struct \{(.*?)\} gcd_lora_entry;", (ROOT / "include" / "gcd_amd_lora.h").read_text(), flags=re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    members = [n for decl in body.split(";") if decl.strip() for n in re.findall(r"(\w+)\s*(?:,|$)", decl.strip())]
    assert members == fields, (members, fields)


def test_bad_arguments_return_a_status_and_a_message():
    """Every host argument is checked before anything is launched (no device is needed to be refused)."""
    b.build(verbose=False)
    lib = _lib_lora.load()
    one = ctypes.c_void_p(16)                   # never dereferenced: every call below fails its checks first
    bad = [lambda: lib.gcd_lora_merge(None, 1, 1, None),
           lambda: lib.gcd_lora_merge(one, 0, 1, None),
           lambda: lib.gcd_lora_merge(one, _lib_lora.LORA_MAX_ENTRIES + 1, 1 << 20, None),
           lambda: lib.gcd_lora_merge(one, 3, 2, None),                                        # fewer tiles than entries
           lambda: lib.gcd_lora_project(None, 1, 1, 16, one, 64, None),
           lambda: lib.gcd_lora_project(one, 0, 1, 16, one, 64, None),
           lambda: lib.gcd_lora_project(one, 2, 1, 16, one, 64, None),
           lambda: lib.gcd_lora_project(one, 1, 1, 0, one, 64, None),                          # max_rank
           lambda: lib.gcd_lora_project(one, 1, 1, _lib_lora.LORA_MAX_RANK + 1, one, 64, None),
           lambda: lib.gcd_lora_project(one, 1, 1, 16, None, 64, None),                        # no scratch
           lambda: lib.gcd_lora_project(one, 1, 1, 16, one, 3, None),                          # less than any entry needs
           lambda: lib.gcd_lora_project(one, 1, 1, 16, ctypes.c_void_p(18), 64, None)]         # misaligned scratch
    for k, call in enumerate(bad):
        assert call() == 2, k
        assert lib.gcd_lora_last_error().decode().startswith("gcd_lora_"), k
        with pytest.raises(GcdError):
            _lib_lora.check(2, "gcd_lora")
    for N, K, r in ((0, 4, 4), (4, 0, 4), (4, 4, 0), (4, 4, _lib_lora.LORA_MAX_RANK + 1), (_lib_lora.LORA_MAX_DIM + 1, 4, 4)):
        assert lib.gcd_lora_project_scratch_floats(N, K, r) == -1
        assert lib.gcd_lora_last_error().decode().startswith("gcd_lora_project_scratch_floats")
    pt = _lib_lora.LORA_PROJECT_TILE
    for N, K, r in ((1, 1, 1), (300, 700, 16), (10240, 1280, 16), (64, 2048, 64)):
        want = -(-K // pt) * N * r + -(-N // pt) * r * K
        assert lib.gcd_lora_project_scratch_floats(N, K, r) == (want + 3) // 4 * 4
    # the running sums of a table
    arr = (_lib_lora.LoraEntry * 3)()
    for e, (N, K, r) in zip(arr, ((300, 700, 16), (1, 1, 1), (64, 2048, 64))):
        e.N, e.K, e.r = N, K, r
    mt, ptiles, sf = _lib_lora.fill_table(arr)
    assert [e.merge_tile0 for e in arr] == [0, 55, 56] and mt == 56 + 32
    assert [e.project_tile0 for e in arr] == [0, 6, 7] and ptiles == 7 + 8
    assert [e.scratch0 for e in arr] == [0, lib.gcd_lora_project_scratch_floats(300, 700, 16),
                                         lib.gcd_lora_project_scratch_floats(300, 700, 16) + 4] and sf > arr[2].scratch0
    arr[1].r = 0
    with pytest.raises(GcdError):
        _lib_lora.fill_table(arr)
