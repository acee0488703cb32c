"""CPU: clips of 17..64 frames — the C-ABI surface of the two long-clip temporal-attention entries (argument refusal
without a GPU: they are only ever called here with invalid arguments), their code objects (no spills), and the CPU
oracle against the reference's own VideoUNet at T = 25."""
import re
from pathlib import Path

import pytest
import torch

from conftest import rel_l2

ROOT = Path(__file__).resolve().parent.parent
LONG = ("gcd_attn_temporal_long_f16", "gcd_attn_temporal_long_bwd")


def test_long_clip_entries_declared_and_exported():
    from gcd_amd import _lib
    header = (ROOT / "include" / "gcd_amd.h").read_text()
    declared = set(re.findall(r"^\s*(?:int|int64_t|const char\*)\s+(gcd_\w+)\s*\(", header, flags=re.M))
    lib = _lib.load()
    for name in LONG:
        assert name in declared and name in _lib.SIGNATURES, name
        assert hasattr(lib, name), name
    # the same argument lists as the T <= 16 entries
    assert _lib.SIGNATURES["gcd_attn_temporal_long_f16"] == _lib.SIGNATURES["gcd_attn_temporal_f16"]
    assert _lib.SIGNATURES["gcd_attn_temporal_long_bwd"] == _lib.SIGNATURES["gcd_attn_temporal_bwd"]
    assert lib.gcd_abi_version() == 9


@pytest.mark.parametrize("T", [0, 65, -1, 1000])
def test_long_clip_forward_refuses_frame_counts(T):
    from gcd_amd import _lib
    lib = _lib.load()
    assert lib.gcd_attn_temporal_long_f16(16, 192, 16, 64, 1, T, 4, 1, None) != 0
    assert f"T={T} ".encode() in lib.gcd_last_error() and b"1..64" in lib.gcd_last_error()


@pytest.mark.parametrize("T", [0, 65])
def test_long_clip_backward_refuses_frame_counts(T):
    from gcd_amd import _lib
    lib = _lib.load()
    assert lib.gcd_attn_temporal_long_bwd(16, 192, 16, 64, 16, 192, 1, T, 4, 1, None) != 0
    assert f"T={T} ".encode() in lib.gcd_last_error() and b"1..64" in lib.gcd_last_error()


def test_long_clip_entries_refuse_bad_strides():
    from gcd_amd import _lib
    lib = _lib.load()
    # forward: ld not a multiple of 8, ld < 3C, ldo < C, misaligned q|k|v
    for args in [(16, 196, 16, 64), (16, 184, 16, 64), (16, 192, 16, 56), (18, 192, 16, 64)]:
        assert lib.gcd_attn_temporal_long_f16(*args, 1, 25, 4, 1, None) != 0, args
        assert b"ld=" in lib.gcd_last_error()
    # backward: ld, lddo (fp32 rows of 16-byte pieces), lddq < 3C, misaligned dO
    for args in [(16, 100, 16, 64, 16, 192), (16, 192, 16, 62, 16, 192), (16, 192, 16, 64, 16, 191),
                 (16, 192, 20, 64, 16, 192)]:
        assert lib.gcd_attn_temporal_long_bwd(*args, 1, 25, 4, 1, None) != 0, args
        assert b"ld=" in lib.gcd_last_error()
    assert lib.gcd_attn_temporal_long_f16(None, 192, 16, 64, 1, 25, 4, 1, None) != 0
    assert b"null pointer" in lib.gcd_last_error()
    # the T <= 16 entry keeps its own refusal
    assert lib.gcd_attn_temporal_f16(16, 192, 16, 64, 1, 17, 4, 1, None) != 0
    assert b"T=17" in lib.gcd_last_error()


def test_attn_temporal_refuses_more_than_64_frames_on_the_host():
    """ops.attn_temporal routes T > 16 to the long entry, whose refusal names T and the range (CPU tensors are
    refused first: no fallback)."""
    from gcd_amd import _lib, ops
    with pytest.raises(_lib.GcdError, match="no CPU fallback"):
        ops.attn_temporal(torch.zeros(65, 192, dtype=torch.float16), torch.zeros(65, 64, dtype=torch.float16),
                          1, 65, 1, 1)


def test_long_clip_kernels_compile_without_spills():
    """Both kernels hold the fragments of up to four 16-frame blocks in registers: a spill is a silent slow-down.
    Every instantiation (1..4 blocks) of both kernels, from the code object metadata.  (hipcc cross-compiles without a
    GPU.)"""
    import subprocess
    import tempfile
    from gcd_amd.csrc import build as B
    src = "attn_temporal_long.hip"
    assert src in B.SOURCES
    with tempfile.TemporaryDirectory() as td:
        out = Path(td) / (src + ".s")
        subprocess.check_call([B._hipcc(), *B.FLAGS, *B.EXTRA_FLAGS.get(src, []), "--cuda-device-only", "-S",
                               str(B.CSRC / src), "-o", str(out)], stderr=subprocess.DEVNULL)
        text = out.read_text()
    found = {}
    for m in re.finditer(r"\.name:\s+(\S+)\n(?:.*\n)*?\s+\.sgpr_spill_count:\s+(\d+)\n(?:.*\n)*?"
                         r"\s+\.vgpr_spill_count:\s+(\d+)", text):
        if "attn_temporal_long" in m.group(1):
            found[m.group(1)] = (int(m.group(2)), int(m.group(3)))
    assert len(found) == 8, sorted(found)
    for name, (ss, vs) in found.items():
        assert ss == 0 and vs == 0, f"{name} spills {ss} SGPRs / {vs} VGPRs"


def test_oracle_matches_reference_unet_at_25_frames():
    """The CPU oracle the GPU tests compare against, at T = 25 (past the old 16-frame limit): against the reference's
    own VideoUNet on O.TINY, at fp32 round-off."""
    from oracle import ref_shim, svd_unet_ref as O, weights
    if not ref_shim.available():
        pytest.skip("reference tree not readable here")
    VideoUNet, *_ = ref_shim.reference_classes()
    net = VideoUNet(**O.TINY.as_reference_kwargs()).eval()
    sd = weights.synth_state_dict({k: tuple(v.shape) for k, v in net.state_dict().items()})
    net.load_state_dict(sd)
    T, h, w = 25, 8, 8
    noise, c, uc = weights.synth_inputs(1, T, h, w, O.TINY.context_dim, O.TINY.adm_in_channels + O.TINY.aux_emb_dim, 5)
    x = torch.cat([torch.cat([noise, uc["concat"]], 1), torch.cat([noise, c["concat"]], 1)])
    ts = torch.linspace(-1.5, 1.63, 2 * T)
    ctx = torch.cat([uc["crossattn"], c["crossattn"]])
    y = torch.cat([uc["vector"], c["vector"]])
    ioi = torch.zeros(2, T)
    ioi[1, 20] = 1.0
    with torch.no_grad():
        ref = net(x, ts, context=ctx, y=y, num_video_frames=T, image_only_indicator=ioi)
        got = O.unet_forward(sd, O.TINY, x, ts, ctx, y, T, ioi)
    assert float(ref.std()) > 0.1
    assert rel_l2(got, ref) < 2e-5
