"""CPU: gcd_amd.clip_vision — the torch restatement against tests/golden/clip_vision_tiny.pt (tools/make_golden_clip.py),
the drop-in surface of FrozenOpenCLIPImageEmbedder, and the argument validation of the four entries of
libgcd_amd_clip.so (every check comes before any launch, so the entries are called here with host memory).

Bars.  Tower: the golden records the independent implementation (transformers' CLIPVisionModelWithProjection) in float32
and in float64; `err32` is the rel-L2 between the two, i.e. what one float32 evaluation of this network is off by.  Two
float32 evaluations that sum in different orders are each that far from the float64 value, so they differ by up to
2 x err32; the bar is 4 x err32 (a factor 2 of margin for one sample of the noise).  Preprocess: the float64 chain is
reproduced to 1e-12 (the generator holds torch's operators to a dense-matrix form of the formulae at that bar); the
float32 chain is deterministic torch CPU code, so it reproduces the recording to a few ulp: 1e-6 absolute on values
within [-2, 2.3], far below the recorded float32-float64 gaps it must not be confused with."""
import ctypes

import pytest
import torch

from clip_util import embedder, load_golden, preprocess_case, tower_case
from conftest import rel_l2
from gcd_amd import _lib, _lib_clip, clip_vision as cv
from gcd_amd.conditioning import GeneralConditioner

TOWER = ["w160_s17", "w160_s257", "w1280_s257"]
PRE = ["56x56", "96x160", "72x200", "40x200", "576x1024"]
TINY = dict(width=160, layers=2, heads=2, mlp_width=640, patch_size=14, image_size=56, embed_dim=64)


# ------------------------------------------------------------------------------------------------------------ the pins
@pytest.mark.parametrize("name", TOWER)
def test_restatement_against_the_independent_implementation(name):
    rec, sd, raw = tower_case(name)
    emb = embedder(rec["cfg"], sd)
    with torch.no_grad():
        out = emb(raw)
    assert out.dtype == torch.float32 and tuple(out.shape) == (rec["n"], rec["cfg"]["embed_dim"])
    e, bar = rel_l2(out, rec["out32"]), 4.0 * rec["err32"]
    print(f"{name}: restatement vs golden fp32 {e:.3e} (bar {bar:.3e}; vs fp64 {rel_l2(out, rec['out64']):.3e})")
    assert e < bar


def test_golden_states_its_drifts():
    for name in TOWER:
        rec = load_golden()["tower"][name]
        assert rec["restatement_vs_hf_fp64"] < 1e-12 and 0 < rec["err32"] < 1e-5
        assert rel_l2(rec["out_fp16_autocast"], rec["out32"]) == pytest.approx(rec["drift_fp16"], rel=1e-6)
        assert 1e-4 < rec["drift_fp16"] < rec["drift_bf16"] < 1e-2


@pytest.mark.parametrize("name", PRE)
def test_preprocess_restatement_against_both_recorded_chains(name):
    rec, raw = preprocess_case(name)
    mean, std = torch.tensor(cv.CLIP_MEAN), torch.tensor(cv.CLIP_STD)
    c64 = cv.preprocess_reference(raw.double(), rec["size"], True, mean, std)
    c32 = cv.preprocess_reference(raw, rec["size"], True, mean, std)
    assert tuple(c32.shape) == (rec["n"], 3, rec["size"], rec["size"]) and c32.dtype == torch.float32
    blur = max(rec["H"], rec["W"]) > rec["size"]
    assert tuple(rec["k"]) == ((cv.blur_taps(rec["H"], rec["size"])[0], cv.blur_taps(rec["W"], rec["size"])[0]) if blur else (1, 1))
    if "out64" in rec:
        g64, g32, m64, m32 = rec["out64"], rec["out32"], c64, c32
    else:
        g64, g32 = rec["out64_samples"], rec["out32_samples"]
        m64, m32 = c64.reshape(-1)[rec["sample_index"]], c32.reshape(-1)[rec["sample_index"]]
        assert float(c64.sum()) == pytest.approx(rec["out64_checksum"][0], rel=1e-11)
        assert float(c64.abs().sum()) == pytest.approx(rec["out64_checksum"][1], rel=1e-11)
    assert float((m64 - g64).abs().max()) < 1e-12
    assert float((m32.double() - g32.double()).abs().max()) < 1e-6
    assert float((c32.double() - c64).abs().max()) == pytest.approx(rec["gap32"], rel=0.25)


def test_blur_taps_of_the_sizes_of_interest():
    assert [cv.blur_taps(e, 224)[0] for e in (576, 1024)] == [3, 7]
    assert cv.blur_taps(576, 224)[1] == pytest.approx(0.786, abs=1e-3) and cv.blur_taps(1024, 224)[1] == pytest.approx(1.786, abs=1e-3)
    assert [cv.blur_taps(e, 224)[0] for e in (256, 384)] == [3, 3]
    assert cv.blur_taps(40, 56) == (3, 0.001)
    x = torch.rand(1, 3, 40, 40) * 2 - 1             # no axis shrinks: antialias is a no-op
    mean, std = torch.tensor(cv.CLIP_MEAN), torch.tensor(cv.CLIP_STD)
    assert torch.equal(cv.preprocess_reference(x, 56, True, mean, std), cv.preprocess_reference(x, 56, False, mean, std))


# --------------------------------------------------------------------------------------------------- the drop-in surface
def expected_keys(layers):
    keys = ["class_embedding", "positional_embedding", "proj", "conv1.weight", "ln_pre.weight", "ln_pre.bias"]
    for i in range(layers):
        p = f"transformer.resblocks.{i}."
        keys += [p + k for k in ("ln_1.weight", "ln_1.bias", "attn.in_proj_weight", "attn.in_proj_bias", "attn.out_proj.weight",
                                 "attn.out_proj.bias", "ln_2.weight", "ln_2.bias", "mlp.c_fc.weight", "mlp.c_fc.bias",
                                 "mlp.c_proj.weight", "mlp.c_proj.bias")]
    return keys + ["ln_post.weight", "ln_post.bias"]


def test_state_dict_keys_and_shapes_are_open_clips():
    emb = cv.FrozenOpenCLIPImageEmbedder(vision_cfg=TINY)
    sd = emb.state_dict()
    assert list(sd) == ["model.visual." + k for k in expected_keys(2)]           # mean / std are not persistent
    W, E, G2, P = 160, 64, 16, 14
    shapes = {k[len("model.visual."):]: tuple(v.shape) for k, v in sd.items()}
    assert shapes["class_embedding"] == (W,) and shapes["positional_embedding"] == (G2 + 1, W) and shapes["proj"] == (W, E)
    assert shapes["conv1.weight"] == (W, 3, P, P)
    p = "transformer.resblocks.1."
    assert shapes[p + "attn.in_proj_weight"] == (3 * W, W) and shapes[p + "attn.in_proj_bias"] == (3 * W,)
    assert shapes[p + "mlp.c_fc.weight"] == (640, W) and shapes[p + "mlp.c_proj.weight"] == (W, 640)
    assert not any(q.requires_grad for q in emb.parameters()) and not emb.model.training        # freeze(), as the reference
    assert dict(emb.named_buffers()).keys() == {"mean", "std"}
    assert emb.mean.tolist() == pytest.approx(list(cv.CLIP_MEAN)) and emb.std.tolist() == pytest.approx(list(cv.CLIP_STD))


def test_the_arch_table_is_vit_h_14():
    with torch.device("meta"):
        v = cv.VisionTransformer(**cv.ARCHS["ViT-H-14"])
    assert (v.width, v.layers, v.heads, v.mlp_width, v.patch_size, v.image_size, v.embed_dim) == (1280, 32, 16, 5120, 14, 224, 1024)
    assert v.width // v.heads == 80 and v.kp == 608 and v.ln_pre.eps == 1e-5
    assert list(v.state_dict()) == expected_keys(32)
    assert sum(q.numel() for q in v.parameters()) == 632_076_800
    with pytest.raises(_lib.GcdError, match="unknown arch"):
        cv.FrozenOpenCLIPImageEmbedder(arch="ViT-L-14")


def test_full_open_clip_state_dict_loads_strict():
    emb = cv.FrozenOpenCLIPImageEmbedder(vision_cfg=TINY)
    sd = {k: torch.randn_like(v) for k, v in emb.state_dict().items()}
    text = {"model.logit_scale": torch.zeros(()), "model.token_embedding.weight": torch.zeros(8, 4),
            "model.positional_embedding": torch.zeros(77, 4), "model.ln_final.weight": torch.zeros(4),
            "model.ln_final.bias": torch.zeros(4), "model.text_projection": torch.zeros(4, 4)}
    full = dict(sd, **text)
    emb.load_state_dict(full, strict=True)
    assert len(full) == len(sd) + len(text)                                         # the caller's dict is left alone
    assert all(torch.equal(emb.state_dict()[k], sd[k]) for k in sd)
    # under the conditioner's prefix too (conditioner.embedders.0.open_clip.model.*)
    holder = torch.nn.Module()
    holder.open_clip = cv.FrozenOpenCLIPImageEmbedder(vision_cfg=TINY)
    holder.load_state_dict({"open_clip." + k: v for k, v in full.items()}, strict=True)
    with pytest.raises(RuntimeError, match="Unexpected key"):
        emb.load_state_dict(dict(sd, **{"model.visual.extra": torch.zeros(1)}), strict=True)


def test_version_never_downloads_and_a_local_file_is_loaded(tmp_path, monkeypatch):
    import socket

    def no_network(*a, **k):
        raise AssertionError("the embedder tried to open a socket")
    monkeypatch.setattr(socket, "socket", no_network)
    emb = cv.FrozenOpenCLIPImageEmbedder(version="laion2b_s32b_b79k", vision_cfg=TINY)       # a name, not a file
    assert isinstance(emb.model.visual, cv.VisionTransformer)
    # a local file in open_clip format: visual.* beside the text side
    sd = cv.seeded_state_dict(TINY, 7)
    ckpt = {"visual." + k: v for k, v in sd.items()}
    ckpt.update({"logit_scale": torch.zeros(()), "text_projection": torch.zeros(4, 4)})
    path = tmp_path / "open_clip_pytorch_model.pt"
    torch.save(ckpt, path)
    emb = cv.FrozenOpenCLIPImageEmbedder(version=str(path), vision_cfg=TINY)
    assert all(torch.equal(emb.model.visual.state_dict()[k], v) for k, v in sd.items())
    from safetensors.torch import save_file
    save_file({k: v.contiguous() for k, v in ckpt.items()}, str(tmp_path / "m.safetensors"))
    emb = cv.FrozenOpenCLIPImageEmbedder(version=str(tmp_path / "m.safetensors"), vision_cfg=TINY)
    assert all(torch.equal(emb.model.visual.state_dict()[k], v) for k, v in sd.items())


def test_unsupported_options_raise_naming_the_option():
    with pytest.raises(_lib.GcdError, match="num_image_crops"):
        cv.FrozenOpenCLIPImageEmbedder(vision_cfg=TINY, num_image_crops=2)
    with pytest.raises(_lib.GcdError, match="output_tokens"):
        cv.FrozenOpenCLIPImageEmbedder(vision_cfg=TINY, output_tokens=True)


def test_ucg_unsqueeze_and_repeat_follow_the_reference():
    rec, sd, raw = tower_case("w160_s17")
    with torch.no_grad():
        z = embedder(rec["cfg"], sd)(raw)
        z3 = embedder(rec["cfg"], sd, unsqueeze_dim=True)(raw)
        assert tuple(z3.shape) == (3, 1, 64) and torch.equal(z3[:, 0], z)
        rep, z_again = embedder(rec["cfg"], sd, repeat_to_max_len=True, max_length=5)(raw)
        assert tuple(rep.shape) == (3, 5, 64) and torch.equal(z_again, z) and all(torch.equal(rep[:, i], z) for i in range(5))
        rep3, z3_again = embedder(rec["cfg"], sd, repeat_to_max_len=True, unsqueeze_dim=True, max_length=4)(raw)
        assert tuple(rep3.shape) == (3, 4, 64) and tuple(z3_again.shape) == (3, 1, 64)
        drop = embedder(rec["cfg"], sd, ucg_rate=1.0)
        assert torch.equal(drop(raw), torch.zeros_like(z)) and torch.equal(drop(raw, no_dropout=True), z)
        half = embedder(rec["cfg"], sd, ucg_rate=0.5)
        big = raw[:1].expand(64, -1, -1, -1)
        torch.manual_seed(3)
        out = half(big)
        torch.manual_seed(3)
        keep = torch.bernoulli(0.5 * torch.ones(64))
        assert 0 < int(keep.sum()) < 64 and torch.equal(out, keep[:, None] * z[:1].expand(64, -1))
        assert embedder(rec["cfg"], sd).encode(raw).equal(z)


def kubric_embedder_block(vision_cfg, n_cond_frames=1, n_copies=1):
    """The first emb_models entry of configs/infer_kubric.yaml with its two `target`s pointed at gcd_amd."""
    return {"input_key": "cond_frames_without_noise", "is_trainable": False,
            "target": "gcd_amd.conditioning.FrozenOpenCLIPImagePredictionEmbedder",
            "params": {"n_cond_frames": n_cond_frames, "n_copies": n_copies,
                       "open_clip_embedding_config": {"target": "gcd_amd.clip_vision.FrozenOpenCLIPImageEmbedder",
                                                      "params": {"freeze": True, "vision_cfg": vision_cfg}}}}


def test_general_conditioner_from_the_kubric_block_constructs_and_runs_on_the_cpu():
    import sys
    rec, sd, raw = tower_case("w160_s17")
    cond = GeneralConditioner([kubric_embedder_block(dict(rec["cfg"]))])
    assert not {"open_clip", "kornia"} & set(sys.modules)
    tower = cond.embedders[0].open_clip
    assert isinstance(tower, cv.FrozenOpenCLIPImageEmbedder)
    assert list(cond.state_dict()) == ["embedders.0.open_clip.model.visual." + k for k in expected_keys(2)]
    tower.model.visual.load_state_dict(sd)
    B, T = 1, 3
    out = cond({"cond_frames_without_noise": raw})
    assert set(out) == {"crossattn"} and tuple(out["crossattn"].shape) == (B * T, 1, 64)
    assert rel_l2(out["crossattn"][:, 0], rec["out32"]) < 4.0 * rec["err32"]
    zero = cond({"cond_frames_without_noise": raw}, force_zero_embeddings=["cond_frames_without_noise"])
    assert torch.equal(zero["crossattn"], torch.zeros(B * T, 1, 64))


# ------------------------------------------------------------------------------------------------- argument validation
def _refused(rc, entry, match):
    assert rc == 2
    with pytest.raises(_lib.GcdError, match=match):
        _lib_clip.check(rc, entry)


@pytest.fixture(scope="module")
def host():
    """Real, 16-byte aligned host memory for every pointer argument; no entry below gets as far as reading it."""
    import types
    from gcd_amd.csrc import build
    build.build(verbose=False)                 # a no-op when the libraries are current
    return types.SimpleNamespace(lib=_lib_clip.load(), f32=torch.zeros(1 << 16), f16=torch.zeros(1 << 16, dtype=torch.float16),
                                 o32=torch.zeros(1 << 16), o16=torch.zeros(1 << 16, dtype=torch.float16), v=torch.zeros(64))


def test_preprocess_validation(host):
    h = host
    x, ms, p, im = h.f32.data_ptr(), h.v.data_ptr(), h.o16.data_ptr(), h.o32.data_ptr()

    def call(x=x, sn=3 * 64 * 64, sc=64 * 64, sh=64, sw=1, n=1, H=64, W=64, S=56, P=14, aa=1, mean=ms, std=ms, patches=p,
             Kp=608, img=im):
        return h.lib.gcd_clip_preprocess(x, sn, sc, sh, sw, n, H, W, S, P, aa, mean, std, patches, Kp, img, None)
    for null in ("x", "mean", "std", "patches"):
        _refused(call(**{null: None}), "gcd_clip_preprocess", "null pointer")
    _refused(call(n=0), "gcd_clip_preprocess", "empty problem")
    _refused(call(S=57), "gcd_clip_preprocess", "multiple of P")
    _refused(call(Kp=600), "gcd_clip_preprocess", "Kp=600")
    _refused(call(Kp=576), "gcd_clip_preprocess", "Kp=576")
    _refused(call(W=_lib_clip.CLIP_MAX_WIDTH + 1), "gcd_clip_preprocess", "exceeds 8192")
    _refused(call(x=x + 2), "gcd_clip_preprocess", "misaligned")
    _refused(call(patches=p + 8), "gcd_clip_preprocess", "misaligned")
    _refused(call(img=im + 1), "gcd_clip_preprocess", "misaligned")
    _refused(call(sw=-1), "gcd_clip_preprocess", "strides")
    _refused(call(sh=0), "gcd_clip_preprocess", "strides")
    # reflect padding: H, W > k // 2.  W = 8192 -> 224: factor 36.6, sigma 17.8, k 71 > 63
    _refused(call(W=8192, S=224), "gcd_clip_preprocess", r"antialias kernel \(3, 71\) exceeds 63")
    # H = 1 with a shrinking W: ky = 3, k // 2 = 1, and H = 1 is not > 1
    _refused(call(H=1, W=200), "gcd_clip_preprocess", "reflect padding needs H=1 > 1")
    # W = 5600 -> 224: factor 25, sigma 12, k 49, k // 2 = 24: fine; the same k with W too small cannot happen (W >= S),
    # so the W side of the rule is reached through H: H = 3000 -> 56 gives ky = 105 > 63 first
    _refused(call(H=3000), "gcd_clip_preprocess", "exceeds 63")


def test_tokens_ln_pre_validation(host):
    h = host
    a, o, v = h.f32.data_ptr(), h.o32.data_ptr(), h.v.data_ptr()

    def call(patch=a, ldp=32, cls=v, pos=a, gamma=v, beta=v, eps=1e-5, tok=o, ldo=32, n=2, G2=16, C=32):
        return h.lib.gcd_clip_tokens_ln_pre(patch, ldp, cls, pos, gamma, beta, eps, tok, ldo, n, G2, C, None)
    for null in ("patch", "cls", "pos", "gamma", "beta", "tok"):
        _refused(call(**{null: None}), "gcd_clip_tokens_ln_pre", "null pointer")
    _refused(call(G2=0), "gcd_clip_tokens_ln_pre", "empty problem")
    _refused(call(C=_lib_clip.CLIP_MAX_MODEL_WIDTH + 4, ldp=8192, ldo=8192), "gcd_clip_tokens_ln_pre", "exceeds 4096")
    _refused(call(ldp=31), "gcd_clip_tokens_ln_pre", "row strides")
    _refused(call(ldo=16), "gcd_clip_tokens_ln_pre", "row strides")
    _refused(call(tok=o + 2), "gcd_clip_tokens_ln_pre", "misaligned")
    _refused(call(eps=-1.0), "gcd_clip_tokens_ln_pre", "eps")


def test_attention_validation(host):
    h = host
    q, o = h.f16.data_ptr(), h.o16.data_ptr()

    def call(qkv=q, ld=480, out=o, ldo=160, n=1, S=17, heads=2, pre=0):
        return h.lib.gcd_clip_attn_f16(qkv, ld, out, ldo, n, S, heads, pre, None)
    _refused(call(qkv=None), "gcd_clip_attn_f16", "null pointer")
    _refused(call(out=None), "gcd_clip_attn_f16", "null pointer")
    _refused(call(S=0), "gcd_clip_attn_f16", "empty problem")
    _refused(call(S=_lib_clip.CLIP_ATTN_MAX_S + 1), "gcd_clip_attn_f16", "S=289 exceeds 288")
    # the head dim is part of the layout: rows of 3 * heads * 64 columns (gcd_attn_spatial_f16's head dim) are too short
    _refused(call(ld=3 * 2 * 64), "gcd_clip_attn_f16", "head dim is 80")
    _refused(call(ld=484), "gcd_clip_attn_f16", "16-byte aligned rows")
    _refused(call(qkv=q + 8), "gcd_clip_attn_f16", "16-byte aligned rows")
    _refused(call(ldo=128), "gcd_clip_attn_f16", "ldo=128 below heads")
    _refused(call(out=o + 1), "gcd_clip_attn_f16", "ldo")


def test_bias_gelu_validation(host):
    h = host
    a, o, v = h.f32.data_ptr(), h.o16.data_ptr(), h.v.data_ptr()

    def call(x=a, ldh=64, bias=v, out=o, ldo=64, M=4, N=64):
        return h.lib.gcd_clip_bias_gelu_f16(x, ldh, bias, out, ldo, M, N, None)
    for null in ("x", "bias", "out"):
        _refused(call(**{null: None}), "gcd_clip_bias_gelu_f16", "null pointer")
    _refused(call(M=0), "gcd_clip_bias_gelu_f16", "empty problem")
    _refused(call(N=62), "gcd_clip_bias_gelu_f16", "multiples of 4")
    _refused(call(ldh=66), "gcd_clip_bias_gelu_f16", "multiples of 4")
    _refused(call(ldo=60), "gcd_clip_bias_gelu_f16", "multiples of 4")
    _refused(call(x=a + 4), "gcd_clip_bias_gelu_f16", "misaligned")
    _refused(call(out=o + 4), "gcd_clip_bias_gelu_f16", "misaligned")


def test_gpu_path_refuses_what_it_does_not_support():
    v = cv.VisionTransformer(**dict(TINY, heads=4))               # head dim 40
    with pytest.raises(_lib.GcdError, match="head dim 80"):
        v._check_gpu()
    v = cv.VisionTransformer(**TINY)                                # parameters require grad: forward-only on the GPU
    with pytest.raises(_lib.GcdError, match="forward-only"):
        v._check_gpu()
    with torch.no_grad():
        v._check_gpu()
    v.requires_grad_(False)
    v._check_gpu()
    with pytest.raises(_lib.GcdError, match="no CPU fallback"):
        cv.attention(torch.zeros(17, 480, dtype=torch.float16), torch.zeros(17, 160, dtype=torch.float16), 1, 17, 2)
    assert ctypes.sizeof(ctypes.c_void_p) == 8
