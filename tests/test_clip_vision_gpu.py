"""GPU: the CLIP image tower on HIP (gcd_amd/clip_vision.py, libgcd_amd_clip.so) against float64 references and
tests/golden/clip_vision_tiny.pt (tools/make_golden_clip.py).

Bars.
  attention        1.5e-3 rel-L2 against float64 softmax attention on the fp16-rounded operands: the bar
                   test_kernels_gpu.py holds gcd_attn_spatial_f16 to (the same arithmetic: fp16 P, fp32 accumulation,
                   fp16 output).
  preprocess       fp32 image within 4 x the recorded float32-chain gap of the case (max-abs) of the float64 chain
                   (DESIGN.md §12.2's rule for a stage pinned to a restatement); the fp16 patch matrix is that image rounded
                   once, bit for bit; pad columns are zeros.
  tokens + ln_pre  2e-6 rel-L2 against float64: per element about six fp32 roundings (3.6e-7) plus the error of the two
                   tree-folded row sums, (log2 256 + C / 256) eps ~ 8e-7 at C = 1280, on x_hat of order one.
  bias + GELU      |err| <= 2^-11 |ref| + 1e-6: one rounding to fp16, plus the fp32 cancellation of 1 + erf(t / sqrt 2) in
                   the negative tail (|t| / 2 x 2^-23 <= 6e-7 at t = -10, where gelu itself is below 1e-21).
  tower            2 x the recorded fp16-autocast drift of the independent implementation for that case, against its
                   float32 output: the kernel path rounds at the same places (fp16 operands, fp32 accumulation) but sums
                   in another order and carries fp16 probabilities; twice one sample of that noise is the margin.

Measured on an MI355X: see DESIGN.md §10.1."""
import math

import pytest
import torch
import torch.nn.functional as F

from clip_util import embedder, preprocess_case, seeded_image, tower_case
from conftest import rel_l2
from test_clip_vision_host import kubric_embedder_block

pytestmark = pytest.mark.gpu
TOL_ATTN = 1.5e-3
F16, F32 = torch.float16, torch.float32


def _gen(seed):
    return torch.Generator().manual_seed(seed)


def _h(t):
    return t.to(F16).float()


def _bits(t):
    return t.contiguous().view(torch.int16 if t.dtype == F16 else torch.int32)


# ----------------------------------------------------------------------------------------------------------- attention
def _rows(t):
    """[n, heads, S, 80] -> rows (image, token) x (head, 80)."""
    n, heads, S, d = t.shape
    return t.permute(0, 2, 1, 3).reshape(n * S, heads * d)


def _attn_ref(q, k, v):
    return _rows(F.scaled_dot_product_attention(q.double(), k.double(), v.double())).float()      # scale 1 / sqrt(80)


def _attn_gpu(gpu, q, k, v, q_prescaled=False):
    from gcd_amd import clip_vision as cv
    n, heads, S, _ = q.shape
    qkv = torch.cat([_rows(q), _rows(k), _rows(v)], 1).half().to(gpu)
    out = torch.full((n * S, heads * 80), float("nan"), dtype=F16, device=gpu)
    cv.attention(qkv, out, n, S, heads, q_prescaled=q_prescaled)
    torch.cuda.synchronize()
    return out


@pytest.mark.parametrize("n", [1, 3])
@pytest.mark.parametrize("heads", [1, 2, 16])
@pytest.mark.parametrize("S", [1, 16, 17, 64, 65, 257])
def test_attention_against_float64(gpu, S, heads, n):
    from gcd_amd import clip_vision as cv
    g = _gen(1000 + 10 * S + heads)
    q, k, v = (_h(torch.randn(n, heads, S, 80, generator=g) * 1.5) for _ in range(3))
    if S >= 64:
        k[:, :, 40] *= 4.0                         # a spiked key
    ref = _attn_ref(q, k, v)
    out = _attn_gpu(gpu, q, k, v)
    assert torch.isfinite(out.float()).all()
    e = rel_l2(out.float(), ref)
    print(f"clip attention S={S} heads={heads} n={n}: rel-L2 {e:.3e}")
    assert e < TOL_ATTN
    # two calls are bit-identical
    assert torch.equal(_bits(out), _bits(_attn_gpu(gpu, q, k, v)))
    # every image alone gives the rows it has in the batch, bit for bit
    if n > 1:
        for i in range(n):
            alone = _attn_gpu(gpu, q[i:i + 1], k[i:i + 1], v[i:i + 1])
            assert torch.equal(_bits(alone), _bits(out[i * S:(i + 1) * S])), f"image {i} alone differs from its rows in the batch"
    # q_prescaled: q carries log2(e) / sqrt(80); reference on the fp16-rounded scaled q
    qs = _h(q * cv.ATTN_Q_SCALE_LOG2)
    ref2 = _attn_ref(qs / cv.ATTN_Q_SCALE_LOG2, k, v)
    e2 = rel_l2(_attn_gpu(gpu, qs, k, v, q_prescaled=True).float(), ref2)
    assert e2 < TOL_ATTN, f"prescaled q: rel-L2 {e2:.3e}"


@pytest.mark.parametrize("S", [65, 257])
def test_attention_shifted_logits_and_a_dominant_key(gpu, S):
    """Every logit of a row carries a common offset of about L = 200 (an exp without the max subtraction overflows fp32
    from 89 on), and key i dominates row i by about 13: k loses its component along a unit vector u and gets a u, q gets
    a u with a = sqrt(L sqrt(80)), then k_i += 1.5 q_i' (q' the part of q without the shift)."""
    n, heads, L = 2, 2, 200.0
    g = _gen(2000 + S)
    q0, k, v = (torch.randn(n, heads, S, 80, generator=g) for _ in range(3))
    u = torch.randn(80, generator=g)
    u /= u.norm()
    a = math.sqrt(L * math.sqrt(80.0))
    q0 = q0 - (q0 @ u)[..., None] * u
    k = k - (k @ u)[..., None] * u + 1.5 * q0 + a * u
    q, k, v = _h(q0 + a * u), _h(k), _h(v)
    logits = (q.double() @ k.double().transpose(-1, -2)) / math.sqrt(80.0)
    assert float(logits.min()) > 150.0 and float(torch.softmax(logits, -1).diagonal(dim1=-2, dim2=-1).median()) > 0.5
    out = _attn_gpu(gpu, q, k, v)
    assert torch.isfinite(out.float()).all()
    e = rel_l2(out.float(), _attn_ref(q, k, v))
    print(f"clip attention shifted logits S={S}: rel-L2 {e:.3e}")
    assert e < TOL_ATTN


# ---------------------------------------------------------------------------------------------------------- preprocess
@pytest.mark.parametrize("name", ["56x56", "96x160", "72x200", "40x200", "576x1024"])
def test_preprocess_against_the_float64_chain(gpu, name):
    from gcd_amd import clip_vision as cv
    rec, raw = preprocess_case(name)
    n, H, W, S, P = rec["n"], rec["H"], rec["W"], rec["size"], 14
    if H * W < 100000:                              # a second image, so that the image stride is exercised
        raw = torch.cat([raw, seeded_image(1, H, W, rec["image_seed"] + 50)])
        n += 1
    mean, std = torch.tensor(cv.CLIP_MEAN), torch.tensor(cv.CLIP_STD)
    ref = cv.preprocess_reference(raw.double(), S, True, mean, std)
    kp = (3 * P * P + 31) // 32 * 32
    patches, img = cv.preprocess(raw.to(gpu), S, P, True, mean.to(gpu), std.to(gpu), kp, want_image=True)
    torch.cuda.synchronize()
    gap = float((img.cpu().double() - ref).abs().max())
    print(f"clip preprocess {name}: max-abs vs float64 chain {gap:.3e} (bar 4 x {rec['gap32']:.3e})")
    assert gap <= 4.0 * rec["gap32"]
    # the patch matrix: the fp32 image rounded once, in conv1's (c, py, px) order; pad columns are exact zeros
    G = S // P
    want = img.reshape(n, 3, G, P, G, P).permute(0, 2, 4, 1, 3, 5).reshape(n * G * G, 3 * P * P).half()
    assert tuple(patches.shape) == (n * G * G, kp) and kp == 608
    assert torch.equal(_bits(patches[:, :3 * P * P]), _bits(want))
    assert torch.equal(_bits(patches[:, 3 * P * P:]), torch.zeros(n * G * G, kp - 3 * P * P, dtype=torch.int16, device=gpu))
    # a strided, non-contiguous view of the same pixels: every second column of a wider, taller tensor
    big = torch.full((n, 3, H + 3, 2 * W + 5), float("nan"), device=gpu)
    view = big[:, :, 1:H + 1, 2:2 * W + 2:2]
    view.copy_(raw.to(gpu))
    assert not view.is_contiguous() and view.stride(3) == 2
    patches2, img2 = cv.preprocess(view, S, P, True, mean.to(gpu), std.to(gpu), kp, want_image=True)
    assert torch.equal(_bits(img2), _bits(img)) and torch.equal(_bits(patches2), _bits(patches))
    # no image output asked for: the same patches
    patches3, none = cv.preprocess(raw.to(gpu), S, P, True, mean.to(gpu), std.to(gpu), kp)
    assert none is None and torch.equal(_bits(patches3), _bits(patches))


def test_preprocess_without_antialias(gpu):
    from gcd_amd import clip_vision as cv
    rec, raw = preprocess_case("96x160")
    mean, std = torch.tensor(cv.CLIP_MEAN), torch.tensor(cv.CLIP_STD)
    ref = cv.preprocess_reference(raw.double(), 56, False, mean, std)
    _, img = cv.preprocess(raw.to(gpu), 56, 14, False, mean.to(gpu), std.to(gpu), 608, want_image=True)
    assert float((img.cpu().double() - ref).abs().max()) <= 4.0 * rec["gap32"]


# ------------------------------------------------------------------------------------------- tokens + ln_pre, bias + GELU
@pytest.mark.parametrize("n,G2,C", [(3, 16, 160), (1, 256, 1280), (2, 5, 36)])
def test_tokens_ln_pre_against_float64(gpu, n, G2, C):
    from gcd_amd import clip_vision as cv
    g = _gen(3000 + C)
    patch = torch.randn(n * G2, C, generator=g)
    cls, pos = 0.3 * torch.randn(C, generator=g), 0.3 * torch.randn(G2 + 1, C, generator=g)
    gamma, beta = 1 + 0.1 * torch.randn(C, generator=g), 0.1 * torch.randn(C, generator=g)
    z = torch.cat([cls.double().expand(n, 1, C), patch.double().reshape(n, G2, C)], 1) + pos.double()
    ref = F.layer_norm(z, (C,), gamma.double(), beta.double(), 1e-5).reshape(n * (G2 + 1), C)
    wide = torch.full((n * G2, C + 12), float("nan"), device=gpu)              # strided rows on both sides
    wide[:, :C] = patch.to(gpu)
    out = torch.full((n * (G2 + 1), C + 4), float("nan"), device=gpu)
    cv.tokens_ln_pre(wide[:, :C], cls.to(gpu), pos.to(gpu), gamma.to(gpu), beta.to(gpu), out[:, :C], n)
    torch.cuda.synchronize()
    assert torch.isnan(out[:, C:]).all() and torch.isfinite(out[:, :C]).all()
    e = rel_l2(out[:, :C], ref)
    print(f"clip tokens + ln_pre n={n} G2={G2} C={C}: rel-L2 {e:.3e}")
    assert e < 2e-6


def test_bias_gelu_against_float64(gpu):
    from gcd_amd import clip_vision as cv
    M, N = 37, 172                                 # M N / 4 is no multiple of the 256-thread block
    g = _gen(3100)
    t = torch.cat([torch.tensor([10.0, -10.0, 0.0, -0.0, 6.0, -6.0, -0.7517916, 100.0]),
                   torch.linspace(-0.85, -0.65, 1001),                       # the minimum of GELU
                   torch.linspace(-10.0, 10.0, 2001), 3.0 * torch.randn(M * N, generator=g)])[:M * N].reshape(M, N).float()
    bias = torch.randn(N, generator=g)
    h = t - bias                                    # fp32; h + bias is evaluated in fp32 by the kernel
    want = (h + bias).double()
    ref = 0.5 * want * (1.0 + torch.erf(want / math.sqrt(2.0)))
    hw = torch.full((M, N + 8), float("nan"), device=gpu)
    hw[:, :N] = h.to(gpu)
    out = torch.full((M, N + 4), float("nan"), dtype=F16, device=gpu)
    cv.bias_gelu(hw[:, :N], bias.to(gpu), out[:, :N])
    torch.cuda.synchronize()
    assert torch.isnan(out[:, N:]).all()
    got = out[:, :N].cpu().double()
    assert torch.isfinite(got).all()
    err, tol = (got - ref).abs(), ref.abs() * 2.0 ** -11 + 1e-6
    worst = int((err - tol).argmax())
    print(f"clip bias + GELU: worst err - tol {float((err - tol).max()):.3e} at t = {float(want.reshape(-1)[worst]):.4f}")
    assert bool((err <= tol).all())
    assert float(got.reshape(-1)[0]) == 10.0 and float(got.reshape(-1)[1]) == 0.0


# --------------------------------------------------------------------------------------------------------------- tower
@pytest.mark.parametrize("name", ["w160_s17", "w160_s257", "w1280_s257"])
def test_tower_against_the_independent_implementation(gpu, name):
    rec, sd, raw = tower_case(name)
    emb = embedder(rec["cfg"], sd, device=gpu)
    with torch.no_grad():
        out = emb(raw.to(gpu))
        again = emb(raw.to(gpu))
    torch.cuda.synchronize()
    assert out.dtype == F32 and out.is_cuda and tuple(out.shape) == (rec["n"], rec["cfg"]["embed_dim"])
    e, bar = rel_l2(out, rec["out32"]), 2.0 * rec["drift_fp16"]
    print(f"clip tower {name}: rel-L2 vs the independent fp32 output {e:.3e} (bar {bar:.3e} = 2 x its fp16-autocast drift)")
    assert e < bar
    assert torch.equal(_bits(out), _bits(again)), "two calls differ"
    # a weight changed in place changes the next output (the fp16 packs follow the parameters' versions)
    with torch.no_grad():
        emb.model.visual.ln_post.bias.add_(1.0)
        moved = emb(raw.to(gpu))
    assert rel_l2(moved, rec["out32"]) > 0.05
    del emb
    torch.cuda.empty_cache()


def test_tower_refuses_grad_and_other_head_dims(gpu):
    from gcd_amd import _lib, clip_vision as cv
    rec, sd, raw = tower_case("w160_s17")
    emb = embedder(rec["cfg"], sd, device=gpu, freeze=False)
    with pytest.raises(_lib.GcdError, match="forward-only"):
        emb(raw.to(gpu))
    with torch.no_grad():
        assert torch.isfinite(emb(raw.to(gpu))).all()
    emb = cv.FrozenOpenCLIPImageEmbedder(vision_cfg=dict(rec["cfg"], heads=4)).to(gpu)
    with pytest.raises(_lib.GcdError, match="head dim 80"):
        emb(raw.to(gpu))
    with pytest.raises(_lib.GcdError, match="CPU only"):
        emb.model.visual(raw.to(gpu))


# --------------------------------------------------------------------------------------------- through the conditioner
def test_conditioner_with_the_hip_tower_feeds_the_unet(gpu):
    from gcd_amd.conditioning import GeneralConditioner
    from gcd_amd.video_model import VideoUNet
    from oracle import svd_unet_ref as O, weights
    rec, sd, raw = tower_case("w160_s17")
    T, copies = 3, 2
    cond = GeneralConditioner([kubric_embedder_block(dict(rec["cfg"]), n_cond_frames=1, n_copies=copies)])
    cond.embedders[0].open_clip.model.visual.load_state_dict(sd)
    batch = {"cond_frames_without_noise": raw}
    host = cond(batch)["crossattn"]
    cond = cond.to(gpu)
    batch = {"cond_frames_without_noise": raw.to(gpu)}
    c, uc = cond.get_unconditional_conditioning(batch, force_uc_zero_embeddings=["cond_frames_without_noise"])
    dev = c["crossattn"]
    assert dev.is_cuda and tuple(dev.shape) == tuple(host.shape) == (T * copies, 1, 64)
    e, bar = rel_l2(dev, host), 2.0 * rec["drift_fp16"]
    print(f"clip conditioner: GPU vs CPU run of the same module {e:.3e} (bar {bar:.3e})")
    assert e < bar
    assert torch.equal(dev[0::2], dev[1::2])                                    # n_copies: b t d -> (b s) t d
    assert torch.equal(uc["crossattn"], torch.zeros_like(dev))
    # the context goes into the UNet as it is, on the device
    cfg = O.TINY
    with torch.device("meta"):
        net = VideoUNet(**cfg.as_reference_kwargs())
    shapes = {k: tuple(v.shape) for k, v in net.state_dict().items()}
    net = net.to_empty(device=gpu)
    net.load_state_dict(weights.synth_state_dict(shapes, 0))
    net.eval()
    frames = 2 * T * copies
    g = _gen(4000)
    x = torch.randn(frames, 8, 8, 8, generator=g).to(gpu)
    ts = torch.linspace(-1.5, 1.63, frames).to(gpu)
    y = torch.randn(frames, cfg.adm_in_channels + cfg.aux_emb_dim, generator=g).to(gpu)
    kw = dict(y=y, num_video_frames=T * copies, image_only_indicator=torch.zeros(2, T * copies, device=gpu))
    with torch.no_grad():
        out = net(x, ts, context=torch.cat([uc["crossattn"], dev]), **kw)
        blank = net(x, ts, context=torch.zeros(frames, 1, 64, device=gpu), **kw)
    torch.cuda.synchronize()
    assert torch.isfinite(out).all() and tuple(out.shape) == (frames, 4, 8, 8)
    # the unconditional half saw zeros both times; the conditional half saw the tower's embedding
    assert rel_l2(out[:frames // 2], blank[:frames // 2]) < 1e-5 and rel_l2(out[frames // 2:], blank[frames // 2:]) > 1e-4
