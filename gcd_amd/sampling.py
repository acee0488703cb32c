"""Drop-in for sgm.modules.diffusionmodules.sampling.EulerEDMSampler (reference sampling.py:26-144,
225-230): the `sampler_config.target` socket.

    sampler = EulerEDMSampler(discretization_config, num_steps, guider_config, verbose, device)
    x0 = sampler(denoiser, x, cond, uc=None, num_steps=None)

Two execution paths with identical results:
  * generic — any `denoiser(input, sigma, c)` callable (e.g. the closure DiffusionEngine.sample_video
    builds, diffusion.py:531-532): the reference's step arithmetic in torch, without the reference's
    per-step device->host sync (sampling.py:131 compares a device tensor; with s_churn == 0 the
    comparison cannot change gamma, so it is skipped; otherwise it uses a host copy of the sigmas);
  * fused — when the denoiser is a `FusedDenoiser` around gcd_amd's own Denoiser / OpenAIWrapper /
    VideoUNet and the guider is a LinearPredictionGuider: the whole step (EDM scalings, CFG batch
    assembly, UNet, guidance, Euler update) runs as libgcd_amd kernels on static buffers, one
    hipGraph replay per step, sigma fed from a device table.

The rest of the reference's single-network-evaluation family shares the socket (sampling.py:82-184, 233-377):
HeunEDMSampler, EulerAncestralSampler, DPMPP2SAncestralSampler, DPMPP2MSampler, and EulerEDMSampler with s_churn > 0.
Their generic path is the reference's arithmetic in torch; their fused path is `FusedStageLoop`: every x-update of the
family is a linear combination of at most five tensors with coefficients that depend on the sigma schedule only
(gcd_amd/sampler_stages.py), so one captured launch sequence — EDM scalings, UNet, gcd_sampler_stage_f32 — serves every
stage of every sampler, fed one 12-float row per replay.  Guiders of the fused paths: LinearPredictionGuider (without
additional cond keys) and VanillaCFG.  EulerEDMSampler with s_churn == 0 keeps `FusedEulerLoop`, call for call.
LinearMultistepSampler is not provided (its coefficients come from scipy.integrate.quad, and nothing here imports
scipy); IdentityGuider stays on the generic path (its batch is not doubled).
"""
from __future__ import annotations

import ctypes as C
import os
from typing import Dict, Optional

import torch

from . import _lib, ops, sampler_ops
from .denoiser import Denoiser
from .denoiser_scaling import VScalingWithEDMcNoise
from .guiders import LinearPredictionGuider, VanillaCFG
from .sampler_stages import (ZERO_SIGMA, churn_gammas, get_ancestral_step, stage_table, to_neg_log_sigma,
                             to_sigma)
from .util import append_dims, default, instantiate_from_config
from .video_model import VideoUNet
from .wrappers import OpenAIWrapper

DEFAULT_GUIDER = {"target": "gcd_amd.guiders.IdentityGuider"}


class FusedDenoiser:
    """`denoiser(input, sigma, c)` exactly like the closure in DiffusionEngine.sample_video
    (diffusion.py:526-532), but with its captured objects visible so the sampler may fuse."""

    def __init__(self, denoiser: Denoiser, network, **additional_model_inputs):
        self.denoiser = denoiser
        self.network = network
        self.additional_model_inputs = additional_model_inputs

    def __call__(self, input, sigma, c):
        return self.denoiser(self.network, input, sigma, c, **self.additional_model_inputs)


def _closure_signature(fn, role):
    """The body of a closure as a list of (opcode, operand) with every captured variable replaced by the ROLE of
    the object it holds (`role(cell_contents)`), locals by their index and attributes / constants by value: two
    closures with the same signature execute the same instructions on objects of the same roles, whatever their
    variables are called."""
    import dis
    code = fn.__code__
    sig = []
    for ins in dis.get_instructions(code):
        if ins.opname in ("LOAD_DEREF", "LOAD_CLOSURE", "LOAD_CLASSDEREF"):
            if ins.argval not in code.co_freevars:
                return None
            try:
                v = fn.__closure__[code.co_freevars.index(ins.argval)].cell_contents
            except ValueError:               # empty cell
                return None
            sig.append((ins.opname, role(v)))
        elif ins.opname == "LOAD_FAST":
            sig.append((ins.opname, ins.arg))
        elif ins.opname in ("LOAD_ATTR", "LOAD_METHOD", "LOAD_CONST", "LOAD_GLOBAL", "LOAD_NAME", "KW_NAMES"):
            sig.append((ins.opname, repr(ins.argval)))
        elif ins.opname in ("RESUME", "COPY_FREE_VARS", "NOP", "CACHE", "PRECALL"):
            continue
        else:
            sig.append((ins.opname, ins.arg))
    return tuple(sig)


def _closure_templates():
    """Signatures of the closure bodies `fused_from_closure` accepts, compiled by THIS interpreter: the reference's
    (diffusion.py:531-532 with keyword inputs, :446-447 without) and the same calls on directly captured objects."""
    class _Role:
        pass
    E, DEN, NET, D = _Role(), _Role(), _Role(), {}
    names = {id(E): "engine", id(DEN): "denoiser", id(NET): "network"}

    def role(v):
        return "kwargs" if isinstance(v, dict) else names.get(id(v))

    def engine_kw(input, sigma, c):
        return E.denoiser(E.model, input, sigma, c, **D)

    def engine_plain(input, sigma, c):
        return E.denoiser(E.model, input, sigma, c)

    def direct_kw(input, sigma, c):
        return DEN(NET, input, sigma, c, **D)

    def direct_plain(input, sigma, c):
        return DEN(NET, input, sigma, c)

    return {_closure_signature(f, role) for f in (engine_kw, engine_plain, direct_kw, direct_plain)}


_CLOSURE_TEMPLATES = _closure_templates()


def _closure_role(v):
    if isinstance(v, dict):
        return "kwargs"
    if isinstance(v, Denoiser):
        return "denoiser"
    if isinstance(v, OpenAIWrapper):
        return "network"
    if isinstance(getattr(v, "denoiser", None), Denoiser) and isinstance(getattr(v, "model", None), OpenAIWrapper):
        return "engine"
    return None


def fused_from_closure(fn) -> Optional[FusedDenoiser]:
    """Recover (denoiser, network, additional_model_inputs) from the closure that
    `DiffusionEngine.sample_video` / `sample` build around the plugin stack (diffusion.py:526-532,
    444-447):

        def denoiser(input, sigma, c):
            return self.denoiser(self.model, input, sigma, c, **additional_model_inputs)

    so that a YAML-only switch to `gcd_amd.sampling.EulerEDMSampler` reaches the fused hipGraph loop
    with no edit of the reference.  Accepted shapes: a plain 3-argument Python function whose cells
    hold either an engine object exposing `.denoiser` (a gcd_amd Denoiser) and `.model` (a gcd_amd
    OpenAIWrapper), or those two objects directly, plus at most one dict of keyword inputs; the
    body must be, bytecode for bytecode, that call (`_closure_templates`: the reference's form or the same call on
    directly captured objects) — a closure that does anything else is left on the generic path.  Brittle by
    design: any upstream edit of diffusion.py:526-532 falls back to the generic (slower, same results) path;
    `EulerEDMSampler.last_path` records which path ran.  Returns None when it does not match."""
    import types
    if os.environ.get("GCD_FUSE_CLOSURE", "1") == "0":
        return None
    if not isinstance(fn, types.FunctionType) or fn.__closure__ is None:
        return None
    code = fn.__code__
    if code.co_argcount != 3 or code.co_kwonlyargcount or (code.co_flags & 0x0C):   # *args / **kwargs
        return None
    if not set(code.co_names) <= {"denoiser", "model"}:
        return None
    # the BODY must be one of the two known forms, instruction for instruction: a closure with the same names
    # that scales its input, reorders arguments or post-processes the output stays on the generic path
    if _closure_signature(fn, _closure_role) not in _CLOSURE_TEMPLATES:
        return None
    den = net = extra = None
    for cell in fn.__closure__:
        try:
            v = cell.cell_contents
        except ValueError:                   # empty cell
            return None
        if isinstance(v, dict):
            if extra is not None:
                return None
            extra = v
        elif isinstance(v, Denoiser):
            den = v if den is None else den
        elif isinstance(v, OpenAIWrapper):
            net = v if net is None else net
        elif isinstance(getattr(v, "denoiser", None), Denoiser) and \
                isinstance(getattr(v, "model", None), OpenAIWrapper):
            den, net = v.denoiser, v.model
        else:
            return None
    if den is None or net is None:
        return None
    if not all(isinstance(k, str) for k in (extra or {})):
        return None
    return FusedDenoiser(den, net, **(extra or {}))


def _guider_scale(guider, T: int) -> torch.Tensor:
    """The per-frame guidance scale [T] the fused kernels index by n % T."""
    if type(guider) is VanillaCFG:
        return torch.full((T,), float(guider.scale))
    return guider.scale.reshape(-1)


def _stack_fusable(guider, denoiser, x, cond, uc) -> bool:
    """The conditions of the fused loops that do not depend on the sampler class: gcd_amd's own denoiser / scaling /
    wrapper / UNet, a guider the kernels implement, the three cond keys, whole clips of float32 latents on a GPU."""
    if not isinstance(denoiser, FusedDenoiser):
        return False
    if type(denoiser.denoiser) is not Denoiser or \
            not isinstance(denoiser.denoiser.scaling, VScalingWithEDMcNoise):
        return False
    net = denoiser.network
    if type(net) is not OpenAIWrapper or not isinstance(net.diffusion_model, VideoUNet):
        return False
    if type(guider) is LinearPredictionGuider:
        if guider.additional_cond_keys:
            return False
    elif type(guider) is not VanillaCFG:
        return False
    if not x.is_cuda or x.dtype != torch.float32:
        return False
    if set(cond.keys()) != {"vector", "crossattn", "concat"}:
        return False
    extra = set(denoiser.additional_model_inputs) - {"num_video_frames", "image_only_indicator"}
    T = denoiser.additional_model_inputs.get("num_video_frames")
    if extra or T is None or x.shape[0] % T:
        return False
    if type(guider) is LinearPredictionGuider and T != guider.num_frames:
        return False
    unet = net.diffusion_model
    return x.shape[1] + cond["concat"].shape[1] == unet.in_channels


class BaseDiffusionSampler:
    stage_kind = None          # the row family of gcd_amd.sampler_stages; None: no fused form

    def __init__(self, discretization_config, num_steps: Optional[int] = None, guider_config=None,
                 verbose: bool = False, device: str = "cuda"):
        self.num_steps = num_steps
        self.discretization = instantiate_from_config(discretization_config)
        self.guider = instantiate_from_config(default(guider_config, DEFAULT_GUIDER))
        self.verbose = verbose
        self.device = device
        self.use_graph = True      # fused path: replay one captured step per iteration
        self.last_path = None      # "fused" | "generic" (introspection for tests / bench)

    # -------------------------------------------------------------------------------------------
    def _can_fuse(self, denoiser, x, cond, uc) -> bool:
        return self.stage_kind is not None and _stack_fusable(self.guider, denoiser, x, cond, uc)

    def _fused_loop_class(self):
        return FusedStageLoop

    def _route(self, denoiser, x, cond, uc):
        """The FusedDenoiser to run the fused loop on (given, or recovered from the sample_video closure), or None for
        the generic path; sets `last_path` and says once per process that the generic path runs on a GPU."""
        if not isinstance(denoiser, FusedDenoiser):
            recovered = fused_from_closure(denoiser)
            if recovered is not None and self._can_fuse(recovered, x, cond, uc):
                denoiser = recovered
        if self._can_fuse(denoiser, x, cond, uc):
            self.last_path = "fused"
            return denoiser
        self.last_path = "generic"
        if not EulerEDMSampler._warned_generic and getattr(x, "is_cuda", False):
            # said ONCE per process: the generic path is correct but launches every step from Python (no hipGraph,
            # no fused guidance / Euler update) — a closure that upstream edited no longer matches fused_from_closure
            EulerEDMSampler._warned_generic = True
            import warnings
            warnings.warn(f"gcd_amd.sampling.{type(self).__name__}: the denoiser callable was not recognised as the "
                          "DiffusionEngine.sample_video closure (diffusion.py:526-532) or a FusedDenoiser; running "
                          "the generic per-step path instead of the fused hipGraph loop (see INTEGRATION.md §1)",
                          RuntimeWarning, stacklevel=3)
        return None

    def _call_fused(self, fd: FusedDenoiser, x, cond, uc, num_steps):
        loop = self._fused_loop_class()(self, fd, x, cond, uc, num_steps)
        try:
            with loop:
                for i in range(loop.num_launches):
                    loop.step(i)
        finally:
            loop.close()
        return loop.x

    def prepare_sampling_loop(self, x, cond, uc=None, num_steps=None):
        sigmas = self.discretization(self.num_steps if num_steps is None else num_steps,
                                     device=self.device)
        uc = default(uc, cond)
        x *= torch.sqrt(1.0 + sigmas[0] ** 2.0)          # in place, like sampling.py:54
        num_sigmas = len(sigmas)
        s_in = x.new_ones([x.shape[0]])
        return x, s_in, sigmas, num_sigmas, cond, uc

    def denoise(self, x, denoiser, sigma, cond, uc):
        denoised = denoiser(*self.guider.prepare_inputs(x, sigma, cond, uc))
        return self.guider(denoised, sigma)


class SingleStepDiffusionSampler(BaseDiffusionSampler):
    def sampler_step(self, sigma, next_sigma, denoiser, x, cond, uc, *args, **kwargs):
        raise NotImplementedError

    def euler_step(self, x, d, dt):
        return x + dt * d


class EDMSampler(SingleStepDiffusionSampler):
    def __init__(self, s_churn=0.0, s_tmin=0.0, s_tmax=float("inf"), s_noise=1.0, *args, **kwargs):
        super().__init__(*args, **kwargs)
        self.s_churn, self.s_tmin, self.s_tmax, self.s_noise = s_churn, s_tmin, s_tmax, s_noise
        self.noise_sampler = None  # None: torch.randn_like; a callable x -> noise replays the churn noise

    def possible_correction_step(self, euler_step, x, d, dt, next_sigma, denoiser, cond, uc):
        raise NotImplementedError

    def sampler_step(self, sigma, next_sigma, denoiser, x, cond, uc=None, gamma=0.0):
        sigma_hat = sigma * (gamma + 1.0)
        if gamma > 0:
            eps = (self.noise_sampler(x) if self.noise_sampler else torch.randn_like(x)) * self.s_noise
            x = x + eps * append_dims(sigma_hat ** 2 - sigma ** 2, x.ndim) ** 0.5
        denoised = self.denoise(x, denoiser, sigma_hat, cond, uc)
        d = (x - denoised) / append_dims(sigma_hat, x.ndim)          # to_d, sampling_utils.py:34-35
        dt = append_dims(next_sigma - sigma_hat, x.ndim)
        return self.possible_correction_step(self.euler_step(x, d, dt), x, d, dt, next_sigma,
                                             denoiser, cond, uc)

    # -------------------------------------------------------------------------------------------
    def __call__(self, denoiser, x, cond, uc=None, num_steps=None):
        fd = self._route(denoiser, x, cond, uc)
        if fd is not None:
            return self._call_fused(fd, x, cond, default(uc, cond), num_steps)
        x, s_in, sigmas, num_sigmas, cond, uc = self.prepare_sampling_loop(x, cond, uc, num_steps)
        gammas = [0.0] * (num_sigmas - 1)
        if self.s_churn > 0:              # host copies of the sigmas; with s_churn == 0 there is no device->host sync
            gammas = churn_gammas(self, sigmas.detach().cpu().tolist())
        for i in range(num_sigmas - 1):
            x = self.sampler_step(s_in * sigmas[i], s_in * sigmas[i + 1], denoiser, x, cond, uc, gammas[i])
        return x

    def _fused_loop_class(self):
        # plain Euler keeps its own loop and kernel (gcd_cfg_euler_step), call for call
        return FusedEulerLoop if self.stage_kind == "euler" and self.s_churn == 0 else FusedStageLoop


class AncestralSampler(SingleStepDiffusionSampler):
    def __init__(self, eta=1.0, s_noise=1.0, *args, **kwargs):
        super().__init__(*args, **kwargs)
        self.eta, self.s_noise = eta, s_noise
        self.noise_sampler = lambda x: torch.randn_like(x)

    def ancestral_euler_step(self, x, denoised, sigma, sigma_down):
        d = (x - denoised) / append_dims(sigma, x.ndim)
        dt = append_dims(sigma_down - sigma, x.ndim)
        return self.euler_step(x, d, dt)

    def ancestral_step(self, x, sigma, next_sigma, sigma_up):
        # both branches are evaluated: one noise tensor is drawn per step, also where sigma' = 0 discards it
        up = append_dims(sigma_up, x.ndim) if torch.is_tensor(sigma_up) else sigma_up
        noise = self.noise_sampler(x) if self.noise_sampler else torch.randn_like(x)     # None: torch.randn_like
        return torch.where(append_dims(next_sigma, x.ndim) > 0.0, x + noise * self.s_noise * up, x)

    def __call__(self, denoiser, x, cond, uc=None, num_steps=None):
        fd = self._route(denoiser, x, cond, uc)
        if fd is not None:
            return self._call_fused(fd, x, cond, default(uc, cond), num_steps)
        x, s_in, sigmas, num_sigmas, cond, uc = self.prepare_sampling_loop(x, cond, uc, num_steps)
        for i in range(num_sigmas - 1):
            x = self.sampler_step(s_in * sigmas[i], s_in * sigmas[i + 1], denoiser, x, cond, uc)
        return x


class FusedEulerLoop:
    """Device-resident EulerEDM loop: static buffers + one hipGraph replay per step.

    Step i computes, entirely in libgcd_amd kernels on a side stream:
        c_in, c_noise   <- sigma_i                         (gcd_edm_scalings)
        net             <- VideoUNet([x*c_in | concat] for [uc | c])   (engine.run, CFG batch 2*nx)
        x               <- Euler(CFG(denoiser affine(net)))            (gcd_cfg_euler_step)
    The first step runs eagerly (it also records the workspace placement), the second is captured
    into a hipGraph, later steps replay it; sigma is read from a 2-float device buffer refreshed by
    a device-to-device copy from the sigma table before each replay.
    """

    def __init__(self, sampler: "EDMSampler", fd: FusedDenoiser, x, cond, uc, num_steps=None):
        unet: VideoUNet = fd.network.diffusion_model
        self.eng = eng = unet.engine
        if eng.packed is None:
            eng.pack()
        self.T = T = fd.additional_model_inputs["num_video_frames"]
        ioi = fd.additional_model_inputs.get("image_only_indicator")
        self.dev = dev = x.device
        self.sigmas = sampler.discretization(
            sampler.num_steps if num_steps is None else num_steps,
            device=sampler.device).to(device=dev, dtype=torch.float32)
        self.num_steps = len(self.sigmas) - 1
        x *= torch.sqrt(1.0 + self.sigmas[0] ** 2.0)     # caller's tensor, like sampling.py:54
        nx = x.shape[0]
        N = 2 * nx
        f32 = dict(device=dev, dtype=torch.float32)
        # static buffers; batch order [uc | c] as in guiders.py:89-100
        self.x = x.detach().clone().contiguous()
        self.concat2 = torch.cat((uc["concat"], cond["concat"]), 0).to(**f32).contiguous()
        self.ctx2 = torch.cat((uc["crossattn"], cond["crossattn"]), 0).to(**f32).contiguous()
        self.y2 = torch.cat((uc["vector"], cond["vector"]), 0).to(**f32).contiguous()
        self.net_out = torch.empty(N, unet.out_channels, *x.shape[2:], **f32)
        self.c_in, self.c_noise = torch.empty(N, **f32), torch.empty(N, **f32)
        self.sig = torch.empty(2, **f32)
        self.scale = _guider_scale(sampler.guider, T).to(**f32).contiguous()
        self.alphas = eng.blend_alphas(ioi, N, T)
        self.use_graph = sampler.use_graph
        self.lib = _lib.load()
        self.graph = C.c_void_p()
        self.side = eng.side_stream(dev)       # one per (engine, device), reused across sampler calls
        self._ctx = None
        self._eager_done = 0
        self._keepalive = None

    # the side stream is current inside `with loop:` so that every launch lands on it
    def __enter__(self):
        self.side.wait_stream(torch.cuda.current_stream(self.dev))
        self._ctx = torch.cuda.stream(self.side)
        self._ctx.__enter__()
        return self

    def __exit__(self, *exc):
        self.side.synchronize()
        self._ctx.__exit__(*exc)
        self._ctx = None
        torch.cuda.current_stream(self.dev).wait_stream(self.side)
        return False

    def launch_step(self):
        ops.edm_scalings(self.sig, self.c_in, self.c_noise)
        self.eng.run(self.x, self.concat2, self.c_in, self.c_noise, self.ctx2, self.y2, self.T, None,
                     self.net_out, alphas=self.alphas)
        ops.cfg_euler_step(self.x, self.net_out, self.scale, self.sig, self.x, self.T)

    def step(self, i: int):
        """Run step i (sigma_i -> sigma_{i+1}); indices beyond the schedule wrap (benchmarking)."""
        k = i % self.num_steps
        self.sig.copy_(self.sigmas[k:k + 2])
        self._launch_or_replay()

    @property
    def num_launches(self) -> int:
        """Calls of `step` per clip."""
        return self.num_steps

    def _launch_or_replay(self):
        if not self.use_graph or self._eager_done < 1:
            self.launch_step()
            self._eager_done += 1
        elif not self.graph:
            _lib.check(self.lib.gcd_graph_begin_capture(self.side.cuda_stream), "graph capture")
            try:
                self.launch_step()
            finally:
                _lib.check(self.lib.gcd_graph_end_capture(self.side.cuda_stream, C.byref(self.graph)),
                           "graph instantiate")
            # the captured launches read the engine's cached cross-attention vectors: keep them alive
            # for the graph's lifetime even if another call replaces the engine's cache entry
            self._keepalive = self.eng.packed.get("ca_cache")
            _lib.check(self.lib.gcd_graph_launch(self.graph, self.side.cuda_stream), "graph launch")
        else:
            _lib.check(self.lib.gcd_graph_launch(self.graph, self.side.cuda_stream), "graph launch")

    def close(self):
        if self.graph:
            self.lib.gcd_graph_destroy(self.graph)
            self.graph = C.c_void_p()


class FusedStageLoop(FusedEulerLoop):
    """Device-resident loop of the whole sampler family: FusedEulerLoop's buffers, side stream and graph handling, with
    the step replaced by a STAGE (gcd_amd/sampler_stages.py):
        coef            <- row k of the stage table                       (device-to-device copy, before the replay)
        c_in, c_noise   <- coef[0]                                        (gcd_edm_scalings)
        net             <- VideoUNet([x*c_in | concat] for [uc | c])      (engine.run)
        x, h0, h1       <- row k applied to (x, CFG(denoiser affine(net)), h0, h1, noise)   (gcd_sampler_stage_f32)
    The first stage runs eagerly, the second is captured, every later stage of whatever kind replays that one graph (a
    linear chain).  A stage that consumes noise has its static `noise` buffer filled, eagerly on the side stream, before
    its launch; a draw the reference discards is still made, so the random streams of both paths stay aligned.  h0, h1
    and noise exist only when the table uses them."""

    def __init__(self, sampler, fd: FusedDenoiser, x, cond, uc, num_steps=None):
        super().__init__(sampler, fd, x, cond, uc, num_steps)
        rows, self.draws = stage_table(sampler, self.sigmas)
        self.num_stages = rows.shape[0]
        self.rows = rows.to(self.dev).contiguous()
        self.coef = torch.empty(_lib.SAMPLER_ROW, device=self.dev, dtype=torch.float32)
        self.noise_sampler = getattr(sampler, "noise_sampler", None)
        used = lambda *cols: bool((rows[:, list(cols)] != 0).any())      # noqa: E731
        self.h0 = torch.empty_like(self.x) if used(3, 6, 7) else None
        self.h1 = torch.empty_like(self.x) if used(4, 8, 9) else None
        self.noise = torch.empty_like(self.x) if used(5) else None
        _lib.load_sampler()        # a missing library is an error here, not at the first launch
        for stage, use, scale in self.draws:
            if stage < 0:          # churn on step 0: x_hat before the first stage (sampling.py:102-105)
                self.x += self._draw() * scale

    def _draw(self):
        return self.noise_sampler(self.x) if self.noise_sampler else torch.randn_like(self.x)

    @property
    def num_launches(self) -> int:
        return self.num_stages

    def launch_step(self):
        ops.edm_scalings(self.coef, self.c_in, self.c_noise)
        self.eng.run(self.x, self.concat2, self.c_in, self.c_noise, self.ctx2, self.y2, self.T, None,
                     self.net_out, alphas=self.alphas)
        sampler_ops.sampler_stage(self.x, self.net_out, self.scale, self.coef, self.T, self.h0, self.h1, self.noise)

    def step(self, i: int):
        """Run stage i of the table; indices beyond it wrap (benchmarking)."""
        k = i % self.num_stages
        for stage, use, _ in self.draws:
            if stage == k:
                z = self._draw()
                if use:
                    self.noise.copy_(z)
        self.coef.copy_(self.rows[k])
        self._launch_or_replay()


class EulerEDMSampler(EDMSampler):
    """Deterministic Euler steps, no correction (sampling.py:225-230)."""
    _warned_generic = False    # the generic-path notice is given once per process
    stage_kind = "euler"

    def possible_correction_step(self, euler_step, x, d, dt, next_sigma, denoiser, cond, uc):
        return euler_step


class HeunEDMSampler(EDMSampler):
    """Euler predictor, trapezoidal corrector: two network evaluations per step, one on the last (sampling.py:233-249)."""
    stage_kind = "heun"

    def possible_correction_step(self, euler_step, x, d, dt, next_sigma, denoiser, cond, uc):
        if torch.sum(next_sigma) < ZERO_SIGMA:
            return euler_step            # save a network evaluation if all noise levels are 0
        denoised = self.denoise(euler_step, denoiser, next_sigma, cond, uc)
        d_new = (euler_step - denoised) / append_dims(next_sigma, x.ndim)
        d_prime = (d + d_new) / 2.0
        return torch.where(append_dims(next_sigma, x.ndim) > 0.0, x + d_prime * dt, euler_step)


class EulerAncestralSampler(AncestralSampler):
    """sampling.py:252-259."""
    stage_kind = "euler_ancestral"

    def sampler_step(self, sigma, next_sigma, denoiser, x, cond, uc):
        sigma_down, sigma_up = get_ancestral_step(sigma, next_sigma, eta=self.eta)
        denoised = self.denoise(x, denoiser, sigma, cond, uc)
        x = self.ancestral_euler_step(x, denoised, sigma, sigma_down)
        return self.ancestral_step(x, sigma, next_sigma, sigma_up)


class DPMPP2SAncestralSampler(AncestralSampler):
    """sampling.py:262-299."""
    stage_kind = "dpmpp2s_ancestral"

    def get_variables(self, sigma, sigma_down):
        t, t_next = [to_neg_log_sigma(s) for s in (sigma, sigma_down)]
        h = t_next - t
        s = t + 0.5 * h
        return h, s, t, t_next

    def get_mult(self, h, s, t, t_next):
        mult1 = to_sigma(s) / to_sigma(t)
        mult2 = (-0.5 * h).expm1()
        mult3 = to_sigma(t_next) / to_sigma(t)
        mult4 = (-h).expm1()
        return mult1, mult2, mult3, mult4

    def sampler_step(self, sigma, next_sigma, denoiser, x, cond, uc=None, **kwargs):
        sigma_down, sigma_up = get_ancestral_step(sigma, next_sigma, eta=self.eta)
        denoised = self.denoise(x, denoiser, sigma, cond, uc)
        x_euler = self.ancestral_euler_step(x, denoised, sigma, sigma_down)
        if torch.sum(sigma_down) < ZERO_SIGMA:
            x = x_euler                  # save a network evaluation if all noise levels are 0
        else:
            h, s, t, t_next = self.get_variables(sigma, sigma_down)
            mult = [append_dims(m, x.ndim) for m in self.get_mult(h, s, t, t_next)]
            x2 = mult[0] * x - mult[1] * denoised
            denoised2 = self.denoise(x2, denoiser, to_sigma(s), cond, uc)
            x_dpmpp2s = mult[2] * x - mult[3] * denoised2
            x = torch.where(append_dims(sigma_down, x.ndim) > 0.0, x_dpmpp2s, x_euler)
        return self.ancestral_step(x, sigma, next_sigma, sigma_up)


class DPMPP2MSampler(BaseDiffusionSampler):
    """Second-order multistep, one network evaluation per step (sampling.py:302-377)."""
    stage_kind = "dpmpp2m"

    def get_variables(self, sigma, next_sigma, previous_sigma=None):
        t, t_next = [to_neg_log_sigma(s) for s in (sigma, next_sigma)]
        h = t_next - t
        if previous_sigma is not None:
            h_last = t - to_neg_log_sigma(previous_sigma)
            r = h_last / h
            return h, r, t, t_next
        return h, None, t, t_next

    def get_mult(self, h, r, t, t_next, previous_sigma):
        mult1 = to_sigma(t_next) / to_sigma(t)
        mult2 = (-h).expm1()
        if previous_sigma is not None:
            mult3 = 1 + 1 / (2 * r)
            mult4 = 1 / (2 * r)
            return mult1, mult2, mult3, mult4
        return mult1, mult2

    def sampler_step(self, old_denoised, previous_sigma, sigma, next_sigma, denoiser, x, cond, uc=None):
        denoised = self.denoise(x, denoiser, sigma, cond, uc)
        h, r, t, t_next = self.get_variables(sigma, next_sigma, previous_sigma)
        mult = [append_dims(m, x.ndim) for m in self.get_mult(h, r, t, t_next, previous_sigma)]
        x_standard = mult[0] * x - mult[1] * denoised
        if old_denoised is None or torch.sum(next_sigma) < ZERO_SIGMA:
            return x_standard, denoised  # first step, or all noise levels are 0
        denoised_d = mult[2] * denoised - mult[3] * old_denoised
        x_advanced = mult[0] * x - mult[1] * denoised_d
        return torch.where(append_dims(next_sigma, x.ndim) > 0.0, x_advanced, x_standard), denoised

    def __call__(self, denoiser, x, cond, uc=None, num_steps=None, **kwargs):
        fd = self._route(denoiser, x, cond, uc)
        if fd is not None:
            return self._call_fused(fd, x, cond, default(uc, cond), num_steps)
        x, s_in, sigmas, num_sigmas, cond, uc = self.prepare_sampling_loop(x, cond, uc, num_steps)
        old_denoised = None
        for i in range(num_sigmas - 1):
            x, old_denoised = self.sampler_step(old_denoised, None if i == 0 else s_in * sigmas[i - 1],
                                                s_in * sigmas[i], s_in * sigmas[i + 1], denoiser, x, cond, uc=uc)
        return x
