"""LoRA fine-tuning of the temporal Linears by merged weights: the reference's `ft_strategy="time_lora"`
(sgm/models/diffusion.py:134-155) without peft, and `apply_ft_strategy` for the reference's four strategies.

The engines never see an adapter.  The fp32 weight tensor of an adapted Linear — the tensor both training engines and the
inference engine already read — holds the merged W = W0 + s B A (A [r, K], B [N, r], s = alpha / r); `TimeLora` keeps the
frozen W0 as a copy.  The adapted weights keep `requires_grad=True`, so the engines compute their ordinary gradient dW;
every other parameter of the network is frozen (the adapted Linears' biases too, as peft leaves them).  The adapter
gradients are the chain rule through the merge, dB = s dW A^T and dA = s B^T dW, which is what autograd gives peft's
two-branch forward.  One step:

    loss.backward()           # dW of the adapted weights (p.grad)
    lora.project_grads()      # gcd_lora_project: dW -> A.grad, B.grad (a weight the graph never reached: zeros)
    optimizer.step()          # over lora.parameters() only
    lora.merge()              # gcd_lora_merge: W = W0 + s B A in place; both engines drop their 16-bit forms

or `lora.step(optimizer)` for the last three.  Both kernels are grouped launches of libgcd_amd_lora.so
(include/gcd_amd_lora.h); there is no other path: without a GPU `merge()` and `project_grads()` raise GcdError."""
from __future__ import annotations

import ctypes as C
import math
from typing import Dict, Iterator, List, Optional, Tuple

import torch
from torch import nn

from . import _lib_lora
from ._lib import GcdError

FT_STRATEGIES = ("everything", "time", "time_lora", "dummy")
DUMMY_PARAM = "output_blocks.11.1.time_mixer.mix_factor"          # diffusion.py:161


def adaptable_layers(unet: nn.Module) -> Iterator[Tuple[str, nn.Linear]]:
    """The reference's walk (diffusion.py:137-151): every nn.Linear with "time" in its own (child) name or in its parent's
    qualified name, as (qualified name, module), in the walk's order."""
    for parent_name, parent in unet.named_modules():
        for name, module in parent.named_children():
            if ("time" in name or "time" in parent_name) and isinstance(module, nn.Linear):
                yield (f"{parent_name}.{name}" if parent_name else name), module


def _drop_plan(unet: nn.Module) -> None:
    """The planned engine lays its flat gradient buffer out from the requires_grad flags: a cached plan is stale."""
    unet.__dict__.pop("_gcd_train_plan", None)


def _invalidate(unet: nn.Module) -> None:
    """The weights were written through raw pointers: the inference engine's packed weights and the training engines'
    16-bit operand forms were made from the old values."""
    from . import autograd_ops as A
    inv = getattr(unet, "invalidate", None)
    if callable(inv):
        inv()
    A.PACK.clear()


class TimeLora(nn.Module):
    """The rank-r adapters of a VideoUNet's temporal Linears.  `unet` is a plain attribute, not a sub-module: this module's
    parameters are the adapters alone (what the optimizer and `LitEma(lora)` get), and `unet.parameters()` /
    `unet.state_dict()` keep their names.

    Initialisation follows peft's lora.Linear(base, "default", r): B = 0, A = kaiming_uniform_(a = sqrt 5), i.e.
    U(-1 / sqrt K, 1 / sqrt K), and lora_alpha = 1, so s = 1 / r."""

    def __init__(self, unet: nn.Module, r: int = 16, alpha: float = 1.0, generator: Optional[torch.Generator] = None):
        super().__init__()
        if not 1 <= int(r) <= _lib_lora.LORA_MAX_RANK:
            raise ValueError(f"TimeLora: r = {r} outside 1 .. {_lib_lora.LORA_MAX_RANK}")
        object.__setattr__(self, "unet", unet)
        self.r, self.alpha, self.scale = int(r), float(alpha), float(alpha) / int(r)
        layers = list(adaptable_layers(unet))
        if not layers:
            raise ValueError("TimeLora: the network has no Linear with 'time' in its name")
        if len(layers) > _lib_lora.LORA_MAX_ENTRIES:
            raise ValueError(f"TimeLora: {len(layers)} layers, at most {_lib_lora.LORA_MAX_ENTRIES}")
        self.names: List[str] = [n for n, _ in layers]
        object.__setattr__(self, "_layers", [m for _, m in layers])
        self.lora_A = nn.ParameterList()
        self.lora_B = nn.ParameterList()
        for i, (_, m) in enumerate(layers):
            w = m.weight
            N, K = w.shape
            if w.dtype != torch.float32 or not w.is_contiguous():
                raise GcdError(f"TimeLora: {self.names[i]}.weight must be contiguous fp32")
            if w.device.type == "meta":
                a = torch.empty(self.r, K, dtype=torch.float32, device="meta")
            else:
                bound = 1.0 / math.sqrt(K)
                a = torch.empty(self.r, K, dtype=torch.float32).uniform_(-bound, bound, generator=generator).to(w.device)
            self.lora_A.append(nn.Parameter(a))
            self.lora_B.append(nn.Parameter(torch.zeros(N, self.r, dtype=torch.float32, device=w.device)))
        self._flags: Optional[Dict[str, bool]] = None
        self._table = None            # (addresses, gradient addresses, device bytes, merge tiles, project tiles)
        self._scratch: Optional[torch.Tensor] = None
        self._merged: Optional[tuple] = None
        self.attach()

    # ------------------------------------------------------------------------------------------------------------ state
    @property
    def attached(self) -> bool:
        return self._flags is not None

    def weights(self) -> List[nn.Parameter]:
        """The adapted (live, merged) weight tensors, in layer order."""
        return [m.weight for m in self._layers]

    def w0(self) -> List[torch.Tensor]:
        return [self._buffers[f"w0_{i}"] for i in range(len(self.names))]

    def _versions(self) -> tuple:
        return tuple(p._version for p in (*self.lora_A, *self.lora_B))

    def attach(self) -> None:
        """Copy W0, freeze everything but the adapted weights, drop a cached training plan, merge."""
        if self.attached:
            raise GcdError("TimeLora: already attached")
        unet = self.unet
        for i, m in enumerate(self._layers):
            self.register_buffer(f"w0_{i}", m.weight.detach().clone(), persistent=False)
        self._flags = {n: p.requires_grad for n, p in unet.named_parameters()}
        unet.requires_grad_(False)
        for m in self._layers:
            m.weight.requires_grad_(True)
        _drop_plan(unet)
        if self._device().type == "cuda":
            self.merge()
        else:
            # no kernel without a GPU.  The one state that needs none: B == 0, where the merge is W0's own bits and the
            # weights already hold them.  Anything else has to merge() on the device.
            if not all(b.device.type == "meta" or not bool(b.detach().any()) for b in self.lora_B):
                raise GcdError("TimeLora: attaching adapters with B != 0 needs the network on a GPU")
            self._merged = self._versions()

    def unmerge(self) -> None:
        """Detach: the weights get W0 back bit for bit, the requires_grad flags are what they were before `attach`."""
        if not self.attached:
            raise GcdError("TimeLora: not attached")
        with torch.no_grad():
            for m, w0 in zip(self._layers, self.w0()):
                m.weight.data.copy_(w0)
                m.weight.grad = None
        for n, p in self.unet.named_parameters():
            p.requires_grad_(self._flags[n])
        self._flags, self._merged = None, None
        for i in range(len(self.names)):
            del self._buffers[f"w0_{i}"]
        _drop_plan(self.unet)
        _invalidate(self.unet)

    def _device(self) -> torch.device:
        return self._layers[0].weight.device

    # ---------------------------------------------------------------------------------------------------------- kernels
    def _need_gpu(self, what: str) -> torch.device:
        if not self.attached:
            raise GcdError(f"TimeLora.{what}: not attached")
        dev = self._device()
        if dev.type != "cuda":
            raise GcdError(f"TimeLora.{what} runs on the GPU (the network is on {dev}): gcd_amd has no CPU fallback")
        if torch.cuda.is_current_stream_capturing():
            raise GcdError(f"TimeLora.{what} may not run inside a stream capture")
        return dev

    def _device_table(self, dev: torch.device, need_grads: bool):
        """The table of gcd_lora_entry on the device, rebuilt (one host-to-device copy) only when an address in it changes;
        the merge reads no gradient field and takes the cached table whatever those hold."""
        base, grads = [], []
        for m, w0, a, b in zip(self._layers, self.w0(), self.lora_A, self.lora_B):
            w = m.weight
            g = w.grad
            if need_grads and g is not None and (g.dtype != torch.float32 or not g.is_contiguous() or g.device != dev
                                                 or g.shape != w.shape):
                raise GcdError(f"TimeLora.project_grads needs contiguous fp32 weight gradients on {dev}, got {g.dtype}, "
                               f"strides {g.stride()}, on {g.device}")
            base.append((w0.data_ptr(), w.data_ptr(), a.data_ptr(), b.data_ptr(), w.shape[0], w.shape[1]))
            grads.append((0 if g is None else g.data_ptr(), 0 if a.grad is None else a.grad.data_ptr(),
                          0 if b.grad is None else b.grad.data_ptr()))
        base_key, grad_key = (str(dev), self.scale, tuple(base)), tuple(grads)
        if self._table is not None and self._table[0] == base_key and (not need_grads or self._table[1] == grad_key):
            return self._table
        if torch.cuda.is_current_stream_capturing():
            raise GcdError("TimeLora: the layer table would be rebuilt inside a stream capture")
        # (every operand is looked at here, where an address changed, not on every call: a tensor that moved or changed
        #  its type has another address)
        for t in (*self.weights(), *self.w0(), *self.lora_A, *self.lora_B):
            if t.device != dev:
                raise GcdError(f"TimeLora: an operand is on {t.device}, the network on {dev}")
            if t.dtype != torch.float32 or not t.is_contiguous():
                raise GcdError("TimeLora: every operand must be contiguous fp32")
        arr = (_lib_lora.LoraEntry * len(base))()
        for e, (w0, w, a, b, N, K), (dw, da, db) in zip(arr, base, grads):
            e.W0, e.W, e.A, e.B, e.dW, e.dA, e.dB = w0, w, a, b, dw or None, da or None, db or None
            e.N, e.K, e.r, e.scale = N, K, self.r, self.scale
        mt, pt, sf = _lib_lora.fill_table(arr)
        tab = torch.frombuffer(bytearray(bytes(arr)), dtype=torch.uint8).to(dev)
        if self._scratch is None or self._scratch.numel() < sf or self._scratch.device != dev:
            self._scratch = torch.empty(sf, dtype=torch.float32, device=dev)
        self._table = (base_key, grad_key, tab, mt, pt)
        return self._table

    @torch.no_grad()
    def merge(self) -> None:
        """W = W0 + s B A for every adapted layer (one launch), then both engines drop what they packed from the old W."""
        dev = self._need_gpu("merge")
        _, _, tab, mt, _ = self._device_table(dev, need_grads=False)
        lib = _lib_lora.load()
        _lib_lora.check(lib.gcd_lora_merge(tab.data_ptr(), len(self.names), mt, torch.cuda.current_stream().cuda_stream),
                        "gcd_lora_merge")
        _invalidate(self.unet)
        self._merged = self._versions()

    @torch.no_grad()
    def project_grads(self) -> None:
        """A.grad = s B^T dW and B.grad = s dW A^T from the adapted weights' .grad, which may have been accumulated over
        several backward passes; a weight whose .grad is None (the graph never reached it) counts as dW = 0.  The adapters'
        .grad are OVERWRITTEN: the projection is linear, so projecting the accumulated dW once is the accumulated
        gradient.  Raises when A or B have changed since the last merge(): dW would belong to other weights."""
        dev = self._need_gpu("project_grads")
        if self._merged != self._versions():
            raise GcdError("TimeLora.project_grads: A or B have changed since the last merge(); the live weights, and with "
                           "them dW, belong to the old adapters — call merge() after every optimizer step")
        for p in (*self.lora_A, *self.lora_B):
            if p.grad is None:
                p.grad = torch.empty_like(p)
            elif p.grad.dtype != torch.float32 or not p.grad.is_contiguous() or p.grad.device != dev:
                raise GcdError("TimeLora.project_grads: an adapter holds a .grad that is not contiguous fp32 on its device")
        _, _, tab, _, pt = self._device_table(dev, need_grads=True)
        lib = _lib_lora.load()
        _lib_lora.check(lib.gcd_lora_project(tab.data_ptr(), len(self.names), pt, self.r, self._scratch.data_ptr(),
                                             self._scratch.numel(), torch.cuda.current_stream().cuda_stream),
                        "gcd_lora_project")

    def zero_grad(self, set_to_none: bool = True) -> None:
        """The adapters' gradients, as nn.Module.zero_grad does (None, or zeros in place), and the adapted weights' dW, which
        the next backward pass would otherwise add to: always None — the planned engine takes a live .grad for an
        accumulation window."""
        super().zero_grad(set_to_none=set_to_none)
        for w in self.weights():
            w.grad = None

    def step(self, optimizer, *args, **kwargs) -> None:
        """project -> optimizer.step(*args, **kwargs) -> merge; dW is consumed (the weights' .grad are set to None)."""
        self.project_grads()
        optimizer.step(*args, **kwargs)
        self._merged = None           # the optimizer may write through raw pointers, which no version counter sees
        for w in self.weights():
            w.grad = None
        self.merge()

    # ------------------------------------------------------------------------------------- the reference's checkpoints
    def reference_state_dict(self) -> Dict[str, torch.Tensor]:
        """The network's state dict under the names of the reference's checkpoint of a network holding peft layers:
        <layer>.base_layer.weight | bias, <layer>.lora_A.default.weight, <layer>.lora_B.default.weight, every other key
        unchanged.  base_layer.weight is W0, not the merged weight."""
        if not self.attached:
            raise GcdError("TimeLora.reference_state_dict: not attached")
        out: Dict[str, torch.Tensor] = {}
        w0 = dict(zip(self.names, self.w0()))
        adapted = set(self.names)
        for k, v in self.unet.state_dict().items():
            layer, _, leaf = k.rpartition(".")
            if layer in adapted:
                out[f"{layer}.base_layer.{leaf}"] = (w0[layer] if leaf == "weight" else v).detach()
            else:
                out[k] = v.detach()
        for n, a, b in zip(self.names, self.lora_A, self.lora_B):
            out[f"{n}.lora_A.default.weight"] = a.detach()
            out[f"{n}.lora_B.default.weight"] = b.detach()
        return out

    @torch.no_grad()
    def load_reference_state_dict(self, sd: Dict[str, torch.Tensor], merge: bool = True) -> None:
        """The inverse: W0, the adapters and every other tensor of the network from a reference checkpoint's names, then
        merge().  merge=False leaves the weights holding W0 and the adapters unmerged (loading without a GPU):
        project_grads() refuses until merge() has run."""
        if not self.attached:
            raise GcdError("TimeLora.load_reference_state_dict: not attached")
        want = set(self.reference_state_dict())
        if set(sd) != want:
            missing, extra = sorted(want - set(sd)), sorted(set(sd) - want)
            raise KeyError(f"load_reference_state_dict: missing {missing[:4]}{'...' if len(missing) > 4 else ''}, "
                           f"unexpected {extra[:4]}{'...' if len(extra) > 4 else ''}")
        adapted = set(self.names)
        plain = {}
        for k, v in sd.items():
            head, _, leaf = k.rpartition(".")
            if head.endswith(".base_layer") and head[:-len(".base_layer")] in adapted:
                plain[f"{head[:-len('.base_layer')]}.{leaf}"] = v
            elif not (k.endswith(".lora_A.default.weight") or k.endswith(".lora_B.default.weight")):
                plain[k] = v
        flags = {n: p.requires_grad for n, p in self.unet.named_parameters()}
        self.unet.load_state_dict(plain)              # (its post hook invalidates the inference engine)
        for n, p in self.unet.named_parameters():
            p.requires_grad_(flags[n])
        for n, m, w0, a, b in zip(self.names, self._layers, self.w0(), self.lora_A, self.lora_B):
            w0.copy_(m.weight)
            a.copy_(sd[f"{n}.lora_A.default.weight"])
            b.copy_(sd[f"{n}.lora_B.default.weight"])
        if merge:
            self.merge()
        else:
            from . import autograd_ops as A
            A.PACK.clear()


def apply_ft_strategy(unet: nn.Module, strategy: str, **kw) -> Optional[TimeLora]:
    """The reference's `ft_strategy` (diffusion.py:127-170) on a VideoUNet: `everything` leaves every flag alone, `time`
    freezes every parameter without "time" in its name, `dummy` all but DUMMY_PARAM, `time_lora` attaches and returns a
    `TimeLora(unet, **kw)` (the optimizer then gets ITS parameters).  The other three return None."""
    if strategy not in FT_STRATEGIES:
        raise NotImplementedError(f"ft_strategy {strategy!r}: one of {FT_STRATEGIES}")
    if strategy == "time_lora":
        return TimeLora(unet, **kw)
    if kw:
        raise TypeError(f"ft_strategy {strategy!r} takes no options, got {sorted(kw)}")
    if strategy in ("time", "dummy"):
        key = "time" if strategy == "time" else DUMMY_PARAM
        for name, p in unet.named_parameters():
            if key not in name:
                p.requires_grad_(False)
        _drop_plan(unet)
    return None
