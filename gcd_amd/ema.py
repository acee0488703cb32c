"""Exponential moving average of the trainable weights: drop-in for `sgm.modules.ema.LitEma` (ema.py:5-86), and the host
side of the device tables of include/gcd_amd_train_optim.h.

Reference: `DiffusionEngine(use_ema=..., ema_decay_rate=...)` keeps `self.model_ema = LitEma(self.model, decay=...)`, calls
`self.model_ema(self.model)` in `on_train_batch_end` (diffusion.py:383-385) and validates / samples inside `ema_scope`
(diffusion.py:388-403: store, copy_to, ..., restore).  Here:

  * `LitEma`: the same constructor, the same buffers (`decay`, `num_updates`, one shadow per trainable parameter named by the
    parameter's name with the dots removed — a reference checkpoint's `model_ema.*` keys load unchanged) and methods.
    `forward(model)` is ONE pass of `gcd_ema_update` over every shadow, not a Python loop over ~1430 tensors;
  * `AdamHIP(..., ema=lit_ema)` (training.py) makes the optimizer's fused update pass own the EMA: do not call
    `forward(model)` as well;
  * `ema_scope(model, ema)`: the reference's context manager.

`copy_to` and `restore` write the parameters through `.data`, which torch's version counters do not see: both drop every
packed operand form that was made from the old values (the network's `invalidate()`, `autograd_ops.PACK.clear()`).
"""
from __future__ import annotations

import contextlib
import ctypes as C
import weakref
from typing import Iterable, List, Optional, Sequence, Tuple

import torch
from torch import nn

from . import _lib
from ._lib import GcdError


class DeviceTable:
    """The device table of `gcd_optim_tensor` entries: built once, rebuilt only when a pointer (or an element count) in it
    changes, never inside a stream capture."""

    def __init__(self, what: str):
        self.what = what
        self.key: Optional[tuple] = None
        self.dev: Optional[torch.Tensor] = None
        self.count = 0
        self.chunks = 0
        self.rebuilds = 0

    def reset(self) -> None:
        self.key = None

    def update(self, rows: Sequence[Tuple[int, int, int, int, int, int]], device) -> bool:
        """rows: (p, g, m, v, ema, numel) as addresses, 0 = absent.  Returns True when the table was rebuilt."""
        key = tuple(rows)
        if key == self.key and self.dev is not None and self.dev.device == device:
            return False
        # a rebuild copies a host table to the device: not something a stream capture can hold
        if device.type == "cuda" and torch.cuda.is_current_stream_capturing():
            raise RuntimeError(f"{self.what}: the tensor table would be rebuilt inside a stream capture (a parameter, "
                               "gradient, moment or shadow address differs from the step before the capture)")
        live = [r for r in key if r[5] > 0]
        if not live:
            raise GcdError(f"{self.what}: no tensor to work on")
        arr = (_lib.OptimTensor * len(live))()
        chunk0 = 0
        for e, (p, g, m, v, ema, n) in zip(arr, live):
            e.p, e.g, e.m, e.v, e.ema, e.n, e.chunk0 = p or None, g or None, m or None, v or None, ema or None, n, chunk0
            chunk0 += -(-n // _lib.OPTIM_CHUNK)
        self.dev = torch.frombuffer(bytearray(bytes(arr)), dtype=torch.uint8).to(device)
        self.key, self.count, self.chunks = key, len(live), chunk0
        self.rebuilds += 1
        return True


def new_state_block(device, **fields) -> torch.Tensor:
    """A `gcd_optim_state` in device memory as a 16-element int32 tensor (view it as float32 for the fp32 fields)."""
    st = _lib.OptimState()
    st.loss_scale = 1.0
    for k, v in fields.items():
        setattr(st, k, v)
    return torch.frombuffer(bytearray(bytes(st)), dtype=torch.int32).to(device)


def read_state_block(block: torch.Tensor) -> "_lib.OptimState":
    """The one synchronising read of a state block."""
    return _lib.OptimState.from_buffer_copy(block.detach().cpu().numpy().tobytes())


def invalidate_packed(model: Optional[nn.Module]) -> None:
    """After writing parameters through `.data`: drop the packed fp16 / bf16 operand forms made from the old values."""
    from . import autograd_ops as A
    if model is not None:
        for mod in model.modules():
            inv = getattr(mod, "invalidate", None)
            if callable(inv):
                inv()
    A.PACK.clear()


class LitEma(nn.Module):
    def __init__(self, model, decay=0.9999, use_num_upates=True):
        super().__init__()
        if decay < 0.0 or decay > 1.0:
            raise ValueError("Decay must be between 0 and 1")
        self.m_name2s_name = {}
        trainable = [(n, p) for n, p in model.named_parameters() if p.requires_grad]
        # (the reference makes these two on the CPU and lets Lightning move the module; here they are made where the
        #  weights live, because the kernels advance `num_updates` on the device)
        dev = trainable[0][1].device if trainable else torch.device("cpu")
        self.register_buffer("decay", torch.tensor(decay, dtype=torch.float32, device=dev))
        self.register_buffer("num_updates", torch.tensor(0 if use_num_upates else -1, dtype=torch.int, device=dev))
        self._by_id = {}
        for name, p in trainable:
            s_name = name.replace(".", "")       # '.' is not allowed in buffer names
            self.m_name2s_name.update({name: s_name})
            self.register_buffer(s_name, p.clone().detach().data)
            self._by_id[id(p)] = (weakref.ref(p), s_name)
        self.collected_params = []
        self._model = weakref.ref(model)
        self._table = DeviceTable("LitEma")
        self._state: Optional[torch.Tensor] = None
        self._cfg = _lib.OptimConfig()
        self._decay_seen: Optional[tuple] = None

    # -- what AdamHIP(ema=...) needs -------------------------------------------------------------------------------------
    def shadow_of(self, p: torch.Tensor) -> Optional[torch.Tensor]:
        """The shadow buffer of parameter `p` (matched by identity), or None when `p` is not one of the EMA'd module's."""
        hit = self._by_id.get(id(p))
        if hit is None or hit[0]() is not p:
            return None
        return self._buffers[hit[1]]

    def decay_value(self) -> float:
        """`decay` as a host float: read from the device when the buffer has changed (construction, load_state_dict)."""
        seen = (self.decay.data_ptr(), self.decay._version)
        if self._decay_seen is None or self._decay_seen[0] != seen:
            self._decay_seen = (seen, float(self.decay))
        return self._decay_seen[1]

    def fill_config(self, cfg: "_lib.OptimConfig", device) -> None:
        if self.num_updates.device != device or self.num_updates.dtype != torch.int32:
            raise GcdError(f"LitEma: num_updates must be an int32 tensor on {device} (it is {self.num_updates.dtype} on "
                           f"{self.num_updates.device}): move the module with .to(device)")
        cfg.use_ema = 1
        cfg.ema_decay = self.decay_value()
        cfg.ema_count = self.num_updates.data_ptr()

    # -- the reference's methods ------------------------------------------------------------------------------------------
    def reset_num_updates(self):
        del self.num_updates
        self.register_buffer("num_updates", torch.tensor(0, dtype=torch.int, device=self.decay.device))

    @torch.no_grad()
    def forward(self, model):
        rows, dev = [], None
        for key, p in model.named_parameters():
            if not p.requires_grad:
                assert key not in self.m_name2s_name
                continue
            s = self._buffers[self.m_name2s_name[key]]
            if p.dtype != torch.float32 or s.dtype != torch.float32 or not p.is_contiguous() or not s.is_contiguous():
                raise GcdError(f"LitEma: parameter {key} and its shadow must be contiguous fp32")
            if s.device != p.device or s.shape != p.shape:
                raise GcdError(f"LitEma: the shadow of {key} is {tuple(s.shape)} on {s.device}, the parameter "
                               f"{tuple(p.shape)} on {p.device}")
            dev = p.device
            rows.append((p.data_ptr(), 0, 0, 0, s.data_ptr(), p.numel()))
        if dev is None:
            return
        if dev.type != "cuda":
            raise GcdError("LitEma.forward runs gcd_ema_update on the GPU; gcd_amd has no CPU fallback")
        self._table.update(rows, dev)
        if self._state is None or self._state.device != dev:
            self._state = new_state_block(dev)
        self.fill_config(self._cfg, dev)
        lib = _lib.load_train()
        _lib.check_train(lib.gcd_ema_update(self._table.dev.data_ptr(), self._table.count, self._table.chunks,
                                            C.byref(self._cfg), self._state.data_ptr(),
                                            torch.cuda.current_stream().cuda_stream), "gcd_ema_update")

    def copy_to(self, model):
        m_param = dict(model.named_parameters())
        shadow_params = dict(self.named_buffers())
        for key in m_param:
            if m_param[key].requires_grad:
                m_param[key].data.copy_(shadow_params[self.m_name2s_name[key]].data)
            else:
                assert key not in self.m_name2s_name
        self._model = weakref.ref(model)
        invalidate_packed(model)

    def store(self, parameters):
        """Save the current parameters for restoring later."""
        self.collected_params = [param.clone() for param in parameters]

    def restore(self, parameters):
        """Restore the parameters stored with `store` (after validating / saving with the EMA weights)."""
        for c_param, param in zip(self.collected_params, parameters):
            param.data.copy_(c_param.data)
        invalidate_packed(self._model())


@contextlib.contextmanager
def ema_scope(model: nn.Module, ema: Optional[LitEma]):
    """`DiffusionEngine.ema_scope` (diffusion.py:388-403): run the block on the EMA weights, then put the training weights
    back.  `ema=None` (use_ema off) runs the block on the weights as they are."""
    if ema is not None:
        ema.store(model.parameters())
        ema.copy_to(model)
    try:
        yield None
    finally:
        if ema is not None:
            ema.restore(model.parameters())
