"""The memory contract (tests/memcontract.py; DESIGN.md "Memory contract") of the three launching entries of
libgcd_amd_loss.so: operands are views in guarded allocations, outputs start as zeros in one run and as a NaN bit pattern
in the other (guards too), the two runs are bit-identical, every payload element is written, no guard is touched, a null
`wmap` is honoured, and the clean run meets the bar of the entry's own test (tests/test_loss_device_gpu.py: 1e-6 absolute
for the map, 2e-6 for the loss and its gradient against the fp64 oracle; equality for the saved (tau, quota)).  The
library has no scratch operand and no optional destination, and nothing reduces with floating-point atomics, so there is
no bit-equality waiver."""
import pytest
import torch

import memcontract as mc
from oracle import loss_ref as R
from oracle.make_golden_loss import pd_semantic_frames

pytestmark = pytest.mark.gpu
F32, F64, I32 = torch.float32, torch.float64, torch.int32
EQUAL = ("maxabs", 1e-30)          # the harness compares with <: any difference at all fails
PERSON, VEHICLE = 7.0, 3.0
CASES = []


def case(cid, entries, **kw):
    def deco(fn):
        CASES.append(mc.Case(cid, entries, fn, **kw))
        return fn
    return deco


def _loss_module():
    from gcd_amd.training import StandardDiffusionLoss
    return StandardDiffusionLoss(sigma_sampler_config={"target": "gcd_amd.training.EDMSampling", "params": {}},
                                 loss_weighting_config={"target": "gcd_amd.training.EDMWeighting", "params": {}},
                                 pd_person_weight=PERSON, pd_vehicle_weight=VEHICLE)


def _map_case(ctx, BT, hw, latent):
    from gcd_amd import loss_device
    jpg = pd_semantic_frames(BT, *hw, seed=43)
    loss = _loss_module()
    out = ctx.out_flat("wmap", (BT, 1, *latent), F32)
    loss_device.class_weight_map(ctx.inp_flat(jpg, name="gt_rgb"), latent, loss._pd_classes(), out=out)
    return ctx.ref(lambda: {"wmap": (loss._pd_class_weight_map(jpg, latent).double().reshape(1, -1), ("maxabs", 1e-6))})


case("loss_class_map_48x80_to_6x10", ("gcd_loss_class_map",))(lambda ctx: _map_case(ctx, 2, (48, 80), (6, 10)))
case("loss_class_map_50x83_to_6x10", ("gcd_loss_class_map",))(lambda ctx: _map_case(ctx, 2, (50, 83), (6, 10)))


def _problem(shape, with_map):
    C_, H, W = shape
    g = torch.Generator().manual_seed(C_ * H * W)
    out, tgt = torch.randn(3, C_, H, W, generator=g), torch.randn(3, C_, H, W, generator=g)
    w, up = torch.rand(3, generator=g) + 0.5, torch.randn(3, generator=g)
    jpg = pd_semantic_frames(3, 8 * H, 8 * W, seed=7) if with_map else None
    wmap = _loss_module()._pd_class_weight_map(jpg, (H, W)) if with_map else None
    return out, tgt, w, up, jpg, wmap


def _saved_state(out, tgt, wmap, loss_type, keep):
    """(bit pattern of tau, quota) per frame from a sort on the CPU, `all` formed in fp32 as the kernel forms it."""
    diff = out - tgt
    raw = diff ** 2 if loss_type == "l2" else diff.abs()
    flat = (raw + raw * wmap * 0.5 if wmap is not None else raw).reshape(out.shape[0], -1)
    state = torch.zeros(out.shape[0], 2, dtype=I32)
    if keep:
        tau = flat.sort(dim=1, descending=True)[0][:, keep - 1]
        state[:, 0] = tau.view(I32)
        state[:, 1] = keep - (flat > tau[:, None]).sum(1).to(I32)
    return state


def _oracle(out, tgt, w, up, jpg, loss_type, keep):
    n = out[0].numel()
    kw = dict(loss_type=loss_type, focus_top=(keep + 0.5) / n, focus_steps=1) if keep else dict(loss_type=loss_type)
    leaf = out.double().requires_grad_(True)
    w4 = w.double()[:, None, None, None]
    loss = R.get_loss_pd(leaf, tgt.double(), w4, 1, jpg, PERSON, VEHICLE, **kw) if jpg is not None else \
        R.get_loss(leaf, tgt.double(), w4, 1, **kw)
    grad, = torch.autograd.grad((loss * up.double()).sum(), leaf)
    return loss.detach(), grad


def _fwd_case(ctx, shape, with_map, loss_type, keep):
    from gcd_amd import loss_device
    out, tgt, w, up, jpg, wmap = _problem(shape, with_map)
    loss = ctx.out_flat("loss", (3,), F32)
    state = ctx.out_flat("state", (3, 2), I32)
    loss_device.focal_fwd(ctx.inp_flat(out, name="out"), ctx.inp_flat(tgt, name="tgt"), ctx.inp_flat(w, name="w"),
                          ctx.inp_flat(wmap, name="wmap") if with_map else None, keep, loss_type, loss, state)

    def ref():
        want, _ = _oracle(out, tgt, w, up, jpg, loss_type, keep)
        return {"loss": (want.reshape(1, -1), 2e-6),
                "state": (_saved_state(out, tgt, wmap, loss_type, keep).double().reshape(1, -1), EQUAL)}
    return ctx.ref(ref)


def _bwd_case(ctx, shape, with_map, loss_type, keep):
    from gcd_amd import loss_device
    out, tgt, w, up, jpg, wmap = _problem(shape, with_map)
    dout = ctx.out_flat("dout", out.shape, F32)
    loss_device.focal_bwd(ctx.inp_flat(out, name="out"), ctx.inp_flat(tgt, name="tgt"), ctx.inp_flat(w, name="w"),
                          ctx.inp_flat(wmap, name="wmap") if with_map else None, ctx.inp_flat(up, name="g"),
                          ctx.inp_flat(_saved_state(out, tgt, wmap, loss_type, keep), name="state"), keep, loss_type, dout)
    return ctx.ref(lambda: {"dout": (_oracle(out, tgt, w, up, jpg, loss_type, keep)[1].reshape(1, -1), 2e-6)})


for _name, _shape in (("n140", (4, 5, 7)), ("n1025", (1, 5, 205))):
    for _map, _type, _keep in ((True, "l2", 14), (False, "l1", 14), (True, "l1", 0), (False, "l2", 0)):
        _id = f"{_name}_{_type}_{'wmap' if _map else 'null_wmap'}_keep{_keep}"
        case("loss_focal_fwd_" + _id, ("gcd_loss_focal_fwd",))(
            lambda ctx, a=(_shape, _map, _type, _keep): _fwd_case(ctx, *a))
        case("loss_focal_bwd_" + _id, ("gcd_loss_focal_bwd",))(
            lambda ctx, a=(_shape, _map, _type, _keep): _bwd_case(ctx, *a))


@pytest.mark.parametrize("c", CASES, ids=[c.id for c in CASES])
def test_contract(gpu, c):
    mc.run_contract(c, gpu)


def test_every_kernel_launching_export_has_a_case():
    from gcd_amd import _lib_loss
    launching = set(_lib_loss.LOSS_SIGNATURES) - {"gcd_loss_abi_version", "gcd_loss_last_error"}
    covered = {e for c in CASES for e in c.entries}
    assert launching == covered, launching ^ covered
    assert all(not c.atomic for c in CASES), "no bit-equality waiver: there are no floating-point read-modify-write reductions"
