#!/usr/bin/env python3
"""tests/golden/render_pardom_tiny.pt: what the reference's ParallelDomain dataset renders from tiny clouds (data only).

The *unmodified* `ParallelDomainSynthViewDataset.synth_rgb` of the reference's `sgm/data/pardom_arbit.py` is run on the
CPU, unbound, on a plain namespace object that carries the attributes the method reads.  The modules the file imports and
this machine lacks are replaced by empty stand-ins (as tools/make_golden_render.py does for `sgm/data/geometry.py`, whose
loader and fixtures this file reuses), and the method's hard-coded `cuda:` device is redirected to the CPU inside this
process.  The class-colour table is made by executing the lines of the dataset's constructor that build it, read from
the reference's file at run time, on the fixture's ontology items.

What is recorded per frame: the colours the method handed to `project_points_to_pixels` (columns 3:6 of its float64
cloud), that function's outputs (image and weights whole, uv and depth at a sample of the finite points) in the layout
tests/render_util.check_splat reads, and the frames the method returned.

Stage 2 as in tools/make_golden_render.py: `blur_into_black` calls torchvision, which is not installed, so
`torchvision.transforms.functional.gaussian_blur` is that file's torch restatement; of the method's lines only that blur
is a restatement.  The clip is recorded twice, as the method returned it (the reference's dtypes) and as the float64 chain
over the same splat images, with the largest gap between the two.

Fixtures: 17 stored views (view 16 is what `reproject` renders) of 40 points, float16 positions, uint8 colours and ids;
four points of every view are +inf, -inf and 65504, and the generator refuses to write unless the reference masked every
one of them out; it keeps the refusals of tools/make_golden_render.py (uv + 0.5 within 1e-9 of an integer, a depth within
1e-9 of 0.1, a depth maximum within 1e-9 of 64, a non-zero image value below 1e-40).  No id is out of range.

Usage: python tools/make_golden_render_pardom.py [--reference DIR]      (DIR: the reference's gcd-model directory)
"""
from __future__ import annotations

import argparse
import importlib.util
import sys
import textwrap
import types
from pathlib import Path

import numpy as np
import torch

ROOT = Path(__file__).resolve().parent.parent
OUT = ROOT / "tests" / "golden" / "render_pardom_tiny.pt"
STUBS = ("lovely_tensors", "lovely_numpy", "pytorch_lightning")
V, N_VIEW, SRC_VIEW = 17, 40, 16
FRAME_HW = (16, 24)
UVD_SAMPLE = 128
N_CLASSES = 12


def load_base():
    spec = importlib.util.spec_from_file_location("make_golden_render", ROOT / "tools" / "make_golden_render.py")
    m = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(m)
    return m


def load_reference(base, ref_dir: Path):
    """(the reference's geometry module, its pardom_arbit module), both executed from the reference's files as they are."""
    geo = base.load_reference_geometry(ref_dir)
    tv = sys.modules["torchvision"]
    fn = types.ModuleType("torchvision.transforms.functional")
    fn.gaussian_blur = lambda img, kernel_size, sigma: base.gaussian_blur(img, kernel_size, sigma)
    sys.modules["torchvision.transforms.functional"] = fn
    tv.transforms.functional = fn
    for name in STUBS:
        try:
            importlib.import_module(name)
        except Exception:
            sys.modules[name] = types.ModuleType(name)
    sys.modules["lovely_tensors"].__dict__.setdefault("monkey_patch", lambda: None)
    sys.modules["lovely_numpy"].__dict__.setdefault("lo", None)
    sys.modules["pytorch_lightning"].__dict__.setdefault("LightningDataModule", object)
    # `from sgm.data import common, geometry`: the executed geometry module, and nothing of common (the method uses none)
    sgm, data, common = types.ModuleType("sgm"), types.ModuleType("sgm.data"), types.ModuleType("sgm.data.common")
    sgm.__path__, data.__path__ = [], []
    sgm.data, data.common, data.geometry = data, common, geo
    saved = {k: sys.modules.get(k) for k in ("sgm", "sgm.data", "sgm.data.common", "sgm.data.geometry")}
    sys.modules.update({"sgm": sgm, "sgm.data": data, "sgm.data.common": common, "sgm.data.geometry": geo})
    opts = np.get_printoptions()
    spec = importlib.util.spec_from_file_location("reference_pardom_arbit", ref_dir / "sgm" / "data" / "pardom_arbit.py")
    m = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(m)
    np.set_printoptions(**opts)
    torch.set_printoptions(profile="default")
    for k, v in saved.items():
        if v is None:
            sys.modules.pop(k, None)
        else:
            sys.modules[k] = v
    return geo, m


def reference_palette(ref_dir: Path, items):
    """The constructor's own lines, from `semantic_id_rgb_dict = ...` to `self.ontology['semantic_id_rgb_map'] = ...`, executed on
    `items`."""
    lines = (ref_dir / "sgm" / "data" / "pardom_arbit.py").read_text().splitlines()
    first = next(i for i, l in enumerate(lines) if "semantic_id_rgb_dict = {" in l)
    last = next(i for i, l in enumerate(lines) if "self.ontology['semantic_id_rgb_map'] = " in l)
    assert 0 < last - first < 12
    holder = types.SimpleNamespace(ontology=dict(items=items))
    exec(textwrap.dedent("\n".join(lines[first:last + 1])), dict(np=np, torch=torch, self=holder))
    return holder.ontology["semantic_id_rgb_map"]


class cuda_is_the_cpu:
    """Inside the block `tensor.to('cuda:0')` stays on the CPU."""

    def __enter__(self):
        self.saved = saved = torch.Tensor.to

        def to(t, *a, **k):
            a = tuple("cpu" if isinstance(x, str) and x.startswith("cuda") else x for x in a)
            if isinstance(k.get("device"), str) and k["device"].startswith("cuda"):
                k["device"] = "cpu"
            return saved(t, *a, **k)
        torch.Tensor.to = to

    def __exit__(self, *exc):
        torch.Tensor.to = self.saved
        return False


def cameras(geo, T):
    """Per frame: a camera-to-world matrix (float32) on an arc around the scene."""
    out = []
    for t in range(T):
        pos = np.array([0.4 + 0.3 * t, -5.0 + 0.2 * t, 1.1 + 0.1 * t])
        out.append(torch.tensor(geo.extrinsics_from_look_at(pos, np.array([0.1, 0.0, 0.2])), dtype=torch.float32))
    return torch.stack(out)


def normalised_intrinsics(T, H, W):
    """(T, 3, 3) float32 on the unit image, a little different per frame.  The focal length that survives the aspect-ratio
    correction is 0.8 W (+ 1 % per frame), which is what base.scene_cloud places its points with."""
    ar = W / H
    K = torch.zeros(T, 3, 3, dtype=torch.float32)
    for t in range(T):
        f = 0.8 * (1.0 + 0.01 * t)
        fx, fy = (f, 1.1) if ar > 640.0 / 480.0 + 1e-3 else (0.9, f * W / H) if ar < 640.0 / 480.0 - 1e-3 else (f, f * W / H)
        K[t] = torch.tensor([[fx, 0.0, (0.5 * W - 0.3) / W], [0.0, fy, (0.5 * H + 0.2) / H], [0.0, 0.0, 1.0]])
    return K


def make_cloud(base, geo, g, T, H, W, RTs, far):
    xyz, rgb, segm = [], [], []
    for t in range(T):
        x, c = base.scene_cloud(geo, g, V * N_VIEW, H, W, RTs[t], special=True, far=far)
        x = x.reshape(V, N_VIEW, 3).half()
        # stored float16 clouds of unbounded scenes hold infinities and the largest finite value
        x[:, N_VIEW - 4, 0] = float("inf")
        x[:, N_VIEW - 3, 1] = float("-inf")
        x[:, N_VIEW - 2, 2] = float("inf")
        x[:, N_VIEW - 1, 0] = 65504.0
        ids = torch.randint(0, N_CLASSES, (V, N_VIEW, 1), generator=g, dtype=torch.uint8)
        ids[0, 4, 0], ids[SRC_VIEW, 5, 0], ids[3, 6, 0] = 0, N_CLASSES - 1, 3
        xyz.append(x)
        rgb.append((c * 255.0).round().to(torch.uint8).reshape(V, N_VIEW, 3))
        segm.append(ids)
    tag = [torch.zeros(V, N_VIEW, 1, dtype=torch.uint8) for _ in range(T)]
    return dict(xyz=xyz, rgb=rgb, segm=segm, tag=tag)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reference", default=None)
    args = ap.parse_args()
    if args.reference is None:
        sys.path.insert(0, str(ROOT))
        from oracle.ref_shim import REF
        args.reference = REF
    ref_dir = Path(args.reference)
    base = load_base()
    geo, pardom = load_reference(base, ref_dir)
    method = pardom.ParallelDomainSynthViewDataset.synth_rgb
    g = torch.Generator().manual_seed(20251)

    # an ontology: ids 0 .. 11 without 5 (a row no item names), class 3 black
    items = [dict(id=k, name=f"class{k}", color=dict(zip("rgb", torch.randint(1, 256, (3,), generator=g).tolist())))
             for k in range(N_CLASSES) if k != 5]
    items[3]["color"] = dict(r=0, g=0, b=0)
    assert items[3]["id"] == 3
    table = reference_palette(ref_dir, items)
    assert table.dtype == torch.float64 and tuple(table.shape) == (N_CLASSES, 3) and not bool(table[3].any()) and not bool(table[5].any())
    palette = torch.zeros(256, 3, dtype=torch.float64)
    palette[:N_CLASSES] = table

    clouds, cases = {}, []
    calls = []
    real_project = geo.project_points_to_pixels

    def recording_project(xyzrgb, K, RT, H, W, spread_radius=2):
        out = real_project(xyzrgb, K, RT, H, W, spread_radius=spread_radius)
        calls.append(dict(xyzrgb=xyzrgb.clone(), K=K.clone(), RT=RT.clone(), H=H, W=W, radius=spread_radius, out=out))
        return out

    def add(name, cloud, modality, modal_time, T, radius, hw, reproject=False):
        H, W = hw
        pcl = clouds[cloud]
        assert len(pcl["xyz"]) >= T
        holder = types.SimpleNamespace(
            model_frames=T, data_gpu=0, render_width=W, render_height=H, frame_height=FRAME_HW[0], frame_width=FRAME_HW[1],
            modal_time=modal_time, spread_radius=radius, reproject_rgbd=reproject,
            ontology=dict(items=items, semantic_id_rgb_map=table))
        Kn, RTs = normalised_intrinsics(T, H, W), cams[:T].clone()
        del calls[:]
        geo.project_points_to_pixels = recording_project
        try:
            with cuda_is_the_cpu():
                rgb_ref, rep_ref = method(holder, pcl, modality, RTs, Kn, calc_reproject=reproject)
        finally:
            geo.project_points_to_pixels = real_project
        assert (rep_ref is not None) == reproject and len(calls) == T * (2 if reproject else 1)
        frames, f64, rep64 = [], [], []
        for t in range(T):
            rec = calls[t * (2 if reproject else 1)]
            img, pw, uv, depth = rec["out"]
            fname = f"{name}[{t}]"
            assert rec["xyzrgb"].dtype == torch.float64 and rec["xyzrgb"].shape == (V * N_VIEW, 6)
            # the non-finite points: none of them may have reached the image
            uvi = (uv + 0.5).type(torch.int32)
            mask = (uvi[:, 0] >= 0) & (uvi[:, 0] < W) & (uvi[:, 1] >= 0) & (uvi[:, 1] < H) & (depth[:, 0] > 0.1)
            odd = torch.zeros(V, N_VIEW, dtype=torch.bool)
            odd[:, N_VIEW - 4:] = True
            assert not bool(mask[odd.reshape(-1)].any()), f"{fname}: the reference let a non-finite point through"
            assert bool(torch.isfinite(img).all()) and bool(torch.isfinite(pw).all()), f"{fname}: a non-finite pixel"
            finite = torch.isfinite(uv).all(dim=1) & torch.isfinite(depth[:, 0])
            visible = base.edge_checks(fname, img, uv[finite], depth[finite], H, W)
            assert visible == int(mask.sum())
            pool = torch.nonzero(finite & ~odd.reshape(-1))[:, 0]
            gen = torch.Generator().manual_seed(1000 * len(cases) + t)
            idx = pool[torch.randperm(pool.numel(), generator=gen)[:UVD_SAMPLE]].sort().values
            front = depth[idx, 0] > 0.1
            small = uv[idx][front].abs().min().item()
            assert small >= 1e-2, f"{fname}: a sampled uv of {small:.2e} in front of the camera; the relative bar needs |uv| >= 1e-2"
            fr = dict(name=fname, colours=rec["xyzrgb"][:, 3:6].contiguous(), K=rec["K"], RT=rec["RT"], H=H, W=W, radius=radius,
                      visible=visible, img=img.contiguous(), pixel_weights=pw.contiguous(), uvd_idx=idx,
                      uv=uv[idx].contiguous(), depth=depth[idx].contiguous())
            assert float(depth[mask].max()) >= 64.0 if "far" in cloud else float(depth[mask].max()) < 64.0
            f64.append(base.fill_chain(img, 21, 5.25, FRAME_HW, all_f64=True)[1])
            again = base.fill_chain(img, 21, 5.25, FRAME_HW, all_f64=False)[1]
            assert torch.equal(again.to(rgb_ref.dtype), rgb_ref[t]), f"{fname}: the executed method and fill_chain differ"
            if reproject:
                rec2 = calls[2 * t + 1]
                assert torch.equal(rec2["xyzrgb"], rec["xyzrgb"].reshape(V, N_VIEW, 6)[SRC_VIEW])
                fr["reproject_img"] = rec2["out"][0].contiguous()
                assert bool((fr["reproject_img"].sum(dim=-1) != 0).any()), f"{fname}: view {SRC_VIEW} alone renders nothing"
                base.edge_checks(fname + " reproject", rec2["out"][0], rec2["out"][2][finite.reshape(V, N_VIEW)[SRC_VIEW]],
                                 rec2["out"][3][finite.reshape(V, N_VIEW)[SRC_VIEW]], H, W)
                rep64.append(base.fill_chain(fr["reproject_img"], 3, 0.75, FRAME_HW, all_f64=True)[1])
            frames.append(fr)
            print(f"{fname:22s} visible={visible:4d} covered={int((pw > 0).sum()):4d}/{H * W} colours {fr['colours'].dtype}")
        f64 = torch.stack(f64)
        c = dict(name=name, cloud=cloud, modality=modality, modal_time=modal_time, T=T, radius=radius, render_hw=hw,
                 frame_hw=FRAME_HW, reproject=reproject, intrinsics=Kn, extrinsics=RTs, frames=frames,
                 rgb_ref=rgb_ref.contiguous(), rgb_f64=f64, gap=(rgb_ref.double() - f64).abs().max().item())
        if reproject:
            rep64 = torch.stack(rep64)
            c.update(reproject_ref=rep_ref.contiguous(), reproject_f64=rep64, gap_reproject=(rep_ref.double() - rep64).abs().max().item())
        print(f"{name}: frames {rgb_ref.dtype}, dtype gap {c['gap']:.3e}" + (f", reproject {c['gap_reproject']:.3e}" if reproject else ""))
        cases.append(c)
        return c

    cams = cameras(geo, 4)
    clouds["near_24x40"] = make_cloud(base, geo, g, 4, 24, 40, cams, far=False)
    clouds["far_24x40"] = make_cloud(base, geo, g, 1, 24, 40, cams, far=True)
    clouds["near_24x28"] = make_cloud(base, geo, g, 1, 24, 28, cams, far=False)
    clouds["near_24x32"] = make_cloud(base, geo, g, 1, 24, 32, cams, far=False)
    for pcl in clouds.values():
        for ids in pcl["segm"]:
            assert int(ids.max()) < N_CLASSES
    ids = torch.cat([i.reshape(-1) for i in clouds["near_24x40"]["segm"]])
    assert bool((ids == 0).any()) and bool((ids == N_CLASSES - 1).any()) and bool((ids == 3).any()) and bool((ids == 5).any())

    add("rgb", "near_24x40", "rgb", 0, 1, 1, (24, 40), reproject=True)
    add("segm_m0", "near_24x40", "segm", 0, 2, 1, (24, 40))                     # the shipped configs: all PALETTE
    add("segm_m3", "near_24x40", "segm", 3, 3, 1, (24, 40), reproject=True)     # RGB; BLEND at 1/3; BLEND at 2/3
    add("segm_m2", "near_24x40", "segm", 2, 4, 2, (24, 40))                     # RGB; BLEND at 1/2; PALETTE; PALETTE
    add("segm_m0_far", "far_24x40", "segm", 0, 1, 1, (24, 40))                  # depths of 64 .. 1600: the square-root branch
    add("segm_m0_24x28", "near_24x28", "segm", 0, 1, 1, (24, 28))               # narrower than 640 / 480: fx := fy
    add("segm_m0_24x32", "near_24x32", "segm", 0, 1, 1, (24, 32))               # 640 / 480 itself: the dead band
    try:
        with cuda_is_the_cpu():
            method(types.SimpleNamespace(model_frames=1, data_gpu=0, render_width=40, render_height=24, reproject_rgbd=False),
                   clouds["near_24x40"], "depth", cams[:1], normalised_intrinsics(1, 24, 40))
        raise AssertionError("the reference was expected to refuse an unknown modality")
    except ValueError:
        pass

    for pcl in clouds.values():
        del pcl["tag"]                              # the method reads the key and nothing of its value
    torch.save(dict(clouds=clouds, cases=cases, items=items, palette=palette, n_classes=N_CLASSES, src_view=SRC_VIEW,
                    frame_hw=FRAME_HW), OUT)
    print(f"{OUT.relative_to(ROOT)}: {OUT.stat().st_size} bytes")
    assert OUT.stat().st_size < 1024 * 1024


if __name__ == "__main__":
    main()
