"""The stage table of the fused sampler family (host, pure torch, no GPU).

A STAGE is one network evaluation followed by one elementwise update of the state (gcd_sampler_stage_f32,
include/gcd_amd_sampler.h).  `stage_table(sampler, sigmas)` turns a sampler object and its float32 sigma schedule into

    rows  [n_stages, 12] float32:  {sigma, a_cur, a_den, a_h0, a_h1, a_noise, s0_cur, s0_den, s1_cur, s1_den, 0, 0}
    draws list of (stage, used, scale) in the order in which the reference consumes its random stream

so that, with D the guided denoiser output at `sigma` on the current state,

    new = a_cur cur + a_den D + a_h0 h0 + a_h1 h1 + a_noise noise
    h0  = s0_cur cur + s0_den D      (only if the pair is not (0, 0));   h1 likewise;   cur = new.

The coefficients are the reference's own formulas (sgm sampling.py / sampling_utils.py), evaluated on the float32
schedule with the torch operations the reference uses (`log`, `expm1`, `minimum`, `** 0.5`); sigma' = 0 is handled
explicitly — the reference's -log 0, expm1(-inf) and 1 / (2 r) are never USED on that step, and no coefficient here is
inf or NaN.

`draws`: before stage `stage` is launched one noise tensor is drawn; `used` says whether the stage adds it (with
coefficient `scale`, also in the row's a_noise) or the reference draws and discards it (the ancestral samplers at
sigma' = 0: torch.where evaluates both branches).  stage == -1: churn on step 0, applied to the state before the loop
as x += scale * noise.  The churn noise of step i + 1 is folded into the LAST stage of step i, which is exact: the
reference replaces x by x_hat before anything else reads it.
"""
from __future__ import annotations

from typing import List, Tuple

import torch

ROW = 12
SIGMA, A_CUR, A_DEN, A_H0, A_H1, A_NOISE, S0_CUR, S0_DEN, S1_CUR, S1_DEN = range(10)
# the reference's "save a network evaluation if all noise levels are 0" threshold (sampling.py:237, 282, 345)
ZERO_SIGMA = 1e-14

Draw = Tuple[int, bool, float]


def get_ancestral_step(sigma_from, sigma_to, eta=1.0):
    """sampling_utils.py:22-31."""
    if not eta:
        return sigma_to, 0.0
    sigma_up = torch.minimum(sigma_to, eta * (sigma_to ** 2 * (sigma_from ** 2 - sigma_to ** 2) / sigma_from ** 2) ** 0.5)
    sigma_down = (sigma_to ** 2 - sigma_up ** 2) ** 0.5
    return sigma_down, sigma_up


def to_neg_log_sigma(sigma):
    return sigma.log().neg()


def to_sigma(neg_log_sigma):
    return neg_log_sigma.neg().exp()


def churn_gammas(sampler, sig_host) -> List[float]:
    """gamma of every step of an EDMSampler, from host copies of the sigmas (the reference compares device tensors)."""
    n = len(sig_host) - 1
    if not sampler.s_churn > 0:
        return [0.0] * n
    return [min(sampler.s_churn / n, 2 ** 0.5 - 1) if sampler.s_tmin <= sig_host[i] <= sampler.s_tmax else 0.0
            for i in range(n)]


def _row(sigma, a_cur, a_den, **kw) -> torch.Tensor:
    r = torch.zeros(ROW, dtype=torch.float32)
    r[SIGMA], r[A_CUR], r[A_DEN] = sigma, a_cur, a_den
    idx = dict(a_h0=A_H0, a_h1=A_H1, a_noise=A_NOISE, s0_cur=S0_CUR, s0_den=S0_DEN, s1_cur=S1_CUR, s1_den=S1_DEN)
    for k, v in kw.items():
        r[idx[k]] = v
    return r


def _euler_row(sigma, sigma_to) -> torch.Tensor:
    """x + (sigma_to - sigma) (x - D) / sigma  =  (sigma_to / sigma) x + (1 - sigma_to / sigma) D."""
    ratio = sigma_to / sigma
    return _row(sigma, ratio, 1.0 - ratio)


def _edm(sampler, s, heun: bool):
    n = len(s) - 1
    gam = churn_gammas(sampler, s.tolist())
    hat = [s[i] * (gam[i] + 1.0) for i in range(n)]
    # s_noise sqrt(sigma_hat^2 - sigma^2) of every step that churns (sampling.py:102-105)
    churn = [float(sampler.s_noise * (hat[i] ** 2 - s[i] ** 2) ** 0.5) if gam[i] > 0 else 0.0 for i in range(n)]
    rows, draws = [], []
    if churn[0] != 0.0:
        draws.append((-1, True, churn[0]))
    for i in range(n):
        nxt = s[i + 1]
        first = _euler_row(hat[i], nxt)
        step = [first]
        if heun and not float(nxt) < ZERO_SIGMA:
            first[S0_CUR] = 1.0                      # h0 <- x
            first[S1_CUR] = 1.0 / hat[i]             # h1 <- d = (x - D) / sigma_hat
            first[S1_DEN] = -1.0 / hat[i]
            dt = nxt - hat[i]
            half = dt / (2.0 * nxt)                  # x + dt (d + (euler - D') / sigma') / 2
            step.append(_row(nxt, half, -half, a_h0=1.0, a_h1=dt / 2.0))
        if i + 1 < n and churn[i + 1] != 0.0:
            step[-1][A_NOISE] = churn[i + 1]
            draws.append((len(rows) + len(step) - 1, True, churn[i + 1]))
        rows += step
    return rows, draws


def _ancestral(sampler, s, second_order: bool):
    n = len(s) - 1
    rows, draws = [], []
    for i in range(n):
        sig, nxt = s[i], s[i + 1]
        down, up = get_ancestral_step(sig, nxt, eta=sampler.eta)
        step = [_euler_row(sig, down)]
        if second_order and not float(down) < ZERO_SIGMA:
            t, t_next = to_neg_log_sigma(sig), to_neg_log_sigma(down)
            h = t_next - t
            mid = t + 0.5 * h
            mult1 = to_sigma(mid) / to_sigma(t)
            mult2 = (-0.5 * h).expm1()
            mult3 = to_sigma(t_next) / to_sigma(t)
            mult4 = (-h).expm1()
            step = [_row(sig, mult1, -mult2, s0_cur=1.0),                       # x2, h0 <- x
                    _row(to_sigma(mid), 0.0, -mult4, a_h0=mult3)]               # mult3 x - mult4 D(x2)
        noise = float(sampler.s_noise * up) if float(nxt) > 0.0 else 0.0
        step[-1][A_NOISE] = noise
        draws.append((len(rows) + len(step) - 1, noise != 0.0, noise))          # drawn every step, discarded at sigma' = 0
        rows += step
    return rows, draws


def _dpmpp2m(sampler, s):
    n = len(s) - 1
    rows = []
    for i in range(n):
        sig, nxt = s[i], s[i + 1]
        last = float(nxt) < ZERO_SIGMA
        if float(nxt) > 0.0:
            t, t_next = to_neg_log_sigma(sig), to_neg_log_sigma(nxt)
            h = t_next - t
            mult1 = to_sigma(t_next) / to_sigma(t)
            mult2 = (-h).expm1()
        else:                                        # exp(-inf) / sigma = 0, expm1(-inf) = -1: x <- D
            h, mult1, mult2 = None, 0.0, -1.0
        if i == 0 or last or h is None:
            row = _row(sig, mult1, -mult2)
        else:
            r = (t - to_neg_log_sigma(s[i - 1])) / h
            mult3, mult4 = 1 + 1 / (2 * r), 1 / (2 * r)
            row = _row(sig, mult1, -mult2 * mult3, a_h0=mult2 * mult4)          # mult1 x - mult2 (mult3 D - mult4 old)
        if i + 1 < n:
            row[S0_DEN] = 1.0                        # h0 <- D for the next step
        rows.append(row)
    return rows, []


def stage_table(sampler, sigmas) -> Tuple[torch.Tensor, List[Draw]]:
    """(rows [n_stages, 12] float32 on the CPU, draws) for a sampler of gcd_amd.sampling and its sigma schedule."""
    s = torch.as_tensor(sigmas).detach().to(device="cpu", dtype=torch.float32)
    if s.dim() != 1 or len(s) < 2 or not bool((s[:-1] > 0).all()):
        raise ValueError("stage_table: sigmas must be a 1-D schedule of positive levels (the last may be 0)")
    kind = getattr(sampler, "stage_kind", None)
    if kind == "euler":
        rows, draws = _edm(sampler, s, heun=False)
    elif kind == "heun":
        rows, draws = _edm(sampler, s, heun=True)
    elif kind == "euler_ancestral":
        rows, draws = _ancestral(sampler, s, second_order=False)
    elif kind == "dpmpp2s_ancestral":
        rows, draws = _ancestral(sampler, s, second_order=True)
    elif kind == "dpmpp2m":
        rows, draws = _dpmpp2m(sampler, s)
    else:
        raise NotImplementedError(f"stage_table: {type(sampler).__name__} has no stage form")
    rows = torch.stack(rows)
    if not bool(torch.isfinite(rows).all()):
        raise ValueError(f"stage_table: non-finite coefficient for {type(sampler).__name__} on {s.tolist()}")
    return rows, draws
