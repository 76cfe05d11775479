"""An independent, extended-precision evaluation of the four statistics operations of include/raftx.h
(raftx_motion_stats, raftx_channel_stats, raftx_channel_stats_poly, raftx_response_stats), written from the formulas in
their header comments with numpy.longdouble broadcasting -- not from the loops of oracle/raftx_oracle.c or of the kernels.

Every operation is "channel c is y_c(ih,w) = sum_j coef[c,j,w] Xi[ih,j,w]" with its own complete complex coefficient:
    poly_coef    L0 + i w L1 - w^2 L2 (+ Gw)          raftx_channel_stats_poly, raftx_response_stats
    power_coef   w^pow[c] L[c,j]                      raftx_channel_stats
    motion_coef  diag(1, 1, 1, deg, deg, deg)         raftx_motion_stats
followed by   std[c] = sqrt(0.5 sum_{ih,w} |y_c|^2),   psd[c,w] = sum_ih 0.5 |y_c|^2 / dw   (stats).

Next to psd and std, stats returns the NON-CANCELLING envelope of the same sums,
    S[c,h,w] = sum_j |coef[c,j,w]| |Xi[h,j,w]|,   env_psd[c,w] = 0.5 sum_h S^2 / dw,   env_var[c] = 0.5 sum_{h,w} S^2,
which is what the forward error of an fp64 evaluation is proportional to.  The tolerance is that forward error bound, for
a dot product of nDof complex terms followed by squaring and a sum of nw * nResp non-negative terms: with eps = 2^-52 and
K = 2 (nDof + 8) eps,
    |psd_dev - psd_ref| <= K env_psd,      |std_dev^2 - std_ref^2| <= (K + nw nResp eps) env_var.
It is derived, not tuned: a failure is a finding, not a reason to widen it."""
from collections import namedtuple

import numpy as np

LD, CLD = np.longdouble, np.clongdouble
EPS = 2.0 ** -52                                       # of the fp64 arithmetic under test

Stats = namedtuple("Stats", "std psd env_psd env_var")


def _extended():
    """The reference is only a reference if it carries more than fp64 (x87 extended on x86-64: eps = 2^-63)."""
    eps = np.finfo(LD).eps
    assert eps <= 2.0 ** -63, "numpy.longdouble is no wider than fp64 here (eps = %g): no independent reference" % eps


def poly_coef(w, L, Gw=None):
    """coef[...,c,j,w] = L[...,c,0,j] + (i w) L[...,c,1,j] + (i w)^2 L[...,c,2,j] (+ Gw[...,c,j,w])."""
    _extended()
    w = np.asarray(w, dtype=LD)
    L = np.asarray(L, dtype=LD)
    coef = (L[..., 0, :, None] - w * w * L[..., 2, :, None]).astype(CLD) + CLD(1j) * (w * L[..., 1, :, None])
    return coef if Gw is None else coef + np.asarray(Gw, dtype=CLD)


def power_coef(w, L, pow):
    """coef[...,c,j,w] = w^pow[c] L[...,c,j]."""
    _extended()
    w = np.asarray(w, dtype=LD)
    wp = np.stack([w ** int(p) for p in pow])                              # [c,w]; w^0 = 1 at w = 0 too
    return (np.asarray(L, dtype=LD)[..., :, :, None] * wp[:, None, :]).astype(CLD)


def motion_coef(nw):
    """coef[j,j',w] of the six platform motions: translations in m, rotations in degrees."""
    _extended()
    deg = LD(180) / (LD(4) * np.arctan(LD(1)))
    return (np.diag(np.array([1, 1, 1, deg, deg, deg], dtype=LD))[:, :, None] * np.ones(nw, dtype=LD)).astype(CLD)


def stats(coef, Xi, dw):
    """coef [...,nChan,nDof,nw] (complete complex coefficient of Xi_j), Xi [...,nResp,nDof,nw]; leading axes broadcast.
    Returns Stats(std [...,nChan], psd [...,nChan,nw], env_psd [...,nChan,nw], env_var [...,nChan]) in longdouble."""
    _extended()
    coef = np.asarray(coef, dtype=CLD)[..., :, None, :, :]                 # [...,c,1,j,w]
    Xi = np.asarray(Xi, dtype=CLD)[..., None, :, :, :]                     # [...,1,h,j,w]
    dw = LD(dw)
    y = (coef * Xi).sum(axis=-2)                                           # [...,c,h,w]
    y2 = y.real * y.real + y.imag * y.imag
    S = (np.abs(coef) * np.abs(Xi)).sum(axis=-2)
    return Stats(std=np.sqrt(LD(0.5) * y2.sum(axis=(-2, -1))), psd=LD(0.5) * y2.sum(axis=-2) / dw,
                 env_psd=LD(0.5) * (S * S).sum(axis=-2) / dw, env_var=LD(0.5) * (S * S).sum(axis=(-2, -1)))


def numpy_c128(coef, Xi, dw):
    """(std, psd) of the same formula in plain complex128 / float64 NumPy: a correct fp64 evaluation, which has to sit
    inside the bound if the bound is right."""
    coef = np.asarray(coef).astype(np.complex128)[..., :, None, :, :]
    y = (coef * np.asarray(Xi, dtype=np.complex128)[..., None, :, :, :]).sum(axis=-2)
    y2 = y.real * y.real + y.imag * y.imag
    return np.sqrt(0.5 * y2.sum(axis=(-2, -1))), 0.5 * y2.sum(axis=-2) / float(dw)


def bound_factors(nDof, nResp, nw):
    """(K, K + nw nResp eps): the factors of env_psd and env_var in the bound."""
    K = 2.0 * (nDof + 8) * EPS
    return LD(K), LD(K + nw * nResp * EPS)


def used(ref, std, psd, nDof, nResp, mask=None):
    """The largest fraction of the bound that (std, psd) use against ref: (of the psd bound, of the variance bound).
    Where the envelope is zero the result has to be exactly zero (fraction 0, else inf).  psd may be None; mask (boolean,
    over the bins) restricts the psd comparison."""
    nw = ref.psd.shape[-1]
    Kp, Kv = bound_factors(nDof, nResp, nw)

    def frac(err, env):
        with np.errstate(divide="ignore", invalid="ignore"):
            f = np.where(env > 0, err / env, np.where(err == 0, LD(0), LD(np.inf)))
        return float(np.max(f)) if f.size else 0.0

    std = np.asarray(std, dtype=LD)
    f_var = frac(np.abs(std * std - ref.std * ref.std), Kv * ref.env_var)
    f_psd = 0.0
    if psd is not None:
        err, env = np.abs(np.asarray(psd, dtype=LD) - ref.psd), Kp * ref.env_psd
        if mask is not None:
            err, env = err[..., mask], env[..., mask]
        f_psd = frac(err, env)
    return f_psd, f_var
