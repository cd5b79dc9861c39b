"""Residual + dropout + LayerNorm / RMSNorm, forward and backward, in closed form (include/pasero_hip.h: pk_residual_ln_fwd,
pk_residual_ln_bwd).  Plain torch, no autograd, any floating dtype and device: the tests run these functions in fp64 on the
CPU as the reference and, unchanged, in the storage type on the GPU as the per-op path the kernels are measured against.
tests/test_ln_ref_cpu.py holds them to oracle/ref_cpu.py, torch.nn.functional.layer_norm and torch autograd."""
import torch


def fwd(x, residual, keep, p, gamma, beta, eps, rms, store=None):
    """z = residual + x * keep / (1 - p); y = LayerNorm(z) * gamma + beta, or RMSNorm(z) * gamma with `rms`.
    x, residual [rows, d]; keep: bool mask [rows, d] or None; gamma None: the residual-only pass (z alone).
    `store`: the storage type of the tensors when the arithmetic runs in a wider one — the kernels take the statistics on the
    stored z, so a 16-bit `store` rounds z to it whenever z is computed (residual or dropout; otherwise z is x).
    Returns (z, mean [rows] or None for RMSNorm, rstd [rows], y)."""
    z = x
    if keep is not None:
        z = z * keep.to(x.dtype) / (1.0 - p)
    if residual is not None:
        z = residual + z
    if store in (torch.bfloat16, torch.float16) and (keep is not None or residual is not None):
        z = z.to(store).to(x.dtype)
    if gamma is None:
        return z, None, None, None
    mean = None if rms else z.mean(-1, keepdim=True)
    zc = z if rms else z - mean
    rstd = torch.rsqrt((zc * zc).mean(-1, keepdim=True) + eps)
    y = zc * rstd * gamma
    if beta is not None:
        y = y + beta
    return z, None if rms else mean.squeeze(-1), rstd.squeeze(-1), y


def bwd(dy, dz_extra, z, gamma, mean, rstd, keep, p, rms):
    """dz = LN_bwd(dy; z, gamma, mean, rstd) (if gamma) + dz_extra (if given); dres = dz; dx = dz * keep / (1 - p);
    dgamma = sum over rows of dy * xhat; dbeta = sum over rows of dy (None for RMSNorm).  mean / rstd [rows] are inputs: the
    statistics are not recomputed from z.  Returns (dres, dx, dgamma, dbeta)."""
    dz = dgamma = dbeta = None
    if gamma is not None:
        rs = rstd.unsqueeze(-1)
        xhat = (z if rms else z - mean.unsqueeze(-1)) * rs
        g = dy * gamma
        t = g - xhat * (g * xhat).mean(-1, keepdim=True)
        if not rms:
            t = t - g.mean(-1, keepdim=True)
        dz = rs * t
        dgamma = (dy * xhat).sum(0)
        dbeta = None if rms else dy.sum(0)
    if dz_extra is not None:
        dz = dz_extra if dz is None else dz + dz_extra
    dx = dz if keep is None else dz * keep.to(dz.dtype) / (1.0 - p)
    return dz, dx, dgamma, dbeta
