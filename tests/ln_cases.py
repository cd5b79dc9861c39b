"""Shared inputs of the LayerNorm tests (tests/test_ln_ref_cpu.py, tests/test_layernorm_rows_gpu.py): seeded, built on the CPU,
every value representable in the storage type before anything is computed.

Row families
  unit      randn
  distinct  row r = m_r + s_r * randn, m_r = (r mod 7) - 3, s_r = 2^((r mod 5) - 2): neighbouring rows differ in mean by >= 1
            and in rstd by a factor >= 2, so statistics taken from the wrong row are a gross error
  offset    every row = c + s * randn, |mean| >> std: c / s = 64 for fp32 and fp16 (16, 0.25), 16 for bf16 (4, 0.25) — what a
            one-pass variance E[z^2] - mu^2 loses
  constant  every element of row r = (r mod 5) - 2: variance 0 (rstd = eps^-1/2), one row in five all zeros
`x` and `residual` are two draws of the family (their sum has the family's structure too), gamma = 1 + 0.1 randn,
beta = 0.1 randn, dy and dz_extra are randn with the per-row scales of `distinct`.

Shapes: the smallest that reach each arm of launch_fwd / launch_bwd (csrc/layernorm.hip).  A wave owns a row and a lane
16-byte chunks of it (8 elements of a 16-bit type, 4 of fp32), NCH = ceil(d / 16-byte chunks / 64) rounded up to 1/2/4/8/16;
NCH >= 4 is the LEAN backward; 16-bit rows of 512 / 1024 take the specialised kernels; 4 rows per workgroup, the forward grid is
capped at 2048 workgroups (a second trip of the row loop beyond 8192 rows), the backward grid at 1024 for d <= 512 and at 512
beyond (4096 / 2048 rows).

The bound of the GPU tests (its derivation is in tests/test_layernorm_rows_gpu.py) lives here too: the CPU controls of
tests/test_ln_ref_cpu.py apply it to deliberately wrong results."""
import math

import torch

FAMILIES = ('unit', 'distinct', 'offset', 'constant')
DTYPES = (torch.bfloat16, torch.float16, torch.float32)
EPS = 1e-5
ROWS_PER_BLOCK, FWD_CAP, BWD_CAP_NARROW, BWD_CAP_WIDE = 4, 2048, 1024, 512
MANT = {torch.bfloat16: 7, torch.float16: 10, torch.float32: 23}
U = 2.0 ** -24   # the unit round-off of the fp32 sums

# (rows, d) -> what it reaches
SHAPES_16 = {
    (1, 8): 'one chunk, one row, three idle waves', (3, 64): 'one idle wave',
    (5, 128): 'NCH 1, two workgroups', (5, 520): 'NCH 2, 65 chunks: one lane has a second chunk',
    (9, 512): 'specialised, NCH 1', (9, 1024): 'specialised, NCH 2',
    (3, 1032): 'LEAN NCH 4', (3, 2056): 'LEAN NCH 8, ragged', (2, 4096): 'LEAN NCH 8, full',
    (2, 4104): 'forward only, NCH 16 ragged', (2, 8192): 'forward only, NCH 16 full',
    (8197, 64): 'forward loop: 2050 workgroups of rows on a grid of 2048',
    (4101, 64): 'backward loop, cap 1024, NCH 1', (4101, 512): 'backward loop, cap 1024, specialised',
    (2053, 520): 'backward loop, cap 512, NCH 2 with the next-row prefetch', (2053, 1032): 'backward loop, cap 512, LEAN',
}
# fp32 has no non-LEAN kernel beyond d = 512 (d > 512 means more than 128 chunks, NCH >= 4, which is LEAN): the d > 512 cap
# is reached with the LEAN kernel at (2053, 520), and the prefetching NCH 2 loop at (4101, 264) under the d <= 512 cap
SHAPES_32 = {
    (1, 4): 'one chunk, one row, three idle waves', (3, 64): 'one idle wave',
    (5, 128): 'NCH 1, two workgroups', (5, 264): 'NCH 2, 66 chunks',
    (3, 520): 'LEAN NCH 4', (3, 1032): 'LEAN NCH 8, ragged', (2, 2048): 'LEAN NCH 8, full',
    (2, 2052): 'forward only, NCH 16 ragged', (2, 4096): 'forward only, NCH 16 full',
    (8197, 64): 'forward loop',
    (4101, 64): 'backward loop, cap 1024, NCH 1', (4101, 264): 'backward loop, cap 1024, NCH 2 with the next-row prefetch',
    (2053, 520): 'backward loop, cap 512, LEAN',
}
# beyond the arms of the dispatch: the specialised 16-bit forward kernel works from its second register set only on a second
# trip of its row loop, which the shapes above never take at d = 512 / 1024 (tests/test_layernorm_rows_gpu.py runs it apart)
SPECIALISED_FWD_LOOP = (8197, 512)


def shapes(dtype, backward=False):
    table = SHAPES_32 if dtype == torch.float32 else SHAPES_16
    return [s for s, what in table.items() if not (backward and what.startswith('forward'))]


def bwd_cap(rows, d):
    """the workgroup cap a backward shape is meant to exceed, or None"""
    cap = BWD_CAP_NARROW if d <= 512 else BWD_CAP_WIDE
    return cap if rows > cap * ROWS_PER_BLOCK else None


def bwd_workspace_bytes(rows, d):
    blocks = min(-(-rows // ROWS_PER_BLOCK), FWD_CAP, BWD_CAP_NARROW if d <= 512 else BWD_CAP_WIDE)
    return max(blocks, 1) * 2 * d * 4


def row_scales(rows):
    r = torch.arange(rows)
    return ((r % 7) - 3).float().unsqueeze(1), torch.exp2(((r % 5) - 2).float()).unsqueeze(1)


def family_rows(family, rows, d, dtype, g):
    n = torch.randn(rows, d, generator=g)
    if family == 'unit':
        t = n
    elif family == 'distinct':
        m, s = row_scales(rows)
        t = m + s * n
    elif family == 'offset':
        t = (4.0 if dtype == torch.bfloat16 else 16.0) + 0.25 * n
    elif family == 'constant':
        t = (((torch.arange(rows) % 5) - 2).float().unsqueeze(1)).expand(rows, d).clone()
    else:
        raise ValueError(family)
    return t.to(dtype)


def make(family, rows, d, dtype, seed=0):
    """CPU tensors in `dtype`: x, residual [rows, d] of the family, gamma, beta [d], dy, dz_extra [rows, d]"""
    g = torch.Generator().manual_seed(1000003 * seed + 7919 * rows + 31 * d + FAMILIES.index(family))
    _, s = row_scales(rows)
    return {'x': family_rows(family, rows, d, dtype, g), 'residual': family_rows(family, rows, d, dtype, g),
            'gamma': (1 + 0.1 * torch.randn(d, generator=g)).to(dtype), 'beta': (0.1 * torch.randn(d, generator=g)).to(dtype),
            'dy': (s * torch.randn(rows, d, generator=g)).to(dtype), 'dz_extra': (s * torch.randn(rows, d, generator=g)).to(dtype)}


# ---- the bound of tests/test_layernorm_rows_gpu.py (derived in its docstring), shared with the CPU controls ----
def chain(d, dtype):
    """additions behind a row sum: a lane's own elements (whole 16-byte chunks), six butterfly steps, the rounded 1 / d and the
    product with it"""
    epv = 4 if dtype == torch.float32 else 8
    return math.ceil(d / (64 * epv)) * epv + 8


def ulp_of(m, dtype):
    return torch.exp2(torch.floor(torch.log2(m.clamp_min(1e-300))) - MANT[dtype])


def rowwise(t, like):
    return t.double().reshape(like.shape)


def allowed(per, want, dtype, cond=None, ulps=1):
    """per row of `want` ([n, d], or [n] for one value per row or column): 2 err_per + ulps * ulp_T(max |want|) + cond"""
    w = want if want.dim() == 2 else want.unsqueeze(1)
    err_per = (rowwise(per, w) - w).abs().amax(1)
    return 2 * err_per + ulps * ulp_of(w.abs().amax(1), dtype) + (0 if cond is None else cond)


def miss(got, want):
    w = want if want.dim() == 2 else want.unsqueeze(1)
    return (rowwise(got, w) - w).abs().amax(1)


def fwd_conds(z, rstd, gamma, d, dtype):
    """cond per row for z, mean, rstd, y from the fp64 z [rows, d] and rstd [rows]"""
    c = chain(d, dtype) * U
    dmu = c * z.abs().amax(1)
    return {'z': None, 'mean': dmu, 'rstd': c * rstd, 'y': dmu * rstd * gamma.double().abs().max()}
