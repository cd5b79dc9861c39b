"""pk_residual_ln_fwd / pk_residual_ln_bwd / pk_residual_ln_bwd_partials + pk_ln_param_grads (csrc/layernorm.hip) and the
fused pk_gemm_ln_fwd (csrc/gemmln.hip), row by row against tests/ln_ref.py in fp64, at every arm of launch_fwd / launch_bwd
(the shapes and row families of tests/ln_cases.py), through the C ABI itself so that every output can be pre-filled.

Tolerance: the measured rule of tests/test_adapter_rows_gpu.py, applied per row (per column for dgamma / dbeta) so that a
tensor's largest row does not hide its smallest.  want = ln_ref in fp64 on the CPU over the storage-type inputs; per = ln_ref
on the GPU in the storage type (fp32 for fp32); got = the kernel.  For row r
    err_got <= 2 * err_per + ulp_T(max_j |want_rj|) + cond_r
(factor 2 and the one ulp: that file's rule — both paths round at the same points and differ in the order of their sums).
cond_r is the fp32 rounding of the row sums, which ulp_T does not see in fp32 and on `offset` / `constant` rows.  From the code:
a lane adds its elements one after the other, then six butterfly steps (common.h: wave_sum) and the product with a rounded 1/d,
    c = lane_chain + 8,   lane_chain = ceil(d / (64 * EPV)) * EPV   (EPV = 8 elements of a 16-bit type or 4 of fp32 per chunk)
— not ceil(d / 64): a lane owns whole 16-byte chunks, so at d = 520 (65 chunks of 8) lane 0 adds 16 values, not 9; the chain
the code has is used.  A sum of n terms with a chain of c additions is off by at most c * 2^-24 * sum|term|, hence
    dmu_r = c * 2^-24 * max_j |z_rj|          (the mean is sum / d, sum|z| / d <= max|z|)
    cond(mean) = dmu_r      cond(rstd) = c * 2^-24 * rstd_r      cond(y) = dmu_r * rstd_r * max|gamma|      cond(z) = 0
(rstd: the variance sum has the same chain plus three roundings per term, halved by the power -1/2, plus rsqrtf's ulp — less
than c * 2^-24 relative for c >= 9; the error of the mean enters the variance squared).  Backward takes its statistics as
inputs (the reference's, rounded to fp32, which want and per are fed too), its two row sums have the same chain:
    cond(dres) = cond(dx) = c * 2^-24 * max_j |want_rj|
dgamma / dbeta are sums over rows: a wave adds ceil(rows / (4 * workgroups)) rows, a workgroup its 4 waves, the reduction kernel
every 64th slab and then a tree of 6 steps: c_col = ceil(rows / 4 / workgroups) + 4 + ceil(workgroups / 64) + 6, three more for
dgamma (xhat and the product dy * xhat are rounded before they are added).  The terms of a column have either sign, so the
magnitude a column's rounding scales with is the sum of the terms' magnitudes, not the possibly cancelled |want_c|:
    cond(dgamma_c) = (c_col + 3) * 2^-24 * sum_r |dy_rc * xhat_rc|      cond(dbeta_c) = c_col * 2^-24 * sum_r |dy_rc|
`constant` rows: y = beta and rstd = eps^-1/2 within cond (and the rounding of y to the storage type).

Every output is filled with NaN before the call and must come back finite, the `ln` workspace is filled with 0xFF and its slabs
must come back finite; every row-shaped output has one guard row of NaN behind `rows` (dgamma / dbeta 8 guard elements) which
must still be NaN afterwards; an output that was not asked for keeps its NaN.

mean and rstd are fp32 whatever the storage type, so ulp_T of a 16-bit T bounds them loosely: where z is x (no residual, no
dropout — the same bits in every path) they are held to the same rule with T = fp32 as well (`check_stats_fp32`).

The worst err_got / allowed per output is printed per test.  Measured on an MI355X (884 tests, 18 to 23 s; worst per output):
    z 0.350  mean 0.196  rstd 0.414  y 0.250  mean (fp32 rule) 0.051  rstd (fp32 rule) 0.143
    dres 0.250  dx 0.250  dgamma 0.560  dbeta 0.250
(0.250 is half a 16-bit ulp of rounding against the two ulps the per-op path earns; the fp32 figures are the tight ones: rstd
on `offset` rows, dgamma end to end at three rows, z under dropout, where the kernel multiplies by a rounded 1 / (1 - p)).
Builds with the arithmetic wrong on purpose — a one-pass variance; the next row's statistics in the prefetching backward; the
second register set of either specialised kernel fed the wrong row or the other set's statistics; the LEAN backward reading
its first row's statistics on every trip; the slab reduction stopping at 512 slabs — each failed this file, and all but the
LEAN one passed the kernel-level LayerNorm tests of tests/test_kernels_gpu.py.
"""
import ctypes
import math

import pytest
import torch

import ln_cases as C
import ln_ref as R

pytestmark = pytest.mark.gpu

EPS = C.EPS
SEED, OFFSET = 1234, 7
U = C.U
NAN = float('nan')
WORST = {}
_cases = {}


class PkLnParamGrad(ctypes.Structure):
    """include/pasero_hip.h"""
    _fields_ = [('workspace', ctypes.c_void_p), ('dgamma', ctypes.c_void_p), ('dbeta', ctypes.c_void_p)]


@pytest.fixture(scope='module', autouse=True)
def _need_gpu():
    if not torch.cuda.is_available():
        pytest.skip('needs a GPU')
    yield
    print('\nworst err_got / allowed per output over the file: ' + ', '.join(f'{k} {v:.3f}' for k, v in sorted(WORST.items())))


def lib():
    from pasero_amd import lib as L
    return L


def code(dtype):
    return {torch.float32: 0, torch.bfloat16: 1, torch.float16: 2}[dtype]


def ptr(t):
    return None if t is None else t.data_ptr()


chain, ulp_of = C.chain, C.ulp_of


def bwd_blocks(rows, d):
    return C.bwd_workspace_bytes(rows, d) // (2 * d * 4)


# ---------------------------------------------------------------------------------------------------------------------
# inputs and references, built once per (family, shape, dtype, seed)
# ---------------------------------------------------------------------------------------------------------------------
class Case:
    def __init__(self, family, rows, d, dtype, seed=0):
        self.family, self.rows, self.d, self.dtype = family, rows, d, dtype
        self.t = C.make(family, rows, d, dtype, seed)
        self.g = {k: v.cuda() for k, v in self.t.items()}
        self.f = {k: v.double() for k, v in self.t.items()}
        self.memo = {}

    def keep(self, p, offset=OFFSET):
        """the mask of (SEED, offset) as pk_dropout draws it, or None"""
        if not p:
            return None
        key = ('keep', p, offset)
        if key not in self.memo:
            from pasero_amd import functional as F
            ones = torch.ones(self.rows, self.d, dtype=self.dtype, device='cuda')
            self.memo[key] = F.dropout(ones, p, SEED, offset) != 0
        return self.memo[key]

    def want_fwd(self, res, beta, rms, p=0.0, gamma=True):
        """(z, mean, rstd, y) in fp64 on the GPU, computed on the CPU"""
        key = ('fwd', res, beta, rms, p, gamma)
        if key not in self.memo:
            f, keep = self.f, self.keep(p)
            out = R.fwd(f['x'], f['residual'] if res else None, None if keep is None else keep.cpu(), p, f['gamma'] if gamma else None,
                        f['beta'] if beta else None, EPS, rms, store=self.dtype)
            self.memo[key] = tuple(None if o is None else o.cuda() for o in out)
        return self.memo[key]

    def per_fwd(self, res, beta, rms, p=0.0, gamma=True):
        g = self.g
        return R.fwd(g['x'], g['residual'] if res else None, self.keep(p), p, g['gamma'] if gamma else None,
                     g['beta'] if beta else None, EPS, rms)

    def bwd_inputs(self, rms):
        """z in the storage type and the reference's statistics rounded to fp32 (GPU), as every backward path gets them"""
        key = ('bwd_in', rms)
        if key not in self.memo:
            z, mean, rstd, _ = self.want_fwd(True, False, rms)
            self.memo[key] = (z.to(self.dtype), None if rms else mean.float(), rstd.float())
        return self.memo[key]

    def want_bwd(self, rms, extra, p=0.0, gamma=True):
        """(dres, dx, dgamma, dbeta, sum_r |dy xhat|, sum_r |dy|) in fp64 on the GPU, computed on the CPU"""
        key = ('bwd', rms, extra, p, gamma)
        if key not in self.memo:
            f, keep = self.f, self.keep(p)
            z, mean, rstd = (None if v is None else v.double().cpu() for v in self.bwd_inputs(rms))
            out = R.bwd(f['dy'] if gamma else None, f['dz_extra'] if extra else None, z if gamma else None,
                        f['gamma'] if gamma else None, mean, rstd, None if keep is None else keep.cpu(), p, rms)
            mags = (None, None)
            if gamma:
                xhat = (z if rms else z - mean.unsqueeze(1)) * rstd.unsqueeze(1)
                mags = ((f['dy'] * xhat).abs().sum(0), f['dy'].abs().sum(0))
            self.memo[key] = tuple(None if o is None else o.cuda() for o in out + mags)
        return self.memo[key]

    def per_bwd(self, rms, extra, p=0.0, gamma=True):
        g = self.g
        z, mean, rstd = self.bwd_inputs(rms)
        return R.bwd(g['dy'] if gamma else None, g['dz_extra'] if extra else None, z if gamma else None, g['gamma'] if gamma else None,
                     None if mean is None else mean.to(self.dtype), rstd.to(self.dtype), self.keep(p), p, rms)


def case(family, rows, d, dtype, seed=0):
    key = (family, rows, d, dtype, seed)
    if key not in _cases:
        while len(_cases) >= 6:
            _cases.pop(next(iter(_cases)))
        _cases[key] = Case(family, rows, d, dtype, seed)
    return _cases[key]


# ---------------------------------------------------------------------------------------------------------------------
# the kernels through the C ABI, into NaN-filled outputs with a guard row
# ---------------------------------------------------------------------------------------------------------------------
def nan_rows(rows, d, dtype):
    return torch.full((rows + 1, d) if d else (rows + 1,), NAN, dtype=dtype, device='cuda')


def guard_ok(name, full, n, asked):
    if asked:
        assert torch.isnan(full[n:]).all(), f'{name}: the guard behind the output was written'
        assert torch.isfinite(full[:n]).all(), f'{name}: not every element was written'
        return full[:n]
    assert torch.isnan(full).all(), f'{name}: written although not asked for'
    return None


def k_fwd(x, residual, gamma, beta, rms, want_z, p=0.0, offset=OFFSET, eps=EPS):
    L = lib()
    rows, d = x.shape
    ln = gamma is not None
    z, y = nan_rows(rows, d, x.dtype), nan_rows(rows, d, x.dtype)
    mean, rstd = nan_rows(rows, 0, torch.float32), nan_rows(rows, 0, torch.float32)
    L.check(L.load().pk_residual_ln_fwd(ptr(x), ptr(residual), ptr(gamma), ptr(beta), ptr(z) if want_z else None, ptr(y) if ln else None,
                                        ptr(mean) if ln and not rms else None, ptr(rstd) if ln else None, rows, d, eps, p, SEED, offset,
                                        code(x.dtype), L.stream_ptr()), 'pk_residual_ln_fwd')
    torch.cuda.synchronize()
    return (guard_ok('z', z, rows, want_z), guard_ok('mean', mean, rows, ln and not rms), guard_ok('rstd', rstd, rows, ln),
            guard_ok('y', y, rows, ln))


def ln_workspace(rows, d):
    L = lib()
    nbytes = L.load().pk_residual_ln_bwd_workspace(rows, d)
    assert nbytes == C.bwd_workspace_bytes(rows, d)
    ws = L.workspace(nbytes, torch.device('cuda', torch.cuda.current_device()), 'ln')
    ws.fill_(0xFF)
    return ws, nbytes


def k_bwd(dy, extra, z, gamma, mean, rstd, dres=True, dx=False, dgamma=False, dbeta=False, p=0.0, offset=OFFSET, defer_ws=None):
    """pk_residual_ln_bwd, or pk_residual_ln_bwd_partials into `defer_ws` (then no parameter gradients come back)"""
    L = lib()
    ref = dy if dy is not None else extra
    rows, d = ref.shape
    o_res, o_x = nan_rows(rows, d, ref.dtype), nan_rows(rows, d, ref.dtype)
    o_g, o_b = (torch.full((d + 8,), NAN, dtype=ref.dtype, device='cuda') for _ in range(2))
    pg = gamma is not None and (dgamma or dbeta)
    common = (rows, d, p, SEED, offset, code(ref.dtype), L.stream_ptr())
    if defer_ws is not None:
        L.check(L.load().pk_residual_ln_bwd_partials(ptr(dy), ptr(extra), ptr(z), ptr(gamma), ptr(mean), ptr(rstd), ptr(o_res) if dres else None,
                                                     ptr(o_x) if dx else None, ptr(defer_ws), defer_ws.numel(), *common),
                'pk_residual_ln_bwd_partials')
    else:
        ws, nbytes = ln_workspace(rows, d) if pg else (None, 0)
        L.check(L.load().pk_residual_ln_bwd(ptr(dy), ptr(extra), ptr(z), ptr(gamma), ptr(mean), ptr(rstd), ptr(o_res) if dres else None,
                                            ptr(o_x) if dx else None, ptr(o_g) if dgamma else None, ptr(o_b) if dbeta else None, ptr(ws),
                                            nbytes, *common), 'pk_residual_ln_bwd')
        if pg:
            torch.cuda.synchronize()
            assert torch.isfinite(ws[:nbytes].view(torch.float32)).all(), 'a workgroup left part of its slab unwritten'
    torch.cuda.synchronize()
    return (guard_ok('dres', o_res, rows, dres), guard_ok('dx', o_x, rows, dx), guard_ok('dgamma', o_g, d, dgamma and defer_ws is None),
            guard_ok('dbeta', o_b, d, dbeta and defer_ws is None))


# ---------------------------------------------------------------------------------------------------------------------
# the bound
# ---------------------------------------------------------------------------------------------------------------------
def check(rep, name, got, per, want, dtype, cond=None, ulps=1):
    """per row of `want` ([n, d]; [n] for one value per row or column): err_got <= 2 err_per + ulps * ulp_T(max|want|) + cond"""
    err_got, allowed = C.miss(got, want), C.allowed(per, want, dtype, cond, ulps)
    ratios = torch.where(err_got > 0, err_got / allowed.clamp_min(1e-300), torch.zeros_like(err_got))
    ratio, at = (v.item() for v in ratios.max(0))
    rep[name] = max(rep.get(name, 0.0), ratio)
    WORST[name] = max(WORST.get(name, 0.0), ratio)
    assert ratio <= 1.0, (f'{name}: row/column {at}: kernel {err_got[at].item():.3e} allowed {allowed[at].item():.3e} '
                          f'({ratio:.2f} of the bound)')


def fwd_conds(want, gamma, d, dtype):
    return C.fwd_conds(want[0], want[2], gamma, d, dtype)


def check_fwd(rep, got, per, want, gamma, d, dtype, z_ulps=1):
    conds = fwd_conds(want, gamma, d, dtype) if want[2] is not None else {'z': None}
    for name, g, p, w in zip(('z', 'mean', 'rstd', 'y'), got, per, want):
        if g is None:
            continue
        check(rep, name, g, p, w, dtype, conds[name], ulps=z_ulps if name == 'z' else 1)


def check_stats_fp32(rep, got, c, want, rms):
    """mean and rstd are fp32 whatever the storage type, and ulp_T of a 16-bit T is a loose bound on them.  Where z is x (no
    residual, no dropout: the same bits in every path) they are also held to the rule with T = fp32: per = ln_ref in fp32 over
    the 16-bit inputs, cond with the 16-bit kernels' chain"""
    per = R.fwd(c.g['x'].float(), None, None, 0.0, c.g['gamma'].float(), None, EPS, rms)
    conds = fwd_conds(want, c.g['gamma'], c.d, c.dtype)
    if not rms:
        check(rep, 'mean (fp32 rule)', got[1], per[1], want[1], torch.float32, conds['mean'])
    check(rep, 'rstd (fp32 rule)', got[2], per[2], want[2], torch.float32, conds['rstd'])


def check_bwd(rep, got, per, want, rows, d, dtype):
    c = chain(d, dtype) * U
    nb = bwd_blocks(rows, d)
    c_col = math.ceil(rows / 4 / nb) + 4 + math.ceil(nb / 64) + 6
    dres, dx, dgamma, dbeta, mag_g, mag_b = want
    for name, g, p, w, cond in (('dres', got[0], per[0], dres, None), ('dx', got[1], per[1], dx, None),
                                ('dgamma', got[2], per[2], dgamma, None if mag_g is None else (c_col + 3) * U * mag_g),
                                ('dbeta', got[3], per[3], dbeta, None if mag_b is None else c_col * U * mag_b)):
        if g is None:
            continue
        check(rep, name, g, p, w, dtype, c * w.abs().amax(1) if cond is None else cond)


def same(a, b):
    return all((u is None) == (v is None) and (u is None or torch.equal(u, v)) for u, v in zip(a, b))


def ids(v):
    return str(v).replace('torch.', '').replace(' ', '')


FWD_CASES = [(dt, s) for dt in C.DTYPES for s in C.shapes(dt)]
BWD_CASES = [(dt, s) for dt in C.DTYPES for s in C.shapes(dt, backward=True)]


# ---------------------------------------------------------------------------------------------------------------------
# forward
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('rms', [False, True], ids=['ln', 'rms'])
@pytest.mark.parametrize('family', C.FAMILIES)
@pytest.mark.parametrize('dtype,shape', FWD_CASES, ids=ids)
def test_forward(dtype, shape, family, rms):
    rows, d = shape
    if (rows, d) == (8197, 64):
        assert rows > C.FWD_CAP * C.ROWS_PER_BLOCK     # ln_grid: the row loop takes a second trip
    c = case(family, rows, d, dtype)
    g, rep = c.g, {}
    # (residual, want_z, beta): every operand set the dispatch tells apart; the long shapes keep the two the models use
    variants = [(True, True, not rms), (False, False, not rms), (True, False, not rms), (False, True, not rms)]
    if not rms:
        variants += [(True, True, False), (False, False, False)]
    if rows > 1000:
        variants = variants[:2]
    for res, want_z, beta in variants:
        got = k_fwd(g['x'], g['residual'] if res else None, g['gamma'], g['beta'] if beta else None, rms, want_z)
        want, per = c.want_fwd(res, beta, rms), c.per_fwd(res, beta, rms)
        assert (got[1] is None) == rms
        check_fwd(rep, got, per, want, g['gamma'], d, dtype)
        if not res and dtype != torch.float32:
            check_stats_fp32(rep, got, c, want, rms)
        if family == 'constant':
            conds = fwd_conds(want, g['gamma'], d, dtype)
            b = g['beta'].double() if beta else torch.zeros(d, dtype=torch.float64, device='cuda')
            if not rms:   # RMSNorm does not centre: a constant row is not its degenerate case
                half_ulp = 0.5 * ulp_of(b.abs().unsqueeze(0) + conds['y'].unsqueeze(1), dtype)
                assert ((got[3].double() - b).abs() <= conds['y'].unsqueeze(1) + half_ulp).all()
                assert ((got[2].double() - EPS ** -0.5).abs() <= conds['rstd']).all()
    # the residual-only pass of the pre-norm blocks: z alone
    got = k_fwd(g['x'], g['residual'], None, None, False, True)
    check_fwd(rep, got, c.per_fwd(True, False, False, gamma=False), c.want_fwd(True, False, False, gamma=False), g['gamma'], d, dtype)
    print(f'forward {family} {shape} {ids(dtype)} rms {rms}: ' + ', '.join(f'{k} {v:.3f}' for k, v in rep.items()))


@pytest.mark.parametrize('dtype', [torch.bfloat16, torch.float16], ids=ids)
def test_specialised_forward_takes_a_second_trip(dtype):
    """residual_ln_fwd16_kernel keeps the next row in a second register set and works from it on every second trip of its row
    loop: C.SPECIALISED_FWD_LOOP is the smallest shape at which it does (the forward grid is capped at 2048 workgroups for
    every d).  Each of its five instances (launch_fwd: `fl` 5, 4, 7, 1, 3) against the reference, and rows of both trips
    against calls on the row alone"""
    rows, d = C.SPECIALISED_FWD_LOOP
    assert rows > C.FWD_CAP * C.ROWS_PER_BLOCK and d == 512
    c = case('distinct', rows, d, dtype)
    g, rep = c.g, {}
    for res, p, ln in ((True, 0.0, True), (False, 0.0, True), (True, 0.25, True), (True, 0.0, False), (True, 0.25, False)):
        got = k_fwd(g['x'], g['residual'] if res else None, g['gamma'] if ln else None, g['beta'] if ln else None, False, res or p > 0, p=p)
        check_fwd(rep, got, c.per_fwd(res, ln, False, p, gamma=ln), c.want_fwd(res, ln, False, p, gamma=ln), g['gamma'], d, dtype)
        if not res:
            check_stats_fp32(rep, got, c, c.want_fwd(res, ln, False, p), False)
        if not p:
            for r in (0, 5, C.FWD_CAP * C.ROWS_PER_BLOCK, rows - 1):
                one = slice(r, r + 1)
                alone = k_fwd(g['x'][one], g['residual'][one] if res else None, g['gamma'] if ln else None, g['beta'] if ln else None, False,
                              res, p=p)
                assert same(alone, tuple(None if t is None else t[one] for t in got)), (res, ln, r)
    print(f'specialised forward loop {ids(dtype)}: ' + ', '.join(f'{k} {v:.3f}' for k, v in rep.items()))


DROP_SHAPES = {torch.float32: [(5, 128), (5, 264), (3, 520)]}
DROP_SHAPES[torch.bfloat16] = DROP_SHAPES[torch.float16] = [(5, 128), (5, 520), (9, 512), (9, 1024), (3, 1032)]


@pytest.mark.parametrize('family', C.FAMILIES)
@pytest.mark.parametrize('dtype,shape', [(dt, s) for dt in C.DTYPES for s in DROP_SHAPES[dt]], ids=ids)
def test_forward_with_dropout(dtype, shape, family):
    """the mask is a pure function of (seed, offset, element index): pk_dropout's mask is the mask the LayerNorm kernels apply —
    the general one (dropout + LayerNorm without residual stays off the specialised kernels, launch_fwd: `fl` 6 has no
    instance) and, with a residual of zeros, the specialised one at d = 512 / 1024"""
    rows, d = shape
    c = case(family, rows, d, dtype)
    g, rep = c.g, {}
    ones, zeros = torch.ones_like(g['x']), torch.zeros_like(g['x'])
    for p in (0.25, 0.1) if shape in ((9, 512), (5, 264)) else (0.25,):
        keep = c.keep(p)
        assert 0 < keep.float().mean().item() < 1 or rows * d < 64
        for res in (None, zeros):
            z = k_fwd(ones, res, g['gamma'], g['beta'], False, True, p=p)[0]
            assert torch.equal(z != 0, keep)
        z2 = k_fwd(ones, None, g['gamma'], g['beta'], False, True, p=p, offset=OFFSET + 1)[0]
        assert not torch.equal(z2 != 0, keep), 'a second offset gave the same mask'
        for res, rms in ((True, False), (False, False), (True, True), (False, True)):
            got = k_fwd(g['x'], g['residual'] if res else None, g['gamma'], None if rms else g['beta'], rms, True, p=p)
            check_fwd(rep, got, c.per_fwd(res, not rms, rms, p), c.want_fwd(res, not rms, rms, p), g['gamma'], d, dtype)
            dropped = ~keep
            if not res:
                assert (got[0][dropped] == 0).all()
            else:
                assert torch.equal(got[0][dropped], g['residual'][dropped])
        got = k_fwd(g['x'], g['residual'], None, None, False, True, p=p)   # residual + dropout alone
        check_fwd(rep, got, c.per_fwd(True, False, False, p, gamma=False), c.want_fwd(True, False, False, p, gamma=False), g['gamma'], d, dtype)
    print(f'forward+dropout {family} {shape} {ids(dtype)}: ' + ', '.join(f'{k} {v:.3f}' for k, v in rep.items()))


# ---------------------------------------------------------------------------------------------------------------------
# backward
# ---------------------------------------------------------------------------------------------------------------------
def bwd_combos(rms, long_rows):
    """(dres, dx, p, extra, dgamma, dbeta): everything launch_bwd branches on"""
    outs = [(True, False, 0.0), (True, True, 0.0), (True, True, 0.25), (False, True, 0.0), (False, True, 0.25)]
    grads = [(False, False), (True, False)] if rms else [(False, False), (True, True), (True, False), (False, True)]
    if long_rows:    # the loop shapes: one call per kernel form and output set, the parameter gradients in each form
        both = (True, False) if rms else (True, True)
        return [(True, True, 0.25, True) + both, (True, False, 0.0, False) + both, (True, True, 0.0, True, True, False),
                (False, True, 0.25, False, False, False)] + ([] if rms else [(True, False, 0.0, True, False, True)])
    return [(r, x, p, e) + gr for (r, x, p) in outs for e in (False, True) for gr in grads]


@pytest.mark.parametrize('rms', [False, True], ids=['ln', 'rms'])
@pytest.mark.parametrize('family', C.FAMILIES)
@pytest.mark.parametrize('dtype,shape', BWD_CASES, ids=ids)
def test_backward(dtype, shape, family, rms):
    rows, d = shape
    cap = C.bwd_cap(rows, d)
    if rows > 1000:
        assert cap is not None and lib().load().pk_residual_ln_bwd_workspace(rows, d) == cap * 2 * d * 4   # the loop is entered
    c = case(family, rows, d, dtype)
    g, rep = c.g, {}
    z, mean, rstd = c.bwd_inputs(rms)
    for dres, dx, p, extra, dgamma, dbeta in bwd_combos(rms, rows > 1000):
        got = k_bwd(g['dy'], g['dz_extra'] if extra else None, z, g['gamma'], mean, rstd, dres=dres, dx=dx, dgamma=dgamma, dbeta=dbeta, p=p)
        check_bwd(rep, got, c.per_bwd(rms, extra, p), c.want_bwd(rms, extra, p), rows, d, dtype)
        if dx and p:
            assert (got[1][~c.keep(p)] == 0).all(), 'dx is not exactly 0 where the mask drops'
    # gamma == NULL: the pass-through of the pre-norm blocks, dz = dz_extra
    for dres, dx, p in ((True, True, 0.25), (False, True, 0.0), (True, False, 0.0)):
        got = k_bwd(None, g['dz_extra'], None, None, None, None, dres=dres, dx=dx, p=p)
        check_bwd(rep, got, c.per_bwd(rms, True, p, gamma=False), c.want_bwd(rms, True, p, gamma=False), rows, d, dtype)
        if dres:
            assert torch.equal(got[0], g['dz_extra'])
    print(f'backward {family} {shape} {ids(dtype)} rms {rms}: ' + ', '.join(f'{k} {v:.3f}' for k, v in rep.items()))


@pytest.mark.parametrize('rms', [False, True], ids=['ln', 'rms'])
@pytest.mark.parametrize('dtype,shape', BWD_CASES, ids=ids)
def test_forward_then_backward(dtype, shape, rms):
    """end to end on the kernel's own z, mean, rstd (family `distinct`); want and per are chained likewise"""
    rows, d = shape
    c = case('distinct', rows, d, dtype)
    g, f, rep, p = c.g, c.f, {}, 0.25
    keep = c.keep(p)
    beta = None if rms else g['beta']
    z, mean, rstd, y = k_fwd(g['x'], g['residual'], g['gamma'], beta, rms, True, p=p)
    got = k_bwd(g['dy'], g['dz_extra'], z, g['gamma'], mean, rstd, dres=True, dx=True, dgamma=True, dbeta=not rms, p=p)
    wz, wmean, wrstd, _ = R.fwd(f['x'], f['residual'], keep.cpu(), p, f['gamma'], None if rms else f['beta'], EPS, rms, store=dtype)
    want = R.bwd(f['dy'], f['dz_extra'], wz, f['gamma'], wmean, wrstd, keep.cpu(), p, rms)
    xhat = (wz if rms else wz - wmean.unsqueeze(1)) * wrstd.unsqueeze(1)
    want = tuple(None if o is None else o.cuda() for o in want + ((f['dy'] * xhat).abs().sum(0), f['dy'].abs().sum(0)))
    pz, pmean, prstd, _ = R.fwd(g['x'], g['residual'], keep, p, g['gamma'], beta, EPS, rms)
    per = R.bwd(g['dy'], g['dz_extra'], pz, g['gamma'], pmean, prstd, keep, p, rms)
    check_bwd(rep, got, per, want, rows, d, dtype)
    print(f'forward->backward {shape} {ids(dtype)} rms {rms}: ' + ', '.join(f'{k} {v:.3f}' for k, v in rep.items()))


# ---------------------------------------------------------------------------------------------------------------------
# the deferred parameter gradients
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('n', [1, 2, 3, 4])
@pytest.mark.parametrize('dtype,shape', [(torch.bfloat16, (9, 512)), (torch.float16, (2053, 520)), (torch.float32, (5, 264))], ids=ids)
def test_deferred_parameter_gradients_are_the_direct_ones_bit_for_bit(dtype, shape, n):
    """pk_residual_ln_bwd_partials per LayerNorm + one pk_ln_param_grads == pk_residual_ln_bwd (include/pasero_hip.h)"""
    L = lib()
    rows, d = shape
    nbytes = L.load().pk_residual_ln_bwd_workspace(rows, d)
    items = (PkLnParamGrad * n)()
    keepalive, direct = [], []
    for i in range(n):
        c = Case('distinct', rows, d, dtype, seed=i)
        z, mean, rstd = c.bwd_inputs(False)
        extra, p = (c.g['dz_extra'] if i % 2 else None), (0.25 if i < 2 else 0.0)
        args = (c.g['dy'], extra, z, c.g['gamma'], mean, rstd)
        direct.append(k_bwd(*args, dres=True, dx=bool(p), dgamma=i != 1, dbeta=i != 2, p=p, offset=OFFSET + i))
        ws = torch.full((nbytes // 4,), NAN, dtype=torch.float32, device='cuda').view(torch.uint8)
        dres, dx, _, _ = k_bwd(*args, dres=True, dx=bool(p), p=p, offset=OFFSET + i, defer_ws=ws)
        assert torch.isfinite(ws.view(torch.float32)).all()
        assert torch.equal(dres, direct[i][0]) and (dx is None) == (direct[i][1] is None) and (dx is None or torch.equal(dx, direct[i][1]))
        # item 1 asks for no dgamma, item 2 for no dbeta
        dg, db = (torch.full((d + 8,), NAN, dtype=dtype, device='cuda') for _ in range(2))
        items[i] = PkLnParamGrad(ws.data_ptr(), dg.data_ptr() if i != 1 else None, db.data_ptr() if i != 2 else None)
        keepalive.append((ws, dg, db, c))
    L.check(L.load().pk_ln_param_grads(items, n, rows, d, code(dtype), L.stream_ptr()), 'pk_ln_param_grads')
    torch.cuda.synchronize()
    for i, (ws, dg, db, _) in enumerate(keepalive):
        got_g, got_b = guard_ok('dgamma', dg, d, i != 1), guard_ok('dbeta', db, d, i != 2)
        for got, want in ((got_g, direct[i][2]), (got_b, direct[i][3])):
            assert (got is None) == (want is None) and (got is None or torch.equal(got, want)), i


# ---------------------------------------------------------------------------------------------------------------------
# exact properties
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('rms', [False, True], ids=['ln', 'rms'])
@pytest.mark.parametrize('dtype,shape', FWD_CASES, ids=ids)
def test_runs_repeat_and_rows_do_not_depend_on_their_neighbours(dtype, shape, rms):
    """two runs agree bit for bit; row r of a call (on the loop shapes: rows of the first and of the second trip) has the bits
    of a call on that row alone — dgamma / dbeta, sums over rows, excepted.  Without dropout: the mask follows the element index."""
    rows, d = shape
    c = case('distinct', rows, d, dtype)
    g = c.g
    beta = None if rms else g['beta']
    backward = shape in C.shapes(dtype, backward=True)
    fwd = k_fwd(g['x'], g['residual'], g['gamma'], beta, rms, True)
    assert same(fwd, k_fwd(g['x'], g['residual'], g['gamma'], beta, rms, True))
    z, mean, rstd, y = fwd
    if backward:
        kw = dict(dres=True, dx=True, dgamma=True, dbeta=not rms)
        bwd = k_bwd(g['dy'], g['dz_extra'], z, g['gamma'], mean, rstd, **kw)
        assert same(bwd, k_bwd(g['dy'], g['dz_extra'], z, g['gamma'], mean, rstd, **kw))
        drop = k_bwd(g['dy'], None, z, g['gamma'], mean, rstd, p=0.25, **kw)
        assert same(drop, k_bwd(g['dy'], None, z, g['gamma'], mean, rstd, p=0.25, **kw))
    trip = {8197: C.FWD_CAP, 4101: C.BWD_CAP_NARROW, 2053: C.BWD_CAP_WIDE}.get(rows, 0) * C.ROWS_PER_BLOCK
    for r in sorted({0, 3, 4, trip, trip + 2, rows - 1} & set(range(rows))):
        one = slice(r, r + 1)
        f1 = k_fwd(g['x'][one], g['residual'][one], g['gamma'], beta, rms, True)
        assert same(f1, tuple(None if t is None else t[one] for t in fwd)), r
        if backward:
            b1 = k_bwd(g['dy'][one], g['dz_extra'][one], z[one], g['gamma'], None if rms else mean[one], rstd[one], dres=True, dx=True)
            assert same(b1[:2], (bwd[0][one], bwd[1][one])), r


# ---------------------------------------------------------------------------------------------------------------------
# the fused block end on ill-conditioned rows
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('rms', [False, True], ids=['ln', 'rms'])
@pytest.mark.parametrize('family', ['offset', 'distinct'])
@pytest.mark.parametrize('dtype', [torch.bfloat16, torch.float16], ids=ids)
def test_fused_block_end_on_ill_conditioned_rows(dtype, family, rms):
    """pk_gemm_ln_fwd: the residual carries the family; per = torch matmul + ln_ref in the storage type.  z has one more ulp_T:
    the fused kernel rounds the GEMM result once where per rounds twice (tests/test_gemm_ln_gpu.py)"""
    from pasero_amd import functional as F
    M, K, N = 130, 64, 512
    c = case(family, M, N, dtype)
    gen = torch.Generator().manual_seed(M + K + N)
    x = torch.randn(M, K, generator=gen).to(dtype)
    w = (torch.randn(N, K, generator=gen) / K ** 0.5).to(dtype)
    b = (0.1 * torch.randn(N, generator=gen)).to(dtype)
    xg, wg, bg = x.cuda(), w.cuda(), b.cuda()
    assert F.gemm_ln_eligible(xg, wg)
    beta = None if rms else c.g['beta']
    y, z, mean, rstd = F.gemm_ln_fwd(xg, wg, bg, c.g['residual'], c.g['gamma'], beta, EPS, rms=rms)
    torch.cuda.synchronize()
    want = R.fwd(x.double() @ w.double().t() + b.double(), c.f['residual'], None, 0.0, c.f['gamma'], None if rms else c.f['beta'], EPS,
                 rms, store=dtype)
    want = tuple(None if o is None else o.cuda() for o in want)
    per = R.fwd(xg @ wg.t() + bg, c.g['residual'], None, 0.0, c.g['gamma'], beta, EPS, rms)
    rep = {}
    assert all(torch.isfinite(t).all() for t in (y, z, rstd))
    check_fwd(rep, (z, mean, rstd, y), per, want, c.g['gamma'], N, dtype, z_ulps=2)
    print(f'fused block end {family} {ids(dtype)} rms {rms}: ' + ', '.join(f'{k} {v:.3f}' for k, v in rep.items()))
