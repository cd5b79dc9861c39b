"""tests/ln_ref.py (the closed forms the LayerNorm GPU tests compare against) is right: in fp64, on every row family of
tests/ln_cases.py, for LayerNorm and RMSNorm, with and without residual / dropout mask / dz_extra, its forward equals
oracle/ref_cpu.py and torch.nn.functional.layer_norm and its backward, fed the exact statistics, equals torch autograd of the
composed `residual + x * keep / (1 - p) -> norm`.  1e-12 of max|value|; 1e-9 on `constant` rows, where rstd = eps^-1/2 = 316
amplifies the round-off of the mean.  (oracle.ref_cpu.rms_norm computes in fp32 as its original does: ln_ref is held to it at
fp32 precision, and to the fp64 statement of the same formula at 1e-12.)
A negative control shows that the `offset` family sees what it is there for: a one-pass fp32 variance E[z^2] - mu^2 misses
the fp64 rstd by more than 100 times what tests/test_layernorm_rows_gpu.py allows a kernel.  A second one does the same for
`distinct`: a row normalised with its neighbour's statistics misses that bound grossly in every storage type."""
import itertools

import pytest
import torch
import torch.nn.functional as TF

import ln_cases as C
import ln_ref as R
from oracle import ref_cpu as O

SHAPES = [(1, 8), (5, 72), (9, 264)]
P = 0.25


def close(got, want, tol):
    assert got.shape == want.shape
    assert (got - want).abs().max().item() <= tol * max(want.abs().max().item(), 1e-300), \
        ((got - want).abs().max().item(), want.abs().max().item())


def inputs(family, rows, d):
    t = {k: v.double() for k, v in C.make(family, rows, d, torch.float32, seed=1).items()}
    t['keep'] = torch.rand(rows, d, generator=torch.Generator().manual_seed(rows * d)) >= P
    return t


@pytest.mark.parametrize('family', C.FAMILIES)
@pytest.mark.parametrize('rows,d', SHAPES)
def test_forward_equals_the_oracle_and_torch(family, rows, d):
    tol = 1e-9 if family == 'constant' else 1e-12
    t = inputs(family, rows, d)
    for res, drop, beta in itertools.product((False, True), (False, True), (False, True)):
        residual, keep = (t['residual'] if res else None), (t['keep'] if drop else None)
        zin = (t['x'] * keep / (1 - P) if drop else t['x']) + (residual if res else 0)
        z, mean, rstd, y = R.fwd(t['x'], residual, keep, P, t['gamma'], t['beta'] if beta else None, C.EPS, False)
        close(z, zin, 1e-15)
        close(y, O.layer_norm(zin, t['gamma'], t['beta'] if beta else None, C.EPS), tol)
        close(y, TF.layer_norm(zin, (d,), t['gamma'], t['beta'] if beta else None, C.EPS), tol)
        close(mean, zin.mean(1), tol)
        close(rstd, 1 / torch.sqrt(zin.var(1, unbiased=False) + C.EPS), tol)
        z2, mean2, rstd2, y2 = R.fwd(t['x'], residual, keep, P, t['gamma'], None, C.EPS, True)
        assert mean2 is None and torch.equal(z2, z)
        close(y2, zin * torch.rsqrt((zin * zin).mean(1, keepdim=True) + C.EPS) * t['gamma'], 1e-12)
        close(y2, O.rms_norm(zin, t['gamma'], C.EPS), 2.0 ** -20)   # the oracle's RMSNorm is fp32 arithmetic
        close(rstd2, torch.rsqrt((zin * zin).mean(1) + C.EPS), 1e-12)
    z, mean, rstd, y = R.fwd(t['x'], t['residual'], None, 0.0, None, None, C.EPS, False)
    assert mean is None and rstd is None and y is None and torch.equal(z, t['residual'] + t['x'])


def test_forward_rounds_z_to_a_16_bit_storage_type():
    t = inputs('distinct', 5, 72)
    for store in (torch.bfloat16, torch.float16):
        z, mean, _, _ = R.fwd(t['x'], t['residual'], None, 0.0, t['gamma'], None, C.EPS, False, store=store)
        assert torch.equal(z, (t['x'] + t['residual']).to(store).double()) and torch.equal(mean, z.mean(1))
        z, _, _, _ = R.fwd(t['x'], None, None, 0.0, t['gamma'], None, C.EPS, False, store=store)
        assert z is t['x']                                # no residual, no dropout: z is x, which is stored already
    z, _, _, _ = R.fwd(t['x'], t['residual'], None, 0.0, t['gamma'], None, C.EPS, False, store=torch.float32)
    assert torch.equal(z, t['x'] + t['residual'])


@pytest.mark.parametrize('rms', [False, True], ids=['ln', 'rms'])
@pytest.mark.parametrize('family', C.FAMILIES)
@pytest.mark.parametrize('rows,d', SHAPES)
def test_backward_equals_autograd(family, rows, d, rms):
    tol = 1e-9 if family == 'constant' else 1e-12
    eps = C.EPS
    t = inputs(family, rows, d)
    for res, drop, extra in itertools.product((False, True), (False, True), (False, True)):
        x, residual = t['x'].clone().requires_grad_(), t['residual'].clone().requires_grad_()
        gamma, beta = t['gamma'].clone().requires_grad_(), t['beta'].clone().requires_grad_()
        keep = t['keep'] if drop else None
        zin = (x * keep / (1 - P) if drop else x) + (residual if res else 0)
        if rms:
            y = zin * torch.rsqrt((zin * zin).mean(1, keepdim=True) + eps) * gamma
        else:
            y = TF.layer_norm(zin, (d,), gamma, beta, eps)
        loss = (y * t['dy']).sum() + ((zin * t['dz_extra']).sum() if extra else 0)
        loss.backward()
        z, mean, rstd, _ = R.fwd(t['x'], t['residual'] if res else None, keep, P, t['gamma'], None if rms else t['beta'], eps, rms)
        dres, dx, dgamma, dbeta = R.bwd(t['dy'], t['dz_extra'] if extra else None, z, t['gamma'], mean, rstd, keep, P, rms)
        close(dx, x.grad, tol)
        if res:
            close(dres, residual.grad, tol)
        close(dgamma, gamma.grad, tol)
        if rms:
            assert dbeta is None
        else:
            close(dbeta, beta.grad, tol)
    # the pass-through of the pre-norm blocks: no LayerNorm, dz = dz_extra
    dres, dx, dgamma, dbeta = R.bwd(None, t['dz_extra'], None, None, None, None, t['keep'], P, False)
    assert torch.equal(dres, t['dz_extra']) and dgamma is None and dbeta is None
    close(dx, t['dz_extra'] * t['keep'] / (1 - P), 1e-15)


@pytest.mark.parametrize('rows,d', [(5, 128), (5, 264), (64, 512)])
def test_a_one_pass_fp32_variance_fails_the_offset_family(rows, d):
    """the allowance is that of tests/test_layernorm_rows_gpu.py for rstd in fp32: twice the per-op path's error (ln_ref in
    fp32), one fp32 ulp at rstd, and (lane chain + 8) * 2^-24 * rstd"""
    z32 = C.make('offset', rows, d, torch.float32)['x']
    gamma = torch.ones(d)
    _, _, want, _ = R.fwd(z32.double(), None, None, 0.0, gamma.double(), None, C.EPS, False)
    _, _, per, _ = R.fwd(z32, None, None, 0.0, gamma, None, C.EPS, False)
    one_pass = torch.rsqrt((z32 * z32).mean(1) - z32.mean(1) ** 2 + C.EPS)
    assert one_pass.dtype == torch.float32
    allowed = C.allowed(per, want, torch.float32, C.chain(d, torch.float32) * C.U * want)
    two_pass = (C.miss(per, want) / allowed).max().item()
    miss = (C.miss(one_pass, want) / allowed).max().item()
    print(f'offset fp32 ({rows}, {d}): one-pass rstd misses by {miss:.0f} x the allowance, two-pass by {two_pass:.2f} x')
    assert two_pass <= 1.0
    assert miss > 100.0


@pytest.mark.parametrize('dtype', C.DTYPES, ids=str)
def test_a_neighbours_statistics_fail_the_distinct_family(dtype):
    """every row of y normalised with the mean and rstd of the row before it, rounded to the storage type as a kernel would
    store it, against the allowance of tests/test_layernorm_rows_gpu.py for y (per = ln_ref in the storage type)"""
    rows, d = 9, 264
    t = C.make('distinct', rows, d, dtype)
    f = {k: v.double() for k, v in t.items()}
    z, mean, rstd, want = R.fwd(f['x'], None, None, 0.0, f['gamma'], f['beta'], C.EPS, False, store=dtype)
    per = R.fwd(t['x'], None, None, 0.0, t['gamma'], t['beta'], C.EPS, False)[3]
    wrong = ((z - mean.roll(1).unsqueeze(1)) * rstd.roll(1).unsqueeze(1) * f['gamma'] + f['beta']).to(dtype)
    allowed = C.allowed(per, want, dtype, C.fwd_conds(z, rstd, t['gamma'], d, dtype)['y'])
    ratios = C.miss(wrong, want) / allowed
    print(f'distinct {dtype}: the neighbour\'s statistics miss by {ratios.min().item():.0f} .. {ratios.max().item():.0f} x the allowance; '
          f'the per-op path itself by {(C.miss(per, want) / allowed).max().item():.2f} x')
    assert (C.miss(per, want) <= allowed).all()
    assert ratios.min().item() > 10.0
