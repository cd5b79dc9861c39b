"""pk_lstm_fwd / pk_lstm_bwd (csrc/lstm.hip) through `functional.lstm_fwd` and `hybrid.LSTMFn` against tests/hybrid_ref.py in
fp64 over the same storage-type inputs.  The tolerance is measured (the rule of test_adapter_rows_gpu.py): the per-op
composition in the same storage type — one torch matmul and the pointwise operations per step, h and c rounded at every step
— runs on every input on the GPU, and the kernel may be off by at most twice that path's own error plus one ulp of the storage
type at the output's magnitude (factor 2: the MFMA tiles add in another order).  The worst ratio is printed per test.  The
kernels write into outputs the test filled with NaN, over a scratch buffer filled with NaN.
Exact properties: a T-step call is T one-step calls bit for bit, and a row does not depend on the rows that share the call."""
import math

import pytest
import torch

import hybrid_ref as R

pytestmark = pytest.mark.gpu

# (B, T, In, H): one row and one step; a partial row tile; H = 96 (K not a multiple of 32) with two row tiles and an input
# width that is no multiple of 64; five row tiles
SHAPES = [(1, 1, 64, 64), (3, 5, 128, 64), (17, 9, 160, 96), (70, 3, 64, 128)]
DTYPES = [torch.float32, torch.bfloat16, torch.float16]
MANT = {torch.bfloat16: 7, torch.float16: 10, torch.float32: 23}
_cache = {}


def make(B, T, In, H, dtype, state=False, pad=0):
    """inputs on the GPU in `dtype`; gx is the storage-type product every path starts from (its rows `pad` elements apart
    beyond 4H when asked)"""
    key = (B, T, In, H, dtype, state, pad)
    if key not in _cache:
        g = torch.Generator().manual_seed(B * 1000 + T * 100 + In + H)
        rnd = lambda *shape, scale=1.0: (torch.randn(*shape, generator=g) * scale).to(dtype).cuda()
        x, w_ih, b_ih = rnd(B, T, In), rnd(4 * H, In, scale=In ** -0.5), rnd(4 * H, scale=0.1)
        gx = x @ w_ih.t() + b_ih
        if pad:
            wide = torch.full((B, T, 4 * H + pad), float('nan'), dtype=dtype, device='cuda')
            wide[..., :4 * H] = gx
            gx = wide[..., :4 * H]
        t = {'gx': gx, 'w_hh': rnd(4 * H, H, scale=H ** -0.5), 'b_hh': rnd(4 * H, scale=0.1),
             'h0': rnd(B, H, scale=0.5) if state else None, 'c0': rnd(B, H) if state else None, 'dy': rnd(B, T, H)}
        _cache[key] = t
    return _cache[key]


def nan_outputs(B, T, H, dtype):
    """y, c, gates, hT, cT for `functional.lstm_fwd(out=...)`, filled with NaN"""
    return tuple(torch.full(s, float('nan'), dtype=dtype, device='cuda')
                 for s in ((B, T, H), (B, T, H), (B, T, 4 * H), (B, H), (B, H)))


def nan_scratch(B, H, dtype):
    from pasero_amd import functional as F, lib
    nbytes = lib.load().pk_lstm_bwd_scratch(B, H, F.dtype_code(torch.empty(0, dtype=dtype)))
    lib.workspace(nbytes, torch.device('cuda', torch.cuda.current_device()), 'lstm').fill_(0xFF)


def ulp_at(want, dtype):
    return 2.0 ** (math.floor(math.log2(max(want.abs().max().item(), 1e-30))) - MANT[dtype])


def bound_check(what, got, per, want, dtype, worst):
    err_new = (got.double().cpu() - want).abs().max().item()
    err_per = (per.double().cpu() - want).abs().max().item()
    ulp = ulp_at(want, dtype)
    ratio = err_new / max(2 * err_per + ulp, 1e-300)
    worst[0] = max(worst[0], ratio)
    print(f'  {what}: kernel {err_new:.3e} per-op {err_per:.3e} ulp {ulp:.3e} -> {ratio:.3f} of the bound')
    assert torch.isfinite(got).all(), what
    assert err_new <= 2 * err_per + ulp, what


def f64(t):
    return {k: (None if v is None else v.double().cpu()) for k, v in t.items()}


@pytest.mark.parametrize('dtype', DTYPES, ids=str)
@pytest.mark.parametrize('state', [False, True], ids=['zero-state', 'h0-c0'])
@pytest.mark.parametrize('shape', SHAPES, ids=str)
def test_forward(shape, state, dtype):
    from pasero_amd import functional as F
    t = make(*shape, dtype, state=state)
    ref = f64(t)
    want = R.lstm(ref['gx'], ref['w_hh'], ref['b_hh'], ref['h0'], ref['c0'])
    per = R.lstm(t['gx'], t['w_hh'], t['b_hh'], t['h0'], t['c0'])
    B, T, _, H = shape
    y, c, gates, hT, cT = F.lstm_fwd(t['gx'], t['w_hh'], t['b_hh'], t['h0'], t['c0'], out=nan_outputs(B, T, H, dtype))
    torch.cuda.synchronize()
    worst = [0.0]
    for name, got, p, w in (('y', y, per[0], want[0]), ('hT', hT, per[1], want[1]), ('cT', cT, per[2], want[2])):
        bound_check(name, got, p, w, dtype, worst)
    assert torch.isfinite(c).all() and torch.isfinite(gates).all()
    assert torch.equal(hT, y[:, -1]) and torch.equal(cT, c[:, -1])
    print(f'{shape} {dtype} state {state}: worst {worst[0]:.3f} of the bound')


@pytest.mark.parametrize('dtype', DTYPES, ids=str)
@pytest.mark.parametrize('shape', SHAPES[1:], ids=str)
def test_t_steps_equal_t_one_step_calls(shape, dtype):
    from pasero_amd import functional as F
    t = make(*shape, dtype, state=True)
    y, c, gates, hT, cT = F.lstm_fwd(t['gx'], t['w_hh'], t['b_hh'], t['h0'], t['c0'])
    h, cc = t['h0'], t['c0']
    for step in range(shape[1]):
        y1, c1, g1, h, cc = F.lstm_fwd(t['gx'][:, step:step + 1], t['w_hh'], t['b_hh'], h, cc)
        assert torch.equal(y1[:, 0], y[:, step]) and torch.equal(c1[:, 0], c[:, step]), step
        assert torch.equal(g1[:, 0], gates[:, step]), step
    assert torch.equal(h, hT) and torch.equal(cc, cT)


@pytest.mark.parametrize('dtype', DTYPES, ids=str)
def test_a_row_does_not_depend_on_the_other_rows(dtype):
    from pasero_amd import functional as F
    t = make(*SHAPES[3], dtype, state=True)
    y, c, _, hT, cT = F.lstm_fwd(t['gx'], t['w_hh'], t['b_hh'], t['h0'], t['c0'])
    for b in (0, 15, 16, 37, 69):   # first and last row of a tile, a middle one, the last of the partial tile
        y1, c1, _, h1, cc1 = F.lstm_fwd(t['gx'][b:b + 1], t['w_hh'], t['b_hh'], t['h0'][b:b + 1], t['c0'][b:b + 1])
        assert torch.equal(y1[0], y[b]) and torch.equal(c1[0], c[b]) and torch.equal(h1[0], hT[b]) and torch.equal(cc1[0], cT[b]), b


@pytest.mark.parametrize('dtype', DTYPES, ids=str)
def test_gx_rows_wider_than_4h(dtype):
    from pasero_amd import functional as F
    shape = SHAPES[2]
    t, wide = make(*shape, dtype, state=False), make(*shape, dtype, state=False, pad=8)
    assert wide['gx'].stride(1) == 4 * shape[3] + 8 and torch.equal(wide['gx'], t['gx'])
    a = F.lstm_fwd(t['gx'], t['w_hh'], t['b_hh'])
    b = F.lstm_fwd(wide['gx'], t['w_hh'], t['b_hh'])
    assert all(torch.equal(u, v) for u, v in zip(a, b)) and torch.isfinite(b[0]).all()


@pytest.mark.parametrize('dtype', DTYPES, ids=str)
@pytest.mark.parametrize('state', [False, True], ids=['zero-state', 'h0-c0'])
@pytest.mark.parametrize('shape', SHAPES, ids=str)
def test_backward(shape, state, dtype):
    from pasero_amd import functional as F
    from pasero_amd.hybrid import LSTMFn
    t = make(*shape, dtype, state=state)

    def grads(fn, src):
        leaves = [src[k].detach().clone().requires_grad_() for k in ('gx', 'w_hh', 'b_hh')]
        y = fn(*leaves, src['h0'], src['c0'])[0]
        y.backward(src['dy'])
        return [leaf.grad for leaf in leaves]
    want = grads(R.lstm, f64(t))
    per = grads(R.lstm, t)
    got = grads(LSTMFn.apply, t)
    # the kernel alone, into an output and over a scratch that are NaN before the call: the same bits
    B, T, _, H = shape
    y, c, gates, _, _ = F.lstm_fwd(t['gx'], t['w_hh'], t['b_hh'], t['h0'], t['c0'], out=nan_outputs(B, T, H, dtype))
    nan_scratch(B, H, dtype)
    dg = F.lstm_bwd(t['dy'], t['w_hh'], c, gates, t['c0'], out=torch.full_like(gates, float('nan')))
    torch.cuda.synchronize()
    assert torch.isfinite(dg).all() and torch.equal(dg, got[0])
    worst = [0.0]
    for name, g, p, w in zip(('dgx', 'dW_hh', 'db_hh'), got, per, want):
        bound_check(name, g, p, w, dtype, worst)
    print(f'{shape} {dtype} state {state}: worst {worst[0]:.3f} of the bound')
