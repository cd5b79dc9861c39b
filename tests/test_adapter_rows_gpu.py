"""pk_adapter_rows (csrc/adapter.hip) against an fp64 restatement of
    y = x + s * (act(LN(x) W_down^T + b_down) W_up^T + b_up)
over the same 16-bit inputs.  The tolerance is measured: the existing per-op sequence (autograd.AdapterFn under no_grad)
runs on every input, and the kernel may be off by at most twice the per-op path's own error plus one ulp of the storage
type at max|y| (factor 2: both round at the same three points — after LayerNorm, after the activation, at the output —
and differ only in the order of their sums).  Rows at or beyond `rows` are neither read (NaN there) nor written (a
sentinel there, compared bit for bit); two calls on one input agree bit for bit."""
import math

import pytest
import torch

pytestmark = pytest.mark.gpu

ROWS = [1, 5, 32, 33, 70]                      # one partial tile, a full tile, one row into the second, three tiles
SHAPES = [(128, 8), (1024, 64), (2048, 72)]    # (d, p): the smallest, the recipe's, the widest tile with p % 16 == 8
MANT = {torch.bfloat16: 7, torch.float16: 10, torch.float32: 23}
worst = {'ratio': 0.0}


def make(rows, d, p, dtype, seed, ln=True, biases=True):
    g = torch.Generator().manual_seed(seed)

    def rnd(*shape, scale=1.0, shift=0.0):
        return (torch.randn(*shape, generator=g) * scale + shift).to(dtype).cuda()
    t = {'x': rnd(rows, d), 'down_w': rnd(p, d, scale=d ** -0.5), 'up_w': rnd(d, p, scale=p ** -0.5),
         'ln_w': rnd(d, scale=0.1, shift=1.0) if ln else None, 'ln_b': rnd(d, scale=0.1) if ln else None,
         'down_b': rnd(p, scale=0.05) if biases else None, 'up_b': rnd(d, scale=0.05) if biases else None}
    return t


def ref64(t, act, scaling, eps):
    f = {k: (None if v is None else v.double().cpu()) for k, v in t.items()}
    h = f['x']
    if f['ln_w'] is not None:
        mean = h.mean(dim=1, keepdim=True)
        var = ((h - mean) ** 2).mean(dim=1, keepdim=True)
        h = (h - mean) / torch.sqrt(var + eps) * f['ln_w'] + f['ln_b']
    a = h @ f['down_w'].t()
    if f['down_b'] is not None:
        a = a + f['down_b']
    if act == 'relu':
        a = a.clamp_min(0)
    elif act == 'gelu_tanh':
        a = 0.5 * a * (1 + torch.tanh(math.sqrt(2 / math.pi) * (a + 0.044715 * a ** 3)))
    u = a @ f['up_w'].t()
    if f['up_b'] is not None:
        u = u + f['up_b']
    return f['x'] + scaling * u


def perop(t, act, scaling, eps):
    from pasero_amd.autograd import AdapterFn
    with torch.no_grad():
        return AdapterFn.apply(t['x'], t['x'], t['ln_w'], t['ln_b'], eps, t['down_w'], t['down_b'], t['up_w'], t['up_b'], act,
                               scaling, None)


def check(rows, d, p, dtype, seed, act='relu', scaling=1.0, ln=True, biases=True, alias=False, expect_fused=True):
    from pasero_amd import functional as F
    eps = 1e-5
    t = make(rows, d, p, dtype, seed, ln=ln, biases=biases)
    assert F.adapter_rows_fused(rows, d, p, dtype) == expect_fused
    want = ref64(t, act, scaling, eps)
    per = perop(t, act, scaling, eps)
    # 8 more rows behind the input and the output: NaN to read, a sentinel to overwrite
    x_full = torch.full((rows + 8, d), float('nan'), dtype=dtype, device='cuda')
    x_full[:rows] = t['x']
    y_full = x_full if alias else torch.full((rows + 8, d), 3.0, dtype=dtype, device='cuda')
    tail = y_full[rows:].clone()

    def run(xf, yf):
        return F.adapter_rows(xf[:rows], t['ln_w'], t['ln_b'], t['down_w'], t['down_b'], t['up_w'], t['up_b'], act=act,
                              scaling=scaling, eps=eps, out=yf[:rows])
    got = run(x_full, y_full)
    torch.cuda.synchronize()
    assert got.data_ptr() == y_full.data_ptr()
    ints = {2: torch.int16, 4: torch.int32}[tail.element_size()]
    assert torch.equal(y_full[rows:].view(ints), tail.view(ints)), 'rows beyond `rows` were written'
    assert torch.isfinite(got).all(), 'a row beyond `rows` (NaN) was read'
    # determinism, and (aliased) the same bits as the call into a separate output
    x2 = torch.full((rows + 8, d), float('nan'), dtype=dtype, device='cuda')
    x2[:rows] = t['x']
    again = run(x2, torch.full((rows + 8, d), 3.0, dtype=dtype, device='cuda'))
    assert torch.equal(got, again)
    err_new = (got.double().cpu() - want).abs().max().item()
    err_per = (per.double().cpu() - want).abs().max().item()
    ulp = 2.0 ** (math.floor(math.log2(want.abs().max().item())) - MANT[dtype])
    ratio = err_new / max(err_per, 1e-30)
    worst['ratio'] = max(worst['ratio'], ratio)
    print(f'rows {rows} d {d} p {p} {dtype} act {act} s {scaling} ln {ln} biases {biases} alias {alias}: kernel {err_new:.3e} '
          f'per-op {err_per:.3e} ratio {ratio:.3f} ulp {ulp:.3e} (worst ratio so far {worst["ratio"]:.3f})')
    assert err_new <= 2 * err_per + ulp


@pytest.mark.parametrize('dtype', [torch.bfloat16, torch.float16])
@pytest.mark.parametrize('d,p', SHAPES)
@pytest.mark.parametrize('rows', ROWS)
def test_tile_edges(rows, d, p, dtype):
    check(rows, d, p, dtype, seed=rows * 7 + d + p)


@pytest.mark.parametrize('dtype', [torch.bfloat16, torch.float16])
@pytest.mark.parametrize('opts', [dict(ln=False), dict(biases=False), dict(act='none'), dict(act='gelu_tanh'),
                                  dict(scaling=0.5), dict(alias=True), dict(alias=True, ln=False, biases=False, act='gelu_tanh')],
                         ids=lambda o: '-'.join(f'{k}={v}' for k, v in o.items()))
def test_options_at_the_smallest_shape(opts, dtype):
    for rows in (5, 33):
        check(rows, 128, 8, dtype, seed=3 + rows, **opts)


def test_fp32_takes_the_three_launch_route():
    check(33, 128, 8, torch.float32, seed=11, expect_fused=False)
    check(5, 128, 8, torch.float32, seed=12, scaling=0.5, act='gelu_tanh', expect_fused=False)


@pytest.mark.parametrize('dtype', [torch.bfloat16, torch.float16])
def test_a_bottleneck_outside_the_fused_range_takes_the_three_launch_route(dtype):
    check(33, 128, 12, dtype, seed=13, expect_fused=False)
    check(5, 1024, 12, dtype, seed=14, scaling=0.5, expect_fused=False)
