"""pk_moe_gemm / pk_moe_gemm_wgrad / gather / combine (csrc/moe.hip): the three grouped forms against fp64 over row distributions
chosen to break the tiling.  The tolerance is measured: pk_gemm runs each expert's contiguous slice with host-known counts, and
the grouped kernel may be off from fp64 by at most twice pk_gemm's own error plus one ulp of the storage type at max|C| — the
rule of tests/test_adapter_rows_gpu.py (same rounding points, different summation order)."""
import math

import pytest
import torch

pytestmark = pytest.mark.gpu

DISTS = {
    'zero_first': [0, 1, 129, 7],          # an expert without rows first; one row; tile + 1 rows
    'zero_middle': [5, 0, 130, 3],
    'zero_last': [9, 128, 1, 0],
    'all_on_one': [0, 0, 137, 0],
    'two_experts': [65, 65],               # E = 2, 2S = 130
    'many_experts': [2, 2] + [1] * 126,    # E = 128, 2S = 130
}
EXTRA = 6  # rows of capacity beyond offsets[E]: NaN in the inputs, a sentinel in the outputs
MANT = {torch.float32: 23, torch.bfloat16: 7, torch.float16: 10}


def ulp_at(max_abs, dtype):
    return 2.0 ** (math.floor(math.log2(max(max_abs, 1e-30))) - MANT[dtype])


def ptrs(tensors):
    return torch.tensor([t.data_ptr() for t in tensors], dtype=torch.int64).cuda()


def check(name, got, ref, base, dtype):
    """got, base: the grouped kernel's and pk_gemm's outputs; ref: fp64"""
    e_g = float((got.double() - ref).abs().max())
    e_b = float((base.double() - ref).abs().max())
    bound = 2 * e_b + ulp_at(float(ref.abs().max()), dtype)
    print(f'{name}: grouped err {e_g:.3e}, pk_gemm err {e_b:.3e}, bound {bound:.3e}, ratio {e_g / bound:.3f}')
    assert e_g <= bound, name


@pytest.mark.parametrize('dist', list(DISTS))
@pytest.mark.parametrize('dtype', [torch.float32, torch.bfloat16, torch.float16], ids=['fp32', 'bf16', 'fp16'])
@pytest.mark.parametrize('D, Fd', [(128, 128), (128, 264), (1024, 512)])
def test_grouped_forms(D, Fd, dtype, dist):
    from pasero_amd import functional as F
    counts = DISTS[dist]
    E, n = len(counts), sum(counts)
    rows = n + EXTRA
    offs = [0]
    for c in counts:
        offs.append(offs[-1] + c)
    offsets = torch.tensor(offs, dtype=torch.int32).cuda()
    gen = torch.Generator(device='cuda').manual_seed(D + Fd + E)
    rnd = lambda *shape, scale=1.0: (torch.randn(*shape, generator=gen, device='cuda') * scale).to(dtype)
    W = [rnd(Fd, D, scale=D ** -0.5) for _ in range(E)]
    b = [rnd(Fd, scale=0.1) for _ in range(E)]
    x, dy = rnd(rows, D), rnd(rows, Fd)
    x[n:], dy[n:] = float('nan'), float('nan')
    act = 'gelu' if dist == 'zero_middle' else 'relu'
    sentinel = lambda *shape: torch.full(shape, -7.25, dtype=dtype, device='cuda')

    # forward: C_e = act(A_e W_e^T + b_e), with the pre-activation
    h, pre = sentinel(rows, Fd), sentinel(rows, Fd)
    F.moe_gemm(x, ptrs(W), offsets, Fd, bias_ptrs=ptrs(b), act=act, preact=pre, out=h)
    h2 = F.moe_gemm(x, ptrs(W), offsets, Fd, bias_ptrs=ptrs(b), act=act, out=sentinel(rows, Fd))
    assert torch.equal(h[:n], h2[:n])                                        # two calls are bitwise equal
    assert (h[n:] == -7.25).all() and (pre[n:] == -7.25).all()               # nothing written beyond offsets[E]
    assert not torch.isnan(h[:n]).any()                                      # nothing read beyond it either
    # dX with act': C_e = (A_e W_e) * act'(aux)
    aux = pre if act != 'relu' else h
    dx = F.moe_gemm(dy, ptrs(W), offsets, D, b_col=True, out=sentinel(rows, D))
    Wt = [w.t().contiguous() for w in W]   # (kept alive: the table holds raw addresses)
    dxa = F.moe_gemm(x, ptrs(Wt), offsets, Fd, b_col=True, act=act, aux=aux, mode=2,
                     out=sentinel(rows, Fd))
    assert (dx[n:] == -7.25).all() and (dxa[n:] == -7.25).all() and not torch.isnan(dx[:n]).any()
    assert torch.equal(dx[:n], F.moe_gemm(dy, ptrs(W), offsets, D, b_col=True)[:n])
    assert torch.equal(dxa[:n], F.moe_gemm(x, ptrs(Wt), offsets, Fd, b_col=True, act=act, aux=aux, mode=2)[:n])
    # weight gradient
    dW = [sentinel(Fd, D) for _ in range(E)]
    db = [sentinel(Fd) for _ in range(E)]
    F.moe_gemm_wgrad(dy, x, offsets, ptrs(dW), ptrs(db))
    dW2 = [sentinel(Fd, D) for _ in range(E)]
    db2 = [sentinel(Fd) for _ in range(E)]
    F.moe_gemm_wgrad(dy, x, offsets, ptrs(dW2), None)
    F.moe_gemm_wgrad(dy, None, offsets, None, ptrs(db2))
    for e, c in enumerate(counts):
        assert torch.equal(dW[e], dW2[e]) and torch.equal(db[e], db2[e])
        if c == 0:
            assert (dW[e] == 0).all() and (db[e] == 0).all()                 # an expert without rows: exactly 0

    acts = {'relu': torch.relu, 'gelu': torch.nn.functional.gelu}
    for e, c in enumerate(counts):
        if c == 0:
            continue
        lo, hi = offs[e], offs[e + 1]
        xe, dye, We = x[lo:hi].double(), dy[lo:hi].double(), W[e].double()
        pre_ref = xe @ We.t() + b[e].double()
        base_pre = torch.empty(c, Fd, dtype=dtype, device='cuda')
        base_h = F.gemm(x[lo:hi], W[e], bias=b[e], act=act, preact=base_pre)
        tag = f'{dist} {D}x{Fd} expert {e} ({c} rows)'
        check(tag + ' forward', h[lo:hi], acts[act](pre_ref), base_h, dtype)
        check(tag + ' preact', pre[lo:hi], pre_ref, base_pre, dtype)
        check(tag + ' dX', dx[lo:hi], dye @ We, F.gemm(dy[lo:hi], W[e], b_col=True), dtype)
        a64 = aux[lo:hi].double().requires_grad_()
        dact, = torch.autograd.grad(acts[act](a64).sum(), a64)
        check(tag + " dX act'", dxa[lo:hi], (xe @ We.t()) * dact,
              F.gemm(x[lo:hi], Wt[e], b_col=True, act=act, aux=aux[lo:hi], mode=2), dtype)
        base_db = torch.empty(Fd, dtype=dtype, device='cuda')
        base_dw = F.gemm(dy[lo:hi], x[lo:hi], a_col=True, b_col=True, asum_out=base_db)
        check(tag + ' dW', dW[e], dye.t() @ xe, base_dw, dtype)
        check(tag + ' db', db[e], dye.sum(0), base_db, dtype)


@pytest.mark.parametrize('dtype', [torch.float32, torch.bfloat16], ids=['fp32', 'bf16'])
def test_gather_combine_dot(dtype):
    from pasero_amd import functional as F
    from test_moe_gate_gpu import make_logits, make_pad
    S, E, D = 65, 4, 136
    logits, pad = make_logits(S, E, 5), make_pad(S, 'scattered', 5)
    r = F.moe_gate(logits.cuda(), pad.cuda())
    n = int(r.offsets[-1])
    gen = torch.Generator(device='cuda').manual_seed(3)
    x = torch.randn(S, D, generator=gen, device='cuda').to(dtype)
    ys = torch.randn(2 * S, D, generator=gen, device='cuda').to(dtype)
    token_of, slot_of = r.token_of[:n].long(), r.slot_of.long()
    real = (~pad).cuda()
    xg = F.moe_gather(x, r)
    assert torch.equal(xg[:n], x[token_of])
    k_of = (slot_of[token_of, 1] == torch.arange(n, device='cuda')).long()
    scaled = F.moe_gather(x, r, scaled=True)
    assert torch.equal(scaled[:n], (x[token_of].float() * r.top_w[token_of, k_of, None]).to(dtype))
    safe = slot_of.clamp_min(0)
    want = (r.top_w[:, 0, None] * ys[safe[:, 0]].float() + r.top_w[:, 1, None] * ys[safe[:, 1]].float()) * real[:, None]
    out = F.moe_combine(ys, r)
    # (w0 a + w1 b: the kernel may fuse the second product into the addition — one rounding fewer than torch's three — so the
    # two agree to one ulp of the storage type at max|out|; every other form here has a single rounding and is exact)
    assert float((out.double() - want.double()).abs().max()) <= ulp_at(float(want.abs().max()), dtype)
    assert (out[pad.cuda()] == 0).all() and torch.equal(out, F.moe_combine(ys, r))
    plain = F.moe_combine(ys, r, weighted=False)
    assert torch.equal(plain, ((ys[safe[:, 0]].float() + ys[safe[:, 1]].float()) * real[:, None]).to(dtype))
    dots = F.moe_dot(x, ys, r)
    ref = torch.stack([(x.double() * ys[safe[:, k]].double()).sum(1) for k in range(2)], 1) * real[:, None]
    assert float((dots.double() - ref).abs().max()) <= 1e-5 * float(ref.abs().max())   # fp32 accumulation of 136 products
    assert torch.equal(dots, F.moe_dot(x, ys, r))
