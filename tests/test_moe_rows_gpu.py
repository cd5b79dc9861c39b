"""pk_moerows (csrc/moe_rows.hip): the mixture-of-experts layer for the rows of a decoding step in one native call, expert
weights at fan-in scale.  The grouped route against MixtureOfExperts.forward in eval mode (bitwise); the few route against the
fp64 restatement fed the same 16-bit inputs and the kernel's own routing, by the project's rule for a second 16-bit path:
e_few <= 2 * e_grouped + one ulp at max|y|."""
import contextlib
import math

import pytest
import torch

from moe_ref import ACTS

pytestmark = pytest.mark.gpu

DTYPES = {'bf16': torch.bfloat16, 'f16': torch.float16, 'f32': torch.float32}
MANT = {'bf16': 7, 'f16': 10}
# the smallest that can go wrong: one row; several experts; sizes that are no multiple of the 32-column tile (320) with an odd
# expert count; most experts empty; 33 slots per expert (three 16-slot chunks, a 1-slot tail, two passes over K); more rows
SHAPES = [(1, 2, 64, 64), (5, 4, 128, 128), (17, 7, 192, 320), (3, 256, 64, 64), (33, 4, 128, 128), (64, 16, 256, 192)]
PAD_ROWS = 3


def make_layer(rows, E, D, F, dtype, bias, act, seed=0):
    """(MixtureOfExperts on the device in eval mode, x (rows, D)); (33, 4, ...): every row chooses experts 0 and 1"""
    from pasero_amd.moe import MixtureOfExperts
    gen = torch.Generator().manual_seed(7919 * rows + 31 * E + D + F + seed)
    layer = MixtureOfExperts(D, F, E, E, activation_fn=act, has_bias=bias)
    x = torch.randn(rows, D, generator=gen)
    with torch.no_grad():
        layer.gate.weight.copy_(torch.randn(E, D, generator=gen) * (2.0 / math.sqrt(D)))
        for ex in layer.experts:
            ex.fc1.weight.copy_(torch.randn(F, D, generator=gen) / math.sqrt(D))
            ex.fc2.weight.copy_(torch.randn(D, F, generator=gen) / math.sqrt(F))
            if bias:
                ex.fc1.bias.copy_(torch.randn(F, generator=gen) * 0.1)
                ex.fc2.bias.copy_(torch.randn(D, generator=gen) * 0.1)
        if (rows, E) == (33, 4):
            x[:, 0] = 4.0
            layer.gate.weight[:, 0] = torch.tensor([3.0, 2.5, -3.0, -3.0])
    return layer.to(dtype).cuda().eval(), x.to(dtype).cuda()


def tables_of(layer):
    ex = layer.experts
    groups = (tuple(e.fc1.weight for e in ex), tuple(e.fc2.weight for e in ex),
              tuple(e.fc1.bias for e in ex) if layer.has_bias else None, tuple(e.fc2.bias for e in ex) if layer.has_bias else None)
    return layer._tables.get(groups)


@contextlib.contextmanager
def few_max(rows):
    from pasero_amd import functional as F
    prev = F.moe_rows_few_max(rows)
    try:
        yield
    finally:
        F.moe_rows_few_max(prev)


def run(layer, x, expect_few):
    """pk_moerows with y allocated PAD_ROWS rows too long and filled with NaN, the scratch pre-filled with 0xFF bytes; checks
    the route taken, the rows beyond, x, and that a second call gives the same bits"""
    from pasero_amd import lib
    from pasero_amd.lib import ACT, check, dtype_code, ptr, stream_ptr
    L = lib.load()
    rows, D = x.shape
    E, Fd, dt = layer.expert_count, layer.expert_dim, dtype_code(x)
    assert bool(L.pk_moerows_few(rows, E, D, Fd, dt)) == expect_few
    w1, w2, b1, b2 = tables_of(layer)
    nbytes = L.pk_moerows_scratch(rows, E, D, Fd, dt)
    assert nbytes > 0
    x0 = x.clone()
    outs = []
    for _ in range(2):
        y = torch.full((rows + PAD_ROWS, D), float('nan'), dtype=x.dtype, device=x.device)
        scratch = torch.full((nbytes,), 0xFF, dtype=torch.uint8, device=x.device)
        check(L.pk_moerows(ptr(x), ptr(y), ptr(layer.gate.weight), ptr(w1), ptr(b1), ptr(w2), ptr(b2), rows, E, D, Fd,
                           ACT[layer.act_name], dt, ptr(scratch), nbytes, stream_ptr()), 'pk_moerows')
        torch.cuda.synchronize()
        assert bool(torch.isnan(y[rows:]).all())           # rows >= `rows` are untouched
        assert not bool(torch.isnan(y[:rows]).any())
        outs.append(y[:rows].clone())
    assert torch.equal(x, x0)
    assert torch.equal(outs[0], outs[1])                   # two calls give the same bits
    return outs[0]


def module_forward(layer, x):
    with torch.no_grad():
        return layer(x.unsqueeze(0), None)[0].squeeze(0)


# ---- the grouped route: bitwise the module ----
@pytest.mark.parametrize('act', ['relu', 'gelu'])
@pytest.mark.parametrize('bias', [True, False])
@pytest.mark.parametrize('rows,E,D,F', SHAPES + [(5, 4, 72, 40)])
def test_grouped_route_fp32_is_the_module(rows, E, D, F, bias, act):
    layer, x = make_layer(rows, E, D, F, torch.float32, bias, act)
    assert torch.equal(run(layer, x, expect_few=False), module_forward(layer, x))


@pytest.mark.parametrize('dtype', ['bf16', 'f16'])
@pytest.mark.parametrize('rows,E,D,F,threshold', [s + (0,) for s in SHAPES] + [(5, 4, 72, 40, 256), (300, 4, 64, 64, 256)])
def test_grouped_route_16bit_is_the_module(rows, E, D, F, threshold, dtype):
    """threshold 0 forces it; sizes the few-rows kernels do not take (D % 64, more rows than the threshold) choose it"""
    layer, x = make_layer(rows, E, D, F, DTYPES[dtype], True, 'gelu')
    with few_max(threshold):
        got = run(layer, x, expect_few=False)
    assert torch.equal(got, module_forward(layer, x))


# ---- the few route ----
def routing_of(layer, x):
    """the kernel's own routing: pk_moerows_route over the gate logits of the same pk_gemm call pk_moerows makes"""
    from pasero_amd import functional as F
    from test_moe_route_rows_gpu import route
    r = route(F.gemm(x, layer.gate.weight))
    return r['top_idx'].long().cpu(), r['top_w'].double().cpu()


def restatement(layer, x, top_idx, top_w):
    """fp64: y[t] = sum_k top_w[t][k] * expert_{top_idx[t][k]}(x[t]) on the 16-bit inputs"""
    xd = x.double().cpu()
    y = torch.zeros_like(xd)
    act = ACTS[layer.act_name]
    for t in range(xd.size(0)):
        for k in range(2):
            ex = layer.experts[int(top_idx[t, k])]
            h = xd[t] @ ex.fc1.weight.double().cpu().t()
            if layer.has_bias:
                h = h + ex.fc1.bias.double().cpu()
            o = act(h) @ ex.fc2.weight.double().cpu().t()
            if layer.has_bias:
                o = o + ex.fc2.bias.double().cpu()
            y[t] += top_w[t, k] * o
    return y


@pytest.mark.parametrize('act', ['relu', 'gelu'])
@pytest.mark.parametrize('bias', [True, False])
@pytest.mark.parametrize('dtype', ['bf16', 'f16'])
@pytest.mark.parametrize('rows,E,D,F', SHAPES)
def test_few_route_against_fp64(rows, E, D, F, dtype, bias, act):
    layer, x = make_layer(rows, E, D, F, DTYPES[dtype], bias, act)
    few = run(layer, x, expect_few=True)
    with few_max(0):
        grouped = run(layer, x, expect_few=False)
    top_idx, top_w = routing_of(layer, x)
    if (rows, E) == (33, 4):
        assert top_idx.sort(dim=1).values.tolist() == [[0, 1]] * rows   # 33 slots for each of two experts, none for the others
    if E == 256:
        assert top_idx.unique().numel() <= 2 * rows  # most experts are empty
    want = restatement(layer, x, top_idx, top_w)
    e_few = (few.double().cpu() - want).abs().max().item()
    e_grouped = (grouped.double().cpu() - want).abs().max().item()
    ulp = 2.0 ** (math.floor(math.log2(want.abs().max().item())) - MANT[dtype])
    print(f'few {e_few:.3e} grouped {e_grouped:.3e} ulp at max|y| {ulp:.3e} (max|y| {want.abs().max().item():.3f})')
    assert e_few <= 2 * e_grouped + ulp


def test_few_route_through_the_functional_wrapper():
    from pasero_amd import functional as F
    layer, x = make_layer(5, 4, 128, 128, torch.bfloat16, True, 'relu')
    w1, w2, b1, b2 = tables_of(layer)
    y = F.moe_rows(x, layer.gate.weight, w1, w2, b1, b2, layer.expert_dim, layer.act_name)
    assert torch.equal(y, run(layer, x, expect_few=True))
