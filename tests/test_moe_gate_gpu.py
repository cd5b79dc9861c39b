"""pk_moe_gate / pk_moe_gate_bwd (csrc/moe.hip) against tests/moe_ref.py in fp64: exact routing, gate values and weights within
4 fp32 ulps at max|value|, exact counts, the lower-index tie rule, bitwise repeatability, and the backward through the
normalisation, the mask and the softmax."""
import numpy as np
import pytest
import torch

from moe_ref import gate_ref, route_ref

pytestmark = pytest.mark.gpu


def make_logits(S, E, seed):
    """random logits whose three best experts per token are spaced a unit apart: the fp64 gate values at ranks 1..3 differ by
    far more than fp32 rounding, so the ranking does not depend on it"""
    gen = torch.Generator().manual_seed(seed)
    logits = torch.randn(S, E, generator=gen)
    k = min(E, 3)
    pick = torch.rand(S, E, generator=gen).argsort(1)[:, :k]
    top = logits.max(1, keepdim=True).values
    logits.scatter_(1, pick, top + torch.arange(k, 0, -1, dtype=torch.float32))
    return logits


def make_pad(S, pattern, seed):
    if pattern == 'none':
        return torch.zeros(S, dtype=torch.bool)
    if pattern == 'all':
        return torch.ones(S, dtype=torch.bool)
    pad = torch.rand(S, generator=torch.Generator().manual_seed(seed)) < 0.3
    pad[0] = S > 1  # (scattered: at least one padding token where there is room for a real one too)
    pad[-1] = False
    return pad


def ulps(x):
    return 4 * float(np.spacing(np.float32(max(float(x.abs().max()), 1e-30))))


@pytest.mark.parametrize('pattern', ['none', 'scattered', 'all'])
@pytest.mark.parametrize('E', [2, 3, 4, 128, 256])
@pytest.mark.parametrize('S', [1, 63, 64, 65, 257])
def test_gate_against_fp64(S, E, pattern):
    from pasero_amd import functional as F
    logits, pad = make_logits(S, E, 1000 * S + E), make_pad(S, pattern, S + E)
    ref = gate_ref(logits, pad)
    if not pad.all():
        assert ref['rank_gap'] >= 1e-4, ref['rank_gap']
    r = F.moe_gate(logits.cuda(), pad.cuda())
    r2 = F.moe_gate(logits.cuda(), pad.cuda())
    torch.cuda.synchronize()
    offsets, slot_of, token_of = route_ref(ref['top_idx'], E)
    n = int(offsets[-1])
    assert torch.equal(r.top_idx.cpu().long(), ref['top_idx'])
    assert torch.equal(r.offsets.cpu(), offsets) and torch.equal(r.slot_of.cpu(), slot_of)
    assert torch.equal(r.token_of.cpu()[:n], token_of)
    assert torch.equal(r.top1_count.cpu().long(), ref['top1_count'])
    gv_err = (r.gate_value.cpu().double() - ref['gate_value']).abs().max()
    tw_err = (r.top_w.cpu().double() - ref['top_w']).abs().max()
    print(f'S {S} E {E} {pattern}: gate_value err {float(gv_err):.2e} (bound {ulps(ref["gate_value"]):.2e}), top_w err '
          f'{float(tw_err):.2e} (bound {ulps(ref["top_w"]):.2e})')
    assert gv_err <= ulps(ref['gate_value']) and tw_err <= ulps(ref['top_w'])
    assert (r.gate_value.cpu()[pad] == 0).all() and (r.top_w.cpu()[pad] == 0).all()
    # fixed-order fp32 sums of at most S terms in [0, 1]: S ulps of the sum at the very most
    assert (r.prob_sum.cpu().double() - ref['prob_sum']).abs().max() <= S * float(np.spacing(np.float32(max(1.0, S))))
    lb = float(ref['lb_loss'])
    assert abs(float(r.lb_loss) - lb) <= 1e-5 * max(abs(lb), 1e-30) + (0 if n else 1e-30)
    for name in ('gate_value', 'top_idx', 'top_w', 'top1_count', 'prob_sum', 'lb_coef', 'lb_loss', 'offsets', 'slot_of'):
        assert torch.equal(getattr(r, name), getattr(r2, name)), name   # two calls agree bit for bit
    assert torch.equal(r.token_of[:n], r2.token_of[:n])


def test_ties_go_to_the_lower_index():
    from pasero_amd import functional as F
    logits = torch.tensor([[1.0, 1.0, 1.0, 0.0], [0.0, 2.0, 2.0, 2.0], [3.0, 0.0, 0.0, 3.0], [0.5, 0.5, 0.5, 0.5]])
    r = F.moe_gate(logits.cuda(), None)
    assert r.top_idx.cpu().tolist() == [[0, 1], [1, 2], [0, 3], [0, 1]]
    wide = torch.zeros(5, 200)
    wide[1, 70] = wide[1, 199] = wide[1, 3] = 1.0   # equal values in different lanes and registers of the wave
    wide[2, 130] = 2.0
    r = F.moe_gate(wide.cuda(), None)
    assert r.top_idx.cpu().tolist() == [[0, 1], [3, 70], [130, 0], [0, 1], [0, 1]]
    assert torch.equal(r.top_idx.cpu().long(), gate_ref(wide, torch.zeros(5, dtype=torch.bool))['top_idx'])


@pytest.mark.parametrize('S, E', [(1, 2), (65, 3), (257, 4), (64, 128), (63, 256)])
def test_gate_bwd_against_fp64_autograd(S, E):
    from pasero_amd import functional as F
    logits, pad = make_logits(S, E, 7 * S + E), make_pad(S, 'scattered' if S > 1 else 'none', S)
    gen = torch.Generator().manual_seed(S * E)
    d_top_w = torch.randn(S, 2, generator=gen)
    lb_up = torch.randn((), generator=gen).abs() + 0.5
    lg = logits.double().requires_grad_()
    ref = gate_ref(lg, pad)
    ((ref['top_w'] * d_top_w.double()).sum() + 3.0 * lb_up.double() * ref['lb_loss']).backward()
    r = F.moe_gate(logits.cuda(), pad.cuda())
    got = F.moe_gate_bwd(d_top_w.cuda(), r, lb_up.cuda(), 3.0).cpu().double()
    err = float((got - lg.grad).abs().max() / lg.grad.abs().max())
    print(f'S {S} E {E}: gate backward rel err {err:.2e}')
    assert err <= 1e-5                      # fp32 arithmetic on O(1) values over at most 256 terms
    assert (got[pad] == 0).all()
    only_w = F.moe_gate_bwd(d_top_w.cuda(), r).cpu().double()   # without the load-balancing term
    lg2 = logits.double().requires_grad_()
    (gate_ref(lg2, pad)['top_w'] * d_top_w.double()).sum().backward()
    assert float((only_w - lg2.grad).abs().max() / lg2.grad.abs().max()) <= 1e-5


def test_a_row_of_nan_logits_still_routes_inside_the_tables():
    """a non-finite activation must not become an index outside the expert range: the row takes experts 0 and 1"""
    from pasero_amd import functional as F
    logits = make_logits(5, 4, 3)
    logits[2] = float('nan')
    r = F.moe_gate(logits.cuda(), None)
    torch.cuda.synchronize()
    assert r.top_idx.cpu()[2].tolist() == [0, 1]
    assert int(r.offsets[-1]) == 10 and int(r.slot_of.min()) >= 0 and int(r.slot_of.max()) == 9
    keep = [0, 1, 3, 4]
    assert torch.equal(r.top_idx.cpu()[keep].long(), gate_ref(logits[keep], torch.zeros(4, dtype=torch.bool))['top_idx'])
