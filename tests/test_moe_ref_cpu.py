"""tests/moe_ref.py (the fp64 restatement the GPU tests compare against) replayed against what the real reference recorded in
tests/golden/moe.npz for one MoE layer: output, gate values, load-balancing loss and every gradient within 1e-5 of the
recorded fp32 values relative to max|value|, routing identical."""
import numpy as np
import torch

from conftest import load_golden
from moe_ref import gate_ref, layer_ref, route_ref
from moe_utils import layer_weights, relmax


def _replay():
    g = load_golden('moe')
    wg, w1, b1, w2, b2 = layer_weights(g)
    leaves = [wg] + w1 + b1 + w2 + b2
    for t in leaves:
        t.requires_grad_()
    x = torch.from_numpy(g['layer:x']).double().requires_grad_()
    pad = torch.from_numpy(g['layer:pad']).reshape(-1)
    y, gate = layer_ref(x.view(-1, x.size(-1)), pad, wg, w1, b1, w2, b2, act='relu')
    dy = torch.from_numpy(g['layer:dy']).double().view_as(y)
    ((y * dy).sum() + float(g['layer:lb_weight']) * gate['lb_loss']).backward()
    return g, x, y, gate, wg, w1, b1, w2, b2


def test_fixture_obeys_its_seed_rule():
    g = load_golden('moe')
    assert float(g['min_gap']) >= 1e-3
    assert float(g['model:search_min_gap']) >= 1e-3 * float(g['model:search_max_logit'])
    pad = g['layer:pad']
    assert pad.any() and pad[2, 2:].all() and not pad[0].any()   # padding tokens, one sentence tail fully padded
    assert g['layer:gate_value'].shape[-1] == 4


def test_layer_output_gate_and_loss():
    g, x, y, gate, *_ = _replay()
    assert relmax(y.detach().view(g['layer:y'].shape), g['layer:y']) <= 1e-5
    gv = gate['gate_value'].detach().view(g['layer:gate_value'].shape)
    assert relmax(gv, g['layer:gate_value']) <= 1e-5
    assert abs(float(gate['lb_loss']) - float(g['layer:lb_loss'])) <= 1e-5 * abs(float(g['layer:lb_loss']))
    pad = torch.from_numpy(g['layer:pad'])
    assert (y.detach().view(*pad.shape, -1)[pad] == 0).all() and (torch.from_numpy(g['layer:y'])[pad] == 0).all()
    assert gate['rank_gap'] >= 1e-3


def test_routing_is_the_reference_s():
    g, x, y, gate, *_ = _replay()
    rec = torch.from_numpy(g['layer:gate_value']).view(-1, 4)
    pad = torch.from_numpy(g['layer:pad']).reshape(-1)
    top = rec.topk(2).indices
    top[pad] = -1
    assert torch.equal(top, gate['top_idx'])
    offsets, slot_of, token_of = route_ref(gate['top_idx'], 4)
    assert int(offsets[-1]) == 2 * int((~pad).sum()) and (offsets[1:] > offsets[:-1]).all()   # every expert has a token
    assert (slot_of[pad] == -1).all() and sorted(slot_of[~pad].flatten().tolist()) == list(range(int(offsets[-1])))
    for s in range(int(offsets[-1])):
        e = int(np.searchsorted(offsets.numpy(), s, side='right')) - 1
        assert e in gate['top_idx'][int(token_of[s])].tolist()


def test_gradients():
    g, x, y, gate, wg, w1, b1, w2, b2 = _replay()
    assert relmax(x.grad, g['layer:dx']) <= 1e-5
    assert relmax(wg.grad, g['layer:grad:gate.weight']) <= 1e-5
    for e in range(4):
        for t, name in ((w1, 'fc1.weight'), (b1, 'fc1.bias'), (w2, 'fc2.weight'), (b2, 'fc2.bias')):
            assert relmax(t[e].grad, g[f'layer:grad:experts.{e}.{name}']) <= 1e-5, (e, name)


def test_ties_go_to_the_lower_index():
    logits = torch.tensor([[1.0, 1.0, 1.0, 0.0], [0.0, 2.0, 2.0, 2.0], [3.0, 0.0, 0.0, 3.0]])
    gate = gate_ref(logits, torch.zeros(3, dtype=torch.bool))
    assert gate['top_idx'].tolist() == [[0, 1], [1, 2], [0, 3]]
