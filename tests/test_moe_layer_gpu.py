"""The mixture-of-experts layer through MoEFn (pasero_amd.moe): fp32 against what the real reference recorded
(tests/golden/moe.npz), bf16 against tests/moe_ref.py in fp64 over the same bf16 inputs, the gate values through
`return_layers`, and forward + backward without a host synchronisation."""
import numpy as np
import pytest
import torch

import paramgen
from conftest import load_golden
from moe_ref import layer_ref
from moe_utils import layer_weights, moe_model, relmax

pytestmark = pytest.mark.gpu


def build_layer(g, dtype, gate_scale=1.0):
    from pasero_amd.moe import MixtureOfExperts
    wg, w1, b1, w2, b2 = layer_weights(g, torch.float32)
    layer = MixtureOfExperts(128, 128, 4, 4, activation_fn='relu')
    with torch.no_grad():
        layer.gate.weight.copy_(wg * gate_scale)
        for e, ex in enumerate(layer.experts):
            ex.fc1.weight.copy_(w1[e]); ex.fc1.bias.copy_(b1[e]); ex.fc2.weight.copy_(w2[e]); ex.fc2.bias.copy_(b2[e])
    return layer.to(dtype).cuda()


@pytest.mark.parametrize('grouped', [True, False], ids=['grouped', 'per_expert'])
def test_fp32_layer_against_the_reference(grouped):
    from pasero_amd import functional as F
    g = load_golden('moe')
    layer = build_layer(g, torch.float32)
    x = torch.from_numpy(g['layer:x']).cuda().requires_grad_()
    pad = torch.from_numpy(g['layer:pad']).cuda()
    prev = F.moe_use_grouped(int(grouped))
    try:
        y, gate_value, meta = layer(x, pad)
        ((y * torch.from_numpy(g['layer:dy']).cuda()).sum() + float(g['layer:lb_weight']) * layer.lb_loss).backward()
        torch.cuda.synchronize()
    finally:
        F.moe_use_grouped(int(prev))
    assert meta == {} and gate_value.dtype == torch.float32 and gate_value.shape == g['layer:gate_value'].shape
    errs = {'y': relmax(y.detach().cpu(), g['layer:y']), 'gate_value': relmax(gate_value.cpu(), g['layer:gate_value']),
            'dx': relmax(x.grad.cpu(), g['layer:dx'])}
    for name, p in layer.named_parameters():
        errs[name] = relmax(p.grad.cpu(), g['layer:grad:' + name])
    lb_err = abs(float(layer.lb_loss) - float(g['layer:lb_loss'])) / abs(float(g['layer:lb_loss']))
    print('fp32 layer, worst relative errors:', {k: f'{v:.1e}' for k, v in sorted(errs.items(), key=lambda kv: -kv[1])[:4]},
          f'lb_loss {lb_err:.1e}')
    assert all(v <= 1e-4 for v in errs.values()), errs
    assert lb_err <= 1e-5
    assert (y.detach()[pad] == 0).all() and (x.grad[pad] == 0).all()


def test_bf16_layer_against_fp64():
    g = load_golden('moe')
    bf = torch.bfloat16
    # the gate weights times 2 and a seeded input (paramgen seed 17, found by a search on the CPU) whose fp64 gate values at
    # ranks 1..3 are at least 0.02 apart for EVERY real token — a scale alone does not get the fixture's own input there
    layer = build_layer(g, bf, gate_scale=2.0)
    S, D = 15, 128
    x = torch.from_numpy(paramgen.make_array(17, 'moe_bf16_x', (S, D))).to(bf)
    dy = torch.from_numpy(g['layer:dy']).to(bf).view(S, D)
    pad = torch.from_numpy(g['layer:pad']).view(S)
    wg = layer.gate.weight.detach().cpu()
    ws = [[getattr(getattr(ex, fc), kind).detach().cpu() for ex in layer.experts]
          for fc, kind in (('fc1', 'weight'), ('fc1', 'bias'), ('fc2', 'weight'), ('fc2', 'bias'))]
    leaves = [wg.double().requires_grad_()] + [[t.double().requires_grad_() for t in group] for group in ws]
    x64 = x.double().requires_grad_()
    y_ref, gate = layer_ref(x64, pad, leaves[0], *leaves[1:], act='relu', logits_dtype=bf)
    assert gate['rank_gap'] >= 0.02, gate['rank_gap']       # on the fp64 values, every real token
    (y_ref * dy.double()).sum().backward()
    # the same formula per op in torch bf16 (CPU): its error against fp64 measures the precision of the format here
    xb = x.clone().requires_grad_()
    wb = [wg.clone().requires_grad_()] + [[t.clone().requires_grad_() for t in group] for group in ws]
    y_bf, _ = layer_ref(xb, pad, wb[0], *wb[1:], act='relu', dtype=bf)
    (y_bf * dy).sum().backward()

    xg = x.cuda().view(3, 5, D).requires_grad_()
    y, gate_value, _ = layer(xg, pad.view(3, 5).cuda())
    (y * dy.cuda().view(3, 5, D)).sum().backward()
    torch.cuda.synchronize()
    top = gate_value.view(S, 4).cpu().topk(2).indices
    top[pad] = -1
    assert torch.equal(top, gate['top_idx'])                # routing identical
    ulp = lambda t: 2.0 ** (np.floor(np.log2(float(t.abs().max()))) - 7)

    def ok(name, got, ref, torch_bf):
        e, e_bf = float((got.double().cpu() - ref).abs().max()), float((torch_bf.double() - ref).abs().max())
        print(f'bf16 {name}: err {e:.3e}, torch bf16 err {e_bf:.3e}, bound {2 * e_bf + ulp(ref):.3e}')
        assert e <= 2 * e_bf + ulp(ref), name
    ok('y', y.detach().view(S, D), y_ref.detach(), y_bf.detach())
    ok('dx', xg.grad.view(S, D), x64.grad, xb.grad)
    ok('gate.weight', layer.gate.weight.grad, leaves[0].grad, wb[0].grad)
    for e, ex in enumerate(layer.experts):
        for j, (fc, kind) in enumerate((('fc1', 'weight'), ('fc1', 'bias'), ('fc2', 'weight'), ('fc2', 'bias'))):
            ok(f'experts.{e}.{fc}.{kind}', getattr(getattr(ex, fc), kind).grad, leaves[1 + j][e].grad, wb[1 + j][e].grad)


def test_return_layers_gives_the_gate_values():
    g = load_golden('moe')
    cfg, model = moe_model(g)
    model = model.cuda().eval()
    from model_utils import text_batch
    b = text_batch(g, 'cuda')
    with torch.no_grad():
        _, _, outs = model.encoder(b['encoder_input'], b['encoder_input_length'], return_layers=['enc_1_gate', 'enc_0_gate'])
    assert set(outs) == {'enc_1_gate'}
    gv = outs['enc_1_gate']
    assert gv.shape == (int(g['B']), int(g['S']), 4) and gv.dtype == torch.float32
    real = torch.arange(int(g['S']), device='cuda')[None] < b['encoder_input_length'][:, None]
    assert torch.allclose(gv[real].sum(-1), torch.ones_like(gv[real].sum(-1)), atol=1e-6) and (gv[~real] == 0).all()


def test_forward_and_backward_do_not_synchronise_the_host():
    """method: torch.cuda.set_sync_debug_mode('error') around a warmed-up forward + backward (this torch build honours it on
    ROCm: the control below, a .item(), raises under it)"""
    g = load_golden('moe')
    layer = build_layer(g, torch.bfloat16)
    x = torch.from_numpy(g['layer:x']).to(torch.bfloat16).cuda().requires_grad_()
    pad = torch.from_numpy(g['layer:pad']).cuda()
    dy = torch.from_numpy(g['layer:dy']).to(torch.bfloat16).cuda()

    def step():
        y, _, _ = layer(x, pad)
        torch.autograd.backward([y, layer.lb_loss], [dy, torch.ones_like(layer.lb_loss)])
    step()                                    # builds the pointer tables and the workspaces
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode('error')
    try:
        step()
        with pytest.raises(RuntimeError):
            layer.lb_loss.item()              # the control: a host read IS caught
    finally:
        torch.cuda.set_sync_debug_mode('default')
    torch.cuda.synchronize()
