"""The whole fp32 moe_transformer against what the real reference recorded (tests/golden/moe.npz): one training step (loss,
logs, gradients), a greedy search through pasero_amd.decode on the per-op path, and the checkpoint layouts."""
import numpy as np
import pytest
import torch

from conftest import load_golden
from model_utils import text_batch
from moe_utils import moe_model

pytestmark = pytest.mark.gpu


def _step(model, batch):
    model.zero_grad(set_to_none=True)
    loss, logs = model(**batch)
    loss.backward()
    torch.cuda.synchronize()
    return loss, logs, {k: p.grad.clone() for k, p in model.named_parameters()}


def test_training_step_against_the_reference():
    g = load_golden('moe')
    cfg, model = moe_model(g)
    model = model.cuda().train()
    batch = text_batch(g, 'cuda')
    loss, logs, grads = _step(model, batch)
    ref = float(g['model:loss'])
    print(f'loss {float(loss):.6f} (reference {ref:.6f}), lb_loss {logs["lb_loss"]:.6f} ({float(g["model:logs_lb_loss"]):.6f})')
    assert abs(float(loss) - ref) <= 1e-4 * abs(ref)
    for key in ('loss', 'nll_loss', 'lb_loss'):
        assert abs(logs[key] - float(g['model:logs_' + key])) <= 1e-4 * abs(float(g['model:logs_' + key])), key
    assert logs['num_tokens'] == int(g['model:logs_num_tokens']) and logs['num_lines'] == int(g['model:logs_num_lines'])
    assert logs['capacity'] == float(g['model:logs_capacity']) == 0
    names = [str(n) for n in g['model:grad_names']]
    assert set(names) == set(grads)
    stride, worst = int(g['model:grad_stride']), 0.0
    for name, norm, total in zip(names, g['model:grad_norms'], g['model:grad_sums']):
        # the bounds of tests/test_model_gpu.py for fp32 gradients: the norm within 2e-4 (the tight check), a strided sample within
        # 1e-2 of the tensor's typical element (a ReLU pre-activation within round-off of 0 flips its derivative); a key bias
        # shifts all scores of a row equally — its gradient is mathematically zero, what is left is round-off
        atol = 2e-5 if name.endswith('k_proj.bias') else 2e-6
        assert abs(float(grads[name].double().norm()) - float(norm)) <= 2e-4 * float(norm) + atol, name
        # the sum of ALL elements: n terms each within 2e-4 of the tensor's typical element
        assert abs(float(grads[name].double().sum()) - float(total)) <= 2e-4 * float(norm) * np.sqrt(grads[name].numel()) + atol, name
        got, want = grads[name].cpu().reshape(-1)[::stride].double(), torch.from_numpy(g['model:gradsample:' + name]).double()
        typical = float(norm) / np.sqrt(grads[name].numel())
        err = float((got - want).abs().max())
        worst = max(worst, err / max(float(want.abs().max()), typical, 1e-30))
        assert err <= 1e-2 * max(float(want.abs().max()), typical) + (atol if name.endswith('k_proj.bias') else 1e-7), name
    print(f'worst sampled gradient error / typical element: {worst:.2e}')
    _, _, again = _step(model, batch)
    assert all(torch.equal(grads[k], again[k]) for k in grads)   # two steps: bitwise equal gradients


def _greedy(model, g, batch):
    from pasero_amd.decode import get_plan, sampling
    with torch.no_grad():
        enc_out, enc_mask, _ = model.encoder(batch['encoder_input'], batch['encoder_input_length'])
        prompt = torch.full((int(g['B']), 1), model.cfg.bos_idx, dtype=torch.long, device='cuda')
        hyps = sampling(model.decoder, enc_out, enc_mask, int(g['model:max_output_len']), {}, decoder_input=prompt,
                        sampling_temperature=0, return_scores=True)
    assert get_plan(model.decoder) is None   # an MoE decoder takes the per-op decoding path
    return hyps


def test_greedy_search_reproduces_the_reference():
    g = load_golden('moe')
    assert float(g['model:search_min_gap']) >= 1e-3 * float(g['model:search_max_logit'])
    cfg, model = moe_model(g)
    model = model.cuda().eval()
    hyps = _greedy(model, g, text_batch(g, 'cuda'))
    for b, nbest in enumerate(hyps):
        np.testing.assert_array_equal(nbest[0]['tokens'].cpu().numpy(), g[f'model:search:{b}:tokens'])
        ref = float(g[f'model:search:{b}:score'])
        assert abs(float(nbest[0]['pos_scores'].sum()) - ref) <= 1e-4 * max(1.0, abs(ref))


@pytest.mark.parametrize('layout', ['stacked', 'fused'])
def test_checkpoint_layouts_give_the_same_bits(layout):
    from pasero_amd import moe
    g = load_golden('moe')
    cfg, model = moe_model(g)
    basic = {k: v.clone() for k, v in model.state_dict().items()}
    batch = text_batch(g, 'cuda')
    model = model.cuda().eval()
    with torch.no_grad():
        want = model.decoder(*model.encoder(batch['encoder_input'], batch['encoder_input_length'])[:2],
                             batch['decoder_input'][:, :-1])[0].clone()
    sd = dict(basic)
    moe.stack_expert_params(sd, concat=layout == 'fused')
    _, other = moe_model(g)
    with torch.no_grad():
        for p in other.parameters():
            p.zero_()
    other.eval()
    other.update_state_dict(sd)
    other.load_state_dict(sd)
    other = other.cuda()
    with torch.no_grad():
        got = other.decoder(*other.encoder(batch['encoder_input'], batch['encoder_input_length'])[:2],
                            batch['decoder_input'][:, :-1])[0]
    assert torch.equal(got, want)


def test_decoding_when_every_decoder_layer_is_a_mixture():
    """decoder_expert_interval=1 (the configuration's default): layer 0 has no fc1; incremental decoding through the public
    search must run on the per-op path and give what a full forward pass over its own output gives"""
    from pasero_amd.decode import get_plan
    g = load_golden('moe')
    cfg, model = moe_model(g, decoder_expert_interval=1, encoder_expert_interval=1)
    model = model.cuda().eval()
    assert get_plan(model.decoder) is None
    batch = text_batch(g, 'cuda')
    hyps = _greedy(model, g, batch)
    with torch.no_grad():
        enc_out, enc_mask, _ = model.encoder(batch['encoder_input'], batch['encoder_input_length'])
        for b, nbest in enumerate(hyps):
            tokens = nbest[0]['tokens']
            assert tokens.numel() >= 1
            full = torch.cat([torch.tensor([cfg.bos_idx], device='cuda'), tokens[:-1]])[None]
            logits, _ = model.decoder(enc_out[b:b + 1], enc_mask[b:b + 1], full)
            assert torch.equal(logits[0].argmax(-1), tokens)   # the greedy choice at every position, without a cache
