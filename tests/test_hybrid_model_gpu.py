"""The whole `hybrid_transformer` against what the real reference recorded (tests/golden/hybrid.npz).  fp32: one training step
(loss within 1e-4 relative, the project's standing figure; gradients under the bounds test_moe_model_gpu.py applies to the
same digests), teacher-forced and incremental logits, the `return_layers` probabilities, and the recorded greedy and beam
searches token for token through pasero_amd.decode.  bf16: incremental decoding equals teacher forcing step by step (the
recurrence rounds h and c at every step either way); dropout; the adapter variant."""
import json

import numpy as np
import pytest
import torch

from conftest import load_golden
from hybrid_utils import hybrid_model
from model_utils import rel, text_batch

pytestmark = pytest.mark.gpu
ZERO_GRADS = ('k_proj.bias', 'inner_proj.bias')   # a bias that shifts every score of a softmax row: round-off only


def _step(model, batch):
    model.zero_grad(set_to_none=True)
    loss, logs = model(**batch)
    loss.backward()
    torch.cuda.synchronize()
    return loss, logs, {k: p.grad.clone() for k, p in model.named_parameters() if p.grad is not None}


@pytest.fixture(scope='module')
def fp32():
    g = load_golden('hybrid')
    cfg, model = hybrid_model(g)
    return g, cfg, model.cuda(), text_batch(g, 'cuda')


def test_training_step_against_the_reference(fp32):
    g, cfg, model, batch = fp32
    loss, logs, grads = _step(model.train(), batch)
    ref = float(g['loss'])
    print(f'loss {float(loss):.6f} (reference {ref:.6f})')
    assert abs(float(loss) - ref) <= 1e-4 * abs(ref)
    for key in ('loss', 'nll_loss'):
        assert abs(logs[key] - float(g['logs_' + key])) <= 1e-4 * abs(float(g['logs_' + key])), key
    assert logs['num_tokens'] == int(g['logs_num_tokens']) and logs['num_lines'] == int(g['logs_num_lines'])
    names = [str(n) for n in g['grad_names']]
    assert set(names) == set(grads)
    stride, worst = int(g['grad_stride']), 0.0
    for name, norm, total in zip(names, g['grad_norms'], g['grad_sums']):
        atol = 2e-5 if name.endswith(ZERO_GRADS) else 2e-6
        assert abs(float(grads[name].double().norm()) - float(norm)) <= 2e-4 * float(norm) + atol, name
        assert abs(float(grads[name].double().sum()) - float(total)) <= 2e-4 * float(norm) * np.sqrt(grads[name].numel()) + atol, name
        got, want = grads[name].cpu().reshape(-1)[::stride].double(), torch.from_numpy(g['gradsample:' + name]).double()
        typical = float(norm) / np.sqrt(grads[name].numel())
        err = float((got - want).abs().max())
        worst = max(worst, err / max(float(want.abs().max()), typical, 1e-30))
        assert err <= 1e-2 * max(float(want.abs().max()), typical) + (atol if name.endswith(ZERO_GRADS) else 1e-7), name
    print(f'worst sampled gradient error / typical element: {worst:.2e}')
    assert float(grads['decoder.attention.inner_proj.bias'].abs().max()) == 0.0
    _, _, again = _step(model, batch)
    assert all(torch.equal(grads[k], again[k]) for k in grads)   # two steps: bitwise equal gradients


def _encode(model, batch):
    enc_out, enc_mask, _ = model.encoder(batch['encoder_input'], batch['encoder_input_length'])
    return enc_out, enc_mask


def _incremental(dec, enc_out, enc_mask, dec_in):
    state, steps = {}, []
    for t in range(dec_in.size(1)):
        steps.append(dec(enc_out, enc_mask, dec_in[:, t:t + 1], state=state)[0])
    return torch.cat(steps, dim=1), state


def test_logits_probabilities_and_state(fp32):
    g, cfg, model, batch = fp32
    model.eval()
    dec, dec_in = model.decoder, batch['decoder_input'][:, :-1]
    with torch.no_grad():
        enc_out, enc_mask = _encode(model, batch)
        assert rel(enc_out, g['enc_out']) <= 2e-5
        logits, layers = dec(enc_out, enc_mask, dec_in, return_layers=[dec.cross_attn_key])
        inc, state = _incremental(dec, enc_out, enc_mask, dec_in)
        none, _ = dec(enc_out, enc_mask, dec_in)
    # 2e-5 of the range: the project's fp32 decoder-logits bound (tools/make_beam_golden.py's seed rule rests on it)
    print(f'teacher-forced {rel(logits, g["logits"]):.2e}, incremental {rel(inc, g["inc_logits"]):.2e}')
    assert rel(logits, g['logits']) <= 2e-5 and rel(inc, g['inc_logits']) <= 2e-5
    probs = layers[dec.cross_attn_key]
    assert list(layers) == [dec.cross_attn_key] and probs.shape == g['attn_probs'].shape
    assert rel(probs, g['attn_probs']) <= 2e-5
    assert (probs[enc_mask[:, None, None, :].expand_as(probs)] == 0).all()
    assert torch.equal(none, logits)
    assert {k: list(v.shape) for k, v in state.items()} == json.loads(str(g['state_shapes']))
    with torch.no_grad():
        features, _ = dec(enc_out, enc_mask, dec_in, project=False, prompt_mask=None, meta={})
    assert features.shape == (*dec_in.shape, cfg.embed_dim)


def test_searches_reproduce_the_reference(fp32):
    from pasero_amd.decode import beam_search, sampling
    g, cfg, model, batch = fp32
    model.eval()
    B = int(g['B'])
    with torch.no_grad():
        enc_out, enc_mask = _encode(model, batch)
        prompt = torch.full((B, 1), cfg.bos_idx, dtype=torch.long, device='cuda')
        greedy = sampling(model.decoder, enc_out, enc_mask, int(g['max_output_len']), {}, decoder_input=prompt,
                          sampling_temperature=0, return_scores=True)
        beam = beam_search(model.decoder, enc_out, enc_mask, int(g['max_output_len']), int(g['beam_size']), {},
                           decoder_input=prompt, return_scores=True)
    for b, nbest in enumerate(greedy):
        np.testing.assert_array_equal(nbest[0]['tokens'].cpu().numpy(), g[f'greedy:{b}:tokens'])
        ref = float(g[f'greedy:{b}:score'])
        assert abs(float(nbest[0]['pos_scores'].sum()) - ref) <= 1e-4 * max(1.0, abs(ref))
    assert [len(nb) for nb in beam] == g['beam:n_hyps'].tolist()
    for b, nbest in enumerate(beam):
        for i, h in enumerate(nbest):
            np.testing.assert_array_equal(h['tokens'].cpu().numpy(), g[f'beam:{b}:{i}:tokens'])
            ref = float(g[f'beam:{b}:{i}:score'])
            assert abs(float(h['score']) - ref) <= 1e-4 * max(1.0, abs(ref))


def test_bf16_incremental_equals_teacher_forced_step_by_step():
    g = load_golden('hybrid')
    cfg, model = hybrid_model(g)
    model = model.to(torch.bfloat16).cuda().eval()
    batch = text_batch(g, 'cuda')
    dec_in = batch['decoder_input'][:, :-1]
    with torch.no_grad():
        enc_out, enc_mask = _encode(model, batch)
        full, _ = model.decoder(enc_out, enc_mask, dec_in)
        inc, _ = _incremental(model.decoder, enc_out, enc_mask, dec_in)
        # a two-token prompt in the first call, one token per call after it
        state = {}
        first = model.decoder(enc_out, enc_mask, dec_in[:, :2], state=state)[0]
        rest = model.decoder(enc_out, enc_mask, dec_in[:, 2:3], state=state)[0]
    assert torch.isfinite(full).all()
    for t in range(dec_in.size(1)):
        assert torch.equal(inc[:, t], full[:, t]), t
    assert torch.equal(torch.cat([first, rest], dim=1), full[:, :3])


def test_mixed_parameter_dtypes_are_refused_by_name():
    g = load_golden('hybrid')
    cfg, model = hybrid_model(g)
    model = model.cuda().eval()
    model.decoder.layers[1].weight_hh_l0.data = model.decoder.layers[1].weight_hh_l0.data.to(torch.bfloat16)
    batch = text_batch(g, 'cuda')
    with torch.no_grad(), pytest.raises(TypeError, match='lstm_fwd: tensors of dtype'):
        model.decoder(*_encode(model, batch), batch['decoder_input'][:, :-1])


def test_dropout_step_is_finite_and_follows_the_seed():
    from pasero_amd import rng
    g = load_golden('hybrid')
    cfg, model = hybrid_model(g, dropout=0.1)
    model = model.cuda().train()
    batch = text_batch(g, 'cuda')
    losses = []
    for seed in (1, 1, 2):
        rng.manual_seed(seed)
        loss, _, grads = _step(model, batch)
        assert torch.isfinite(loss) and all(torch.isfinite(v).all() for v in grads.values())
        losses.append(float(loss))
    assert losses[0] == losses[1] and losses[0] != losses[2]
    assert abs(losses[0] - float(g['loss'])) > 1e-4 * float(g['loss'])   # (dropout is on)


def test_adapter_variant_trains_its_encoder_adapters_only():
    g = load_golden('hybrid')
    cfg, model = hybrid_model(g, adapter=True, encoder_adapters=['a'], decoder_adapters=['a'])
    model = model.cuda().train()
    loss, logs, grads = _step(model, text_batch(g, 'cuda'))
    assert torch.isfinite(loss) and logs['num_tokens'] == int(g['logs_num_tokens'])
    assert grads and all('.adapters.' in k and k.startswith('encoder.') for k in grads)
    assert all(torch.isfinite(v).all() for v in grads.values()) and any(float(v.abs().max()) > 0 for v in grads.values())
    assert all(p.grad is None for n, p in model.named_parameters() if n.startswith('decoder.'))
