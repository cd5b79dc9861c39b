"""tests/hybrid_ref.py (the fp64 restatement the GPU tests compare against) replayed against what the real reference recorded
in tests/golden/hybrid.npz: teacher-forced and incremental logits, the attention probabilities, the training loss and every
gradient within 1e-5 of the recorded fp32 values relative to max|value| (the bound of test_moe_ref_cpu.py for the same
fp64-vs-recorded-fp32 comparison).  Two gradients are mathematically zero — a bias that shifts every score of a softmax row
equally (the encoder's k_proj.bias, the attention's inner_proj.bias): the restatement gives round-off of fp64 there and the
recorded fp32 values are round-off of fp32, checked against the 2e-5 test_moe_model_gpu.py allows such a gradient."""
import json

import numpy as np
import torch

import hybrid_ref as R
from conftest import golden_cfg, load_golden
from hybrid_utils import fp64_state
from model_utils import text_batch
from moe_utils import relmax

ZERO_GRADS = ('k_proj.bias', 'inner_proj.bias')


def _decoder_inputs(g):
    return (torch.from_numpy(g['enc_out']).double(), torch.from_numpy(g['enc_mask']), text_batch(g)['decoder_input'][:, :-1])


def test_fixture_obeys_its_seed_rule_and_size_limit():
    import os
    from conftest import GOLDEN
    g = load_golden('hybrid')
    assert float(g['search_min_gap']) >= 1e-3 * float(g['search_max_logit'])
    assert os.path.getsize(os.path.join(GOLDEN, 'hybrid.npz')) <= os.path.getsize(os.path.join(GOLDEN, 'moe.npz'))
    lengths = (~g['enc_mask']).sum(axis=1)
    assert len(set(lengths.tolist())) > 1 and g['enc_mask'].any()          # different source lengths: padded keys exist
    assert max(len(g[f'beam:{b}:0:tokens']) for b in range(int(g['B']))) > 1
    assert max(len(g[f'greedy:{b}:tokens']) for b in range(int(g['B']))) >= 3
    assert float(g['inc_vs_full']) <= 1e-5


def test_teacher_forced_logits_and_attention():
    g = load_golden('hybrid')
    cfg, P = golden_cfg(g), fp64_state(g)
    enc_out, enc_mask, dec_in = _decoder_inputs(g)
    logits, probs = R.decoder_forward(P, cfg, enc_out, enc_mask, dec_in)
    assert relmax(logits, g['logits']) <= 1e-5
    assert relmax(probs, g['attn_probs']) <= 1e-5 and probs.shape == g['attn_probs'].shape
    assert (probs[torch.from_numpy(g['enc_mask'])[:, None, None, :].expand_as(probs)] == 0).all()


def test_incremental_equals_teacher_forced():
    g = load_golden('hybrid')
    cfg, P = golden_cfg(g), fp64_state(g)
    enc_out, enc_mask, dec_in = _decoder_inputs(g)
    full, _ = R.decoder_forward(P, cfg, enc_out, enc_mask, dec_in)
    state, steps = {}, []
    for t in range(dec_in.size(1)):
        steps.append(R.decoder_forward(P, cfg, enc_out, enc_mask, dec_in[:, t:t + 1], state=state)[0])
        if t == 0:
            assert {k: list(v.shape) for k, v in state.items()} == json.loads(str(g['state_shapes']))
    inc = torch.cat(steps, dim=1)
    assert relmax(inc, full) <= 1e-12                    # fp64: the same arithmetic in another order
    assert relmax(inc, g['inc_logits']) <= 1e-5
    # a prompt of two tokens in the first call, then one token per call
    state = {}
    first = R.decoder_forward(P, cfg, enc_out, enc_mask, dec_in[:, :2], state=state)[0]
    rest = R.decoder_forward(P, cfg, enc_out, enc_mask, dec_in[:, 2:3], state=state)[0]
    assert relmax(torch.cat([first, rest], dim=1), full[:, :3]) <= 1e-12


def test_training_step_loss_and_gradients():
    from oracle import ref_cpu as O
    g = load_golden('hybrid')
    cfg, P = golden_cfg(g), fp64_state(g)
    for p in {id(v): v for v in P.values()}.values():
        p.requires_grad_()
    batch = text_batch(g)
    enc_out, enc_mask = O.encoder(P, cfg, batch['encoder_input'], batch['encoder_input_length'])
    assert relmax(enc_out.detach(), g['enc_out']) <= 1e-5 and np.array_equal(enc_mask.numpy(), g['enc_mask'])
    logits, _ = R.decoder_forward(P, cfg, enc_out, enc_mask, batch['decoder_input'][:, :-1])
    loss, nll, ntok = R.label_smoothed_ce(logits, batch['decoder_input'][:, 1:], cfg.padding_idx, cfg.label_smoothing)
    loss.backward()
    assert abs(float(loss.detach()) - float(g['loss'])) <= 1e-5 * abs(float(g['loss']))
    assert ntok == int(g['logs_num_tokens'])
    assert abs(float(nll.detach()) / np.log(2) - float(g['logs_nll_loss'])) <= 1e-5 * abs(float(g['logs_nll_loss']))
    stride = int(g['grad_stride'])
    names = [str(n) for n in g['grad_names']]
    assert 'decoder.layers.1.weight_hh_l0' in names and 'decoder.attention.inner_proj.weight' in names
    for name, norm, total in zip(names, g['grad_norms'], g['grad_sums']):
        grad = P[name].grad
        want = g['gradsample:' + name]
        if name.endswith(ZERO_GRADS):
            assert (grad is None or float(grad.abs().max()) <= 1e-12) and float(np.abs(want).max()) <= 2e-5, name
            continue
        assert relmax(grad.reshape(-1)[::stride], want) <= 1e-5, name
        assert abs(float(grad.norm()) - float(norm)) <= 1e-5 * float(norm), name
