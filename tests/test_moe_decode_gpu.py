"""Native decoding of `moe_transformer` decoders (pk_decoder_step_moe: the decoding step with a mixture layer's feed-forward
block as one pk_moerows call), switched on with `decode.moe_native`: what the plan is keyed on, the incremental decoding and the
searches the real reference recorded (tests/golden/moe_decode.npz, written by tools/make_moe_decode_golden.py), the bf16 step
against the per-op path, and a beam search in which a sentence leaves the batch."""
import copy
import math

import numpy as np
import pytest
import torch

import paramgen
from conftest import load_golden
from moe_utils import moe_model

pytestmark = pytest.mark.gpu
VARIANTS = ('mix', 'all')   # decoder_expert_interval 2 (a dense and a mixture layer) and 1 (layer 0 has no fc1)
BF16_MANT = 7


@pytest.fixture
def native():
    """the switch on for the test, restored afterwards"""
    from pasero_amd import decode
    prev = decode.moe_native(True)
    yield decode
    decode.moe_native(prev)


def load_variant(name, seed_key='seed'):
    g = load_golden('moe_decode')
    p = name + ':'
    c = {k[len(p):]: g[k] for k in g.files if k.startswith(p)}
    c.update(V=g['V'], S=g['S'], max_output_len=g['max_output_len'], beam_size=g['beam_size'])
    cfg, model = moe_model({'cfg': c['cfg'], 'moe_cfg': c['moe_cfg'], 'V': c['V'], 'seed': c[seed_key]})
    return c, cfg, model.cuda().eval()


def encode(c, model, B, seed):
    b = paramgen.make_text_batch(int(seed), int(B), int(c['S']), 5, int(c['V']))
    with torch.no_grad():
        enc_out, enc_mask, _ = model.encoder(torch.from_numpy(b['encoder_input']).cuda(),
                                             torch.from_numpy(b['encoder_input_length']).cuda())
    return enc_out, enc_mask


def gate_keys(decoder):
    return [layer.gate_key for layer in decoder.layers if hasattr(layer, 'gate_key')]


def run_steps(model, enc_out, enc_mask, tokens, return_gates=False):
    """logits (steps, B, V) fp32 of the incremental calls after the first one, whether the native step ran and — with
    return_gates, which sends every call to the per-op path — the gate values (calls, layers, B, E) of EVERY call"""
    dec = model.decoder
    keys = gate_keys(dec) if return_gates else []
    state, out, gates = {}, [], []
    with torch.no_grad():
        for t in range(tokens.size(1)):
            logits, layers = dec(enc_out, enc_mask, tokens[:, t:t + 1], state=state, return_layers=keys)
            if t > 0:
                out.append(logits[:, -1].float().clone())
            if return_gates:
                gates.append(torch.stack([layers[k][:, -1].float() for k in keys]))
    return torch.stack(out), '_pk_decode' in state, (torch.stack(gates) if return_gates else None)


# ---- what the plan is keyed on ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('name', VARIANTS)
def test_the_switch_is_part_of_the_plan_key(name):
    from pasero_amd import decode
    c, cfg, model = load_variant(name)
    dec = model.decoder
    prev = decode.moe_native(False)
    try:
        assert decode.get_plan(dec) is None                 # today's behaviour
        decode.moe_native(True)
        plan = decode.get_plan(dec)
        assert plan is not None and plan.c_moe is not None
        want = [4 if hasattr(layer, 'moe_layer') else 0 for layer in dec.layers]
        assert [m.E for m in plan.c_moe] == want and sum(want) > 0
        assert all((m.F, bool(m.gate_w), bool(m.w1), bool(m.w2)) == ((128, True, True, True) if m.E else (0, False, False, False))
                   for m in plan.c_moe)
        for lw, m in zip(plan.c_layers, plan.c_moe):       # fc1 / fc2 of a mixture layer are NULL
            assert (lw.fc1_w is None) == (lw.fc2_w is None) == bool(m.E)
        assert decode.get_plan(dec) is plan                 # cached
        decode.moe_native(False)
        assert decode.get_plan(dec) is None
    finally:
        decode.moe_native(prev)


def test_moved_and_replaced_parameters_rebuild_the_plan(native):
    c, cfg, model = load_variant('mix')
    dec = model.decoder
    enc = encode(c, model, 3, c['seed'])
    tokens = torch.from_numpy(c['tf:tokens'])[:3, :3].cuda()
    plan = native.get_plan(dec)
    assert plan is not None
    before, engaged, _ = run_steps(model, *enc, tokens)
    assert engaged
    # the experts' storage replaced behind the plan's back: the cheap fingerprint does not see it, the full one does
    for expert in next(layer for layer in dec.layers if hasattr(layer, 'moe_layer')).moe_layer.experts:
        expert.fc2.weight.data = expert.fc2.weight.data.clone() * 0.5
        expert.fc1.bias.data = expert.fc1.bias.data.clone() + 0.25
    assert native.get_plan(dec) is plan and plan.full != native._full_fingerprint(dec)
    after, engaged, _ = run_steps(model, *enc, tokens)
    assert engaged and native.get_plan(dec) is not plan
    with pytest.MonkeyPatch.context() as m:
        m.setenv('PASERO_NO_NATIVE_DECODE', '1')
        perop, off, _ = run_steps(model, *enc, tokens)
    assert not off
    bound = 2e-5 * (perop.max() - perop.min()).item()
    assert (after - perop).abs().max().item() <= bound < (before - perop).abs().max().item()   # the new values were read
    # another dtype: a new plan of that dtype
    plan32 = native.get_plan(dec)
    model.to(torch.bfloat16)
    plan16 = native.get_plan(dec)
    assert plan16 is not None and plan16 is not plan32 and plan16.c_plan.dtype == 1 and plan16.c_moe is not None


# ---- the reference's recorded incremental decoding ------------------------------------------------------------------------------
@pytest.mark.parametrize('on', [True, False])
@pytest.mark.parametrize('name', VARIANTS)
def test_recorded_incremental_logits(name, on):
    """fixture (a): the logits of every call after the first within 2e-5 x the logit range (the project's decoder bound) of
    the reference's, on the native step (switch on) and on the per-op path (switch off)"""
    from pasero_amd import decode
    c, cfg, model = load_variant(name)
    enc = encode(c, model, c['tf:B'], c['seed'])
    tokens = torch.from_numpy(c['tf:tokens']).cuda()
    want = torch.from_numpy(c['tf:logits'])
    prev = decode.moe_native(on)
    try:
        got, engaged, _ = run_steps(model, *enc, tokens)
        assert engaged == on and (decode.get_plan(model.decoder) is not None) == on
        _, _, gates = run_steps(model, *enc, tokens, return_gates=True)
    finally:
        decode.moe_native(prev)
    err, bound = (got.cpu() - want).abs().max().item(), 2e-5 * (want.max() - want.min()).item()
    print(f'{name} {"native" if on else "per-op"}: |logits - reference| {err:.3e}, bound {bound:.3e}')
    assert got.shape == want.shape and err <= bound
    for i, key in enumerate(str(k) for k in c['tf:gate_keys']):   # the recorded gate values, through return_layers (per-op)
        assert (gates[1:, i].cpu() - torch.from_numpy(c['tf:gate:' + key])).abs().max().item() <= 1e-5


def search(c, cfg, model, kind, B):
    """(hyps, rows per decoder call, whether the native step ran)"""
    from pasero_amd.decode import beam_search, sampling
    dec = model.decoder
    enc_out, enc_mask = encode(c, model, B, c['shrink:seed' if kind == 'shrink' else 'seed'])
    log = {'rows': [], 'engaged': False}
    inner = dec.forward

    def forward(encoder_out, encoder_mask, decoder_input, **kw):
        out = inner(encoder_out, encoder_mask, decoder_input, **kw)
        log['rows'].append(encoder_out.size(0))
        log['engaged'] |= '_pk_decode' in kw['state']
        return out
    dec.forward = forward
    prompt = torch.full((B, 1), cfg.bos_idx, dtype=torch.long, device='cuda')
    try:
        if kind == 'greedy':
            hyps = sampling(dec, enc_out, enc_mask, int(c['max_output_len']), {}, decoder_input=prompt, sampling_temperature=0,
                            return_scores=True)
            for nbest in hyps:
                nbest[0]['score'] = nbest[0]['pos_scores'].sum()
        else:
            hyps = beam_search(dec, enc_out, enc_mask, int(c['max_output_len']), int(c['beam_size']), {}, decoder_input=prompt)
    finally:
        del dec.forward
    return hyps, log['rows'], log['engaged']


def assert_recorded(c, kind, hyps, rows):
    r = kind + ':'
    assert rows == [int(x) for x in c[r + 'rows']]
    assert [len(nb) for nb in hyps] == [int(n) for n in c[r + 'n_hyps']]
    for b, nbest in enumerate(hyps):
        for i, h in enumerate(nbest):
            q = f'{r}{b}:{i}:'
            np.testing.assert_array_equal(h['tokens'].cpu().numpy(), c[q + 'tokens'])
            ref = float(c[q + 'score'])
            assert abs(float(h['score']) - ref) <= 1e-4 * max(1.0, abs(ref))


@pytest.mark.parametrize('on', [True, False])
@pytest.mark.parametrize('kind', ['greedy', 'beam'])
@pytest.mark.parametrize('name', VARIANTS)
def test_recorded_searches_of_the_reference(name, kind, on):
    """fixture (b), with the switch on and with it off"""
    from pasero_amd import decode
    c, cfg, model = load_variant(name)
    # the seed rule the tool checked
    assert float(c[kind + ':min_gap']) >= 1e-3 * float(c[kind + ':max_logit'])
    assert int(c[kind + ':n_long']) >= 2 and float(c['gate_gap']) >= 1e-3 and int(c['experts_used']) >= 3
    assert bool(c['differs_with_rolled_gate'])
    prev = decode.moe_native(on)
    try:
        hyps, rows, engaged = search(c, cfg, model, kind, int(c['search:B']))
        assert engaged == on and (decode.get_plan(model.decoder) is not None) == on
    finally:
        decode.moe_native(prev)
    assert_recorded(c, kind, hyps, rows)


@pytest.mark.parametrize('name', VARIANTS)
def test_grouped_route_inside_the_step(name, native):
    """pk_moerows_few_max(0) against the default: the recorded greedy tokens either way (fp32 always takes the grouped route;
    the bf16 model takes the few route by default and the grouped one at 0 — its searches need not agree token for token, its
    steps are compared below)"""
    from pasero_amd import functional as F
    c, cfg, model = load_variant(name)
    results = []
    for threshold in (None, 0):
        prev = F.moe_rows_few_max(-1 if threshold is None else threshold)
        try:
            hyps, rows, engaged = search(c, cfg, model, 'greedy', int(c['search:B']))
        finally:
            F.moe_rows_few_max(prev)
        assert engaged
        assert_recorded(c, 'greedy', hyps, rows)
        results.append([nb[0]['tokens'].tolist() for nb in hyps])
    assert results[0] == results[1]


# ---- the bf16 step against the per-op path ----------------------------------------------------------------------------------------
TOKEN_SEED, PARITY_B, PARITY_STEPS = 1, 5, 6   # chosen on the CPU with the reference: the fp32 model alone meets the condition below
GAP = 2.0 ** -5


def valid_steps(gates):
    """per sentence: the number of calls after the first that come before the first call (the first included) at which some
    mixture layer's rank-2 / rank-3 gate-value gap is < 2^-5.  gates (calls, layers, B, E) of the fp32 model."""
    top = gates.topk(3, dim=-1).values
    small = ((top[..., 1] - top[..., 2]) < GAP).any(dim=1)   # (calls, B)
    out = []
    for b in range(small.size(1)):
        idx = small[:, b].nonzero().flatten()
        first = int(idx[0]) if idx.numel() else small.size(0)
        out.append(max(0, first - 1))
    return out


@pytest.mark.parametrize('threshold', [None, 0])
def test_bf16_step_parity(threshold, native, monkeypatch):
    """the native bf16 model and the per-op bf16 model against the fp32 per-op model: e_native <= 2 e_perop + one bf16 ulp at
    max|logit| (the project's rule for a second 16-bit path), the few route (default threshold) and the grouped route (0).
    A routing flip is a discontinuity, not an error: a sentence is compared only up to the step before the first one where some
    mixture layer's fp32 rank-2 / rank-3 gate-value gap is < 2^-5 — bf16 inputs and logits carry ~2^-8 relative error, 8 x that
    allowed for the layers upstream, and with p (1 - p) <= 1/4 that moves a gate value by < 0.01."""
    from pasero_amd import functional as F
    c, cfg, model32 = load_variant('mix')
    model16 = copy.deepcopy(model32).to(torch.bfloat16)
    gen = torch.Generator().manual_seed(TOKEN_SEED)
    tokens = torch.randint(4, int(c['V']), (PARITY_B, PARITY_STEPS + 1), generator=gen)
    tokens[:, 0] = cfg.bos_idx
    tokens = tokens.cuda()
    enc32, enc16 = encode(c, model32, PARITY_B, c['seed']), encode(c, model16, PARITY_B, c['seed'])
    want, engaged, gates = run_steps(model32, *enc32, tokens, return_gates=True)
    assert not engaged
    valid = valid_steps(gates.cpu())
    print(f'valid steps per sentence {valid} of {PARITY_STEPS}')
    assert sum(valid) >= PARITY_B * PARITY_STEPS / 2 and sum(v >= 3 for v in valid) >= 3
    mask = torch.zeros(PARITY_STEPS, PARITY_B, dtype=torch.bool)
    for b, v in enumerate(valid):
        mask[:v, b] = True
    mask = mask.cuda()
    prev = F.moe_rows_few_max(-1 if threshold is None else threshold)
    try:
        a, engaged, _ = run_steps(model16, *enc16, tokens)
    finally:
        F.moe_rows_few_max(prev)
    assert engaged
    with monkeypatch.context() as m:
        m.setenv('PASERO_NO_NATIVE_DECODE', '1')
        b, off, _ = run_steps(model16, *enc16, tokens)
    assert not off
    e_native, e_perop = (a - want)[mask].abs().max().item(), (b - want)[mask].abs().max().item()
    ulp = 2.0 ** (math.floor(math.log2(want[mask].abs().max().item())) - BF16_MANT)
    print(f'bf16 step parity: native {e_native:.3e} per-op {e_perop:.3e} ulp {ulp:.3e}')
    assert e_native <= 2 * e_perop + ulp


# ---- beam search: a sentence leaves the batch ---------------------------------------------------------------------------------------
@pytest.mark.parametrize('name', VARIANTS)
def test_beam_search_when_a_sentence_leaves_the_batch(name):
    """the recorded search of the fixture's `shrink` model: the switch on gives what the per-op search gives, and both what the
    reference recorded"""
    from pasero_amd import decode
    c, cfg, model = load_variant(name, seed_key='shrink:seed')
    assert len(set(int(x) for x in c['shrink:rows'])) > 1
    assert float(c['shrink:min_gap']) >= 1e-3 * float(c['shrink:max_logit'])
    found = {}
    prev = decode.moe_native()
    try:
        for on in (True, False):
            decode.moe_native(on)
            hyps, rows, engaged = search(c, cfg, model, 'shrink', int(c['shrink:B']))
            assert engaged == on
            assert_recorded(c, 'shrink', hyps, rows)
            found[on] = [[(h['tokens'].tolist(), float(h['score'])) for h in nb] for nb in hyps]
    finally:
        decode.moe_native(prev)
    for nb_on, nb_off in zip(found[True], found[False]):
        assert [t for t, _ in nb_on] == [t for t, _ in nb_off]
        assert all(abs(x - y) <= 1e-4 * max(1.0, abs(y)) for (_, x), (_, y) in zip(nb_on, nb_off))
