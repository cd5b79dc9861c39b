"""pasero_amd.decode.sampling / sample_on_the_fly / search end to end: the recorded searches of the real reference
(tests/golden/sampling_search.npz, written by tools/make_sampling_golden.py) with the native decoding step on and off,
seeding, the one host read per step, and the options that are refused."""
import numpy as np
import pytest
import torch

import paramgen
from conftest import load_golden
from model_utils import build_model

pytestmark = pytest.mark.gpu
CASES = ['full', 'greedy_penalty', 'greedy_prompts', 'greedy_stop', 'topk', 'topk1', 'topp']


def load_case(name):
    g = load_golden('sampling_search')
    p = name + ':'
    c = {k[len(p):]: g[k] for k in g.files if k.startswith(p)}
    cfg, model = build_model({'cfg': c['cfg'], 'V': c['V'], 'seed': c['seed']}, torch.float32, 'cuda')
    model.eval()
    B, S, V, seed = (int(c[k]) for k in ('B', 'S', 'V', 'seed'))
    b = paramgen.make_text_batch(seed, B, S, 5, V)
    with torch.no_grad():
        enc_out, enc_mask, _ = model.encoder(torch.from_numpy(b['encoder_input']).cuda(),
                                             torch.from_numpy(b['encoder_input_length']).cuda())
    return c, cfg, model, enc_out, enc_mask


def options(c):
    stop = [torch.from_numpy(c['stop_sequence'])] if c['stop_sequence'].size else []
    return dict(return_scores=bool(c['return_scores']), sampling_temperature=float(c['sampling_temperature']),
                sampling_topk=int(c['sampling_topk']), sampling_topp=float(c['sampling_topp']),
                repeat_penalty=float(c['repeat_penalty']), blacklist=[int(x) for x in c['blacklist']], stop_sequences=stop,
                decoder_input=torch.from_numpy(c['prompt']).cuda())


def spied(dec, log):
    inner = dec.forward

    def forward(encoder_out, encoder_mask, decoder_input, **kw):
        out = inner(encoder_out, encoder_mask, decoder_input, **kw)
        log['rows'].append(encoder_out.size(0))
        log['engaged'] |= '_pk_decode' in kw['state']
        return out
    dec.forward = forward


@pytest.mark.parametrize('native', [True, False])
@pytest.mark.parametrize('name', CASES)
def test_recorded_searches_of_the_reference(name, native, monkeypatch):
    """identical tokens per yielded step, identical rows per decoder call, pos_scores within 2 * 2e-5 * max|logit| per
    position; every recorded choice has a margin of at least 1e-3 (50 x the decoder bound)"""
    from pasero_amd.decode import sample_on_the_fly, sampling, get_plan
    if not native:
        monkeypatch.setenv('PASERO_NO_NATIVE_DECODE', '1')
    c, cfg, model, enc_out, enc_mask = load_case(name)
    assert float(c['draw_margin']) >= 1e-3 and float(c['boundary_margin']) >= 1e-3
    assert float(c['greedy_gap']) >= 1e-3 * float(c['max_logit'])
    log = {'rows': [], 'engaged': False}
    spied(model.decoder, log)
    uniforms = torch.from_numpy(c['uniforms']).cuda()
    try:
        steps = [{k: v.clone() for k, v in out.items()} for out in sample_on_the_fly(
            model.decoder, enc_out, enc_mask, int(c['max_output_len']), {}, uniforms=uniforms, **options(c))]
        hyps = sampling(model.decoder, enc_out, enc_mask, int(c['max_output_len']), {}, uniforms=uniforms, **options(c))
    finally:
        del model.decoder.forward
    n = len(c['rows'])
    assert log['rows'] == [int(r) for r in c['rows']] * 2
    assert [s['tokens'].size(1) for s in steps] == [int(w) for w in c['widths']]
    tokens = torch.cat([s['tokens'] for s in steps], dim=1)
    np.testing.assert_array_equal(tokens.cpu().numpy(), c['tokens'])
    tol = 2 * 2e-5 * float(c['max_logit'])
    if bool(c['return_scores']):
        got = torch.cat([s['pos_scores'] for s in steps], dim=1).cpu().numpy()
        want = c['pos_scores']
        assert got.shape == want.shape
        assert np.array_equal(np.isinf(got), np.isinf(want))
        fin = np.isfinite(want)
        print(f'{name}: pos_scores err {np.abs(got - want)[fin].max():.3e}, bound {tol:.3e}')
        assert np.abs(got - want)[fin].max() <= tol
    else:
        assert all('pos_scores' not in s for s in steps)
    # `sampling`: the one-element n-best lists, cut at the padding
    pad = cfg.padding_idx
    assert len(hyps) == int(c['B']) and all(len(h) == 1 for h in hyps)
    for b, (h,) in enumerate(hyps):
        row = c['tokens'][b]
        keep = int((row != pad).sum())
        np.testing.assert_array_equal(h['tokens'].cpu().numpy(), row[:keep])
        if bool(c['return_scores']):
            want = c['pos_scores'][b][row != pad]
            assert h['pos_scores'].shape == want.shape
            f = np.isfinite(want)
            assert np.abs(h['pos_scores'].cpu().numpy() - want)[f].max() <= tol
            if f.all():
                assert abs(float(h['score']) - float(want.sum())) <= tol * max(1, len(want))
        else:
            assert 'score' not in h
    assert log['engaged'] == (native and get_plan(model.decoder) is not None)
    assert log['engaged'] == native  # the stock layer: the native step takes it


def _base(B=32, V=8032, S=12, seed=0, embed_gain=1.0):
    from pasero_amd import config as C
    from pasero_amd.transformer import Transformer
    cfg = C.TransformerConfig()
    torch.manual_seed(seed)
    model = Transformer(cfg, C.DistributedConfig(), C.SyntheticTask(V)).to(torch.bfloat16).cuda().eval()
    b = paramgen.make_text_batch(seed + 1, B, S, 4, V)
    with torch.no_grad():
        # the tied output projection: freshly initialised it gives logits of unit spread, a nearly flat distribution
        model.decoder.embed_tokens.weight.mul_(embed_gain)
        enc_out, enc_mask, _ = model.encoder(torch.from_numpy(b['encoder_input']).cuda(),
                                             torch.from_numpy(b['encoder_input_length']).cuda())
    return cfg, model, enc_out, enc_mask


def test_seeding():
    """two searches after rng.manual_seed(s) are token-identical; another seed changes at least one of 32 sentences"""
    from pasero_amd import rng
    from pasero_amd.decode import search
    cfg, model, enc_out, enc_mask = _base()
    runs = []
    for s in (11, 11, 12):
        rng.manual_seed(s)
        hyps = search(model.decoder, enc_out, enc_mask, 12, {}, sampling=True, beam_size=5)
        runs.append([h[0]['tokens'].cpu() for h in hyps])
    assert all(torch.equal(a, b) for a, b in zip(runs[0], runs[1]))
    assert any(not torch.equal(a, b) for a, b in zip(runs[0], runs[2]))


def test_transformer_base_bf16_against_sample_ref():
    """Transformer-base, bf16, V = 8032, 32 sentences, 32 steps, top-p 0.9 with given uniforms, random weights: `sampling`
    and tests/sample_ref.py over the SAME decoder yield the same tokens.  Sentences where sample_ref itself saw a draw
    margin below 1e-5 or a boundary margin within tau (tests/sample_cases.py: reference_tau, per step) are left out; at
    most 10 % of the sentences, the figure coming from the sample_ref run alone.  pos_scores: the kernel's fp32
    log-probability against fp64 on the same bf16 logits, within 1e-5 * max(1, |score|) (fp32 eps times the few
    operations of a log-softmax whose terms are below 100 in magnitude)."""
    from sample_cases import reference_tau
    from sample_ref import sample_ref
    from pasero_amd.decode import sampling
    B, steps = 32, 32
    # embed_gain 8: logits of spread ~8 as a trained model's, so that a nucleus holds tens of tokens and not thousands
    # thinner than 1e-4 (with those, a draw lands within 1e-5 of an edge at one step in five: no seed could meet 10 %)
    cfg, model, enc_out, enc_mask = _base(B=B, S=24, embed_gain=8.0)
    gen = torch.Generator().manual_seed(5)
    uniforms = (torch.floor(torch.rand(steps + 1, B, generator=gen, dtype=torch.float64) * 2 ** 24) / 2 ** 24).float().cuda()
    with torch.no_grad():
        got = sampling(model.decoder, enc_out, enc_mask, steps, {}, sampling_topp=0.9, return_scores=True, uniforms=uniforms)
        state, stats = {}, {}
        prompt = torch.full((B, 1), cfg.bos_idx, dtype=torch.long, device='cuda')
        outs = sample_ref(lambda feed: model.decoder(enc_out, enc_mask, feed, state=state)[0], prompt, steps,
                          cfg.decoder_max_len, cfg.padding_idx, cfg.eos_idx, sampling_topp=0.9, return_scores=True,
                          uniforms=uniforms, stats=stats, tau_fn=reference_tau)
    want_tok = torch.cat([o['tokens'] for o in outs], dim=1)
    want_sc = torch.cat([o['pos_scores'] for o in outs], dim=1)
    left_out = ((stats['draw_margin'] < 1e-5) | stats['boundary_short']).cpu()
    print(f'left out {int(left_out.sum())} of {B} sentences (smallest draw margins '
          f'{sorted(stats["draw_margin"].tolist())[:4]}), {len(outs)} steps')
    assert int(left_out.sum()) <= 0.10 * B
    assert len(outs) >= steps - 1
    for b in range(B):
        if left_out[b]:
            continue
        keep = want_tok[b] != cfg.padding_idx
        assert torch.equal(got[b][0]['tokens'], want_tok[b][keep]), b
        w = want_sc[b][keep]
        assert bool(((got[b][0]['pos_scores'].double() - w).abs() <= 1e-5 * w.abs().clamp(min=1.0)).all()), b


def test_search_dispatch():
    """decoding.py:907-916: without `sampling` the temperature is 0, and beam_size > 1 then means beam search"""
    from pasero_amd.decode import search, beam_search, sampling
    c, cfg, model, enc_out, enc_mask = load_case('topk1')
    a = search(model.decoder, enc_out, enc_mask, 4, {}, beam_size=1)
    b = sampling(model.decoder, enc_out, enc_mask, 4, {}, sampling_temperature=0)
    assert all(torch.equal(x[0]['tokens'], y[0]['tokens']) for x, y in zip(a, b))
    k = search(model.decoder, enc_out, enc_mask, max_output_len=4, beam_size=3, meta={})
    w = beam_search(model.decoder, enc_out, enc_mask, 4, 3, {})
    assert [len(n) for n in k] == [len(n) for n in w] and torch.equal(k[0][0]['tokens'], w[0][0]['tokens'])


def test_one_host_read_per_step():
    """with torch's sync debug mode on 'error' around everything but the flagged read (`bool(has_eos.all())`), a whole
    search runs: the selection and the stop test never synchronise with the host"""
    from pasero_amd import decode
    cfg, model, enc_out, enc_mask = _base(B=4)
    prompt = torch.full((4, 1), cfg.bos_idx, dtype=torch.long, device='cuda')
    stops = [torch.tensor([7, 9], device='cuda')]
    black = [5]
    reads = {'n': 0}
    stock = torch.Tensor.__bool__

    def flagged(self):
        reads['n'] += 1
        torch.cuda.set_sync_debug_mode('default')
        try:
            return stock(self)
        finally:
            torch.cuda.set_sync_debug_mode('error')
    gen = decode.sample_on_the_fly(model.decoder, enc_out, enc_mask, 6, {}, decoder_input=prompt, sampling_topp=0.9,
                                   repeat_penalty=1.2, stop_sequences=stops, blacklist=black, return_scores=True)
    first = next(gen)  # set-up (prompt lengths, the first decoder call's plan) may read; the steps after it may not
    torch.cuda.synchronize()
    torch.Tensor.__bool__ = flagged
    torch.cuda.set_sync_debug_mode('error')
    try:
        steps = sum(1 for _ in gen)
    finally:
        torch.cuda.set_sync_debug_mode('default')
        torch.Tensor.__bool__ = stock
    assert steps >= 3 and reads['n'] == steps + 1  # one read after every yielded step (the first one included)


def test_unsupported_options_raise():
    from pasero_amd.decode import sampling, sample_on_the_fly
    c, cfg, model, enc_out, enc_mask = load_case('topk1')
    dec = model.decoder
    with pytest.raises(NotImplementedError, match='ensembles'):
        sampling(dec, [enc_out, enc_out], [enc_mask, enc_mask], 4, {})
    with pytest.raises(NotImplementedError, match='return_layers'):
        sampling(dec, enc_out, enc_mask, 4, {}, return_layers=['dec_0'])
    with pytest.raises(NotImplementedError, match='sharded'):
        sampling(dec, enc_out, enc_mask, 4, {}, sharded=True)
    with pytest.raises(NotImplementedError, match='decoder-only'):
        next(sample_on_the_fly(dec, [], [], 4, {}, decoder_input=torch.full((2, 1), 2, device='cuda')))
    with pytest.raises(AssertionError, match='nucleus'):
        sampling(dec, enc_out, enc_mask, 4, {}, sampling_topk=5, sampling_topp=0.5)
