"""pasero_amd.decode.beam_search end to end: the recorded searches of the real reference (tests/golden/beam_search.npz,
written by tools/make_beam_golden.py), the native decoding step against the per-op path, the re-ordered state against
`Decoder.reorder_state`, the options that are refused, and one Transformer-base bf16 search against tests/beam_ref.py
over the same decoder."""
import math

import numpy as np
import pytest
import torch

import paramgen
from conftest import load_golden
from model_utils import build_model
from beam_ref import beam_ref

pytestmark = pytest.mark.gpu
CASES = ['a', 'b', 'c', 'd']


def load_case(name):
    g = load_golden('beam_search')
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


def search(c, model, enc_out, enc_mask, spy=None):
    from pasero_amd.decode import beam_search
    dec = model.decoder
    inner = dec.forward
    log = {'rows': [], 'engaged': False}

    def forward(encoder_out, encoder_mask, decoder_input, **kw):
        if spy is not None:
            spy(encoder_out, encoder_mask)
        out = inner(encoder_out, encoder_mask, decoder_input, **kw)
        log['rows'].append(encoder_out.size(0))
        log['engaged'] |= '_pk_decode' in kw['state']
        return out
    dec.forward = forward
    try:
        hyps = beam_search(dec, enc_out, enc_mask, int(c['max_output_len']), int(c['K']), {},
                           decoder_input=torch.from_numpy(c['prompt']).cuda(), return_scores=bool(c['return_scores']),
                           len_penalty=float(c['len_penalty']), blacklist=[int(x) for x in c['blacklist']])
    finally:
        del dec.forward
    return hyps, log


def check_against_fixture(c, hyps, rows):
    """same hypotheses in the same order, identical tokens, the same rows per decoder call; scores within
    2 * len * 2e-5 * max|logit| (2: the sensitivity of log-softmax to a logit perturbation; 2e-5 of the range: the
    project's fp32 decoder bound; len: the scores are sums over the positions)"""
    assert rows == [int(r) for r in c['rows']]
    assert [len(nb) for nb in hyps] == [int(n) for n in c['n_hyps']]
    for b, nbest in enumerate(hyps):
        for i, h in enumerate(nbest):
            q = f'{b}:{i}:'
            np.testing.assert_array_equal(h['tokens'].cpu().numpy(), c[q + 'tokens'])
            tol = 2 * max(1, len(c[q + 'tokens'])) * 2e-5 * float(c['max_logit'])
            assert abs(float(h['score']) - float(c[q + 'score'])) <= tol
            assert abs(float(h['normalized_score']) - float(c[q + 'normalized_score'])) <= tol
            if bool(c['return_scores']):
                got = h['pos_scores'].cpu().numpy()
                assert got.shape == c[q + 'pos_scores'].shape
                assert got.size == 0 or np.abs(got - c[q + 'pos_scores']).max() <= tol


@pytest.mark.parametrize('native', [True, False])
@pytest.mark.parametrize('name', CASES)
def test_recorded_searches_of_the_reference(name, native, monkeypatch):
    if not native:
        monkeypatch.setenv('PASERO_NO_NATIVE_DECODE', '1')
    c, cfg, model, enc_out, enc_mask = load_case(name)
    assert float(c['min_gap']) >= 1e-3 * float(c['max_logit'])
    hyps, log = search(c, model, enc_out, enc_mask)
    check_against_fixture(c, hyps, log['rows'])
    from pasero_amd.decode import get_plan
    assert log['engaged'] == (native and get_plan(model.decoder) is not None)
    if name != 'd':
        assert log['engaged'] == native  # a, b, c: the stock layer, the native step takes it
    else:
        assert not log['engaged']        # d: rotary positions, the per-op path is searched


def test_some_recorded_search_shrinks_its_batch():
    g = load_golden('beam_search')
    assert any(len(set(g[f'{n}:rows'].tolist())) > 1 for n in CASES)


def load_trace_case():
    """the model and batch of tests/golden/beam_trace.npz: its search drops a sentence (12 -> 9 rows) at a later step"""
    g = load_golden('beam_trace')
    cfg, model = build_model(g, torch.float32, 'cuda')
    model.eval()
    B, S, V, seed = (int(g[k]) for k in ('B', 'S', 'V', 'seed'))
    b = paramgen.make_text_batch(seed, B, S, 5, V)
    with torch.no_grad():
        enc_out, enc_mask, _ = model.encoder(torch.from_numpy(b['encoder_input']).cuda(),
                                             torch.from_numpy(b['encoder_input_length']).cuda())
    c = {'K': g['K'], 'max_output_len': g['max_output_len'], 'prompt': np.full((B, 1), cfg.bos_idx, dtype=np.int64),
         'return_scores': False, 'len_penalty': 1.0, 'blacklist': np.zeros(0, dtype=np.int64)}
    return g, c, model, enc_out, enc_mask


@pytest.mark.parametrize('name', ['a', 'trace'])
def test_reordered_state_is_bitwise_reorder_state(name, monkeypatch):
    """at every step of a search: what `DecodeCache.reorder_beam` publishes in `state` (and the cross-attention K|V, the
    mask, the encoder output and its mask the next decoder call reads) is bitwise what `Decoder.reorder_state` and the
    reference's `index_select` of the encoder tensors give on a copy — including the steps where nothing but the
    self-attention caches moved, and ('trace': the recorded search of beam_trace.npz) the step where a sentence leaves"""
    from pasero_amd import decode
    from pasero_amd.transformer import Decoder
    if name == 'trace':
        g, c, model, enc_out, enc_mask = load_trace_case()
    else:
        c, cfg, model, enc_out, enc_mask = load_case(name)
    K = int(c['K'])
    expect = {'enc': enc_out.repeat_interleave(K, dim=0), 'mask': enc_mask.repeat_interleave(K, dim=0), 'n': 0, 'shrunk': 0,
              'inside': False}
    inner = decode.DecodeCache.reorder_beam
    plain = Decoder.reorder_state

    def moved(indices):
        expect['enc'], expect['mask'] = expect['enc'].index_select(0, indices), expect['mask'].index_select(0, indices)

    def checked(self, indices, state, shrink):
        copy = self.clone(state)
        inner(self, indices, state, shrink)
        expect['inside'] = True
        plain(copy, indices)
        expect['inside'] = False
        other = copy['_pk_decode']
        for k, v in state.items():
            if torch.is_tensor(v):
                assert v.shape == copy[k].shape and torch.equal(v, copy[k]), k
        for a, b in zip(self.cross, other.cross):
            assert torch.equal(a, b)
        assert (self.mask is None) == (other.mask is None) and (self.mask is None or torch.equal(self.mask, other.mask))
        assert self.B == other.B and self.t == other.t
        moved(indices)
        expect['n'] += 1
        expect['shrunk'] += int(shrink)

    def plain_spy(state, indices):  # the first re-ordering of a search comes before the native cache exists
        if not expect['inside']:
            moved(indices)
        return plain(state, indices)
    monkeypatch.setattr(decode.DecodeCache, 'reorder_beam', checked)
    monkeypatch.setattr(Decoder, 'reorder_state', staticmethod(plain_spy))

    def spy(encoder_out, encoder_mask):
        assert torch.equal(encoder_out, expect['enc']) and torch.equal(encoder_mask, expect['mask'])
    hyps, log = search(c, model, enc_out, enc_mask, spy=spy)
    assert expect['n'] >= 2 and log['engaged']
    assert (expect['shrunk'] > 0) == (name == 'trace')
    if name == 'trace':
        assert len(set(log['rows'])) > 1
        for b, nbest in enumerate(hyps):
            np.testing.assert_array_equal(nbest[0]['tokens'].cpu().numpy(), g[f'best_{b}'])
    else:
        check_against_fixture(c, hyps, log['rows'])


def test_unsupported_options_raise():
    from pasero_amd.decode import beam_search
    c, cfg, model, enc_out, enc_mask = load_case('c')
    dec, K = model.decoder, 2
    with pytest.raises(NotImplementedError, match='ensembles'):
        beam_search(dec, [enc_out, enc_out], [enc_mask, enc_mask], 4, K, {})
    with pytest.raises(NotImplementedError, match='return_layers'):
        beam_search(dec, enc_out, enc_mask, 4, K, {}, return_layers=['dec_0'])
    with pytest.raises(NotImplementedError, match='sharded'):
        beam_search(dec, enc_out, enc_mask, 4, K, {}, sharded=True)
    with pytest.raises(NotImplementedError, match='decoder-only'):
        beam_search(dec, [], [], 4, K, {}, decoder_input=torch.full((2, 1), 2, device='cuda'))
    with pytest.raises(RuntimeError, match='beam size 17'):
        beam_search(dec, enc_out, enc_mask, 4, 17, {})
    with pytest.warns(UserWarning, match='repeat_penalty'):
        beam_search(dec, enc_out, enc_mask, 2, K, {}, repeat_penalty=1.2)


def test_transformer_base_bf16_against_beam_ref():
    """Transformer-base, bf16, V = 8032, 32 sentences x 5 beams, 32 steps, random weights: `beam_search` and
    tests/beam_ref.py over the SAME decoder give the same n-best lists.  Sentences for which beam_ref itself saw a gap
    below 1e-5 among its best 2K + 1 at some step are left out (the two differ in fp32 rounding of the scores); an exact tie
    between two tokens of one beam is a tie of bf16 logits, decided by the tie rule in both, and is not such a gap.  At
    most 10 % of the sentences may be left out; the figure comes from the beam_ref run alone."""
    from pasero_amd import config as C
    from pasero_amd.decode import beam_search
    from pasero_amd.transformer import Transformer, Decoder
    V, B, K, S, steps, seed = 8032, 32, 5, 24, 32, 0
    cfg = C.TransformerConfig()
    torch.manual_seed(seed)
    model = Transformer(cfg, C.DistributedConfig(), C.SyntheticTask(V)).to(torch.bfloat16).cuda().eval()
    b = paramgen.make_text_batch(seed + 1, B, S, 4, V)
    with torch.no_grad():
        enc_out, enc_mask, _ = model.encoder(torch.from_numpy(b['encoder_input']).cuda(),
                                             torch.from_numpy(b['encoder_input_length']).cuda())
        got = beam_search(model.decoder, enc_out, enc_mask, steps, K, {}, return_scores=True)
        box = {'enc': enc_out.repeat_interleave(K, dim=0), 'mask': enc_mask.repeat_interleave(K, dim=0), 'state': {}}

        def step_fn(feed):
            return model.decoder(box['enc'], box['mask'], feed, state=box['state'])[0]

        def reorder_fn(idx):
            box['enc'], box['mask'] = box['enc'].index_select(0, idx), box['mask'].index_select(0, idx)
            Decoder.reorder_state(box['state'], idx)
        stats = {}
        prompt = torch.full((B, 1), cfg.bos_idx, dtype=torch.long, device='cuda')
        want = beam_ref(step_fn, reorder_fn, prompt, K, steps, cfg.decoder_max_len, cfg.padding_idx, cfg.eos_idx,
                        return_scores=True, stats=stats)
    left_out = [b for b in range(B) if stats['sent_gap'][b] < 1e-5]
    print(f'left out {len(left_out)} of {B} sentences (smallest gaps {sorted(stats["sent_gap"])[:4]}), rows {stats["rows"][:3]}..')
    assert len(left_out) <= 0.10 * B
    for b in range(B):
        if b in left_out:
            continue
        assert len(got[b]) == len(want[b])
        for h, r in zip(got[b], want[b]):
            assert torch.equal(h['tokens'], r['tokens']), b
            assert abs(float(h['score']) - float(r['score'])) <= 1e-4 * max(1.0, abs(float(r['score'])))
