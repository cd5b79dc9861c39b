"""Native decoding of `adapter_transformer` decoders (pk_decoder_step_ex: the decoding step with each layer's adapters
applied by pk_adapter_rows): the recorded searches of the real reference (tests/golden/adapter_search.npz, written by
tools/make_adapter_search_golden.py), the step against the per-op path, what the plan is keyed on, and the stock
decoder's step through both entry points."""
import contextlib
import copy
import ctypes
import json
import math

import numpy as np
import pytest
import torch

import paramgen
from conftest import load_golden
from model_utils import load_paramgen

pytestmark = pytest.mark.gpu
LANGS = ('de', 'fr')
BF16_MANT = 7


def build(cfg_json, V, seed, dtype=torch.float32, **overrides):
    from pasero_amd import adapters  # noqa: F401  (registers the architecture)
    from pasero_amd.config import AdapterTransformerConfig, DistributedConfig, SyntheticTask, get_architecture

    class Task(SyntheticTask):
        def get_langs_or_domains(self, key):
            assert key == 'lang'
            return set(LANGS)
    cfg = AdapterTransformerConfig(**{**json.loads(str(cfg_json)), **overrides})
    model = get_architecture(cfg)(cfg, DistributedConfig(), Task(int(V)))
    load_paramgen(model, int(seed))
    return cfg, model.to(dtype).cuda().eval()


def load_case(name, dtype=torch.float32, **overrides):
    g = load_golden('adapter_search')
    p = name + ':'
    c = {k[len(p):]: g[k] for k in g.files if k.startswith(p)}
    by = [str(x) for x in c['adapters_by']]
    cfg, model = build(c['cfg'], c['V'], c['seed'], dtype, decoder_adapters_by=by, **overrides)
    return c, cfg, model


def encode(c, model, B=None, S=None):
    B, S, V, seed = int(B or c['B']), int(S or c['S']), int(c['V']), int(c['seed'])
    b = paramgen.make_text_batch(seed, B, S, 5, V)
    with torch.no_grad():
        enc_out, enc_mask, _ = model.encoder(torch.from_numpy(b['encoder_input']).cuda(),
                                             torch.from_numpy(b['encoder_input_length']).cuda())
    return enc_out, enc_mask


# ---- recorded searches ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('native', [True, False])
@pytest.mark.parametrize('name', ['g', 'k', 's', 'l'])
def test_recorded_searches_of_the_reference(name, native, monkeypatch):
    from pasero_amd.decode import beam_search, get_plan, sampling
    if not native:
        monkeypatch.setenv('PASERO_NO_NATIVE_DECODE', '1')
    c, cfg, model = load_case(name)
    assert bool(c['differs_without_adapters'])       # the searches read the adapters ...
    assert bool(c['languages_differ']) == (name == 'l')   # ... and, in case l, the right language's
    enc_out, enc_mask = encode(c, model)
    dec, K, B = model.decoder, int(c['K']), int(c['B'])
    for j in range(int(c['n_runs'])):
        r = f'{j}:'
        assert float(c[r + 'min_gap']) >= 1e-3 * float(c[r + 'max_logit'])
        meta = {'lang': str(c[r + 'lang'])} if str(c[r + 'lang']) else {}
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
            if K == 1:
                hyps = sampling(dec, enc_out, enc_mask, int(c['max_output_len']), meta, decoder_input=prompt,
                                sampling_temperature=0, return_scores=True)
            else:
                hyps = beam_search(dec, enc_out, enc_mask, int(c['max_output_len']), K, meta, decoder_input=prompt)
        finally:
            del dec.forward
        assert log['rows'] == [int(x) for x in c[r + 'rows']]
        assert [len(nb) for nb in hyps] == [int(n) for n in c[r + 'n_hyps']]
        for b, nbest in enumerate(hyps):
            for i, h in enumerate(nbest):
                q = f'{r}{b}:{i}:'
                np.testing.assert_array_equal(h['tokens'].cpu().numpy(), c[q + 'tokens'])
                tol = 2 * max(1, len(c[q + 'tokens'])) * 2e-5 * float(c[r + 'max_logit'])  # test_beam_search_gpu.py's own
                assert abs(float(h['score']) - float(c[q + 'score'])) <= tol
        if native:
            assert log['engaged'] and get_plan(dec) is not None
            assert get_plan(dec).c_adapters is not None
        else:
            assert not log['engaged']


# ---- the step against the per-op path -------------------------------------------------------------------------------------
def run_steps(model, enc_out, enc_mask, tokens, meta, native, monkeypatch):
    """logits (steps, B, V) fp32 of the incremental calls after the first one, and whether the native step ran"""
    with monkeypatch.context() as m:
        if not native:
            m.setenv('PASERO_NO_NATIVE_DECODE', '1')
        state, out = {}, []
        with torch.no_grad():
            model.decoder(enc_out, enc_mask, tokens[:, :1], state=state, meta=meta)
            for t in range(1, tokens.size(1)):
                logits, _ = model.decoder(enc_out, enc_mask, tokens[:, t:t + 1], state=state, meta=meta)
                out.append(logits[:, -1].float().clone())
        return torch.stack(out), '_pk_decode' in state


@contextlib.contextmanager
def step_route(fused):
    """which route the step's adapters take (pk_adapter_step_fused): the fused kernel, or the three launches (the default)"""
    from pasero_amd import lib
    L = lib.load()
    prev = L.pk_adapter_step_fused(int(fused))
    try:
        yield
    finally:
        L.pk_adapter_step_fused(prev)


def step_tokens(cfg, V, B, steps, seed=5):
    g = torch.Generator().manual_seed(seed)
    tok = torch.randint(4, int(V), (B, steps + 1), generator=g)
    tok[:, 0] = cfg.bos_idx
    return tok.cuda()


def logit_range(x):
    return (x.max() - x.min()).item()


def assert_fp32_parity(model, enc_out, enc_mask, tokens, meta, monkeypatch, expect_native=True):
    a, engaged = run_steps(model, enc_out, enc_mask, tokens, meta, True, monkeypatch)
    b, off = run_steps(model, enc_out, enc_mask, tokens, meta, False, monkeypatch)
    assert engaged == expect_native and not off
    err = (a - b).abs().max().item()
    print(f'fp32 step parity: |native - per-op| {err:.3e}, bound {2e-5 * logit_range(b):.3e}')
    assert err <= 2e-5 * logit_range(b)  # the project's decoder bound
    return a, b


def assert_bf16_parity(model32, model16, enc_in, tokens, meta, monkeypatch):
    """both 16-bit paths against the fp32 model: native error <= 2 x per-op error + one bf16 ulp at max|logit|"""
    enc32, enc16 = enc_in(model32), enc_in(model16)
    want, _ = run_steps(model32, *enc32, tokens, meta, False, monkeypatch)
    a, engaged = run_steps(model16, *enc16, tokens, meta, True, monkeypatch)
    b, _ = run_steps(model16, *enc16, tokens, meta, False, monkeypatch)
    assert engaged
    e_native, e_perop = (a - want).abs().max().item(), (b - want).abs().max().item()
    ulp = 2.0 ** (math.floor(math.log2(want.abs().max().item())) - BF16_MANT)
    print(f'bf16 step parity: native {e_native:.3e} per-op {e_perop:.3e} ratio {e_native / e_perop:.3f} ulp {ulp:.3e}')
    assert e_native <= 2 * e_perop + ulp


def test_step_parity_fp32_and_bf16(monkeypatch):
    c, cfg, model = load_case('g')
    tokens = step_tokens(cfg, c['V'], 5, 6)
    assert_fp32_parity(model, *encode(c, model, B=5), tokens, {}, monkeypatch)
    model16 = copy.deepcopy(model).to(torch.bfloat16)
    for fused in (True, False):
        with step_route(fused):
            assert_bf16_parity(model, model16, lambda m: encode(c, m, B=5), tokens, {}, monkeypatch)


# ---- what the plan is keyed on --------------------------------------------------------------------------------------------
def test_alternating_languages_get_their_own_adapters(monkeypatch):
    c, cfg, model = load_case('l')
    enc = encode(c, model, B=5)
    tokens = step_tokens(cfg, c['V'], 5, 3)
    perop = {lang: run_steps(model, *enc, tokens, {'lang': lang}, False, monkeypatch)[0] for lang in LANGS}
    bound = 2e-5 * max(logit_range(v) for v in perop.values())
    assert (perop['de'] - perop['fr']).abs().max().item() > 100 * bound  # the languages are told apart by far more
    for lang in ('de', 'fr', 'de', 'de', 'fr'):
        got, engaged = run_steps(model, *enc, tokens, {'lang': lang}, True, monkeypatch)
        assert engaged
        assert (got - perop[lang]).abs().max().item() <= bound
        other = perop['fr' if lang == 'de' else 'de']
        assert (got - other).abs().max().item() > 100 * bound


def stack_sizes(decoder):
    from pasero_amd.decode import get_plan
    plan = get_plan(decoder)
    assert plan is not None
    return None if plan.c_adapters is None else [s.n for s in plan.c_adapters]


def test_layer_subset_stack_and_disabled_adapters(monkeypatch):
    c, cfg, model = load_case('g', decoder_adapter_layer_ids=[1])
    from pasero_amd.adapters import AdapterTransformerDecoderLayer
    assert [type(m) is AdapterTransformerDecoderLayer for m in model.decoder.layers] == [False, True]
    tokens = step_tokens(cfg, c['V'], 5, 3)
    assert_fp32_parity(model, *encode(c, model, B=5), tokens, {}, monkeypatch)
    assert stack_sizes(model.decoder) == [0, 1]

    c, cfg, model = load_case('g', decoder_adapters=['a', 'b'])  # two adapters stacked on every layer
    enc = encode(c, model, B=5)
    both, _ = assert_fp32_parity(model, *enc, tokens, {}, monkeypatch)
    assert stack_sizes(model.decoder) == [2, 2]
    model.decoder.layers[0].adapters['b'].disable()
    one, _ = assert_fp32_parity(model, *enc, tokens, {}, monkeypatch)
    assert stack_sizes(model.decoder) == [1, 2]
    assert (one - both).abs().max().item() > 100 * 2e-5 * logit_range(both)  # the disabled adapter is skipped, not applied
    model.decoder.layers[0].adapters['b'].enable()
    again, _ = assert_fp32_parity(model, *enc, tokens, {}, monkeypatch)
    assert stack_sizes(model.decoder) == [2, 2] and torch.equal(again, both)
    for layer in model.decoder.layers:
        for ad in layer.adapters.values():
            ad.disable()
    assert_fp32_parity(model, *enc, tokens, {}, monkeypatch)
    assert stack_sizes(model.decoder) is None  # nothing in use: the plain step


def test_what_the_native_step_does_not_take(monkeypatch):
    from pasero_amd.adapters import AdapterTransformerDecoderLayer
    from pasero_amd.decode import get_plan
    c, cfg, model = load_case('g', decoder_adapters=['a', 'b', 'c', 'd', 'e'])  # one more than PK_ADAPTER_STACK_MAX
    tokens = step_tokens(cfg, c['V'], 5, 2)
    assert get_plan(model.decoder) is None
    assert_fp32_parity(model, *encode(c, model, B=5), tokens, {}, monkeypatch, expect_native=False)

    class Sub(AdapterTransformerDecoderLayer):
        def forward(self, x, *args, **kwargs):
            return super().forward(x, *args, **kwargs)
    c, cfg, model = load_case('g')
    assert get_plan(model.decoder) is not None
    model.decoder.layers[1].__class__ = Sub
    from pasero_amd import decode
    decode._plans.pop(model.decoder, None)
    assert get_plan(model.decoder) is None

    c, cfg, model = load_case('g')
    model.decoder.layers[0].adapters['default'].residual = False
    assert get_plan(model.decoder) is None


# ---- decoders without adapters ----------------------------------------------------------------------------------------------
def test_stock_decoder_step_is_bitwise_the_same_through_both_entry_points(monkeypatch):
    from pasero_amd import decode, lib
    from pasero_amd.config import DistributedConfig, SyntheticTask, TransformerConfig
    from pasero_amd.transformer import Transformer
    g = load_golden('adapter_search')
    base = {k: v for k, v in json.loads(str(g['g:cfg'])).items() if 'adapter' not in k}
    cfg = TransformerConfig(**base)
    V = int(g['g:V'])
    model = Transformer(cfg, DistributedConfig(), SyntheticTask(V))
    load_paramgen(model, 7)
    model = model.cuda().eval()
    c = {'B': 5, 'S': 7, 'V': V, 'seed': 7}
    enc_out, enc_mask = encode(c, model)
    tokens = step_tokens(cfg, V, 5, 2)
    state = {}
    with torch.no_grad():
        model.decoder(enc_out, enc_mask, tokens[:, :1], state=state)
        model.decoder(enc_out, enc_mask, tokens[:, 1:2], state=state)
    cache = state['_pk_decode']
    plan = cache.plan
    assert plan.c_adapters is None and len(decode._plans[model.decoder][0]) == 2  # plan and key as before
    L = lib.load()
    assert L.pk_decoder_step_scratch_ex(ctypes.byref(plan.c_plan), cache.B, None) == L.pk_decoder_step_scratch(
        ctypes.byref(plan.c_plan), cache.B)
    ids = tokens[:, 2].contiguous()
    pos = model.decoder.embed_positions.shift + state['offset']
    outs = []
    for ex in (False, True):  # the same step twice: it writes the same K/V row at index t both times
        logits = torch.zeros(cache.B, cache.ldl, device='cuda', dtype=torch.float32)
        args = (ctypes.byref(plan.c_plan), lib.ptr(ids), cache.B, cache.t, int(pos), cache.k_tab, cache.v_tab, cache.cap,
                cache.c_tab, lib.ptr(cache.mask), cache.S, lib.ptr(cache.scratch), cache.scratch.numel(), lib.ptr(logits), cache.ldl)
        if ex:
            lib.check(L.pk_decoder_step_ex(*args, None, lib.stream_ptr()), 'pk_decoder_step_ex')
        else:
            lib.check(L.pk_decoder_step(*args, lib.stream_ptr()), 'pk_decoder_step')
        outs.append(logits)
    torch.cuda.synchronize()
    assert torch.equal(outs[0].view(torch.int32), outs[1].view(torch.int32))
    assert outs[0][:, :V].abs().max().item() > 0


# ---- the recipe's width -------------------------------------------------------------------------------------------------------
def test_recipe_width_bf16(monkeypatch):
    """d = 1024, 16 heads, f = 2048, 2 pre-norm decoder layers, p = 64, V = 1003, bf16, 40 rows, 4 steps: the fused
    kernel's real tile shapes (two row tiles, eight column slices) inside the step"""
    from pasero_amd import lib
    assert lib.load().pk_adapter_step_fused(-1) == 0  # the step's default route, by measurement (docs/experiments.md)
    from pasero_amd import functional as F
    g = load_golden('adapter_search')
    over = dict(embed_dim=1024, encoder_attention_heads=16, decoder_attention_heads=16, encoder_ffn_dim=2048,
                decoder_ffn_dim=2048, encoder_layers=1, decoder_layers=2, encoder_prenorm=True, decoder_prenorm=True,
                encoder_adapter_dim=64, decoder_adapter_dim=64)
    V, B = 1003, 40
    cfg, model = build(g['g:cfg'], V, 21, **over)
    assert F.adapter_rows_fused(B, 1024, 64, torch.bfloat16)
    model16 = copy.deepcopy(model).to(torch.bfloat16)
    c = {'B': B, 'S': 9, 'V': V, 'seed': 21}
    tokens = step_tokens(cfg, V, B, 4)
    for fused in (True, False):  # the fused kernel inside the step, then the step's default (the three launches)
        with step_route(fused):
            assert_bf16_parity(model, model16, lambda m: encode(c, m), tokens, {}, monkeypatch)
