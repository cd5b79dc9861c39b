"""`hybrid_transformer` / `adapter_hybrid_transformer` without a GPU: registry and presets, state-dict names and shapes against
the three layouts the real reference recorded (tests/golden/hybrid.npz), what the constructor refuses, initialisation, and
the incremental state's contract with `Decoder.reorder_state`."""
import json
import math

import pytest
import torch

from conftest import golden_names_shapes, load_golden
from hybrid_utils import hybrid_cfg, hybrid_model

PRESETS = {'hybrid_transformer': (512, 512, False), 'hybrid_transformer_small': (512, 512, False),
           'hybrid_transformer_big': (1024, 1024, False), 'rnmt_big': (1024, 1024, False),
           'hybrid_transformer_wide': (1024, 2048, False), 'adapter_hybrid_transformer': (512, 512, True),
           'adapter_hybrid_transformer_big': (1024, 1024, True), 'adapter_hybrid_transformer_wide': (1024, 2048, True)}


@pytest.mark.parametrize('name', sorted(PRESETS))
def test_presets_resolve_to_the_hybrid_models(name):
    from pasero_amd import config as C, hybrid
    embed, hidden, adapter = PRESETS[name]
    cfg = C.CONFIGS[name]()
    assert (cfg.embed_dim, cfg.decoder_hidden_size, cfg.decoder_layers, cfg.decoder_embed_proj) == (embed, hidden, 2, False)
    assert C.get_architecture(cfg) is (hybrid.AdapterHybridTransformer if adapter else hybrid.HybridTransformer)
    assert hasattr(cfg, 'encoder_adapter_dim') == adapter


def test_registry_names():
    from pasero_amd import config as C, hybrid
    assert C.MODELS['hybrid_transformer'] is hybrid.HybridTransformer
    assert C.MODELS['adapter_hybrid_transformer'] is hybrid.AdapterHybridTransformer
    assert issubclass(hybrid.AdapterHybridTransformer, C.MODELS['adapter_transformer'])
    assert C.get_architecture(C.TransformerConfig()) is C.MODELS['transformer']          # the other families are where they were
    assert C.get_architecture(C.AdapterTransformerConfig()) is C.MODELS['adapter_transformer']


@pytest.mark.parametrize('layout', ['', 'same:', 'untied:'])
def test_state_dict_is_the_reference_s(layout):
    g = load_golden('hybrid')
    overrides = json.loads(str(g[layout + 'overrides'])) if layout else {}
    cfg, model = hybrid_model(g, **overrides)
    got = [(k, tuple(v.shape)) for k, v in model.state_dict().items()]
    assert got == golden_names_shapes(g, layout)
    names = [k for k, _ in got]
    assert ('decoder.out_proj.weight' in names) == (layout != 'same:')
    assert ('decoder.embed_proj.weight' in names) == (layout != 'same:')
    assert ('decoder.output_projection.weight' in names) == (layout == 'untied:')
    assert all(p.requires_grad for p in model.parameters())


def test_lstm_module_layout_and_initialisation():
    from pasero_amd.hybrid import LSTM
    torch.manual_seed(0)
    layer = LSTM(input_size=192, hidden_size=64)
    assert [(k, tuple(v.shape)) for k, v in layer.named_parameters()] == [
        ('weight_ih_l0', (256, 192)), ('weight_hh_l0', (256, 64)), ('bias_ih_l0', (256,)), ('bias_hh_l0', (256,))]
    ref = torch.nn.LSTM(192, 64, batch_first=True)
    assert [(k, tuple(v.shape)) for k, v in ref.named_parameters()] == [(k, tuple(v.shape)) for k, v in layer.named_parameters()]
    bound = 1 / math.sqrt(64)
    for p in (q.detach() for q in layer.parameters()):   # uniform in +-1/sqrt(H): inside the bound, and spread over it
        assert float(p.abs().max()) <= bound and float(p.abs().max()) > 0.9 * bound and abs(float(p.mean())) < 0.1 * bound


def test_refusals():
    from pasero_amd import config as C
    from pasero_amd.hybrid import LSTM, HybridTransformer, LSTMDecoder
    task = C.SyntheticTask(61)
    with pytest.raises(NotImplementedError, match='tensor parallelism'):
        HybridTransformer(hybrid_cfg(), C.DistributedConfig(tp_size=2), task)
    with pytest.raises(NotImplementedError, match='tensor parallelism'):
        LSTMDecoder(hybrid_cfg(), C.DistributedConfig(tp_size=2), task)
    with pytest.raises(NotImplementedError, match='decoder'):
        HybridTransformer(hybrid_cfg(model_type='decoder'), C.DistributedConfig(), task)
    with pytest.raises(NotImplementedError, match="model_type='decoder'"):
        LSTMDecoder(hybrid_cfg(model_type='decoder'), C.DistributedConfig(), task)
    with pytest.raises(NotImplementedError, match='decoder_hidden_size 72'):
        HybridTransformer(hybrid_cfg(decoder_hidden_size=72), C.DistributedConfig(), task)
    with pytest.raises(NotImplementedError, match='embed_dim 132'):
        LSTMDecoder(hybrid_cfg(embed_dim=132), C.DistributedConfig(), task)
    with pytest.raises(NotImplementedError, match='hidden size 40'):
        LSTM(64, 40)
    with pytest.raises(NotImplementedError, match='input size 100'):
        LSTM(100, 64)


def test_cpu_tensors_are_refused_not_computed():
    cfg, model = hybrid_model()
    dec = model.decoder.eval()
    with torch.no_grad(), pytest.raises(RuntimeError, match='no CPU fallback'):
        dec(torch.zeros(1, 3, cfg.embed_dim), torch.zeros(1, 3, dtype=torch.bool), torch.zeros(1, 1, dtype=torch.long))


def test_adapter_variant_has_no_decoder_adapters_and_a_frozen_decoder():
    g = load_golden('hybrid')
    cfg, model = hybrid_model(g, adapter=True, encoder_adapters=['a'], decoder_adapters=['a'])
    from pasero_amd.hybrid import AdapterHybridTransformer, LSTMDecoder
    assert type(model) is AdapterHybridTransformer and type(model.decoder) is LSTMDecoder
    names = dict(model.named_parameters())
    assert any('.adapters.' in n for n in names) and not any('.adapters.' in n for n in names if n.startswith('decoder.'))
    assert all(p.requires_grad == ('adapters' in n.split('.')) for n, p in names.items())
    assert not any(p.requires_grad for n, p in names.items() if n.startswith('decoder.'))
    plain = [k for k, _ in golden_names_shapes(g)]
    assert [n for n in model.state_dict() if '.adapters.' not in n] == plain


def test_state_contract():
    """the keys and shapes the searches reorder on dim 0 (recorded from the reference after its first incremental call)"""
    from pasero_amd.transformer import Decoder
    g = load_golden('hybrid')
    cfg, model = hybrid_model(g)
    dec = model.decoder
    shapes = json.loads(str(g['state_shapes']))
    B, S, L, H = int(g['B']), int(g['S']), cfg.decoder_layers, dec.hidden_size
    assert shapes == {'attn_key': [B, 1, S, H], 'prev_hiddens': [B, L, H], 'prev_cells': [B, L, H]}
    assert dec.cross_attn_key == str(g['attn_key_name']) == 'dec_1_cross_attn'
    assert len(dec.layers) == len(dec.layer_norms) == L and dec.max_len == cfg.decoder_max_len
    state = {k: torch.arange(B, dtype=torch.float32).view(B, *[1] * (len(s) - 1)).expand(*s).clone() for k, s in shapes.items()}
    idx = torch.tensor([2, 2, 0, 1, 1])
    Decoder.reorder_state(state, idx)
    for k, s in shapes.items():
        assert list(state[k].shape) == [5] + s[1:] and torch.equal(state[k].reshape(5, -1)[:, 0], idx.float()), k
