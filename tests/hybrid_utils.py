"""helpers shared by the hybrid_transformer tests"""
import json

import torch

import paramgen
from conftest import golden_names_shapes, load_golden


def hybrid_cfg(g=None, adapter=False, **overrides):
    from pasero_amd.config import AdapterHybridTransformerConfig, HybridTransformerConfig
    g = load_golden('hybrid') if g is None else g
    cls = AdapterHybridTransformerConfig if adapter else HybridTransformerConfig
    return cls(**{**json.loads(str(g['cfg'])), **json.loads(str(g['hybrid_cfg'])), **overrides})


def hybrid_model(g=None, adapter=False, **overrides):
    from pasero_amd import hybrid  # noqa: F401  (registers the architectures)
    from pasero_amd.config import DistributedConfig, SyntheticTask, get_architecture
    from model_utils import load_paramgen
    g = load_golden('hybrid') if g is None else g
    cfg = hybrid_cfg(g, adapter=adapter, **overrides)
    model = get_architecture(cfg)(cfg, DistributedConfig(), SyntheticTask(int(g['V'])))
    load_paramgen(model, int(g['seed']))
    return cfg, model


def fp64_state(g):
    """the fixture's paramgen weights as fp64 leaves, tied names sharing one tensor"""
    state = paramgen.make_state_dict(int(g['seed']), golden_names_shapes(g))
    P = {k: torch.from_numpy(v).double() for k, v in state.items()}
    P['decoder.embed_tokens.weight'] = P['encoder.embed_tokens.weight']   # shared_embeddings: the first alias's value
    return P
