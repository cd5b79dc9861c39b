"""helpers shared by the mixture-of-experts tests"""
import json

import numpy as np
import torch

import paramgen
from conftest import golden_names_shapes, load_golden


def moe_cfg(g=None, **overrides):
    from pasero_amd.config import MOETransformerConfig
    g = load_golden('moe') if g is None else g
    return MOETransformerConfig(**{**json.loads(str(g['cfg'])), **json.loads(str(g['moe_cfg'])), **overrides})


def moe_model(g=None, **overrides):
    from pasero_amd import moe  # noqa: F401  (registers the architecture)
    from pasero_amd.config import DistributedConfig, SyntheticTask, get_architecture
    from model_utils import load_paramgen
    g = load_golden('moe') if g is None else g
    cfg = moe_cfg(g, **overrides)
    model = get_architecture(cfg)(cfg, DistributedConfig(), SyntheticTask(int(g['V'])))
    load_paramgen(model, int(g['seed']))
    return cfg, model


def layer_weights(g, dtype=torch.float64):
    """the paramgen weights of the fixture's single MoE layer -> (wg, w1[E], b1[E], w2[E], b2[E])"""
    prefix = str(g['layer:prefix'])
    state = paramgen.make_state_dict(int(g['seed']), [(n, s) for n, s in golden_names_shapes(g) if n.startswith(prefix)])
    t = lambda name: torch.from_numpy(state[prefix + name]).to(dtype)
    E = state[prefix + 'gate.weight'].shape[0]
    return (t('gate.weight'), [t(f'experts.{e}.fc1.weight') for e in range(E)], [t(f'experts.{e}.fc1.bias') for e in range(E)],
            [t(f'experts.{e}.fc2.weight') for e in range(E)], [t(f'experts.{e}.fc2.bias') for e in range(E)])


def relmax(a, b):
    a, b = torch.as_tensor(np.asarray(a)).double(), torch.as_tensor(np.asarray(b)).double()
    return float((a - b).abs().max() / b.abs().max().clamp_min(1e-30))
