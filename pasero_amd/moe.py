"""`moe_transformer`: the Transformer whose feed-forward blocks are top-2 mixtures of experts (the model the NLLB-200 MoE
checkpoints load into).  Mirror of pasero/models/mixture_of_experts.py on top of the pasero_amd layers: the same class
names, configuration fields, parameter names of the reference's `basic` layout (`...layers.N.moe_layer.gate.weight`,
`...moe_layer.experts.E.fc1/fc2.weight/bias`), layer selection by ids or interval, load-balancing loss and checkpoint
conversions (fused / stacked / Tutel-named layouts load; conversion back is provided).

The computation is ROUTED (csrc/moe.hip): the reference's `basic` layer runs every expert over every token and multiplies
by a mostly-zero weight, with one host read per expert; here a gate kernel builds routing tables on the device, each token
runs through its two experts in grouped GEMM launches, and neither direction reads back to the host.  One autograd node
(`MoEFn`) covers gate, route, gather, fc1, fc2 and combine.

Deliberate difference: an expert that received no token gets an exactly ZERO gradient here; the reference
leaves its `.grad` at None (knowing it was unused would need a host read).

Not implemented, refused at construction: `moe_impl='tutel'` (third-party package, expert parallelism), `moe_impl='fused'`
(the reference's own constructor fails; its checkpoint layout still loads), gated (swiglu / geglu) experts, tensor
parallelism.  `capacity_factor` is Tutel's and has no effect in `basic`.  MoE layers take the per-op layer path.  MoE
decoders take the per-op decoding path by default (`decode.build_plan` returns None for an overridden `ffn`); with
`decode.moe_native(True)` (or PASERO_MOE_NATIVE_DECODE=1) their incremental calls run as one native step whose mixture blocks
are pk_moerows calls (csrc/moe_rows.hip: one-launch routing and few-rows expert GEMMs) — that step does not update `lb_loss`.
"""
import logging
from typing import Optional

import torch
import torch.nn as nn
from torch import Tensor

from . import functional as F
from . import modules
from .autograd import Function, _2d, _contig
from .config import register_model
from .transformer import (DummyEncoder, Transformer, TransformerDecoder, TransformerDecoderLayer, TransformerEncoder,
                          TransformerEncoderLayer)

logger = logging.getLogger('mixture_of_experts')

_LEAVES = ('fc1.weight', 'fc1.bias', 'fc2.weight', 'fc2.bias')
# Tutel's names for the stacked tensors of one layer (its fc2 weights are stored transposed) and for the gate
_TUTEL_NAMES = {'fc1.weight': 'tutel_moe_layer.experts.batched_fc1_w', 'fc2.weight': 'tutel_moe_layer.experts.batched_fc2_w',
                'fc1.bias': 'tutel_moe_layer.experts.batched_fc1_bias', 'fc2.bias': 'tutel_moe_layer.experts.batched_fc2_bias',
                'gate.weight': 'tutel_moe_layer.gates.0.wg.weight'}
_TUTEL_COUNT = 'tutel_moe_layer._num_global_experts'


# ---- checkpoint layouts ----
# basic:   <layer>.moe_layer.experts.<e>.fc1.weight ...   one tensor per expert (what the modules here hold)
# stacked: <layer>.moe_layer.fc1.weight (E, F, D) ...      fused: the same with the first two dimensions merged (E * F, D)
# tutel:   the stacked tensors under Tutel's names, fc2 transposed
# Every conversion works layer by layer from the gate: its row count is the number of experts, its name gives the prefix.
def _moe_prefixes(state_dict: dict) -> dict:
    """{'<layer>.moe_layer.': expert count} for every mixture in the checkpoint, whatever its layout"""
    found = {}
    for name, value in state_dict.items():
        for gate in ('gate.weight', _TUTEL_NAMES['gate.weight']):
            if name.endswith('.moe_layer.' + gate):
                found[name[:-len(gate)]] = value.size(0)
    return found


def stack_expert_params(state_dict: dict, concat: bool = False) -> None:
    """basic -> stacked, or fused with `concat`; in place.  Layers that are not in the basic layout are left as they are."""
    for prefix, count in _moe_prefixes(state_dict).items():
        for leaf in _LEAVES:
            per_expert = [f'{prefix}experts.{e}.{leaf}' for e in range(count)]
            if per_expert[0] in state_dict:
                tensors = [state_dict.pop(name) for name in per_expert]
                state_dict[prefix + leaf] = torch.cat(tensors) if concat else torch.stack(tensors)


def unstack_expert_params(state_dict: dict, shard_count: int = 1) -> None:
    """stacked or fused -> basic; in place.  `shard_count`: the checkpoint holds that fraction of the gate's experts."""
    for prefix, count in _moe_prefixes(state_dict).items():
        local = count // shard_count
        for leaf in _LEAVES:
            if prefix + leaf not in state_dict:
                continue
            merged = state_dict.pop(prefix + leaf)
            per_expert_dims = 1 if leaf.endswith('bias') else 2
            if merged.dim() == per_expert_dims:   # fused: split the leading dimension back into (expert, rows)
                merged = merged.reshape(local, merged.size(0) // local, *merged.shape[1:])
            if merged.size(0) != local:
                raise ValueError(f'{prefix}{leaf} holds {merged.size(0)} experts where {local} are expected')
            for e, tensor in enumerate(merged.unbind(0)):
                state_dict[f'{prefix}experts.{e}.{leaf}'] = tensor


def tutel_to_stacked(state_dict: dict) -> None:
    """Tutel's names -> the stacked layout; in place; other layouts are left as they are"""
    for prefix in _moe_prefixes(state_dict):
        state_dict.pop(prefix + _TUTEL_COUNT, None)
        for ours, theirs in _TUTEL_NAMES.items():
            if prefix + theirs in state_dict:
                value = state_dict.pop(prefix + theirs)
                state_dict[prefix + ours] = value.transpose(1, 2) if ours == 'fc2.weight' else value


def stacked_to_tutel(state_dict: dict) -> None:
    """basic or stacked -> Tutel's names (the way back of `tutel_to_stacked`); in place"""
    stack_expert_params(state_dict, concat=False)
    for prefix, count in _moe_prefixes(state_dict).items():
        for ours, theirs in _TUTEL_NAMES.items():
            if prefix + ours in state_dict:
                value = state_dict.pop(prefix + ours)
                state_dict[prefix + theirs] = value.transpose(1, 2) if ours == 'fc2.weight' else value
        state_dict[prefix + _TUTEL_COUNT] = torch.tensor(count)


def to_basic_layout(state_dict: dict, shard_count: int = 1) -> None:
    """any of the four layouts -> basic; in place"""
    tutel_to_stacked(state_dict)
    unstack_expert_params(state_dict, shard_count)


def _option(cfg, name: str, side: str = ''):
    """a mixture-of-experts option of the configuration; `side` ('encoder' / 'decoder') selects the per-stack ones"""
    return getattr(cfg, f'{side}_{name}' if side else name)


# ---- the layer ----
class _PointerTables:
    """device arrays of the experts' parameter addresses for the grouped launches, built once per (layer, placement) — a host
    to device copy — and reused until a parameter moves (`.to()`, a new dtype), as decode.Plan keeps its tables"""

    def __init__(self):
        self.key, self.tables, self.steps = None, None, None

    def get(self, groups):
        key = tuple(p.data_ptr() for g in groups if g is not None for p in g)
        if key != self.key:
            dev = groups[0][0].device
            self.tables = [None if g is None else torch.tensor([p.data_ptr() for p in g], dtype=torch.int64).to(dev)
                           for g in groups]
            self.steps = torch.arange(len(groups[0]), dtype=torch.int64, device=dev)
            self.key = key
        return self.tables

    def strided(self, stacked: Tensor) -> Tensor:
        """addresses of stacked[e] for every e, computed on the device (no copy from the host)"""
        return self.steps * (stacked.stride(0) * stacked.element_size()) + stacked.data_ptr()


class MoEFn(Function):
    """(y, gate_value, lb_loss) = top-2 mixture of E feed-forward experts over x (S, D) with padding mask `pad` (S,):
    gate GEMM -> pk_moe_gate -> gather to slot order -> grouped fc1 (+ activation) -> grouped fc2 -> weighted combine.
    Saved for backward: the slot-ordered input, the activations (and pre-activations where act' needs them), the experts'
    outputs and the gate outputs.  `params`: E fc1 weights, E fc2 weights [, E fc1 biases, E fc2 biases].
    With `F.moe_use_grouped()` off the expert GEMMs run as E pk_gemm launches, the counts read to the host (comparison path)."""

    @staticmethod
    def forward(ctx, x, pad, wg, act: str, has_bias: bool, tables: _PointerTables, *params):
        E = wg.size(0)
        w1, w2 = params[:E], params[E:2 * E]
        b1, b2 = (params[2 * E:3 * E], params[3 * E:]) if has_bias else (None, None)
        x2 = _contig(x)
        logits = F.gemm(x2, wg).float()  # the gate's linear layer in the model's dtype, then fp32 (Top2Gate, use_fp32)
        r = F.moe_gate(logits, pad)
        w1p, w2p, b1p, b2p = tables.get((w1, w2, b1, b2))
        counts = None if F.moe_use_grouped() else r.offsets.tolist()
        xg = F.moe_gather(x2, r)
        fdim = w1[0].size(0)
        pre = torch.empty(xg.size(0), fdim, dtype=x.dtype, device=x.device) if act not in ('none', 'relu') else None
        h = MoEFn._experts(xg, w1, b1, w1p, b1p, r.offsets, counts, fdim, act=act, preact=pre)
        ys = MoEFn._experts(h, w2, b2, w2p, b2p, r.offsets, counts, x2.size(1))
        y = F.moe_combine(ys, r)
        ctx.r, ctx.act, ctx.E, ctx.has_bias, ctx.tables, ctx.counts = r, act, E, has_bias, tables, counts
        ctx.experts, ctx.ptrs = (w1, w2), (w1p, w2p)
        ctx.save_for_backward(x2, wg, xg, h, pre, ys)
        ctx.mark_non_differentiable(r.gate_value)
        return y, r.gate_value, r.lb_loss

    @staticmethod
    def _experts(a, ws, bs, wp, bp, offsets, counts, n, b_col=False, act='none', aux=None, mode=0, preact=None):
        if counts is None:
            return F.moe_gemm(a, wp, offsets, n, bias_ptrs=bp, b_col=b_col, act=act, aux=aux, mode=mode, preact=preact)
        out = torch.empty(a.size(0), n, dtype=a.dtype, device=a.device)
        for e, (lo, hi) in enumerate(zip(counts[:-1], counts[1:])):
            if hi > lo:
                F.gemm(a[lo:hi], ws[e], b_col=b_col, bias=bs[e] if bs is not None else None, act=act,
                       aux=aux[lo:hi] if aux is not None else None, mode=mode,
                       preact=preact[lo:hi] if preact is not None else None, out=out[lo:hi])
        return out

    @staticmethod
    def _wgrad(dy, x, offsets, counts, tables, want_w: bool, want_b: bool):
        E, dev = offsets.numel() - 1, dy.device
        dw = torch.empty(E, dy.size(1), x.size(1), dtype=dy.dtype, device=dev) if want_w else None
        db = torch.empty(E, dy.size(1), dtype=dy.dtype, device=dev) if want_b else None
        if counts is None:
            if want_w or want_b:
                F.moe_gemm_wgrad(dy, x, offsets, tables.strided(dw) if want_w else None, tables.strided(db) if want_b else None)
            return dw, db
        for e, (lo, hi) in enumerate(zip(counts[:-1], counts[1:])):
            if hi == lo:
                for t in (dw, db):
                    if t is not None:
                        t[e].zero_()
            elif want_w:
                F.gemm(dy[lo:hi], x[lo:hi], a_col=True, b_col=True, out=dw[e], asum_out=db[e] if want_b else None)
            elif want_b:
                db[e].copy_(F.colsum(dy[lo:hi]))
        return dw, db

    @staticmethod
    def backward(ctx, dy, _d_gate_value, d_lb):
        x2, wg, xg, h, pre, ys = ctx.saved_tensors
        r, E, act, counts, tables = ctx.r, ctx.E, ctx.act, ctx.counts, ctx.tables
        w1, w2 = ctx.experts
        w1p, w2p = ctx.ptrs
        ng = ctx.needs_input_grad
        first = 6
        want = lambda k: any(ng[first + k * E: first + (k + 1) * E])
        dy2 = _contig(dy)
        dys = F.moe_gather(dy2, r, scaled=True)
        d_top_w = F.moe_dot(dy2, ys, r)
        if act == 'none':
            dh = MoEFn._experts(dys, w2, None, w2p, None, r.offsets, counts, h.size(1), b_col=True)
        else:
            dh = MoEFn._experts(dys, w2, None, w2p, None, r.offsets, counts, h.size(1), b_col=True, act=act,
                                aux=h if pre is None else pre, mode=2)
        dw2, db2 = MoEFn._wgrad(dys, h, r.offsets, counts, tables, want(1), ctx.has_bias and want(3))
        dw1, db1 = MoEFn._wgrad(dh, xg, r.offsets, counts, tables, want(0), ctx.has_bias and want(2))
        # the gate: d logits through the normalisation, the mask and the softmax, plus the load-balancing term
        d_logits = F.moe_gate_bwd(d_top_w, r, d_lb.float() if d_lb is not None else None, 1.0 if d_lb is not None else 0.0)
        dl = d_logits.to(x2.dtype)
        dx = None
        if ng[0]:
            dxs = MoEFn._experts(dh, w1, None, w1p, None, r.offsets, counts, x2.size(1), b_col=True)
            dx = F.moe_combine(dxs, r, weighted=False)
            F.gemm(dl, wg, b_col=True, aux=dx, mode=1, out=dx)
        dwg = F.gemm(dl, x2, a_col=True, b_col=True) if ng[2] else None
        grads = []
        for k, stacked in enumerate((dw1, dw2, db1, db2)[:4 if ctx.has_bias else 2]):
            grads += [stacked[e] if (stacked is not None and ng[first + k * E + e]) else None for e in range(E)]
        return (dx, None, dwg, None, None, None, *grads)


class Top2Gate(nn.Linear):
    """the gate's parameters (`gate.weight` (E, D), no bias); its arithmetic — logits in the model's dtype, fp32 from there
    on — is part of MoEFn"""

    def __init__(self, embed_dim: int, expert_count: int, use_fp32: bool = True):
        super().__init__(embed_dim, expert_count, bias=False)
        self.use_fp32 = use_fp32


class Expert(nn.Module):
    """one expert's parameters (modules.py:231-245; fc1 / fc2 as in the reference's `basic` layout)"""

    def __init__(self, embed_dim: int, expert_dim: int, has_bias: bool = True):
        super().__init__()
        self.fc1 = modules.Linear(embed_dim, expert_dim, bias=has_bias)
        self.fc2 = modules.Linear(expert_dim, embed_dim, bias=has_bias)


class MixtureOfExperts(nn.Module):
    """mixture_of_experts.py:141-199 (BasicMixtureOfExperts): forward(x (B, T, D), padding_mask (B, T)) ->
    (y (B, T, D), gate_value (B, T, E) fp32, {}); `lb_loss` is left on the module for `MOETransformer.compute_loss`"""
    is_sharded = False

    def __init__(self, embed_dim: int, expert_dim: int, local_expert_count: int, global_expert_count: int,
                 activation_fn: str = 'relu', has_bias: bool = True, **kwargs):
        super().__init__()
        if activation_fn in ('swiglu', 'geglu'):
            raise NotImplementedError(f"pasero_amd: activation_fn='{activation_fn}': gated (swiglu / geglu) experts are not "
                                      f"implemented")
        if not 2 <= global_expert_count <= 256:
            raise NotImplementedError(f'pasero_amd: expert count {global_expert_count}: a mixture takes 2 to 256 experts')
        if local_expert_count != global_expert_count:
            raise NotImplementedError('pasero_amd: expert parallelism is not implemented (every device holds all experts)')
        if embed_dim % 8 or expert_dim % 8:
            raise NotImplementedError(f'pasero_amd: embed_dim {embed_dim} / expert_dim {expert_dim} must be multiples of 8')
        self.embed_dim, self.expert_dim, self.expert_count = embed_dim, expert_dim, global_expert_count
        self.has_bias = has_bias
        self.gate = Top2Gate(embed_dim, self.expert_count, use_fp32=True)
        self.experts = nn.ModuleList([Expert(embed_dim, expert_dim, has_bias) for _ in range(self.expert_count)])
        self.act_name = modules.get_activation_fn(activation_fn).name
        self.lb_loss = None
        self._tables = _PointerTables()

    def forward(self, x: Tensor, padding_mask: Optional[Tensor]):
        shape = x.shape
        x2 = _2d(x)
        pad = None if padding_mask is None else _contig(padding_mask.reshape(-1))
        ex = self.experts
        params = [e.fc1.weight for e in ex] + [e.fc2.weight for e in ex]
        if self.has_bias:
            params += [e.fc1.bias for e in ex] + [e.fc2.bias for e in ex]
        y, gate_value, self.lb_loss = MoEFn.apply(x2, pad, self.gate.weight, self.act_name, self.has_bias, self._tables,
                                                  *params)
        return y.view(shape), gate_value.view(*shape[:-1], -1), {}


def _refuse(cfg, dist_cfg):
    if (getattr(dist_cfg, 'tp_size', None) or 1) > 1:
        raise NotImplementedError('pasero_amd: tensor parallelism (tp_size > 1) is not supported for mixtures of experts')
    impl = _option(cfg, 'moe_impl')
    if impl == 'tutel':
        raise NotImplementedError("pasero_amd: moe_impl='tutel' needs the third-party Tutel package and expert parallelism, "
                                  "neither is implemented; use moe_impl='basic' (Tutel checkpoints still load)")
    if impl == 'fused':
        raise NotImplementedError("pasero_amd: moe_impl='fused' is not implemented (the reference's own constructor fails); "
                                  "use moe_impl='basic' (the fused checkpoint layout still loads)")
    if impl != 'basic':
        raise NotImplementedError(f"pasero_amd: moe_impl='{impl}' is unknown (basic)")


class _MOELayerMixin:
    """a Transformer layer whose feed-forward block is a mixture of experts (mixture_of_experts.py:405-478): no fc1 / fc2 /
    fc3, `ffn` overridden (so the fused block tails and the one-call layer step aside, and the native decoding step too unless
    `decode.moe_native` is on)"""

    def _build_moe(self, cfg, dist_cfg, side: str, ffn_dim: int):
        _refuse(cfg, dist_cfg)
        expert_count, expert_dim = _option(cfg, 'expert_count', side), _option(cfg, 'expert_dim', side) or ffn_dim
        del self.fc1, self.fc2, self.fc3
        self.fc1 = self.fc2 = self.fc3 = None  # (plain attributes: the shared layer code asks `fc3 is None`)
        count = expert_count.get(self.layer_id, expert_count.get(str(self.layer_id))) if isinstance(expert_count, dict) \
            else expert_count
        count = count or 0
        if count < 2:
            raise NotImplementedError(f'pasero_amd: layer {self.name}: {count} experts; there should be at least 2')
        self.moe_layer = MixtureOfExperts(embed_dim=cfg.embed_dim, expert_dim=expert_dim, local_expert_count=count,
                                          global_expert_count=count, capacity_factor=_option(cfg, 'capacity_factor'),
                                          activation_fn=cfg.activation_fn, has_bias=cfg.has_bias)
        self.gate_key = f'{self.name}_gate'

    def ffn(self, x: Tensor, residual: Tensor, padding_mask) -> Tensor:
        x, gate_value, metadata = self.moe_layer(x, padding_mask)
        if 'capacity' in metadata:
            self.layer_outputs[f'{self.name}_capacity'] = metadata['capacity']
        if self.gate_key in self.return_layers:
            self.layer_outputs[self.gate_key] = gate_value
        return x

    def _wgrad_open(self, x: Tensor, attns) -> Tensor:
        self._wgrad_close(attns)  # (the grouped weight-gradient launch is built around fc1 / fc2: per-op here)
        return x

    def _ffn_block(self, x: Tensor, residual: Tensor, padding_mask, link) -> Tensor:
        self._ffn_link = None
        if x is residual:
            x, residual = self._prenorm(x, 'ffn_prenorm', self.final_layer_norm)
        else:
            x = self.ffn_prenorm(x)
        x = self.ffn(x, residual, padding_mask)
        return self._block_end(x, residual, self.final_layer_norm, 'ffn_residual', 'ffn_postnorm', None)


class MOETransformerEncoderLayer(_MOELayerMixin, TransformerEncoderLayer):
    def __init__(self, cfg, dist_cfg, layer_id: int):
        super().__init__(cfg, dist_cfg, layer_id)
        self._build_moe(cfg, dist_cfg, 'encoder', cfg.encoder_ffn_dim)


class MOETransformerDecoderLayer(_MOELayerMixin, TransformerDecoderLayer):
    def __init__(self, cfg, dist_cfg, layer_id: int):
        super().__init__(cfg, dist_cfg, layer_id)
        self._build_moe(cfg, dist_cfg, 'decoder', cfg.decoder_ffn_dim)


def _is_moe_layer(cfg, side: str, layer_id: int) -> bool:
    ids, interval = _option(cfg, 'expert_layer_ids', side), _option(cfg, 'expert_interval', side)
    return bool((ids is not None and layer_id in ids) or (interval and (layer_id + 1) % interval == 0))


class MOETransformerEncoder(TransformerEncoder):
    def build_layer(self, layer_id: int) -> nn.Module:
        if _is_moe_layer(self.cfg, 'encoder', layer_id):
            layer = MOETransformerEncoderLayer(self.cfg, self.dist_cfg, layer_id)
        else:
            layer = TransformerEncoderLayer(self.cfg, self.dist_cfg, layer_id)
        return modules.checkpoint_wrapper(layer, activate=self.cfg.checkpoint_activations)


class MOETransformerDecoder(TransformerDecoder):
    def build_layer(self, layer_id: int) -> nn.Module:
        if _is_moe_layer(self.cfg, 'decoder', layer_id):
            layer = MOETransformerDecoderLayer(self.cfg, self.dist_cfg, layer_id)
        else:
            layer = TransformerDecoderLayer(self.cfg, self.dist_cfg, layer_id)
        return modules.checkpoint_wrapper(layer, activate=self.cfg.checkpoint_activations)


@register_model('moe_transformer')
class MOETransformer(Transformer):
    """mixture_of_experts.py:509-671"""

    def __init__(self, cfg, dist_cfg, task):
        _refuse(cfg, dist_cfg)
        super().__init__(cfg, dist_cfg, task)

    moe_cls = MixtureOfExperts

    def build_encoder(self, embed=None):
        if self.cfg.model_type == 'decoder':
            return DummyEncoder()
        return MOETransformerEncoder(self.cfg, self.dist_cfg, self.task, embed=embed)

    def build_decoder(self, embed=None):
        return MOETransformerDecoder(self.cfg, self.dist_cfg, self.task, embed=embed)

    def moe_layers(self):
        layers = list(getattr(self.encoder, 'layers', [])) + list(self.decoder.layers)
        return [layer for layer in layers if hasattr(layer, 'moe_layer')]

    def compute_loss(self, logits: Tensor, target: Tensor, layer_outputs: dict, *args, **kwargs):
        loss, logs = super().compute_loss(logits, target, layer_outputs, *args, **kwargs)
        capacity = [layer_outputs.pop(key) for key in list(layer_outputs) if key.endswith('_capacity')]
        logs['capacity'] = sum(capacity) / max(1, len(capacity))
        weight = _option(self.cfg, 'load_balancing')
        if weight:
            lb = sum(layer.moe_layer.lb_loss.float() for layer in self.moe_layers())
            lb = lb * (target != self.padding_idx).sum()
            loss = loss + weight * lb
            logs['lb_loss'] = lb.item()  # (as the reference: one more host read per step, only with load balancing on)
        return loss, logs

    def update_state_dict(self, state_dict: dict) -> None:
        to_basic_layout(state_dict)
        if self.training:  # fine-tuning a dense checkpoint: gates and experts it lacks keep their initialisation
            before = set(state_dict)
            modules.add_missing_parameters(self, state_dict, r'.*\.moe_layer\.')
            for name in sorted(set(state_dict) - before):
                logger.warning(f'{name}: not in the checkpoint, keeps its initial value')
        super().update_state_dict(state_dict)

    @classmethod
    def shard_state_dict(cls, state_dict, shard_id=0, shard_count=1, total_shard_count=1, **kwargs):
        """mixture_of_experts.py:612-645 for one shard: any layout -> the stacked layout, nothing is split"""
        if shard_count != 1 or shard_id != 0:
            raise NotImplementedError('pasero_amd: expert-parallel (sharded) checkpoints are not supported')
        state_dict = dict(state_dict)
        to_basic_layout(state_dict, shard_count=total_shard_count)
        stack_expert_params(state_dict, concat=False)
        return state_dict

    @classmethod
    def unshard_state_dict(cls, *state_dicts, total_shard_count=1, **kwargs):
        """mixture_of_experts.py:647-671 for one shard: any layout -> the basic layout"""
        if len(state_dicts) != 1:
            raise NotImplementedError('pasero_amd: expert-parallel (sharded) checkpoints are not supported')
        state_dict = dict(state_dicts[0])
        to_basic_layout(state_dict, shard_count=total_shard_count)
        return state_dict
