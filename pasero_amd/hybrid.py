"""`hybrid_transformer` / `adapter_hybrid_transformer`: the Transformer encoder with an LSTM decoder and additive single-head
attention at the first LSTM layer.  Mirror of pasero/models/hybrid.py on top of the pasero_amd layers: the same class names,
configuration fields, parameter names (`decoder.layers.N.weight_ih_l0 ...`, `decoder.attention.{key,query,inner}_proj`) and
incremental state (`prev_hiddens` / `prev_cells` (B, L, hidden), `attn_key` (B, 1, S, hidden)).

The two pieces the per-op model spends its time in are kernels of their own:
  * the recurrence (csrc/lstm.hip, `LSTMFn`): the input-side product over all B T rows is one GEMM (`LinearFn`), the walk over
    t is one launch per step with the whole cell in the epilogue of the h_{t-1} W_hh^T tile;
  * the attention (csrc/addattn.hip, `AdditiveAttentionFn`): scores, mask, softmax and context in one launch, without the
    (B, T, S, hidden) tensor of tanh(key + query).
Everything else (LayerNorm, projections, dropout, embedding, the vocabulary loss) is the package's existing path.

Refused at construction: tensor parallelism, `model_type='decoder'`, a hidden size that is not a multiple of 16, an embedding
size that is not a multiple of 8.  Tensors of different dtypes in one call raise a TypeError.  Incremental calls take the
per-op route (`decode.build_plan` is for Transformer decoders): a step is a handful of launches.
"""
import math
from typing import Optional

import torch
import torch.nn as nn
from torch import Tensor

from . import functional as F
from . import modules
from .adapters import AdapterTransformer
from .autograd import Function, LinearFn, _2d, _contig, weight_grad, wants_grad
from .config import register_model
from .modules import Embedding, Identity
from .transformer import Decoder, Transformer, _bench_block, _bench_region, defined


def _option(cfg, name: str):
    """an option only the hybrid configurations have"""
    return getattr(cfg, name)


class LSTMFn(Function):
    """(y (B, T, H), hT, cT (B, H)) of one LSTM layer from gx = x W_ih^T + b_ih (B, T, 4H), w_hh (4H, H), b_hh (4H,) and the
    optional initial state.  Saved for backward: y, c, the activated gates, w_hh (and h0 / c0).  Backward: d gx from
    pk_lstm_bwd; dW_hh = dGᵀ h_{t-1} and db_hh = colsum(dG) as one (B T)-row weight-gradient GEMM over a copy of y shifted by
    one step.  No gradient towards h0 / c0 (training starts from the zero state), none through hT / cT."""

    @staticmethod
    def forward(ctx, gx, w_hh, b_hh, h0=None, c0=None):
        gx = gx if gx.stride(-1) == 1 else gx.contiguous()
        w_hh, b_hh = _contig(w_hh), _contig(b_hh)
        h0, c0 = (None, None) if h0 is None else (_contig(h0), _contig(c0))
        y, c, gates, hT, cT = F.lstm_fwd(gx, w_hh, b_hh, h0, c0)
        if any(wants_grad(ctx)):
            ctx.save_for_backward(y, c, gates, w_hh, h0, c0)
        ctx.mark_non_differentiable(hT, cT)
        return y, hT, cT

    @staticmethod
    def backward(ctx, dy, _dh, _dc):
        y, c, gates, w_hh, h0, c0 = ctx.saved_tensors
        dg = F.lstm_bwd(_contig(dy), w_hh, c, gates, c0)
        dw = db = None
        want_w, want_b = ctx.needs_input_grad[1], ctx.needs_input_grad[2]
        if want_w:
            h_prev = torch.empty_like(y)
            if h0 is None:
                h_prev[:, 0].zero_()
            else:
                h_prev[:, 0].copy_(h0)
            h_prev[:, 1:].copy_(y[:, :-1])
            r = weight_grad(_2d(dg), _2d(h_prev), want_b)
            dw, db = r if want_b else (r, None)
        elif want_b:
            db = F.colsum(_2d(dg))
        return (dg if ctx.needs_input_grad[0] else None), dw, db, None, None


class AdditiveAttentionFn(Function):
    """(ctx (B, T, D), probs (B, T, S)) = attention of q (B, T, H) over k (B, S, H) with the score weights w (H,) and values
    (B, S, D); `key_pad` (B, S) bool or None.  `w_bias` (inner_proj.bias) shifts every score of a row equally: the kernel
    leaves it out and its gradient is exactly zero.  The probabilities are an output for inspection, not differentiable."""

    @staticmethod
    def forward(ctx, q, k, w, w_bias, key_pad, value):
        q, k, w, value = _contig(q), _contig(k), _contig(w), _contig(value)
        pad = None if key_pad is None else _contig(key_pad)
        probs, out = F.addattn_fwd(q, k, w, pad, value)
        if any(wants_grad(ctx)):
            ctx.save_for_backward(q, k, w, value, probs, w_bias)
        ctx.mark_non_differentiable(probs)
        return out, probs

    @staticmethod
    def backward(ctx, dctx, _dprobs):
        q, k, w, value, probs, w_bias = ctx.saved_tensors
        dq, dk, dw, dvalue = F.addattn_bwd(_contig(dctx), q, k, w, value, probs)
        ng = ctx.needs_input_grad
        db = torch.zeros_like(w_bias) if (w_bias is not None and ng[3]) else None
        return (dq if ng[0] else None, dk if ng[1] else None, dw if ng[2] else None, db, None, dvalue if ng[5] else None)


class LSTM(nn.Module):
    """one batch-first LSTM layer with nn.LSTM's parameter names, gate order (i, f, g, o) and initialisation
    (uniform ±1/sqrt(hidden)): forward(x (B, T, In), hx=(h0, c0) (B, H) or None) -> (y (B, T, H), (hT, cT))"""

    def __init__(self, input_size: int, hidden_size: int):
        super().__init__()
        if hidden_size % 16:
            raise NotImplementedError(f'pasero_amd: LSTM hidden size {hidden_size} must be a multiple of 16')
        if input_size % 8:
            raise NotImplementedError(f'pasero_amd: LSTM input size {input_size} must be a multiple of 8')
        self.input_size, self.hidden_size = input_size, hidden_size
        self.weight_ih_l0 = nn.Parameter(torch.empty(4 * hidden_size, input_size))
        self.weight_hh_l0 = nn.Parameter(torch.empty(4 * hidden_size, hidden_size))
        self.bias_ih_l0 = nn.Parameter(torch.empty(4 * hidden_size))
        self.bias_hh_l0 = nn.Parameter(torch.empty(4 * hidden_size))
        self.reset_parameters()

    def reset_parameters(self) -> None:
        if not modules._fast_init:
            bound = 1.0 / math.sqrt(self.hidden_size)
            for p in self.parameters():
                nn.init.uniform_(p, -bound, bound)

    def forward(self, x: Tensor, hx=None):
        gx = LinearFn.apply(x, self.weight_ih_l0, self.bias_ih_l0)
        h0, c0 = hx if hx is not None else (None, None)
        y, hT, cT = LSTMFn.apply(gx, self.weight_hh_l0, self.bias_hh_l0, h0, c0)
        return y, (hT, cT)


class AttentionLayer(nn.Module):
    """hybrid.py:23-58: forward -> (attn (B, T, kdim), probabilities (B, T, 1, S)); with a non-empty `state` the projected keys
    come from state['attn_key'] (B, 1, S, embed_dim), and a given `state` receives them"""

    def __init__(self, embed_dim: int, kdim: int):
        super().__init__()
        self.key_proj = modules.Linear(kdim, embed_dim)
        self.query_proj = modules.Linear(embed_dim, embed_dim)
        self.inner_proj = modules.Linear(embed_dim, 1)

    def forward(self, query: Tensor, key: Tensor, value: Tensor, key_padding_mask, state: Optional[dict] = None):
        key = state['attn_key'] if state else self.key_proj(key).unsqueeze(1)
        if state is not None:
            state['attn_key'] = key
        q = self.query_proj(query)
        attn, probs = AdditiveAttentionFn.apply(q, key.squeeze(1), self.inner_proj.weight.view(-1), self.inner_proj.bias,
                                                key_padding_mask, value)
        return attn, probs.unsqueeze(2)


def _refuse(cfg, dist_cfg) -> None:
    if (getattr(dist_cfg, 'tp_size', None) or 1) > 1:
        raise NotImplementedError('pasero_amd: tensor parallelism (tp_size > 1) is not supported for the LSTM decoder')
    if cfg.model_type == 'decoder':
        raise NotImplementedError("pasero_amd: model_type='decoder': hybrid_transformer is an encoder-decoder model (its "
                                  "decoder attends to the encoder's output)")
    hidden = _option(cfg, 'decoder_hidden_size')
    if hidden % 16:
        raise NotImplementedError(f'pasero_amd: decoder_hidden_size {hidden} must be a multiple of 16')
    if cfg.embed_dim % 8:
        raise NotImplementedError(f'pasero_amd: embed_dim {cfg.embed_dim} must be a multiple of 8')


class LSTMDecoderWithoutEmbed(Decoder):
    """hybrid.py:80-179"""

    def __init__(self, cfg, dist_cfg, task):
        super().__init__()
        _refuse(cfg, dist_cfg)
        self.cfg, self.dist_cfg, self.task = cfg, dist_cfg, task
        self.hidden_size = hidden = _option(cfg, 'decoder_hidden_size')
        D = cfg.embed_dim
        self.embed_proj = modules.Linear(D, D, bias=True) if _option(cfg, 'decoder_embed_proj') else Identity()
        self.dropout = modules.Dropout(defined(cfg.decoder_dropout, cfg.dropout))
        sizes = [D if layer == 0 else D + hidden for layer in range(cfg.decoder_layers)]
        self.layers = nn.ModuleList([LSTM(input_size=size, hidden_size=hidden) for size in sizes])
        self.layer_norms = nn.ModuleList([modules.LayerNorm(size, eps=cfg.norm_eps) for size in sizes])
        self.attention = AttentionLayer(embed_dim=hidden, kdim=D)
        self.out_proj = modules.Linear(hidden, D, bias=True) if hidden != D else Identity()
        self.cross_attn_key = f'dec_{cfg.decoder_layers - 1}_cross_attn'

    @_bench_region('decoder')
    def forward(self, encoder_out: Tensor, encoder_mask, decoder_input: Tensor, prompt_mask=None,
                state: Optional[dict] = None, return_layers=(), **kwargs):
        """encoder_out (B, S, D), encoder_mask (B, S), decoder_input (B, T, D) -> (features (B, T, D), layer_outputs).
        An empty `state` starts from the zero state (and may carry a prompt, T > 1) and is filled in."""
        return_layers = return_layers or ()
        x = self.embed_proj(decoder_input)
        if state:
            prev_hiddens = list(state['prev_hiddens'].unbind(dim=1))
            prev_cells = list(state['prev_cells'].unbind(dim=1))
        else:
            prev_hiddens = [None] * len(self.layers)
            prev_cells = [None] * len(self.layers)
        x = self.dropout(x)
        layer_outputs = {}
        attn = None
        for i, layer in enumerate(self.layers):
            residual = x
            hx = None if prev_hiddens[i] is None else (prev_hiddens[i].contiguous(), prev_cells[i].contiguous())
            input_ = x if attn is None else torch.cat([x, attn], dim=-1)
            input_ = self.layer_norms[i](input_)
            x, (h, c) = layer(input_, hx=hx)
            x = self.dropout(x)
            if i == 0:
                attn, attn_weights = self.attention(query=x, key=encoder_out, value=encoder_out,
                                                    key_padding_mask=encoder_mask, state=state)
                if self.cross_attn_key in return_layers:
                    layer_outputs[self.cross_attn_key] = attn_weights
            else:
                x = residual + x
            prev_hiddens[i], prev_cells[i] = h, c
        if state is not None:
            state['prev_hiddens'] = torch.stack(prev_hiddens, dim=1)
            state['prev_cells'] = torch.stack(prev_cells, dim=1)
        x = self.out_proj(x) + attn
        return x, layer_outputs


class LSTMDecoder(LSTMDecoderWithoutEmbed):
    """hybrid.py:182-230, plus `project=False` (the features before the vocabulary projection, for the fused training loss);
    `prompt_mask` and `meta` are accepted and ignored as in the reference"""

    def __init__(self, cfg, dist_cfg, task, embed: Optional[Embedding] = None):
        super().__init__(cfg, dist_cfg, task)
        self.embed_tokens = (Embedding(task.decoder_num_embeddings, cfg.embed_dim, self.padding_idx)
                             if embed is None else embed)
        if cfg.tied_output_projection:
            self.output_projection = None
        else:
            self.output_projection = modules.Linear(cfg.embed_dim, task.decoder_num_embeddings, bias=False)
            nn.init.xavier_uniform_(self.output_projection.weight)

    def forward(self, encoder_out: Tensor, encoder_mask, decoder_input: Tensor, prompt_mask=None,
                state: Optional[dict] = None, return_layers=(), meta: dict = {}, project: bool = True, **kwargs):
        x = self.embed_tokens(decoder_input)
        x, layer_outputs = super().forward(encoder_out, encoder_mask, x, state=state, return_layers=return_layers)
        if not project:
            return x, layer_outputs
        with _bench_block('output_projection'):
            if self.output_projection is None:
                x = self.embed_tokens.projection(x)
            else:
                x = self.output_projection(x)
        return x, layer_outputs


@register_model('hybrid_transformer')
class HybridTransformer(Transformer):
    """hybrid.py:61-71"""

    def build_decoder(self, embed: Optional[Embedding] = None):
        return LSTMDecoder(self.cfg, self.dist_cfg, self.task, embed=embed)


@register_model('adapter_hybrid_transformer')
class AdapterHybridTransformer(AdapterTransformer):
    """hybrid.py:74-77: adapters in the encoder only; the LSTM decoder has none and is frozen with the rest"""

    def build_decoder(self, embed: Optional[Embedding] = None):
        return LSTMDecoder(self.cfg, self.dist_cfg, self.task, embed=embed)
