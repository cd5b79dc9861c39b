"""Plain-torch restatement of `hybrid_transformer`'s decoder (pasero/models/hybrid.py) for the tests: the LSTM cell, the
additive attention and the decoder forward, in whatever dtype the inputs have (fp64 in the tests) on whatever device.  Nothing
here comes from pasero_amd; autograd differentiates it.  The encoder half is oracle/ref_cpu.py's."""
import torch


def lstm(gx, w_hh, b_hh, h0=None, c0=None):
    """gx (B, T, 4H) = x W_ih^T + b_ih; gate order i, f, g, o -> y (B, T, H), hT, cT.  On 16-bit tensors this IS the per-op
    composition in that type: one matmul and the pointwise operations per step, each rounding its result."""
    B, T, G = gx.shape
    H = G // 4
    h = gx.new_zeros(B, H) if h0 is None else h0
    c = gx.new_zeros(B, H) if c0 is None else c0
    ys = []
    for t in range(T):
        pre = gx[:, t] + (h @ w_hh.t() + b_hh)
        i, f, g, o = pre.split(H, dim=1)
        c = torch.sigmoid(f) * c + torch.sigmoid(i) * torch.tanh(g)
        h = torch.sigmoid(o) * torch.tanh(c)
        ys.append(h)
    return torch.stack(ys, dim=1), h, c


def additive_attention(q, k, w, key_pad, value):
    """q (B, T, H), k (B, S, H): projection outputs; w (H,); key_pad (B, S) bool or None; value (B, S, D)
    -> probs (B, T, S), ctx (B, T, D).  The reference's four lines (hybrid.py:49-56)."""
    scores = torch.tanh(k.unsqueeze(1) + q.unsqueeze(2)) @ w
    if key_pad is not None:
        scores = scores.masked_fill(key_pad.unsqueeze(1), float('-inf'))
    probs = torch.softmax(scores, dim=2)
    return probs, torch.bmm(probs, value)


def layer_norm(x, w, b, eps):
    mean = x.mean(dim=-1, keepdim=True)
    var = ((x - mean) ** 2).mean(dim=-1, keepdim=True)
    return (x - mean) / torch.sqrt(var + eps) * w + b


def decoder_forward(P, cfg, encoder_out, encoder_mask, tokens, state=None, prefix='decoder.'):
    """LSTMDecoder.forward without dropout -> (logits (B, T, V), attention probabilities (B, T, 1, S)).  P: name -> tensor
    (the state dict); `state`: the incremental state dict of the reference (empty on the first call), updated in place."""
    g = lambda name: P[prefix + name]
    has = lambda name: (prefix + name) in P
    L, eps = cfg.decoder_layers, cfg.norm_eps
    x = g('embed_tokens.weight')[tokens]
    if has('embed_proj.weight'):
        x = x @ g('embed_proj.weight').t() + g('embed_proj.bias')
    if state:
        hs, cs = list(state['prev_hiddens'].unbind(1)), list(state['prev_cells'].unbind(1))
    else:
        hs, cs = [None] * L, [None] * L
    attn = probs = None
    for i in range(L):
        residual = x
        inp = x if attn is None else torch.cat([x, attn], dim=-1)
        inp = layer_norm(inp, g(f'layer_norms.{i}.weight'), g(f'layer_norms.{i}.bias'), eps)
        gx = inp @ g(f'layers.{i}.weight_ih_l0').t() + g(f'layers.{i}.bias_ih_l0')
        x, hs[i], cs[i] = lstm(gx, g(f'layers.{i}.weight_hh_l0'), g(f'layers.{i}.bias_hh_l0'), hs[i], cs[i])
        if i == 0:
            if state:
                key = state['attn_key']
            else:
                key = (encoder_out @ g('attention.key_proj.weight').t() + g('attention.key_proj.bias')).unsqueeze(1)
            if state is not None:
                state['attn_key'] = key
            q = x @ g('attention.query_proj.weight').t() + g('attention.query_proj.bias')
            probs, attn = additive_attention(q, key.squeeze(1), g('attention.inner_proj.weight').view(-1), encoder_mask,
                                             encoder_out)
        else:
            x = residual + x
    if state is not None:
        state['prev_hiddens'], state['prev_cells'] = torch.stack(hs, dim=1), torch.stack(cs, dim=1)
    if has('out_proj.weight'):
        x = x @ g('out_proj.weight').t() + g('out_proj.bias')
    x = x + attn
    out_w = g('output_projection.weight') if has('output_projection.weight') else g('embed_tokens.weight')
    return x @ out_w.t(), probs.unsqueeze(2)


def label_smoothed_ce(logits, target, pad, eps):
    """the reference's training loss (sum over the real target tokens, natural logarithm) in the logits' own dtype"""
    logp = torch.log_softmax(logits.reshape(-1, logits.size(-1)), dim=-1)
    target = target.reshape(-1)
    keep = target != pad
    nll = -logp.gather(1, target.clamp(min=0)[:, None]).squeeze(1)[keep].sum()
    smooth = -logp.mean(dim=-1)[keep].sum()
    return (1 - eps) * nll + eps * smooth, nll, int(keep.sum())
