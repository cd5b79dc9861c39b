"""Plain-torch restatement (fp64 by default) of the mixture-of-experts layer as pasero_amd computes it — gate, top-2 with the
lower-index tie rule, routing tables, routed experts, load-balancing loss — for the tests of csrc/moe.hip and pasero_amd.moe.
Differentiable through torch autograd.  tests/test_moe_ref_cpu.py replays it against the reference's recorded values."""
import torch

ACTS = {
    'none': lambda x: x,
    'relu': torch.relu,
    'gelu': lambda x: torch.nn.functional.gelu(x),
    'gelu_tanh': lambda x: torch.nn.functional.gelu(x, approximate='tanh'),
    'silu': torch.nn.functional.silu,
}


def gate_ref(logits, pad, dtype=torch.float64):
    """logits (S, E), pad (S,) bool -> dict(gate_value (S, E), top_idx (S, 2) [-1 for padding], top_w (S, 2), top1_count (E,),
    prob_sum (E,), lb_loss, rank_gap: the smallest difference between the gate values at ranks 1, 2, 3 of any real token)"""
    S, E = logits.shape
    pad = pad.bool()
    g = logits.to(dtype).softmax(-1).masked_fill(pad[:, None], 0)
    order = torch.sort(-g.detach(), dim=-1, stable=True).indices  # higher value first, lower index among equal values
    gv = g.gather(1, order[:, :2])
    top_idx = order[:, :2].clone()
    den = gv.sum(1, keepdim=True)
    top_w = (gv / torch.where(den == 0, torch.ones_like(den), den)).masked_fill(pad[:, None], 0)
    top_idx[pad] = -1
    real = ~pad
    nt = int(real.sum())
    top1_count = torch.bincount(top_idx[real, 0], minlength=E) if nt else torch.zeros(E, dtype=torch.long)
    prob_sum = g.sum(0)
    lb_loss = E * ((top1_count.to(dtype) / nt) * (prob_sum / nt)).sum() if nt else g.sum() * 0
    srt = g.detach()[real].gather(1, order[real][:, :min(E, 3)])
    gap = float((srt[:, :-1] - srt[:, 1:]).min()) if nt else float('inf')
    if nt and E >= 3:
        gap = min(gap, float((srt[:, 0] - srt[:, 2]).min()))
    return dict(gate_value=g, top_idx=top_idx, top_w=top_w, top1_count=top1_count, prob_sum=prob_sum, lb_loss=lb_loss,
                rank_gap=gap)


def route_ref(top_idx, E):
    """(S, 2) [-1: padding] -> offsets (E+1,), slot_of (S, 2), token_of (2 * S_real,): pairs sorted by expert, token, k"""
    S = top_idx.size(0)
    pairs = sorted((int(top_idx[s, k]), s, k) for s in range(S) for k in range(2) if int(top_idx[s, k]) >= 0)
    offsets = torch.zeros(E + 1, dtype=torch.int32)
    slot_of = torch.full((S, 2), -1, dtype=torch.int32)
    token_of = torch.zeros(len(pairs), dtype=torch.int32)
    for slot, (e, s, k) in enumerate(pairs):
        offsets[e + 1] += 1
        slot_of[s, k] = slot
        token_of[slot] = s
    return torch.cumsum(offsets, 0).to(torch.int32), slot_of, token_of


def layer_ref(x, pad, wg, w1, b1, w2, b2, act='relu', dtype=torch.float64, logits_dtype=None):
    """x (S, D), pad (S,), gate weight (E, D), per-expert lists w1 (F, D), b1 (F,) | None, w2 (D, F), b2 (D,) | None ->
    (y (S, D), gate dict).  logits_dtype: round the gate logits to that type first (the model's dtype, as the layer does)"""
    E = wg.size(0)
    xd = x.to(dtype)
    logits = xd @ wg.to(dtype).t()
    if logits_dtype is not None:
        logits = logits.to(logits_dtype).to(dtype)
    gate = gate_ref(logits, pad, dtype)
    y = torch.zeros_like(xd)
    for e in range(E):
        for k in range(2):
            rows = (gate['top_idx'][:, k] == e).nonzero().flatten()
            if rows.numel() == 0:
                continue
            h = xd[rows] @ w1[e].to(dtype).t()
            if b1 is not None:
                h = h + b1[e].to(dtype)
            o = ACTS[act](h) @ w2[e].to(dtype).t()
            if b2 is not None:
                o = o + b2[e].to(dtype)
            y = y.index_add(0, rows, gate['top_w'][rows, k, None] * o)
    return y, gate
