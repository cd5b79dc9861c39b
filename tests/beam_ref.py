"""Beam search restated in plain torch: the comparator of `pasero_amd.decode.beam_search` on the CPU and its baseline on
the GPU.  It follows the behaviour of pasero's search (prompts, forced tokens, blacklist, 2K candidates of which up to K may
end, sentences that leave the batch once they own K finished hypotheses, length-normalised n-best lists) but picks the
candidates with a STABLE descending sort: among equal scores the lower flat index k*V + v comes first.

    step_fn(feed)        feed (rows, T) int64 -> logits (rows, T, V); the caller closes over encoder output and state
    reorder_fn(indices)  re-order (and shrink) whatever step_fn closes over along the batch dimension
"""
import math

import torch


def prompt_lengths(prompt, pad):
    """index of the last non-pad token + 1, per row"""
    cols = torch.arange(1, prompt.size(1) + 1, device=prompt.device)
    return ((prompt != pad) * cols).amax(dim=1)


def pick(flat, K):
    """(values, indices) of the 2K best per row, descending, ties by lower index; plus the (2K+1)-th (value, index) or None"""
    vals, idx = torch.sort(flat, dim=1, descending=True, stable=True)
    extra = (vals[:, 2 * K], idx[:, 2 * K]) if flat.size(1) > 2 * K else None
    return vals[:, :2 * K], idx[:, :2 * K], extra


def beam_ref(step_fn, reorder_fn, prompt, K, max_output_len, decoder_max_len, pad, eos, return_scores=False,
             len_penalty=1.0, blacklist=(), stats=None):
    """-> list of n-best lists of dicts (tokens, score, normalized_score[, pos_scores]).  `stats`, when a dict, receives
    'rows' (rows per step_fn call), 'min_gap' (smallest difference between neighbouring finite scores among the best
    2K + 1 of any sentence at any step), 'sent_gap' (the same per initial sentence) and 'max_logit'."""
    dev = prompt.device
    B0 = prompt.size(0)
    plen = prompt_lengths(prompt, pad)
    lo, hi = int(plen.min()), int(plen.max())
    max_len = min(decoder_max_len, hi + max_output_len)
    toks = torch.full((B0 * K, max_len), eos, dtype=torch.long, device=dev)
    w = min(prompt.size(1), max_len)
    toks[:, :w] = prompt.repeat_interleave(K, dim=0)[:, :w]
    feed = toks[:, :lo]
    cum = torch.zeros(B0 * K, max_len, device=dev) if return_scores else None
    done = [[] for _ in range(B0)]
    alive = list(range(B0))
    hyp = None
    if stats is not None:
        stats.update(rows=[], min_gap=math.inf, sent_gap=[math.inf] * B0, max_logit=0.0)
    for step in range(lo, max_len):
        logits = step_fn(feed)
        nB = len(alive)
        lp = logits.float().log_softmax(dim=-1)
        sc = lp[:, -1].clone()
        V = sc.size(-1)
        pref = None
        if lp.size(1) > 1:
            nxt = feed[:, 1:]
            pref = lp[:, :-1].gather(2, nxt.unsqueeze(2)).squeeze(2) * (nxt != pad)
            sc += pref.sum(dim=1, keepdim=True)
        for tok in blacklist:
            sc[:, tok] = -math.inf
        if step < hi:
            f = toks[:, step]
            locked = (f != pad) & (f != eos)
            only = torch.full_like(sc, -math.inf).scatter_(1, f[:, None], sc.gather(1, f[:, None]))
            sc = torch.where(locked[:, None], only, sc)
        flat = sc[::K] if hyp is None else (sc + hyp[:, None]).view(nB, K * V)
        vals, idx, extra = pick(flat, K)
        if stats is not None:
            stats['rows'].append(logits.size(0))
            stats['max_logit'] = max(stats['max_logit'], float(logits[:, -1].float().abs().max()))
            run = vals if extra is None else torch.cat([vals, extra[0][:, None]], dim=1)
            src = (idx if extra is None else torch.cat([idx, extra[1][:, None]], dim=1)) // V
            gaps = (run[:, :-1] - run[:, 1:]).double()
            # an exact tie between two tokens of ONE beam is a tie of their logits: a tie in any arithmetic, decided by
            # the tie rule and not by rounding — it does not count as a small gap
            counted = torch.isfinite(run[:, 1:]) & torch.isfinite(run[:, :-1]) & ~((gaps == 0) & (src[:, :-1] == src[:, 1:]))
            gaps = torch.where(counted, gaps, torch.full_like(gaps, math.inf))
            per = gaps.min(dim=1).values.tolist()
            for b, g in enumerate(per):
                stats['sent_gap'][alive[b]] = min(stats['sent_gap'][alive[b]], g)
            stats['min_gap'] = min(stats['min_gap'], min(per))
        beam, tok = idx // V, idx % V
        ends = (tok == eos) & torch.isfinite(vals) & (step >= plen[alive])[:, None]
        keep = list(range(nB))
        if bool(ends[:, :K].any()):
            for b in range(nB):
                for j in range(K):
                    if not ends[b, j] or len(done[alive[b]]) >= K:
                        continue
                    row = b * K + int(beam[b, j])
                    h = {'tokens': toks[row, 1:step + 1].clone(), 'score': -vals[b, j]}
                    if return_scores:
                        p = cum[row, :step].clone()
                        p[step - 1] = vals[b, j]
                        p[1:] = p[1:] - p[:-1].clone()
                        h['pos_scores'] = -p
                    done[alive[b]].append(h)
                    if len(done[alive[b]]) == K:
                        keep.remove(b)
            if all(len(h) >= K for h in done):
                break
        kt = torch.tensor(keep, dtype=torch.long, device=dev)
        beam, tok, vals, ends = beam[kt], tok[kt], vals[kt], ends[kt]
        order = torch.sort(ends.int(), dim=1, stable=True).indices[:, :K]   # the first K that do not end, in order
        src = (kt[:, None] * K + beam.gather(1, order)).view(-1)            # rows of the batch step_fn just saw
        hyp = vals.gather(1, order).view(-1)
        new = tok.gather(1, order).view(-1)
        alive = [alive[b] for b in keep]
        toks = toks[src]
        toks[:, step] = new
        if return_scores:
            cum = cum[src]
            if pref is not None:
                cum[:, :step - 1] = pref.cumsum(dim=1)[src]
            cum[:, step - 1] = hyp
        feed = new[:, None]
        reorder_fn(src)
    nB = len(alive)
    if return_scores:
        cum[:, 1:] = cum[:, 1:] - cum[:, :-1].clone()
        cum = -cum
    out = []
    for b0, nbest in enumerate(done):
        if not nbest:
            i = alive.index(b0)
            h = {'tokens': toks.view(nB, K, -1)[i, 0, 1:], 'score': -hyp.view(nB, K)[i, 0]}
            if return_scores:
                h['pos_scores'] = cum.view(nB, K, -1)[i, 0, :-1]
            nbest = [h]
        for h in nbest:
            h['normalized_score'] = h['score'] / (len(h['tokens']) + 1) ** len_penalty
        nbest = sorted(nbest, key=lambda h: float(h['normalized_score']))
        for h in nbest:
            is_pad = h['tokens'] == pad
            h['tokens'] = h['tokens'][:int((~is_pad).sum())]
            if return_scores:
                h['pos_scores'] = h['pos_scores'][~is_pad]
        out.append(nbest)
    return out


def select_ref(logits, K, V, eos, hyp=None, bias=None, forced=None, pad=1, blacklist=(), eos_counts=None, dtype=torch.float64):
    """one selection step in `dtype` arithmetic (fp64: the comparator of pk_beam_select; fp32: the reference's own
    arithmetic, whose error against fp64 sets the tolerance).  logits (B*K, V).  -> dict of tensors"""
    rows = logits.size(0)
    B = rows // K
    sc = logits.to(dtype).log_softmax(dim=-1)
    if bias is not None:
        sc = sc + bias.to(dtype)[:, None]
    for t in blacklist:
        sc[:, t] = -math.inf
    if forced is not None:
        locked = (forced != pad) & (forced != eos)
        only = torch.full_like(sc, -math.inf).scatter_(1, forced[:, None], sc.gather(1, forced[:, None]))
        sc = torch.where(locked[:, None], only, sc)
    flat = sc[::K] if hyp is None else (sc + hyp.to(dtype)[:, None]).view(B, K * V)
    vals, idx, extra = pick(flat, K)
    beam, tok = idx // V, idx % V
    counts = torch.ones(B, dtype=torch.bool, device=logits.device) if eos_counts is None else eos_counts.bool()
    ends = (tok == eos) & torch.isfinite(vals) & counts[:, None]
    order = torch.sort(ends.int(), dim=1, stable=True).indices[:, :K]
    offs = torch.arange(B, device=logits.device)[:, None] * K
    return {'score': vals, 'beam': beam, 'tok': tok, 'eos': ends, 'extra': None if extra is None else extra[0], 'n_eos': ends[:, :K].sum(dim=1),
            'sel_beam': (beam.gather(1, order) + offs).view(-1), 'sel_tok': tok.gather(1, order).view(-1),
            'sel_score': vals.gather(1, order).view(-1)}
