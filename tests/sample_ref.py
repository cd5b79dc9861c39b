"""Plain-torch fp64 restatement of the sampling search (pasero/decoding.py:1005-1221) under the project's draw rule, in the
role tests/beam_ref.py has for beam search: `select_ref` is one step's choice (what pk_sample_select computes),
`sample_ref` the loop around a decoder.  Draw rule: the kept tokens in the order (probability descending, token id
ascending), M their total probability, the token is the first whose inclusive cumulative probability exceeds u * M."""
import torch


def penalised_logits(logits, history, penalty):
    """decoding.py:1136-1141, in the logits' own dtype (the penalised value is rounded to it)"""
    x = logits.clone()
    if penalty != 1.0 and history is not None and history.size(1) > 0:
        score = torch.gather(x, 1, history)
        score = torch.where(score < 0, score * penalty, score / penalty)
        x.scatter_(1, history, score)
    return x


def select_ref(logits, mode, *, top_k=0, top_p=1.0, u=None, history=None, penalty=1.0, inv_temperature=1.0, blacklist=(),
               finished=None, pad=-1, forced=None):
    """logits (B, V) of any float dtype -> dict of per-row tensors: token, logprob, lse (fp64), n_kept, kept_mass, and what
    the tests judge with: `order` (B, V) token ids in the rule's order, `cum` (B, V) fp64 inclusive cumulative
    probability in that order, `chosen` (the token before forcing), `boundary_margin` (top-p: distance of p to the nearest
    cumulative edge at the nucleus' end; top-k: lp gap between the k-th and (k+1)-th; inf elsewhere), `draw_margin`
    (distance of u * M to the nearest edge of the chosen token's interval, over M), `greedy_gap` (best minus second lp)."""
    B, V = logits.shape
    dev = logits.device
    x = penalised_logits(logits, history, penalty)
    xs = x.float()
    if inv_temperature != 1.0:
        xs = xs * torch.tensor(inv_temperature, dtype=torch.float32, device=dev)  # the scaling is fp32 by contract
    xs = xs.double()
    lse = torch.logsumexp(xs, dim=-1)
    lp = xs - lse[:, None]
    for t in blacklist:
        lp[:, t] = -torch.inf
    if finished is not None:
        keep = lp[:, pad].clone()
        lp.masked_fill_(finished.bool()[:, None], -torch.inf)
        lp[:, pad] = keep
    slp, order = lp.sort(dim=-1, descending=True, stable=True)
    cum = slp.exp().cumsum(dim=-1)
    inf = torch.full((B,), float('inf'), dtype=torch.float64, device=dev)
    bmargin, dmargin = inf.clone(), inf.clone()
    ggap = (slp[:, 0] - slp[:, 1]) if V > 1 else inf.clone()
    ggap = torch.where(torch.isnan(ggap), inf, ggap)
    ar = torch.arange(B, device=dev)
    if mode == 'greedy':
        chosen = order[:, 0]  # lowest id among equals (the sort is stable); 0 on a row of -inf
        n = torch.ones(B, dtype=torch.long, device=dev)
        M = torch.zeros(B, dtype=torch.float64, device=dev)
    else:
        if mode == 'topk':
            n = torch.full((B,), top_k, dtype=torch.long, device=dev)
            if top_k < V:
                gap = slp[:, top_k - 1] - slp[:, top_k]
                bmargin = torch.where(torch.isnan(gap), inf, gap)
        elif mode == 'topp':
            p = float(torch.tensor(top_p, dtype=torch.float32))
            below = (cum <= p).sum(dim=-1)
            n = (below + 1).clamp(max=V)
            hi_edge = (cum[ar, (n - 1)] - p).abs()
            lo_edge = torch.where(below > 0, (cum[ar, (below - 1).clamp(min=0)] - p).abs(), inf)
            bmargin = torch.minimum(hi_edge, lo_edge)
        else:
            n = torch.isfinite(lp).sum(dim=-1)
        M = cum[ar, (n - 1).clamp(min=0)]
        M = torch.where(n > 0, M, torch.zeros_like(M))
        target = u.double().to(dev) * M
        idx = (cum <= target[:, None]).sum(dim=-1)
        idx = torch.minimum(idx, (n - 1).clamp(min=0))
        chosen = order[ar, idx]
        hi_c = cum[ar, idx]
        lo_c = torch.where(idx > 0, cum[ar, (idx - 1).clamp(min=0)], torch.zeros_like(hi_c))
        dmargin = torch.minimum(target - lo_c, hi_c - target) / M.clamp(min=1e-300)
    token = chosen.clone()
    if forced is not None:
        token = torch.where(forced != pad, forced, token)
    return {'token': token, 'chosen': chosen, 'logprob': lp[ar, token], 'lse': lse, 'n_kept': n, 'kept_mass': M, 'order': order,
            'cum': cum, 'lp': lp, 'boundary_margin': bmargin, 'draw_margin': dmargin, 'greedy_gap': ggap}


def mode_of(sampling_temperature, sampling_topk, sampling_topp):
    if sampling_temperature == 0 or sampling_topk == 1:
        return 'greedy'
    if sampling_topk:
        return 'topk'
    return 'topp' if sampling_topp < 1 else 'full'


def sample_ref(step_fn, prompt, max_output_len, decoder_max_len, pad, eos, *, return_scores=False, sampling_temperature=1.0,
               sampling_topk=0, sampling_topp=1.0, repeat_penalty=1.0, blacklist=(), stop_sequences=(), uniforms=None,
               stats=None, tau_fn=None):
    """the loop of sample_on_the_fly; `step_fn(feed)` -> logits (B, T, V) of the decoder for the new tokens `feed`
    (it keeps the incremental state).  Returns the list of yielded dicts.  `stats` (dict) receives 'rows' (rows per decoder
    call), per-sentence minima 'draw_margin', 'boundary_margin', 'greedy_gap' (over the unforced, unfinished steps) and
    'max_logit'.  With `tau_fn` (select_ref's result -> tau of that step's arithmetic, tests/sample_cases.py:
    reference_tau) also 'boundary_short': sentences that had, at some such step, a boundary margin within tau * M."""
    dev = prompt.device
    B = prompt.size(0)
    mode = mode_of(sampling_temperature, sampling_topk, sampling_topp)
    plen = ((prompt != pad) * torch.arange(1, prompt.size(1) + 1, device=dev)).amax(dim=1)
    lo, hi = int(plen.min()), int(plen.max())
    max_len = min(decoder_max_len, hi + max_output_len)
    start = min(lo, max_len - 1)
    tokens = torch.full((B, max_len), pad, dtype=torch.long, device=dev)
    tokens[:, :prompt.size(1)] = prompt
    prompt_mask = tokens == pad
    stops = [torch.as_tensor(s, dtype=torch.long, device=dev) for s in stop_sequences if len(s) > 0]
    stops.append(torch.tensor([eos], dtype=torch.long, device=dev))
    has_eos = torch.zeros(B, dtype=torch.bool, device=dev)
    inf = torch.full((B,), float('inf'), dtype=torch.float64, device=dev)
    short = torch.zeros(B, dtype=torch.bool, device=dev)
    st = {'rows': [], 'draw_margin': inf.clone(), 'boundary_margin': inf.clone(), 'greedy_gap': inf.clone(), 'max_logit': 0.0}
    outs, prev = [], 0
    for i, step in enumerate(range(start, max_len)):
        has_eos = has_eos | (step >= plen + max_output_len)
        logits = step_fn(tokens[:, prev:step])
        st['rows'].append(logits.size(0))
        st['max_logit'] = max(st['max_logit'], float(logits.abs().max()))
        forced = tokens[:, step].clone()
        r = select_ref(logits[:, -1], mode, top_k=sampling_topk, top_p=sampling_topp,
                       u=None if mode == 'greedy' else uniforms[i], history=tokens[:, :step], penalty=repeat_penalty,
                       blacklist=blacklist, finished=has_eos, pad=pad, forced=forced)
        free = prompt_mask[:, step] & ~has_eos  # rows whose token was really chosen at this step
        for k in ('draw_margin', 'boundary_margin'):
            st[k] = torch.where(free, torch.minimum(st[k], r[k]), st[k])
        if tau_fn is not None:
            short |= free & (r['boundary_margin'] <= tau_fn(r) * r['kept_mass'].clamp(min=1e-300))
        if mode == 'greedy':
            st['greedy_gap'] = torch.where(free, torch.minimum(st['greedy_gap'], r['greedy_gap']), st['greedy_gap'])
        tokens[:, step] = r['token']
        out = {'tokens': tokens[:, prev + 1:step + 1].clone()}
        if return_scores:
            last = -r['logprob'].unsqueeze(1)
            if logits.size(1) > 1:
                nxt = tokens[:, prev + 1:step]
                lp = logits[:, :-1].double().log_softmax(dim=-1).gather(2, nxt.unsqueeze(2)).squeeze(2)
                last = torch.cat([-lp, last], dim=1)
            out['pos_scores'] = last
        outs.append(out)
        for s in stops:
            if step + 1 >= len(s):
                has_eos = has_eos | (tokens[:, step + 1 - len(s):step + 1] == s).all(dim=1)
        has_eos = has_eos & (step >= plen)
        prev = step
        if bool(has_eos.all()):
            break
    st['boundary_short'] = short
    if stats is not None:
        stats.update(st)
    return outs
