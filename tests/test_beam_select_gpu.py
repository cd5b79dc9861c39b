"""pk_beam_select / pk_beam_reorder (csrc/beam.hip) against plain torch: an fp64 restatement with a stable sort
(tests/beam_ref.py: select_ref) on seeded inputs (tests/beam_cases.py), the recorded search of beam_trace.npz, and
`index_select` for the cache re-ordering."""
import ctypes
import math

import numpy as np
import pytest
import torch

from conftest import load_golden, golden_cfg
from beam_cases import SELECT_CASES, case_id, make_select_case, clear_positions, skipped_share
from beam_ref import select_ref

pytestmark = pytest.mark.gpu


def run_select(inp, B, K, V):
    from pasero_amd.decode import BeamSelect
    sel = BeamSelect(B, K, V, 'cuda')
    bl = torch.tensor(inp['blacklist'], dtype=torch.int64, device='cuda') if inp['blacklist'] else None
    sel.run(inp['logits'], B, inp['eos'], inp['pad'], hyp=inp['hyp'], forced=inp['forced'], blacklist=bl,
            eos_counts=inp['eos_counts'])
    torch.cuda.synchronize()
    return sel


@pytest.mark.parametrize('case', SELECT_CASES, ids=case_id)
def test_beam_select_against_fp64(case):
    """values: |kernel fp32 score - fp64| <= 2 x (torch's own fp32 `x.float().log_softmax(-1) + hyp` error against fp64 on
    the same input, its maximum over the candidates) + one ulp of the score; indices: equal wherever the fp64 gap to both
    neighbours exceeds 1e-4 or is exactly 0 (a bit-level tie: the lower flat index first); at most 5 % of the positions are
    skipped for a smaller gap."""
    B, K, V = case['B'], case['K'], case['V']
    inp = make_select_case(case, 'cuda')
    assert inp['logits'].stride(0) != V  # ld != V
    sel = run_select(inp, B, K, V)
    kw = dict(hyp=inp['hyp'], forced=inp['forced'], pad=inp['pad'], blacklist=inp['blacklist'], eos_counts=inp['eos_counts'])
    ref = select_ref(inp['logits'], K, V, inp['eos'], **kw)
    R = 2 * K
    score = sel.cand_score[:B * R].view(B, R)
    beam, tok, eosf = (t[:B * R].view(B, R).long() for t in (sel.cand_beam, sel.cand_tok, sel.cand_eos))
    finite = torch.isfinite(ref['score'])
    assert torch.equal(torch.isfinite(score), finite)
    assert bool(((tok >= 0) & (tok < V) & (beam >= 0) & (beam < K)).all())  # -inf slots carry a valid index
    # the reference arithmetic's own error: torch's CPU fp32 `x.float().log_softmax(-1) + hyp` against fp64, same input
    xc = inp['logits'].cpu()
    hc = None if inp['hyp'] is None else inp['hyp'].cpu()
    part = slice(None, None, K) if hc is None else slice(None)
    s32, s64 = xc[part].float().log_softmax(dim=-1), xc[part].double().log_softmax(dim=-1)
    if hc is not None:
        s32, s64 = s32 + hc[:, None], s64 + hc.double()[:, None]
    both = torch.isfinite(s64)
    err_torch = (s32.double() - s64)[both].abs().max().item()
    del s32, s64, xc
    ulp = torch.finfo(torch.float32).eps * ref['score'][finite].abs().max().item() if finite.any() else 0.0
    clear = clear_positions(ref)
    err = (score.double() - ref['score'])[finite].abs().max().item() if finite.any() else 0.0
    print(f'{case_id(case)}: kernel err {err:.3e}, torch fp32 err {err_torch:.3e}, ulp {ulp:.3e}, '
          f'skipped {skipped_share(ref):.4f}')
    assert err <= 2 * err_torch + ulp
    assert skipped_share(ref) <= 0.05
    assert torch.equal(beam[clear], ref['beam'][clear]) and torch.equal(tok[clear], ref['tok'][clear])
    assert torch.equal(eosf[clear].bool(), ref['eos'][clear])
    all_clear = clear.sum(dim=1) == finite.sum(dim=1)  # sentences without a skipped position: the derived outputs too
    if hasattr(all_clear, 'any') and all_clear.any() and bool(finite[all_clear].all()):
        rows_ok = all_clear.repeat_interleave(K)
        assert torch.equal(sel.n_eos[:B].long()[all_clear], ref['n_eos'][all_clear])
        assert torch.equal(sel.sel_beam[:B * K][rows_ok], ref['sel_beam'][rows_ok])
        assert torch.equal(sel.sel_tok[:B * K][rows_ok], ref['sel_tok'][rows_ok])
    if case['variant'] in ('eos_in', 'eos_nocount'):
        assert int(sel.n_eos[:B].sum()) == int(ref['n_eos'].sum()) > 0
    if case['variant'] == 'eos_out':
        assert int(sel.n_eos[:B].sum()) == 0 and int(eosf.sum()) > 0
    # log-sum-exp of the rows that took part
    lse = torch.logsumexp(inp['logits'].double(), dim=-1)
    part = slice(None, None, K) if inp['hyp'] is None else slice(None)
    ok = torch.isfinite(lse[part])
    assert (sel.lse[:B * K][part][ok].double() - lse[part][ok]).abs().max().item() <= 4e-6 * max(1.0, lse[part][ok].abs().max().item())


def test_bit_level_ties_follow_the_tie_rule():
    """16-bit inputs produce equal scores; at least one seeded case has one among its candidates, and a constructed row
    of all-equal logits must come out in index order"""
    found = 0
    for case in SELECT_CASES:
        if case['dtype'] != 'bf16' or case['B'] * case['K'] * case['V'] > 6_000_000 or case['variant'] != 'plain':
            continue
        inp = make_select_case(case, 'cuda')
        ref = select_ref(inp['logits'], case['K'], case['V'], inp['eos'], hyp=inp['hyp'])
        s = ref['score']
        found += int(((s[:, :-1] == s[:, 1:]) & torch.isfinite(s[:, 1:])).sum())
    assert found >= 1
    K, V, B = 3, 5000, 2
    x = torch.zeros(B * K, V, dtype=torch.bfloat16, device='cuda')
    inp = {'logits': x, 'hyp': torch.zeros(B * K, device='cuda'), 'forced': None, 'blacklist': (), 'eos_counts': None,
           'eos': 4999, 'pad': 1}
    sel = run_select(inp, B, K, V)
    assert sel.cand_tok[:B * 2 * K].view(B, 2 * K).tolist() == [list(range(2 * K))] * B
    assert sel.cand_beam[:B * 2 * K].tolist() == [0] * (B * 2 * K)


def test_beam_size_17_is_refused():
    from pasero_amd.decode import BeamSelect
    sel = BeamSelect(1, 17, 61, 'cuda')
    with pytest.raises(RuntimeError, match='beam size 17'):
        sel.run(torch.zeros(17, 61, device='cuda'), 1, 2, 1)


def test_replay_of_the_recorded_search():
    """tests/golden/beam_trace.npz: the recorded logits of every step through pk_beam_select, the hypothesis scores
    carried on the device: the recorded state re-ordering and the recorded next decoder input, exactly"""
    from pasero_amd.decode import BeamSelect
    g = load_golden('beam_trace')
    cfg = golden_cfg(g)
    B, K, V = (int(g[k]) for k in ('B', 'K', 'V'))
    sel = BeamSelect(B, K, V, 'cuda')
    hyp, nB, done = None, B, [0] * B
    alive = list(range(B))
    for i in range(int(g['n_reorders'])):
        logits = torch.from_numpy(g[f'logits_{i}']).cuda()
        assert logits.size(0) == nB * K
        sel.run(logits, nB, cfg.eos_idx, cfg.padding_idx, hyp=hyp)
        n_eos = sel.records(nB)[0]
        keep = []
        for b in range(nB):  # a sentence leaves once it owns K finished hypotheses
            done[alive[b]] += int(n_eos[b])
            if done[alive[b]] < K:
                keep.append(b)
        kt = torch.tensor(keep, device='cuda')
        idx = sel.sel_beam[:nB * K].view(nB, K)[kt].reshape(-1)
        tok = sel.sel_tok[:nB * K].view(nB, K)[kt].reshape(-1)
        hyp = sel.sel_score[:nB * K].view(nB, K)[kt].reshape(-1).contiguous()
        alive, nB = [alive[b] for b in keep], len(keep)
        np.testing.assert_array_equal(idx.cpu().numpy(), g[f'reorder_{i}'])
        if i + 1 < int(g['n_calls']):  # (the last re-ordering of a search that ran into the length limit feeds no call)
            np.testing.assert_array_equal(tok.cpu().numpy()[:, None], g[f'dec_in_{i + 1}'])


@pytest.mark.parametrize('dtype', [torch.float32, torch.bfloat16])
def test_beam_reorder_is_index_select_below_t(dtype):
    from pasero_amd import lib
    from pasero_amd.lib import check, dtype_code, stream_ptr
    n, rows, cap, D, t = 3, 12, 64, 128, 7
    gen = torch.Generator(device='cuda').manual_seed(5)
    src_k = [torch.randn(rows, cap, D, device='cuda', generator=gen).to(dtype) for _ in range(n)]
    src_v = [torch.randn(rows, cap, D, device='cuda', generator=gen).to(dtype) for _ in range(n)]
    poison = lambda: torch.full((rows, cap, D), 777.0, device='cuda', dtype=dtype)
    dst_k, dst_v = [poison() for _ in range(n)], [poison() for _ in range(n)]
    idx = torch.tensor([3, 3, 4, 9, 11, 10, 0, 0, 2], device='cuda')
    P = ctypes.c_void_p
    tab = lambda ts: (P * n)(*[x.data_ptr() for x in ts])
    check(lib.load().pk_beam_reorder(tab(src_k), tab(src_v), tab(dst_k), tab(dst_v), n, idx.data_ptr(), idx.numel(), rows, t,
                                     cap, D, dtype_code(src_k[0]), stream_ptr()), 'pk_beam_reorder')
    torch.cuda.synchronize()
    for s, d in zip(src_k + src_v, dst_k + dst_v):
        assert torch.equal(d[:idx.numel(), :t], s.index_select(0, idx)[:, :t])
        assert bool((d[:idx.numel(), t:] == 777.0).all()) and bool((d[idx.numel():] == 777.0).all())  # untouched
    with pytest.raises(RuntimeError, match='in-place'):
        check(lib.load().pk_beam_reorder(tab(src_k), tab(src_v), tab(src_k), tab(dst_v), n, idx.data_ptr(), idx.numel(), rows,
                                         t, cap, D, dtype_code(src_k[0]), stream_ptr()), 'pk_beam_reorder')
