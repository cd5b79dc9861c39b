"""tests/beam_ref.py (the plain-torch comparator of the native beam search) against the reference's own search: fed the
logits the reference's decoder returned at every step of the recorded search (tests/golden/beam_trace.npz), it must apply
the recorded re-orderings, feed the recorded decoder inputs and end with the recorded best hypotheses."""
import numpy as np
import torch

from conftest import load_golden, golden_cfg
from beam_ref import beam_ref, select_ref


def test_beam_ref_replays_the_recorded_search():
    g = load_golden('beam_trace')
    cfg = golden_cfg(g)
    B, K, n_calls, n_reorders = (int(g[k]) for k in ('B', 'K', 'n_calls', 'n_reorders'))
    calls, reorders = [], []

    def step_fn(feed):
        i = len(calls)
        assert i < n_calls, 'more decoder calls than the reference made'
        calls.append(feed.clone())
        np.testing.assert_array_equal(feed.numpy(), g[f'dec_in_{i}'])
        return torch.from_numpy(g[f'logits_{i}']).unsqueeze(1)

    def reorder_fn(idx):
        i = len(reorders)
        assert i < n_reorders
        np.testing.assert_array_equal(idx.numpy(), g[f'reorder_{i}'])
        reorders.append(idx)

    bos = torch.full((B, 1), cfg.bos_idx, dtype=torch.long)
    stats = {}
    hyps = beam_ref(step_fn, reorder_fn, bos, K, int(g['max_output_len']), cfg.decoder_max_len, cfg.padding_idx, cfg.eos_idx,
                    stats=stats)
    assert len(calls) == n_calls and len(reorders) == n_reorders
    assert len(set(stats['rows'])) > 1  # the 12 -> 9 row shrink
    for b, nbest in enumerate(hyps):
        np.testing.assert_array_equal(nbest[0]['tokens'].numpy(), g[f'best_{b}'])
    assert 0 < stats['min_gap'] < 1e-3  # 9.0e-5 on this trace: far above fp32 rounding of the recorded logits


def test_select_ref_gap_cap_of_the_gpu_test_seeds():
    """the GPU selection test skips index checks where the fp64 gap to a neighbour is below 1e-4 and caps the skipped
    share at 5 % per case: computed here from the comparator alone, on the same seeded inputs"""
    from beam_cases import SELECT_CASES, make_select_case, skipped_share
    for case in SELECT_CASES:
        if case['B'] * case['K'] * case['V'] > 6_000_000:
            continue  # the large cases are checked on the GPU box, with the same function
        inp = make_select_case(case, 'cpu')
        ref = select_ref(inp['logits'], case['K'], case['V'], inp['eos'], hyp=inp['hyp'], forced=inp['forced'], pad=inp['pad'],
                         blacklist=inp['blacklist'], eos_counts=inp['eos_counts'])
        assert skipped_share(ref) <= 0.05, case
