"""pk_moerows_route (csrc/moe_rows.hip: one launch of one workgroup, logits in the model's dtype) against pk_moe_gate on
logits.float() without a padding mask (four launches): top_idx, top_w, offsets, slot_of and token_of[:2 * rows] bit for bit."""
import pytest
import torch

pytestmark = pytest.mark.gpu

DTYPES = {'bf16': torch.bfloat16, 'f16': torch.float16, 'f32': torch.float32}
SIZES = [(1, 2), (5, 4), (17, 7), (64, 128), (3, 256), (1024, 256)]
SENTINEL = -7


def route(logits):
    from pasero_amd import lib
    from pasero_amd.lib import check, dtype_code, ptr, stream_ptr
    rows, E = logits.shape
    dev = logits.device
    out = dict(top_idx=torch.full((rows, 2), SENTINEL, dtype=torch.int32, device=dev),
               top_w=torch.full((rows, 2), float('nan'), dtype=torch.float32, device=dev),
               offsets=torch.full((E + 1,), SENTINEL, dtype=torch.int32, device=dev),
               slot_of=torch.full((rows, 2), SENTINEL, dtype=torch.int32, device=dev),
               token_of=torch.full((2 * rows + 9,), SENTINEL, dtype=torch.int32, device=dev))
    check(lib.load().pk_moerows_route(ptr(logits), rows, E, dtype_code(logits), ptr(out['top_idx']), ptr(out['top_w']),
                                      ptr(out['offsets']), ptr(out['slot_of']), ptr(out['token_of']), stream_ptr()), 'pk_moerows_route')
    return out


def assert_same_as_gate(logits):
    from pasero_amd import functional as F
    rows = logits.size(0)
    got = route(logits)
    want = F.moe_gate(logits.float().contiguous(), None)
    torch.cuda.synchronize()
    for name in ('top_idx', 'top_w', 'offsets', 'slot_of'):
        assert torch.equal(got[name], getattr(want, name)), name
    assert torch.equal(got['token_of'][:2 * rows], want.token_of)
    assert bool((got['token_of'][2 * rows:] == SENTINEL).all())   # entries beyond 2 * rows are not written
    assert int(got['offsets'][-1]) == 2 * rows
    return got


@pytest.mark.parametrize('dtype', list(DTYPES))
@pytest.mark.parametrize('rows,E', SIZES)
def test_random_logits(rows, E, dtype):
    gen = torch.Generator().manual_seed(1000 * rows + E)
    logits = (torch.randn(rows, E, generator=gen) * 3.0).to(DTYPES[dtype]).cuda()
    assert_same_as_gate(logits)


@pytest.mark.parametrize('dtype', list(DTYPES))
def test_ties_take_the_lower_expert(dtype):
    """rows of exactly equal logits, a tie for rank 1, a tie for rank 2 and a tie across the 64-lane boundary"""
    E = 130
    logits = torch.full((6, E), -2.0)
    logits[1] = 0.5                       # all equal: experts 0 and 1
    logits[2, [7, 100]] = 3.0             # rank 1 tie: 7 then 100
    logits[3, 5], logits[3, [60, 70]] = 4.0, 1.0   # rank 2 tie across lanes 60 / 70 - 64: 60
    logits[4, [129, 64, 65]] = 2.0        # three equal: 64 then 65
    logits[5, 128], logits[5, 0] = 1.0, 1.0        # 0 then 128
    got = assert_same_as_gate(logits.to(DTYPES[dtype]).cuda())
    assert got['top_idx'].tolist() == [[0, 1], [0, 1], [7, 100], [5, 60], [64, 65], [0, 128]]
    assert torch.equal(got['top_w'][1], torch.tensor([0.5, 0.5], device='cuda'))


@pytest.mark.parametrize('dtype', list(DTYPES))
def test_every_row_picks_the_first_two_experts(dtype):
    rows, E = 33, 4
    gen = torch.Generator().manual_seed(3)
    logits = torch.randn(rows, E, generator=gen)
    logits[:, 0] += 10.0
    logits[:, 1] += 5.0
    got = assert_same_as_gate(logits.to(DTYPES[dtype]).cuda())
    assert got['offsets'].tolist() == [0, rows, 2 * rows, 2 * rows, 2 * rows]
    assert got['token_of'][:2 * rows].tolist() == list(range(rows)) * 2
    assert got['slot_of'].tolist() == [[t, rows + t] for t in range(rows)]


def test_two_calls_give_the_same_bits():
    gen = torch.Generator().manual_seed(11)
    logits = torch.randn(257, 16, generator=gen).bfloat16().cuda()
    a, b = route(logits), route(logits)
    assert all(torch.equal(a[k], b[k]) for k in a if k != 'top_w') and torch.equal(a['top_w'], b['top_w'])
