"""CPU tests of the LSTM and additive-attention entry points of the C ABI (csrc/lstm.hip, csrc/addattn.hip): every argument check
answers with an error code and a message naming the entry point before anything is launched (the buffers are host memory:
a launch would not get as far as failing politely), and the scratch sizes."""
import ctypes

import pytest

F32, BF16, F16 = 0, 1, 2


@pytest.fixture(scope='module')
def L():
    from pasero_amd import lib
    return lib.load()


@pytest.fixture(scope='module')
def a():
    buf = ctypes.create_string_buffer(1 << 12)   # host memory: every call below must fail before it would be touched
    yield (ctypes.addressof(buf) + 255) // 256 * 256


def _err(L):
    return L.pk_last_error().decode()


def test_scratch_sizes(L):
    assert L.pk_lstm_bwd_scratch(0, 64, BF16) == 0 and L.pk_lstm_bwd_scratch(4, 0, BF16) == 0 and L.pk_lstm_bwd_scratch(4, 64, 7) == 0
    # the fp32 carry of dc [B][H] and W_hh transposed [H][4H], each rounded up to 256 bytes
    assert L.pk_lstm_bwd_scratch(3, 64, BF16) == 768 + 4 * 64 * 64 * 2
    assert L.pk_lstm_bwd_scratch(3, 64, F32) == 768 + 4 * 64 * 64 * 4
    assert L.pk_lstm_bwd_scratch(70, 128, F16) >= 70 * 128 * 4 + 4 * 128 * 128 * 2
    assert L.pk_addattn_bwd_scratch(0, 1, 1, 64) == 0 and L.pk_addattn_bwd_scratch(1, 1, 0, 64) == 0
    # ds fp32 [B][T][S] and one partial dw row per workgroup of 8 queries
    assert L.pk_addattn_bwd_scratch(2, 33, 130, 64) >= 2 * 33 * 130 * 4 + 2 * 5 * 64 * 4
    assert L.pk_addattn_bwd_scratch(2, 33, 130, 64) < L.pk_addattn_bwd_scratch(2, 41, 130, 64)


def test_lstm_fwd_argument_checks(L, a):
    def fwd(gx=a, w=a, b=a, h0=None, c0=None, y=a, c=a, gates=a, B=2, T=3, H=64, dtype=BF16, ldb=3 * 256, ldt=256):
        return L.pk_lstm_fwd(gx, ldb, ldt, w, b, h0, c0, y, c, gates, a, a, B, T, H, dtype, None)
    for kw, word in ((dict(gx=None), 'null'), (dict(w=None), 'null'), (dict(b=None), 'null'), (dict(y=None), 'null'),
                     (dict(c=None), 'null'), (dict(gates=None), 'null'), (dict(h0=a), 'h0 and c0'), (dict(c0=a), 'h0 and c0'),
                     (dict(B=0), 'bad sizes'), (dict(T=0), 'bad sizes'), (dict(H=0), 'bad sizes'), (dict(dtype=3), 'dtype'),
                     (dict(H=72, ldt=288, ldb=864), 'multiple of 16'), (dict(H=8, ldt=32, ldb=96), 'multiple of 16'),
                     (dict(ldt=252), 'strides'), (dict(ldt=260), 'strides'), (dict(ldb=100), 'strides'),
                     (dict(w=a + 8), '16-byte'), (dict(B=16 * 65536), 'too many rows')):
        assert fwd(**kw) == -1, kw
        assert _err(L).startswith('pk_lstm_fwd:') and word in _err(L), (kw, _err(L))


def test_lstm_bwd_argument_checks(L, a):
    def bwd(dy=a, w=a, c=a, gates=a, dg=a, B=2, T=3, H=64, dtype=BF16, scratch=a, nbytes=1 << 20):
        return L.pk_lstm_bwd(dy, w, None, c, gates, None, dg, B, T, H, dtype, scratch, nbytes, None)
    need = L.pk_lstm_bwd_scratch(2, 64, BF16)
    for kw, word in ((dict(dy=None), 'null'), (dict(w=None), 'null'), (dict(c=None), 'null'), (dict(gates=None), 'null'),
                     (dict(dg=None), 'null'), (dict(B=0), 'bad sizes'), (dict(T=-1), 'bad sizes'), (dict(dtype=9), 'dtype'),
                     (dict(H=40), 'multiple of 16'), (dict(scratch=None), 'scratch too small'),
                     (dict(nbytes=need - 1), 'scratch too small'), (dict(dg=a + 4), '16-byte')):
        assert bwd(**kw) == -1, kw
        assert _err(L).startswith('pk_lstm_bwd:') and word in _err(L), (kw, _err(L))


def test_addattn_argument_checks(L, a):
    def fwd(q=a, k=a, w=a, value=a, probs=a, ctx=a, B=2, T=3, S=5, H=64, D=128, dtype=BF16):
        return L.pk_addattn_fwd(q, k, w, None, value, probs, ctx, B, T, S, H, D, dtype, None)
    for kw, word in ((dict(q=None), 'null'), (dict(k=None), 'null'), (dict(w=None), 'null'), (dict(value=None), 'null'),
                     (dict(probs=None), 'null'), (dict(ctx=None), 'null'), (dict(B=0), 'bad sizes'), (dict(T=0), 'bad sizes'),
                     (dict(S=0), 'bad sizes'), (dict(H=0), 'bad sizes'), (dict(D=0), 'bad sizes'), (dict(dtype=-1), 'dtype'),
                     (dict(H=24), 'multiple of 16'), (dict(D=12), 'multiple of 8'), (dict(k=a + 2), '16-byte'),
                     (dict(B=70000), 'too many sentences'), (dict(S=8192, H=512), 'LDS'), (dict(S=1, H=4096 + 512), 'LDS')):
        assert fwd(**kw) == -1, kw
        assert _err(L).startswith('pk_addattn_fwd:') and word in _err(L), (kw, _err(L))

    def bwd(dctx=a, q=a, probs=a, dq=a, dk=a, dw=a, dv=a, B=2, T=3, S=5, H=64, D=128, dtype=F16, scratch=a, nbytes=1 << 20):
        return L.pk_addattn_bwd(dctx, q, a, a, a, probs, dq, dk, dw, dv, B, T, S, H, D, dtype, scratch, nbytes, None)
    need = L.pk_addattn_bwd_scratch(2, 3, 5, 64)
    for kw, word in ((dict(dctx=None), 'null'), (dict(q=None), 'null'), (dict(probs=None), 'null'), (dict(dq=None), 'null'),
                     (dict(dk=None), 'null'), (dict(dw=None), 'null'), (dict(dv=None), 'null'), (dict(S=0), 'bad sizes'),
                     (dict(dtype=4), 'dtype'), (dict(H=100), 'multiple of 16'), (dict(D=4), 'multiple of 8'),
                     (dict(scratch=None), 'scratch too small'), (dict(nbytes=need - 1), 'scratch too small'),
                     (dict(S=4096, H=1024, D=1024), 'LDS'), (dict(S=1024, H=2048, D=1024), 'LDS')):
        assert bwd(**kw) == -1, kw
        assert _err(L).startswith('pk_addattn_bwd:') and word in _err(L), (kw, _err(L))


def test_header_exports_and_bindings_agree():
    import os
    import re
    from conftest import ROOT
    from pasero_amd import lib
    header = open(os.path.join(ROOT, 'include', 'pasero_hip.h')).read()
    declared = set(re.findall(r'\b(pk_(?:lstm|addattn)_[a-z0-9_]+)\s*\(', header))
    assert declared == {n for n in lib.SIGNATURES if n.startswith(('pk_lstm_', 'pk_addattn_'))} and len(declared) == 6
    L = lib.load()
    assert all(hasattr(L, n) for n in declared)
