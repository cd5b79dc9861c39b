"""CPU tests of the adapter entry points of the C ABI (csrc/adapter.hip, csrc/decode.hip): which way a call goes, the
scratch it asks for, the argument checks that come before any launch, and the `_ex` decoding step's scratch."""
import ctypes
import os
import subprocess

import pytest

from conftest import ROOT

F32, BF16, F16 = 0, 1, 2


@pytest.fixture(scope='module')
def L():
    if os.environ.get('PK_ADAPTER_FUSED', '1') in ('0',):
        pytest.fail('PK_ADAPTER_FUSED=0 is set: the documented answers below are those of the default library')
    from pasero_amd import lib
    return lib.load()


@pytest.mark.parametrize('rows', [1, 40, 160])
def test_fused_range_and_scratch(L, rows):
    for dt in (BF16, F16):
        assert L.pk_adapter_rows_fused(rows, 1024, 64, dt) == 1
        assert L.pk_adapter_rows_scratch(rows, 1024, 64, dt) == 0
        for d, p in ((128, 8), (2048, 72), (64, 512), (1024, 512), (2048, 224)):
            assert L.pk_adapter_rows_fused(rows, d, p, dt) == 1, (d, p)
            assert L.pk_adapter_rows_scratch(rows, d, p, dt) == 0
        # p not a multiple of 8, p out of range, d not a multiple of 64, d too wide, a tile beyond 160 KiB of LDS
        for d, p in ((1024, 12), (1024, 4), (1024, 520), (1000, 64), (96, 8), (4096, 64), (2048, 232), (2048, 512)):
            assert L.pk_adapter_rows_fused(rows, d, p, dt) == 0, (d, p)
            need = L.pk_adapter_rows_scratch(rows, d, p, dt)
            assert need >= 2 * rows * (d + p), (d, p)  # LN(x) and the bottleneck activations at least
    assert L.pk_adapter_rows_fused(rows, 1024, 64, F32) == 0
    assert L.pk_adapter_rows_scratch(rows, 1024, 64, F32) >= 4 * rows * (1024 + 64)
    assert L.pk_adapter_rows_scratch(0, 1024, 12, BF16) == 0


def test_argument_checks_come_before_any_launch(L):
    """every call below must fail on the host: there is no GPU here, and the pointers are not device memory"""
    buf = ctypes.create_string_buffer(1 << 16)
    a = ctypes.addressof(buf)
    x, y, wd, wu = a, a + 16384, a + 32768, a + 49152

    def call(x=x, y=y, wd=wd, wu=wu, rows=4, d=128, p=8, act=1, dtype=BF16, scratch=None, nbytes=0):
        return L.pk_adapter_rows(x, y, None, None, wd, None, wu, None, rows, d, p, act, 1.0, 1e-5, dtype, scratch, nbytes, None)

    for kw, word in ((dict(wd=None), 'null'), (dict(wu=None), 'null'), (dict(x=None), 'null'), (dict(y=None), 'null'),
                     (dict(rows=-1), 'bad sizes'), (dict(p=0), 'bad sizes'), (dict(dtype=7), 'dtype'), (dict(act=9), 'activation'),
                     (dict(y=x + 64), 'overlap'),
                     (dict(dtype=F32), 'scratch too small'), (dict(p=12), 'scratch too small'),
                     (dict(p=12, scratch=a, nbytes=L.pk_adapter_rows_scratch(4, 128, 12, BF16) - 1), 'scratch too small'),
                     (dict(x=x + 2, y=y + 2), '16-byte aligned')):
        assert call(**kw) == -1, kw
        msg = L.pk_last_error().decode()
        assert msg.startswith('pk_adapter_rows:') and word in msg, (kw, msg)
    assert call(rows=0) == 0                 # nothing to do: no launch either
    assert call(rows=0, dtype=F32) == 0


def test_step_scratch_ex(L):
    from pasero_amd.decode import PkAdapterStack, PkDecoderLayerWeights, PkDecoderPlan
    n = 3
    layers = (PkDecoderLayerWeights * n)()
    stacks = (PkAdapterStack * n)()
    for dtype in (BF16, F32):
        plan = PkDecoderPlan()
        plan.n_layers, plan.d, plan.heads, plan.ffn, plan.dtype, plan.vocab = n, 1024, 16, 4096, dtype, 1000
        plan.layers = ctypes.cast(layers, ctypes.POINTER(PkDecoderLayerWeights))
        for B in (1, 5, 40):
            base = L.pk_decoder_step_scratch(ctypes.byref(plan), B)
            assert base > 0 and L.pk_decoder_step_scratch_ex(ctypes.byref(plan), B, None) == base
            for s in stacks:
                s.n = 0
            assert L.pk_decoder_step_scratch_ex(ctypes.byref(plan), B, stacks) == base  # no adapters anywhere
            stacks[1].n = 2
            stacks[1].a[0].p, stacks[1].a[1].p = 64, 12
            extra = L.pk_decoder_step_scratch_ex(ctypes.byref(plan), B, stacks) - base
            es = 4 if dtype == F32 else 2
            # the three-launch need of the largest adapter (LN(x), the bottleneck, the scaled bias, the statistics), whichever
            # route the step takes: pk_adapter_step_fused may change between two steps
            assert es * (B * (1024 + 64) + 1024) + 8 * B <= extra <= es * (B * (1024 + 64) + 1024) + 8 * B + 5 * 256
            assert L.pk_adapter_rows_scratch(B, 1024, 12, dtype) <= extra


def test_step_route_switch(L):
    prev = L.pk_adapter_step_fused(-1)
    assert prev == 0  # the default, by measurement: the three launches
    assert L.pk_adapter_step_fused(1) == 0 and L.pk_adapter_step_fused(-1) == 1
    assert L.pk_adapter_step_fused(prev) == 1 and L.pk_adapter_step_fused(-1) == prev


def test_adapter_structs_have_the_layout_of_the_header(tmp_path):
    from pasero_amd import decode
    mirrors = {'PkAdapter': decode.PkAdapter, 'PkAdapterStack': decode.PkAdapterStack}
    lines = ['printf("max %d\\n", PK_ADAPTER_STACK_MAX);']
    for name, cls in mirrors.items():
        lines.append(f'printf("{name} %zu\\n", sizeof({name}));')
        lines += [f'printf("{name}.{f} %zu\\n", offsetof({name}, {f}));' for f, _ in cls._fields_]
    src = tmp_path / 'layout.c'
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "pasero_hip.h"\nint main(void) {\n' + '\n'.join(lines) + '\nreturn 0; }\n')
    exe = tmp_path / 'layout'
    subprocess.run(['gcc', '-I', os.path.join(ROOT, 'include'), str(src), '-o', str(exe)], check=True)
    got = dict(line.split() for line in subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.splitlines())
    assert int(got['max']) == decode.PK_ADAPTER_STACK_MAX
    for name, cls in mirrors.items():
        assert int(got[name]) == ctypes.sizeof(cls)
        for f, _ in cls._fields_:
            assert int(got[f'{name}.{f}']) == getattr(cls, f).offset, (name, f)
