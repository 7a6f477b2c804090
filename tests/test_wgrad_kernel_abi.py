"""CPU-side checks of the scd_wgrad_kernel C-ABI addition: scd_wgrad_kernel_t as the host C compiler lays it out, the
exported symbol, and the entry point's host-side argument checks (no GPU touched)."""
import ctypes
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _c_layout(tmp_path, ctype: str, names):
    cc = shutil.which('gcc') or shutil.which('cc')
    if cc is None:
        pytest.skip('no host C compiler')
    lines = ['#include <stdio.h>', '#include <stddef.h>', '#include "scd.h"', 'int main(void) {',
             f'printf("size %zu\\n", sizeof({ctype}));']
    lines += [f'printf("{n} %zu\\n", offsetof({ctype}, {n}));' for n in names]
    lines += ['printf("families %d %d %d %d %d\\n", SCD_WGRAD_HALO16, SCD_WGRAD_HALO16_DMA, SCD_WGRAD_HALO16_C16, '
              'SCD_WGRAD_GENERIC_SPLIT, SCD_WGRAD_GENERIC_F32);', 'return 0;', '}']
    src = tmp_path / f'{ctype}.c'
    src.write_text('\n'.join(lines))
    exe = tmp_path / ctype
    subprocess.run([cc, '-I', os.path.join(ROOT, 'include'), str(src), '-o', str(exe)], check=True)
    out = subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.split('\n')
    rows = [ln.split() for ln in out if ln]
    return {r[0]: int(r[1]) for r in rows if len(r) == 2}, [r for r in rows if r[0] == 'families'][0][1:]


def test_wgrad_kernel_struct_layout_matches_c_compiler(tmp_path):
    from multimodal_siamese_cd_amd import hip
    names = [f[0] for f in hip.WGRADKERNEL._fields_]
    got, families = _c_layout(tmp_path, 'scd_wgrad_kernel_t', names)
    assert got['size'] == ctypes.sizeof(hip.WGRADKERNEL) == 52  # 13 int32 fields, pinned
    for n in names:
        assert got[n] == getattr(hip.WGRADKERNEL, n).offset, n
    assert families == ['0', '1', '2', '3', '4']
    assert hip.WGRAD_FAMILIES == ('halo16', 'halo16_dma', 'halo16_c16', 'generic_split', 'generic_f32')
    assert tuple(hip.WgradKernel._fields) == tuple(names)


@pytest.fixture(scope='module')
def lib():
    from multimodal_siamese_cd_amd import build, hip
    build.build_lib()
    return hip.load_library()


def test_abi_revision_is_unchanged(lib):
    from multimodal_siamese_cd_amd import hip
    assert hip.ABI_VERSION == 11 == lib.scd_abi_version()  # one symbol appended: the revision moves with the next change
    assert 'scd_wgrad_kernel' in hip.EXPORTED_SYMBOLS
    assert lib.scd_wgrad_kernel is not None


def _desc():
    from multimodal_siamese_cd_amd import hip
    nt, dy, dx = hip._taps(hip.TAPS_3X3)
    d = hip.WGRAD(hip.NHWC(0x100000, 2, 8, 16, 64, 64, hip.DT_F32), hip.NHWC(0x200000, 2, 8, 16, 64, 64, hip.DT_F32), 1,
                  nt, dy, dx)
    d.math, d.tune = hip._MATH_NAMES['x3'], 0
    return d


def test_null_arguments_are_errors_with_a_message(lib):
    from multimodal_siamese_cd_amd import hip
    k = hip.WGRADKERNEL()
    assert lib.scd_wgrad_kernel(None, ctypes.byref(k)) != 0
    assert b'scd_wgrad_kernel: null argument' in lib.scd_last_error()
    assert lib.scd_wgrad_kernel(ctypes.byref(_desc()), None) != 0
    assert b'scd_wgrad_kernel: null argument' in lib.scd_last_error()


def test_valid_descriptor_is_answered_without_gpu(lib):
    from multimodal_siamese_cd_amd import hip
    k = hip.WGRADKERNEL()
    for f, _ in hip.WGRADKERNEL._fields_:
        setattr(k, f, -7)
    assert lib.scd_wgrad_kernel(ctypes.byref(_desc()), ctypes.byref(k)) == 0
    got = hip.wgrad_kernel_of(_desc())
    assert got == hip.WgradKernel('halo16', 3, -1, 64, 64, '2x2', False, False, False, 0, 256, got.nsplit, got.kchunk)
    assert all(getattr(k, f) != -7 for f, _ in hip.WGRADKERNEL._fields_)  # every field is written
    assert got.nsplit >= 1 and (got.nsplit - 1) * got.kchunk < 2 * 8 * 16 // 32 <= got.nsplit * got.kchunk


def test_invalid_descriptor_reports_the_launch_error(lib):
    from multimodal_siamese_cd_amd import hip
    k = hip.WGRADKERNEL()
    d = _desc()
    d.math = 17
    assert lib.scd_wgrad_kernel(ctypes.byref(d), ctypes.byref(k)) != 0
    assert b'scd_conv_math' in lib.scd_last_error()
    d = _desc()
    d.src.n = 3
    assert lib.scd_wgrad_kernel(ctypes.byref(d), ctypes.byref(k)) != 0
    assert b'rows.n=2 src.n=3' in lib.scd_last_error()
