"""CPU-side checks of the frozen-BatchNorm C-ABI additions: scd_bn_bwd_t as the host C compiler lays it out, and the
descriptor entry point's host-side argument checks (no GPU touched)."""
import ctypes
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_bn_bwd_descriptor_layout_matches_c_compiler(tmp_path):
    from multimodal_siamese_cd_amd import hip
    cc = shutil.which('gcc') or shutil.which('cc')
    if cc is None:
        pytest.skip('no host C compiler')
    names = [f[0] for f in hip.BNBWDDESC._fields_]
    lines = ['#include <stdio.h>', '#include <stddef.h>', '#include "scd.h"', 'int main(void) {',
             'printf("size %zu\\n", sizeof(scd_bn_bwd_t));']
    lines += [f'printf("{n} %zu\\n", offsetof(scd_bn_bwd_t, {n}));' for n in names]
    lines += ['return 0;', '}']
    src = tmp_path / 'layout.c'
    src.write_text('\n'.join(lines))
    exe = tmp_path / 'layout'
    subprocess.run([cc, '-I', os.path.join(ROOT, 'include'), str(src), '-o', str(exe)], check=True)
    out = subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.split('\n')
    got = {a: int(b) for a, b in (ln.split() for ln in out if ln)}
    assert got['size'] == ctypes.sizeof(hip.BNBWDDESC)
    for n in names:
        assert got[n] == getattr(hip.BNBWDDESC, n).offset, n


def test_descriptor_argument_checks_without_gpu():
    from multimodal_siamese_cd_amd import build, hip
    build.build_lib()
    lib = hip.load_library()
    assert hip.ABI_VERSION == 11 == lib.scd_abi_version()  # symbols appended: the revision moves with the next change
    d = hip.BNBWDDESC()
    d.form = 17
    assert lib.scd_bn_relu_backward_desc(d, None) == -1 and b'unknown form' in lib.scd_last_error()
    d.form, d.flags = hip.BN_BWD_PLAIN, 2
    assert lib.scd_bn_relu_backward_desc(d, None) == -1 and b'unknown flags' in lib.scd_last_error()
    d.form, d.flags, d.skip_mode = hip.BN_BWD_POOLED, hip.BN_BWD_FROZEN, 2
    assert lib.scd_bn_relu_backward_desc(d, None) == -1 and b'SCD_BN_BWD_POOLED2' in lib.scd_last_error()
    d.form, d.skip_mode = hip.BN_BWD_PLAIN, 0
    assert lib.scd_bn_relu_backward_desc(d, None) == -1 and b'null data' in lib.scd_last_error()
    assert lib.scd_bn_frozen_coeffs(0, 1, None, None, None, None, 1e-5, None, None, None, None, None) == -1
    assert b'bn_frozen_coeffs' in lib.scd_last_error()
