"""CPU-side checks of scd_bn_relu_through, the reduction-free backward through a frozen BatchNorm + ReLU: the symbol is
declared and bound, the ABI revision and the descriptor's layout did not move, and every refusal is made on the host
(no GPU touched) with `through:` in scd_last_error()."""
import ctypes
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SIZEOF_BN_BWD_T = 376  # scd_bn_bwd_t as scd_bn_relu_backward_desc shipped it (x86-64 / LP64)


def test_header_declares_and_binding_exports():
    from multimodal_siamese_cd_amd import hip
    header = open(os.path.join(ROOT, 'include', 'scd.h')).read()
    assert re.search(r'^int scd_bn_relu_through\(const scd_bn_bwd_t \*d, scd_stream_t stream\);', header, re.M)
    assert re.search(r'^#define SCD_ABI_VERSION 11$', header, re.M)
    assert 'networks.py:393-394,396-397' in header[header.index('scd_bn_relu_backward_desc(const'):]
    assert 'scd_bn_relu_through' in hip.EXPORTED_SYMBOLS
    assert hip.EXPORTED_SYMBOLS[-1] == 'scd_bn_relu_through'  # appended
    assert callable(hip.bn_relu_through)


def test_descriptor_size_unchanged(tmp_path):
    from multimodal_siamese_cd_amd import hip
    assert ctypes.sizeof(hip.BNBWDDESC) == SIZEOF_BN_BWD_T
    cc = shutil.which('gcc') or shutil.which('cc')
    if cc is None:
        pytest.skip('no host C compiler')
    src = tmp_path / 'size.c'
    src.write_text('#include <stdio.h>\n#include "scd.h"\n'
                   'int main(void) { printf("%zu\\n", sizeof(scd_bn_bwd_t)); return 0; }\n')
    exe = tmp_path / 'size'
    subprocess.run([cc, '-I', os.path.join(ROOT, 'include'), str(src), '-o', str(exe)], check=True)
    assert int(subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout) == SIZEOF_BN_BWD_T


def _lib():
    from multimodal_siamese_cd_amd import build, hip
    build.build_lib()
    return hip, hip.load_library()


def test_abi_version_stays():
    hip, lib = _lib()
    assert hip.ABI_VERSION == 11 == lib.scd_abi_version()


def _valid(hip):
    """A descriptor that passes every check before `y.data` (host memory is never dereferenced by the checks)."""
    keep = ctypes.create_string_buffer(64)
    d = hip.BNBWDDESC()
    d.form, d.flags, d.nseg = hip.BN_BWD_PLAIN, hip.BN_BWD_FROZEN, 1
    d._keep = keep
    return d, ctypes.addressof(keep)


@pytest.mark.parametrize('case', ['tiles', 'coef', 'unknown form', 'dgamma', 'w_grad', 'null y'])
def test_host_refusals(case):
    hip, lib = _lib()
    d, ptr = _valid(hip)
    if case == 'tiles':
        d.form = hip.BN_BWD_TILES
    elif case == 'coef':
        d.form = hip.BN_BWD_COEF
    elif case == 'unknown form':
        d.form = 17
    elif case == 'dgamma':
        d.dgamma = ptr
    elif case == 'w_grad':
        d.form, d.w_grad = hip.BN_BWD_HEAD, ptr
    assert lib.scd_bn_relu_through(ctypes.byref(d), None) == -1
    err = lib.scd_last_error()
    print(case, err)
    assert b'through:' in err
    want = {'tiles': b'SCD_BN_BWD_TILES', 'coef': b'SCD_BN_BWD_COEF', 'unknown form': b'unknown form 17',
            'dgamma': b'must be null', 'w_grad': b'must be null', 'null y': b'null y.data'}[case]
    assert want in err


def test_null_descriptor_and_unknown_flags():
    hip, lib = _lib()
    assert lib.scd_bn_relu_through(None, None) == -1 and b'through: null descriptor' in lib.scd_last_error()
    d, _ = _valid(hip)
    d.flags = 2
    assert lib.scd_bn_relu_through(ctypes.byref(d), None) == -1 and b'through: unknown flags' in lib.scd_last_error()
