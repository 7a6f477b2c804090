"""CPU-side checks of the input-gradient C-ABI additions: scd_input_grad_t / scd_input_grad_dst_t as the host C
compiler lays them out, and the entry point's host-side argument checks (no GPU touched)."""
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
    lines += ['return 0;', '}']
    src = tmp_path / f'{ctype}.c'
    src.write_text('\n'.join(lines))
    exe = tmp_path / ctype
    subprocess.run([cc, '-I', os.path.join(ROOT, 'include'), str(src), '-o', str(exe)], check=True)
    out = subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.split('\n')
    return {a: int(b) for a, b in (ln.split() for ln in out if ln)}


@pytest.mark.parametrize('ctype,struct', [('scd_input_grad_t', 'INPUTGRAD'), ('scd_input_grad_dst_t', 'INPUTGRADDST')])
def test_input_grad_descriptor_layout_matches_c_compiler(tmp_path, ctype, struct):
    from multimodal_siamese_cd_amd import hip
    st = getattr(hip, struct)
    names = [f[0] for f in st._fields_]
    got = _c_layout(tmp_path, ctype, names)
    assert got['size'] == ctypes.sizeof(st)
    for n in names:
        assert got[n] == getattr(st, n).offset, n


@pytest.fixture(scope='module')
def lib():
    from multimodal_siamese_cd_amd import build, hip
    build.build_lib()
    return hip.load_library()


def _desc(c0=8, cin=5, n=4, h=6, w=7):
    """A valid descriptor over made-up (aligned, never dereferenced) addresses: pair mode, two images each."""
    from multimodal_siamese_cd_amd import hip
    d = hip.INPUTGRAD()
    d.dy = hip.NHWC(0x10000, n, h, w, c0, c0, hip.DT_F32)
    d.w, d.cin = 0x20000, cin
    for i, r in enumerate(d.dst):
        r.dst, r.dst_c, r.c_begin, r.c_count, r.w_c, r.n_begin, r.n_count = 0x30000 + 0x10000 * i, cin, 0, cin, 0, \
            i * (n // 2), n // 2
    return d


def test_abi_revision_is_unchanged(lib):
    from multimodal_siamese_cd_amd import hip
    assert hip.ABI_VERSION == 11 == lib.scd_abi_version()  # symbols appended: the revision moves with the next change
    assert {'scd_input_grad', 'scd_input_grad_supported'} <= set(hip.EXPORTED_SYMBOLS)


def test_valid_descriptor_is_supported_without_gpu(lib):
    for c0, cin in ((8, 1), (64, 5), (128, 16), (72, 10)):
        assert lib.scd_input_grad_supported(_desc(c0=c0, cin=cin)) == 1, (c0, cin)
    d = _desc()
    d.dst[0].dst = None  # one null record is skipped
    assert lib.scd_input_grad_supported(d) == 1
    d = _desc()
    d.dy.dtype = 1  # bf16 storage
    assert lib.scd_input_grad_supported(d) == 1


def _rejected(lib, d):
    assert lib.scd_input_grad_supported(d) == 0
    rc = lib.scd_input_grad(d, None)  # refused on the host, before any device call
    msg = lib.scd_last_error()
    assert b'input_grad' in msg, msg
    return rc, msg


def test_argument_checks_without_gpu(lib):
    d = _desc()
    d.dy.data = None
    assert _rejected(lib, d)[0] == -1
    assert _rejected(lib, _desc(cin=17))[0] == -1
    assert _rejected(lib, _desc(cin=0))[0] == -1
    assert _rejected(lib, _desc(c0=12))[0] == -1
    d = _desc()
    d.dst[1].c_begin, d.dst[1].c_count, d.dst[1].dst_c = 3, 3, 5  # c_begin + c_count > dst_c
    rc, msg = _rejected(lib, d)
    assert rc == -1 and b'dst_c' in msg
    d = _desc()
    d.dst[1].n_begin, d.dst[1].n_count = 3, 2  # images [3, 5) of 4
    rc, msg = _rejected(lib, d)
    assert rc == -1 and b'dy.n' in msg
    d = _desc()
    d.dst[0].w_c = 1  # weight channels [1, 6) of cin 5
    assert _rejected(lib, d)[0] == -1
    d = _desc()
    d.w = None
    assert _rejected(lib, d)[0] == -1
    d = _desc()
    d.dst[0].dst = d.dst[1].dst = None
    assert _rejected(lib, d)[0] == -1
    d = _desc()
    d.dy.dtype = 7
    assert _rejected(lib, d)[0] == -1
    d = _desc()
    d.dy.data = 0x10004  # not 16-byte aligned
    assert _rejected(lib, d)[0] == -2
    d = _desc()
    d.dst[0].dst = 0x30002
    assert _rejected(lib, d)[0] == -2
    assert lib.scd_input_grad(None, None) == -1 and b'input_grad' in lib.scd_last_error()
