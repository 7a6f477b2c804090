"""CPU-side checks of the loss family: the criterion registry, the host-side argument validation of
scd_loss_multi_fwd (no GPU touched) and the losses_t5-11x13 fixture itself."""
import ctypes
import json
import os

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FIXTURE = os.path.join(ROOT, 'tests', 'golden', 'losses_t5-11x13.npz')
LOSS_BAR = 1e-5  # |a - b| <= LOSS_BAR * max(1, |b|)


@pytest.fixture(scope='module')
def lib():
    from multimodal_siamese_cd_amd import build, hip
    build.build_lib()
    return hip.load_library()


def test_registry_resolves_the_built_names():
    from multimodal_siamese_cd_amd.utils import loss_functions as L
    expected = {'BCEWithLogitsLoss': L.bce_with_logits_loss, 'SoftDiceSquaredSumLoss': L.soft_dice_squared_sum_loss,
                'SoftDiceBalancedLoss': L.soft_dice_loss_balanced, 'MeanSquareErrorLoss': L.mse_loss,
                'IoULoss': L.iou_loss, 'DiceLikeLoss': L.dice_like_loss, 'L2': L.mse_loss}
    for name, fn in expected.items():
        assert L.get_criterion(name) is fn, name
        assert isinstance(fn.kind, int), name
    assert L.get_criterion('PowerJaccardLoss') is L.power_jaccard_loss
    assert L.get_criterion('L2') is L.get_criterion('MeanSquareErrorLoss')
    # the reference's SoftDiceLoss and SoftDiceSquaredSumLoss are the same expression
    assert L.soft_dice_squared_sum_loss.kind == L.soft_dice_loss.kind


def test_registry_kinds_match_the_header():
    from multimodal_siamese_cd_amd import hip
    from multimodal_siamese_cd_amd.utils import loss_functions as L
    text = open(os.path.join(ROOT, 'include', 'scd.h')).read()
    for fn, name in ((L.power_jaccard_loss, 'POWER_JACCARD'), (L.soft_dice_loss, 'SOFT_DICE'),
                     (L.soft_dice_loss_balanced, 'SOFT_DICE_BALANCED'), (L.iou_loss, 'IOU'),
                     (L.dice_like_loss, 'DICE_LIKE'), (L.bce_with_logits_loss, 'BCE_LOGITS'), (L.mse_loss, 'MSE')):
        assert f'SCD_LOSS_{name} = {fn.kind},' in text, name
        assert getattr(hip, f'LOSS_{name}') == fn.kind


def test_registry_names_that_stay_off():
    from multimodal_siamese_cd_amd.utils import loss_functions as L
    for name in ('CrossEntropyLoss', 'SoftDiceLoss'):
        with pytest.raises(NotImplementedError):
            L.get_criterion(name)
    with pytest.raises(Exception, match='unknown loss'):
        L.get_criterion('Nope')


def test_abi_version(lib):
    from multimodal_siamese_cd_amd import hip
    assert lib.scd_abi_version() == 11 == hip.ABI_VERSION
    assert 'ABI 11' in hip.version()


def test_term_struct_layout_matches_c_compiler(tmp_path):
    import shutil
    import subprocess
    from multimodal_siamese_cd_amd import hip
    cc = shutil.which('gcc') or shutil.which('cc')
    if cc is None:
        pytest.skip('no host C compiler')
    names = [f[0] for f in hip.LTERM._fields_]
    lines = ['#include <stdio.h>', '#include <stddef.h>', '#include "scd.h"', 'int main(void) {',
             'printf("size %zu\\n", sizeof(scd_loss_term_t));']
    lines += [f'printf("{nm} %zu\\n", offsetof(scd_loss_term_t, {nm}));' for nm in names]
    lines += ['return 0;', '}']
    src = tmp_path / 'layout.c'
    src.write_text('\n'.join(lines))
    exe = tmp_path / 'layout'
    subprocess.run([cc, '-I', os.path.join(ROOT, 'include'), str(src), '-o', str(exe)], check=True)
    out = subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.split('\n')
    got = {a: int(b) for a, b in (ln.split() for ln in out if ln)}
    assert got['size'] == ctypes.sizeof(hip.LTERM)
    for nm in names:
        assert got[nm] == getattr(hip.LTERM, nm).offset, nm


def _fwd(lib, terms, n_terms):
    """scd_loss_multi_fwd with every other argument plausible; validation fails before any pointer is used."""
    from multimodal_siamese_cd_amd import hip
    arr = (hip.LTERM * max(len(terms), 1))(*terms)
    buf = ctypes.create_string_buffer(64)
    p = ctypes.cast(buf, ctypes.c_void_p)
    return lib.scd_loss_multi_fwd(ctypes.cast(arr, ctypes.c_void_p), n_terms, p, 1, 4, p, p, p, 1 << 20, None)


def test_host_side_validation_without_gpu(lib):
    from multimodal_siamese_cd_amd import hip
    buf = ctypes.create_string_buffer(64)
    p = ctypes.cast(buf, ctypes.c_void_p).value
    ok = lambda **kw: hip.LTERM(**{**dict(logits=p, target=p, coef=1.0, kind=hip.LOSS_IOU), **kw})
    cases = {
        'no terms': ([ok()], 0),
        'five terms': ([ok()] * 5, 5),
        'kind out of range': ([ok(kind=7)], 1),
        'negative kind': ([ok(kind=-1)], 1),
        'gtarget on a hard target': ([ok(gtarget=p, soft_target=0)], 1),
        'sigmoid input outside MSE': ([ok(sigmoid_input=1)], 1),
        'null logits': ([ok(logits=None)], 1),
    }
    for what, (terms, n) in cases.items():
        assert _fwd(lib, terms, n) == -1, what
        assert b'loss_multi_fwd' in lib.scd_last_error(), what
    # a subset without a labelled mask
    arr = (hip.LTERM * 1)(ok(select=1))
    rc = lib.scd_loss_multi_fwd(ctypes.cast(arr, ctypes.c_void_p), 1, None, 1, 4, p, p, p, 1 << 20, None)
    assert rc == -1 and b'loss_multi_fwd' in lib.scd_last_error()
    # the other two entry points validate the same way
    arr = (hip.LTERM * 1)(ok(kind=9))
    assert lib.scd_loss_multi_bwd(ctypes.cast(arr, ctypes.c_void_p), 1, p, 1, 4, p, None, None) == -1
    assert b'loss_multi_bwd' in lib.scd_last_error()
    assert lib.scd_loss_multi_loss_from_sums(ctypes.cast(arr, ctypes.c_void_p), 1, 4, p, p, None) == -1
    assert b'loss_multi_loss_from_sums' in lib.scd_last_error()


def test_fixture_loads_and_its_two_precisions_agree():
    z = np.load(FIXTURE, allow_pickle=False)
    meta = json.loads(str(z['meta']))
    assert tuple(meta['shape']) == (5, 1, 11, 13) == z['x'].shape == z['z'].shape == z['t'].shape
    assert z['is_labeled'].tolist() == [1, 0, 1, 1, 0]
    assert sorted(np.unique(z['t']).tolist()) == [0.0, 1.0] and 0.1 < z['t'].mean() < 0.3
    for v in meta['extremes']:
        assert (z['x'] == v).any(), v
    keys = [f'{k}/{f}' for k in meta['kinds'] for f in ('hard', 'soft')] + ['l2cons']
    keys += [f'mmcr/{c}/{m}' for c in ('bce_l2', 'dicelike_pj') for m in ('mixed', 'all', 'none')]
    assert len(meta['kinds']) == 7
    for key in keys:
        l64, l32 = float(z[key + '/loss64']), float(z[key + '/loss32'])
        assert z[key + '/loss64'].dtype == np.float64
        assert np.isfinite(l64) and abs(l32 - l64) <= LOSS_BAR * max(1.0, abs(l64)), key
    assert os.path.getsize(FIXTURE) < 150 * 1024
