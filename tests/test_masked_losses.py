"""CPU-side checks of the per-pixel validity mask: the masked symbols are declared, bound and exported at ABI 11 with
scd_loss_term_t unmoved, every host-side refusal is made without touching a GPU, the masked_losses_t5-11x13 fixture
loads, and every registered criterion takes `valid=`."""
import ctypes
import inspect
import json
import os
import re

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FIXTURE = os.path.join(ROOT, 'tests', 'golden', 'masked_losses_t5-11x13.npz')
LOSS_BAR = 1e-5  # |a - b| <= LOSS_BAR * max(1, |b|)
SYMBOLS = ('scd_loss_masked_workspace_bytes', 'scd_loss_masked_fwd', 'scd_loss_masked_loss_from_sums',
           'scd_loss_masked_bwd', 'scd_threshold_counts_masked_workspace_bytes', 'scd_threshold_counts_masked')


@pytest.fixture(scope='module')
def lib():
    from multimodal_siamese_cd_amd import build, hip
    build.build_lib()
    return hip.load_library()


def test_symbols_declared_bound_and_exported(lib):
    from multimodal_siamese_cd_amd import hip
    text = open(os.path.join(ROOT, 'include', 'scd.h')).read()
    for s in SYMBOLS:
        assert re.search(r'^\w+ ' + s + r'\(', text, flags=re.M), s
        assert s in hip.EXPORTED_SYMBOLS, s
        assert hasattr(lib, s), s
    # appended in front of the pinned tail, which keeps its place
    assert hip.EXPORTED_SYMBOLS[-5:] == ('scd_bn_stats_local', 'scd_bn_stats_from_ranks', 'scd_bn_relu_backward_sums',
                                         'scd_bn_relu_backward_from_sums', 'scd_bn_relu_through')
    assert lib.scd_abi_version() == 11 == hip.ABI_VERSION
    assert ctypes.sizeof(hip.LTERM) == 56  # scd_loss_term_t: four pointers, a float and five int32
    assert hip.LOSS_ROW == 8


def test_workspace_queries(lib):
    # the float records of the unmasked call, then one 8-byte count per record
    for n in (1, 2, 4):
        assert lib.scd_loss_masked_workspace_bytes(n) == lib.scd_loss_multi_workspace_bytes(n) * 3 // 2
    assert lib.scd_threshold_counts_masked_workspace_bytes(1 << 20, 3) == \
        lib.scd_threshold_counts_workspace_bytes(1 << 20, 3) // 7 * 8
    assert lib.scd_threshold_counts_masked_workspace_bytes(100, 0) == 0
    assert lib.scd_threshold_counts_masked_workspace_bytes(100, 17) == 0


def test_loss_refusals_without_gpu(lib):
    from multimodal_siamese_cd_amd import hip
    buf = ctypes.create_string_buffer(64)
    p = ctypes.cast(buf, ctypes.c_void_p).value
    ok = lambda **kw: hip.LTERM(**{**dict(logits=p, target=p, coef=1.0, kind=hip.LOSS_IOU), **kw})
    masks = (ctypes.c_void_p * 4)(p, None, p, None)
    mp = ctypes.cast(masks, ctypes.c_void_p)

    def fwd(terms, n_terms, labeled=p, valid=mp, counts=p):
        arr = (hip.LTERM * max(len(terms), 1))(*terms)
        return lib.scd_loss_masked_fwd(ctypes.cast(arr, ctypes.c_void_p), n_terms, labeled, valid, 1, 4, p, counts, p,
                                       p, 1 << 20, None)

    def bwd(terms, n_terms, labeled=p, valid=mp):
        arr = (hip.LTERM * max(len(terms), 1))(*terms)
        return lib.scd_loss_masked_bwd(ctypes.cast(arr, ctypes.c_void_p), n_terms, labeled, valid, 1, 4, p, None, None)

    def from_sums(terms, n_terms, counts=p):
        arr = (hip.LTERM * max(len(terms), 1))(*terms)
        return lib.scd_loss_masked_loss_from_sums(ctypes.cast(arr, ctypes.c_void_p), n_terms, p, counts, p, None)

    cases = {
        'null counts': (dict(terms=[ok()], n_terms=1, counts=None), b'null counts'),
        'gtarget without a soft target': (dict(terms=[ok(gtarget=p, soft_target=0)], n_terms=1), b'gtarget'),
        'select without labeled': (dict(terms=[ok(select=1)], n_terms=1, labeled=None), b'labeled'),
        'null valid array': (dict(terms=[ok()], n_terms=1, valid=None), b'valid'),
        'no terms': (dict(terms=[ok()], n_terms=0), b'terms'),
        'five terms': (dict(terms=[ok()] * 5, n_terms=5), b'terms'),
        'kind out of range': (dict(terms=[ok(kind=7)], n_terms=1), b'kind'),
    }
    for what, (kw, word) in cases.items():
        assert fwd(**kw) == -1, what
        err = lib.scd_last_error()
        assert b'loss_masked_fwd' in err and word in err, (what, err)
    # the backward validates the same way
    for what, (kw, word) in cases.items():
        if 'counts' in kw:
            continue
        assert bwd(**kw) == -1, what
        err = lib.scd_last_error()
        assert b'loss_masked_bwd' in err and word in err, (what, err)
    assert from_sums([ok()], 1, counts=None) == -1 and b'null counts' in lib.scd_last_error()
    assert from_sums([ok(gtarget=p)], 1) == -1 and b'loss_masked_loss_from_sums' in lib.scd_last_error()
    assert from_sums([ok(kind=9)], 1) == -1 and b'loss_masked_loss_from_sums' in lib.scd_last_error()


def test_threshold_counts_refusals_without_gpu(lib):
    buf = ctypes.create_string_buffer(256)
    base = ctypes.cast(buf, ctypes.c_void_p).value
    p = (base + 15) & ~15

    def call(pred=p, truth=p, valid=p, n=4, thr=p, n_thr=3, counts=p, ws=p, ws_bytes=1 << 20):
        return lib.scd_threshold_counts_masked(pred, truth, valid, n, thr, n_thr, 0, counts, ws, ws_bytes, None)

    for what, kw, word in (('n_thr 0', dict(n_thr=0), b'n_thr'), ('n_thr 17', dict(n_thr=17), b'n_thr'),
                           ('null counts', dict(counts=None), b'null counts'),
                           ('null valid', dict(valid=None), b'valid'), ('null pred', dict(pred=None), b'pred'),
                           ('n 0', dict(n=0), b'n < 1')):
        assert call(**kw) == -1, what
        err = lib.scd_last_error()
        assert b'threshold_counts_masked' in err and word in err, (what, err)
    assert call(pred=p + 4) == -2 and b'16-byte' in lib.scd_last_error()
    assert call(ws_bytes=8) == -5 and b'workspace' in lib.scd_last_error()


def test_python_wrappers_refuse_bad_masks(lib):
    import torch
    from multimodal_siamese_cd_amd import engine
    x = torch.zeros(2, 1, 4, 4)
    with pytest.raises(TypeError, match='bool or uint8'):
        engine._term_masks(torch.zeros(2, 1, 4, 4), 1, x)
    with pytest.raises(ValueError, match='elements'):
        engine._term_masks(torch.zeros(2, 1, 4, 3, dtype=torch.bool), 1, x)
    with pytest.raises(ValueError, match='masks for'):
        engine._term_masks([None], 2, x)
    assert engine._term_masks(None, 3, x) is None and engine._term_masks([None, None], 2, x) is None
    v = torch.ones(2, 1, 4, 4, dtype=torch.bool)
    a, b, c = engine._term_masks([v, None, v], 3, x)
    assert a is c and b is None and a.dtype == torch.uint8 and a.data_ptr() == v.data_ptr()


def test_fixture_loads_and_its_two_precisions_agree():
    z = np.load(FIXTURE, allow_pickle=False)
    meta = json.loads(str(z['meta']))
    assert tuple(meta['shape']) == (5, 1, 11, 13) == z['x'].shape == z['valid'].shape
    base = np.load(os.path.join(ROOT, 'tests', 'golden', 'losses_t5-11x13.npz'), allow_pickle=False)
    for k in ('x', 'z', 'f', 't', 'is_labeled'):  # exactly the inputs of the unmasked fixture
        assert np.array_equal(z[k], base[k]), k
    v = z['valid']
    assert v.dtype == np.uint8 and int(v.sum()) == 449
    assert v.reshape(5, -1).sum(1).tolist() == [103, 0, 105, 143, 98] == meta['valid_per_sample']
    keys = [f'{k}/{f}' for k in meta['kinds'] for f in ('hard', 'soft')]
    keys += [f'mmcr/{c}/{m}' for c in ('bce_l2', 'dicelike_pj') for m in ('mixed', 'all')]
    assert len(meta['kinds']) == 7 and len(keys) == 18
    for key in keys:
        l64, l32 = float(z[key + '/loss64']), float(z[key + '/loss32'])
        assert z[key + '/loss64'].dtype == np.float64
        assert np.isfinite(l64) and abs(l32 - l64) <= LOSS_BAR * max(1.0, abs(l64)), key
        for g in ('gx', 'gz', 'gf', 'gs1', 'gs2'):
            if f'{key}/{g}' in z.files:
                a = z[f'{key}/{g}']
                assert a.shape == v.shape and np.isfinite(a).all() and not a[v == 0].any(), (key, g)
    assert np.abs(z['bce/hard/gx']).max() > 0 and np.abs(z['mmcr/bce_l2/mixed/gs2']).max() > 0
    assert os.path.getsize(FIXTURE) < 150 * 1024


def test_every_registered_criterion_accepts_valid():
    from multimodal_siamese_cd_amd.utils import loss_functions as L
    for name, fn in L._REGISTRY.items():
        params = list(inspect.signature(fn).parameters.values())
        assert [q.name for q in params][2:] == ['valid'], name
        assert params[2].default is None, name
        assert all(q.default is inspect.Parameter.empty for q in params[:2]), name  # the reference's positional pair


def test_masked_criterion_refuses_cpu_tensors(lib):
    import torch
    from multimodal_siamese_cd_amd.utils import loss_functions as L
    x = torch.zeros(1, 1, 4, 4)
    for name, fn in L._REGISTRY.items():
        with pytest.raises(RuntimeError, match='MI355X'):
            fn(x, x, valid=torch.ones(1, 1, 4, 4, dtype=torch.bool))
