"""DATALOADER.INCLUDE_MASKED on the CPU side: absent, the tile-cache dataset and the cache tool are today's (same
files, same item keys, same arrays, same RNG consumption); set, a labelled AOI's masked timestamps become selectable
and the item carries valid = ~(mask_t1 | mask_t2)."""
import filecmp
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, 'tools'))
import make_tile_cache  # noqa: E402

ITEM_KEYS = ['imgs', 'buildings', 'change', 'aug', 'aoi_id', 'year_t1', 'month_t1', 'year_t2', 'month_t2',
             'is_labeled']


def _cfg(root, aois, **aug):
    from multimodal_siamese_cd_amd.utils import experiment_manager as em
    cfg = em.load_cfg('baseline_siamese')
    cfg.PATHS.DATASET = str(root)
    cfg.DATASET.TRAINING_IDS = aois[:2]
    cfg.DATASET.VALIDATION_IDS = aois[2:]
    cfg.DATASET.UNLABELED_IDS = aois[2:]
    cfg.DATALOADER.TRAINING_MULTIPLIER = 2
    cfg.DATALOADER.S2_BANDS = [2, 1, 0]
    cfg.AUGMENTATION.CROP_SIZE = 64
    for k, v in aug.items():
        cfg.AUGMENTATION[k] = v
    return cfg


@pytest.fixture(scope='module')
def caches(tmp_path_factory):
    plain, masked = tmp_path_factory.mktemp('tiles'), tmp_path_factory.mktemp('tiles_masks')
    aois = make_tile_cache.make(str(plain), aois=3, size=(100, 90), months=4)
    assert make_tile_cache.make(str(masked), aois=3, size=(100, 90), months=4, masks=True) == aois
    return plain, masked, aois


def _files(root):
    return sorted(os.path.relpath(os.path.join(d, f), root) for d, _, fs in os.walk(root) for f in fs)


def test_tool_default_output_is_unchanged_and_masks_are_opt_in(caches):
    plain, masked, aois = caches
    assert not [f for f in _files(plain) if 'masks' in f]
    extra = [f for f in _files(masked) if f not in _files(plain)]
    assert extra == [os.path.join(aois[0], 'masks', f'masks_{aois[0]}_2018_02.npy')]  # the one masked timestamp
    for f in _files(plain):  # everything else byte for byte, the metadata included
        assert filecmp.cmp(plain / f, masked / f, shallow=False), f
    m = np.load(masked / extra[0])
    assert m.dtype == np.uint8 and m.shape == (100, 90) and 0.1 < (m != 0).mean() < 0.5


def _same_item(a, b):
    assert list(a) == list(b)
    for k in a:
        if k == 'aug':
            assert vars(a[k]).keys() == vars(b[k]).keys()
            for f, u in vars(a[k]).items():
                w = vars(b[k])[f]
                if isinstance(u, tuple):
                    assert all(np.array_equal(p, q) for p, q in zip(u, w)), f
                else:
                    assert u == w, f
        elif isinstance(a[k], np.ndarray):
            assert a[k].dtype == b[k].dtype and np.array_equal(a[k], b[k]), k
        else:
            assert a[k] == b[k], k


@pytest.mark.parametrize('aug', [dict(), dict(COLOR_SHIFT=True, GAMMA_CORRECTION=True)])
def test_absent_key_is_todays_dataset(caches, aug):
    """No INCLUDE_MASKED key: the item keys are exactly today's, mask files on disk are not even looked at, and the
    items and the RandomState afterwards equal those of an explicit False."""
    from multimodal_siamese_cd_amd.utils import datasets
    plain, masked, aois = caches
    cfg = _cfg(plain, aois, **aug)
    assert 'INCLUDE_MASKED' not in cfg.DATALOADER
    cfg.DATALOADER.INCLUDE_UNLABELED = True
    off = _cfg(masked, aois, **aug)
    off.DATALOADER.INCLUDE_UNLABELED = True
    off.DATALOADER.INCLUDE_MASKED = False
    r1, r2 = np.random.RandomState(5), np.random.RandomState(5)
    d1 = datasets.MultimodalCDDataset(cfg, 'training', rng=r1)
    d2 = datasets.MultimodalCDDataset(off, 'training', rng=r2)
    assert not d1.include_masked and not d2.include_masked
    for i in range(len(d1)):
        a, b = d1[i], d2[i]
        assert list(a) == ITEM_KEYS
        _same_item(a, b)
        # the labelled AOI with a masked month never selects it
        if a['aoi_id'] == aois[0]:
            assert 2 not in (a['month_t1'], a['month_t2'])
    assert r1.get_state()[1].tolist() == r2.get_state()[1].tolist() and r1.get_state()[2] == r2.get_state()[2]
    # and the draws are the reference stream's: randint(0, 3) for the AOI with 3 unmasked months of 4
    first = datasets.MultimodalCDDataset(cfg, 'training', rng=np.random.RandomState(5))[0]
    i0, i1 = sorted(np.random.RandomState(5).randint(0, 3, size=2))
    months = [1, 3, 4]
    assert (first['month_t1'], first['month_t2']) == (months[i0], months[i1])


class _Pick:
    """A stand-in for the RandomState: the timestamp draw returns what it is told, and records its bounds."""

    def __init__(self, picks):
        self.picks, self.bounds = picks, []

    def randint(self, lo, hi, size=None):
        self.bounds.append((lo, hi))
        return np.array(self.picks)


def test_masked_timestamps_become_selectable_and_valid_is_not_m1_or_m2(caches):
    from multimodal_siamese_cd_amd.utils import datasets
    _, masked, aois = caches
    cfg = _cfg(masked, aois)
    cfg.DATALOADER.INCLUDE_MASKED = True
    rng = _Pick([1, 3])
    ds = datasets.MultimodalCDDataset(cfg, 'training', no_augmentations=True, rng=rng)
    it = ds[0]
    assert rng.bounds == [(0, 4)]  # all four months of AOI 0; three without the key
    assert (it['month_t1'], it['month_t2']) == (2, 4)
    assert list(it) == ITEM_KEYS + ['valid']
    m1 = np.load(masked / aois[0] / 'masks' / f'masks_{aois[0]}_2018_02.npy') != 0
    v = it['valid']
    assert v.dtype == np.float32 and v.shape == it['change'].shape == (100, 90, 1)
    assert np.array_equal(v[:, :, 0], (~m1).astype(np.float32)) and 0 < v.mean() < 1  # month 4 has no mask file
    # both timestamps masked: the union; an (H, W, 1) file reads the same
    m2 = np.zeros((100, 90, 1), dtype=np.float32)
    m2[:7] = 3.0
    path = masked / aois[0] / 'masks' / f'masks_{aois[0]}_2018_04.npy'
    np.save(path, m2)
    try:
        v2 = datasets.MultimodalCDDataset(cfg, 'training', no_augmentations=True, rng=_Pick([1, 3]))[0]['valid']
        assert np.array_equal(v2[:, :, 0], (~(m1 | (m2[:, :, 0] != 0))).astype(np.float32))
        np.save(path, np.zeros((5, 5), dtype=np.uint8))
        with pytest.raises(ValueError, match='mask of shape'):
            datasets.MultimodalCDDataset(cfg, 'training', no_augmentations=True, rng=_Pick([1, 3]))[0]
    finally:
        os.remove(path)
    # an AOI without masks: everything valid; an unlabelled item carries the key too
    cfg.DATALOADER.INCLUDE_UNLABELED = True
    ds = datasets.MultimodalCDDataset(cfg, 'training', no_augmentations=True, rng=_Pick([0, 1]))
    assert ds[1]['valid'].all() and ds[1]['valid'].shape == (101, 92, 1)
    assert not ds[2]['is_labeled'] and ds[2]['valid'].all()


def test_set_key_consumes_the_same_random_stream(caches):
    """With the key set the draws are made in the same order and number: for an AOI without masked months the item
    equals the unmasked one, plus `valid`."""
    from multimodal_siamese_cd_amd.utils import datasets
    _, masked, aois = caches
    on, off = _cfg(masked, aois), _cfg(masked, aois)
    on.DATALOADER.INCLUDE_MASKED = True
    r1, r2 = np.random.RandomState(9), np.random.RandomState(9)
    a = datasets.MultimodalCDDataset(on, 'training', rng=r1)[1]
    b = datasets.MultimodalCDDataset(off, 'training', rng=r2)[1]
    assert a.pop('valid').all()
    _same_item(a, b)
    assert r1.get_state()[1].tolist() == r2.get_state()[1].tolist() and r1.get_state()[2] == r2.get_state()[2]
