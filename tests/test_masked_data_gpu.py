"""DATALOADER.INCLUDE_MASKED on the device: batch['valid'] takes the label's crop / flip / rot90.  The mask pattern is
also written as the change label (no buildings at t1, the pattern as buildings at t2, the pattern as t2's mask), so
under any draws valid == 1 - y_change must hold exactly."""
import json
import os
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, 'tools'))
import make_tile_cache  # noqa: E402


@pytest.fixture(scope='module')
def cache(tmp_path_factory):
    root = tmp_path_factory.mktemp('tiles_pattern')
    aois = make_tile_cache.make(str(root), aois=3, size=(100, 90), months=4)
    meta = json.load(open(root / 'metadata.json'))
    rng = np.random.default_rng(3)
    for a, aoi in enumerate(aois):
        h, w = 100 + a, 90 + 2 * a
        pattern = rng.random((h, w)) > 0.6
        pattern[10:30, 5:60] = True   # asymmetric, so a wrong flip or turn shows
        pattern[60:, :8] = False
        np.save(root / aoi / 'buildings' / f'buildings_{aoi}_2018_01.npy', np.zeros((h, w, 1), dtype=np.float32))
        np.save(root / aoi / 'buildings' / f'buildings_{aoi}_2018_04.npy', pattern[:, :, None].astype(np.float32))
        os.makedirs(root / aoi / 'masks', exist_ok=True)
        np.save(root / aoi / 'masks' / f'masks_{aoi}_2018_04.npy', pattern.astype(np.uint8) * (1 + a))
        meta[aoi][3]['masked'] = True
    json.dump(meta, open(root / 'metadata.json', 'w'))
    return root, aois


def _cfg(root, aois, **aug):
    from multimodal_siamese_cd_amd.utils import experiment_manager as em
    cfg = em.load_cfg('baseline_siamese')
    cfg.PATHS.DATASET = str(root)
    cfg.DATASET.TRAINING_IDS = aois
    cfg.DATALOADER.S2_BANDS = [2, 1, 0]
    cfg.DATALOADER.INCLUDE_MASKED = True
    cfg.DATALOADER.TRAINING_MULTIPLIER = 1
    cfg.AUGMENTATION.CROP_SIZE = 64
    cfg.AUGMENTATION.RANDOM_FLIP = True
    cfg.AUGMENTATION.RANDOM_ROTATE = True
    for k, v in aug.items():
        cfg.AUGMENTATION[k] = v
    return cfg


@pytest.mark.parametrize('aug', [dict(), dict(IMAGE_OVERSAMPLING_TYPE='none')])
def test_valid_follows_the_label_through_crop_flip_and_rotate(cache, aug):
    from multimodal_siamese_cd_amd import hip
    from multimodal_siamese_cd_amd.utils import datasets
    hip.load_library()
    dev = torch.device('cuda:0')
    root, aois = cache
    cfg = _cfg(root, aois, **aug)
    seen = set()
    for seed in (11, 12):
        ds = datasets.MultimodalCDDataset(cfg, 'training', dataset_mode='first_last', rng=np.random.RandomState(seed))
        items = [ds[i] for i in range(len(ds))]
        seen |= {(it['aug'].flip_h, it['aug'].flip_v, it['aug'].rot) for it in items}
        batch = datasets.device_collate(items, ds, dev)
        v, y = batch['valid'], batch['y_change']
        assert v.dtype == torch.uint8 and tuple(v.shape) == (3, 1, 64, 64) == tuple(y.shape) and v.is_contiguous()
        assert torch.equal(v.float(), 1 - y)
        assert 0.2 < float(y.mean()) < 0.8
        # the same draws without the key: the same batch, minus `valid`
        off = _cfg(root, aois, **aug)
        off.DATALOADER.INCLUDE_MASKED = False
        # (month 4 is marked masked there, so the unmasked dataset would end at month 3: compare on the arrays the
        # masked items carry instead)
        ds_off = datasets.MultimodalCDDataset(off, 'training', dataset_mode='first_last')
        plain = datasets.device_collate([{k: u for k, u in it.items() if k != 'valid'} for it in items], ds_off, dev)
        assert 'valid' not in plain and sorted(plain) == sorted(k for k in batch if k != 'valid')
        for k in ('x_t1', 'x_t2', 'y_change'):
            assert torch.equal(plain[k], batch[k]), k
    assert len(seen) > 1  # more than one flip / turn combination was exercised


def test_full_tiles_without_augmentations(cache):
    """The evaluation path's collate (no augmentations, batch size 1) carries the full-tile mask."""
    from multimodal_siamese_cd_amd import hip
    from multimodal_siamese_cd_amd.utils import datasets
    hip.load_library()
    dev = torch.device('cuda:0')
    root, aois = cache
    ds = datasets.MultimodalCDDataset(_cfg(root, aois), 'training', no_augmentations=True, dataset_mode='first_last')
    batch = datasets.device_collate([ds[1]], ds, dev)
    assert batch['valid'].dtype == torch.uint8 and tuple(batch['valid'].shape) == (1, 1, 101, 92)
    assert torch.equal(batch['valid'].float(), 1 - batch['y_change'])
