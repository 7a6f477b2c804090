"""Generate tests/golden/masked_losses_t5-11x13.npz by running the REFERENCE loss functions on gathered elements
(build container only).

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_golden_masked_losses.py  [--ref /root/reference]

The contract of the per-pixel validity mask is the gather idiom: `criterion(logits, target, valid=v)` equals the
reference criterion on `logits[v], target[v]`, and each term of a fused recipe runs over the elements that are both in
its sample subset and valid.  So the oracle stays the reference's utils/loss_functions.py itself, evaluated on the CPU
in fp32 and in fp64 on boolean-gathered leaves; autograd's scatter puts the gradients back into the full shape with
zeros at the invalid pixels.  Only data is written; no reference source travels.

Inputs: exactly make_golden_losses.inputs() -- (5, 1, 11, 13), 143 pixels per sample, the +-100 logits included.
Mask: torch.rand(SHAPE, generator=manual_seed(23)) < 0.7, then valid[1] = False, valid[3] = True: 449 of 715 valid,
per sample [103, 0, 105, 143, 98] -- one empty sample, one full sample, and the unlabelled sample 1 of
is_labeled = [1, 0, 1, 1, 0] entirely invalid.

Per kind K and target form F in {hard, soft}: K/F/loss64, K/F/loss32, K/F/gx, soft: K/F/gz.
mmcr/<sup>_<cons>/<mask>/{loss64, loss32, gf, gs1, gs2, mask} for the label masks `mixed` and `all`, every term over
selection AND valid.  A term without any element is dropped, as the reference drops an empty sample subset.

Before anything is written the reference's own fp32 run is asserted to sit within the bars the GPU tests use, measured
against its fp64 run:  |loss32 - loss64| <= 1e-5 max(1, |loss64|),  max|g32 - g64| <= 1e-5 max|g64| per tensor.
"""
from __future__ import annotations

import argparse
import json
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import make_golden_losses as base  # noqa: E402

NAME = 'masked_losses_t5-11x13'
MASK_SEED = 23
MASK_KEEP = 0.7
MASKS = {'mixed': base.LABELED, 'all': [1, 1, 1, 1, 1]}
PER_SAMPLE = [103, 0, 105, 143, 98]


def valid_mask():
    v = torch.rand(base.SHAPE, generator=torch.Generator().manual_seed(MASK_SEED)) < MASK_KEEP
    v[1] = False
    v[3] = True
    return v


def mmcr(sup, cons, l2, lab, valid):
    """train_semisupervised.py:78-113 with LOSS_FACTOR = ALPHA, every term on (its samples) AND valid."""
    lab = torch.tensor(lab, dtype=torch.bool)
    vl = valid & lab.view(-1, 1, 1, 1)
    vn = valid & torch.logical_not(lab).view(-1, 1, 1, 1)

    def fn(f, s1, s2, y):
        loss = None
        if vl.any():
            loss = base.ALPHA * ((sup(f[vl], y[vl]) + sup(s1[vl], y[vl]) + sup(s2[vl], y[vl])) / 3)
        if vn.any():
            p1, p2 = torch.sigmoid(s1), torch.sigmoid(s2)
            c = cons(p1[vn], p2[vn]) if l2 else cons(s1[vn], p2[vn])
            c = (1 - base.ALPHA) * c
            loss = c if loss is None else loss + c
        return loss
    return fn


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--ref', default='/root/reference')
    args = ap.parse_args()
    ref = base.load_reference(args.ref)
    torch.set_num_threads(1)
    x, z, f, t = base.inputs()
    v = valid_mask()
    assert int(v.sum()) == sum(PER_SAMPLE) and v.view(5, -1).sum(1).tolist() == PER_SAMPLE, v.view(5, -1).sum(1)
    rec = {'x': x.float().numpy(), 'z': z.float().numpy(), 'f': f.float().numpy(), 't': t.float().numpy(),
           'valid': v.numpy().astype(np.uint8), 'is_labeled': np.array(base.LABELED, dtype=np.uint8)}
    crit = base.criteria(ref)
    for kind, fn in crit.items():
        base.record(rec, f'{kind}/hard', ['gx'], lambda a, fn=fn: fn(a[v], t.to(a.dtype)[v]), [x])
        base.record(rec, f'{kind}/soft', ['gx', 'gz'], lambda a, b, fn=fn: fn(a[v], torch.sigmoid(b)[v]), [x, z])
    l2 = ref.get_criterion('L2')
    for name, sup, cons, is_l2 in (('bce_l2', crit['bce'], l2, True),
                                   ('dicelike_pj', crit['dice_like'], crit['power_jaccard'], False)):
        for mname, lab in MASKS.items():
            fn = mmcr(sup, cons, is_l2, lab, v)
            base.record(rec, f'mmcr/{name}/{mname}', ['gf', 'gs1', 'gs2'],
                        lambda a, b, c, fn=fn: fn(a, b, c, t.to(a.dtype)), [f, x, z])
            rec[f'mmcr/{name}/{mname}/mask'] = np.array(lab, dtype=np.uint8)
    for k, a in rec.items():  # gradients scattered back: exactly zero at every invalid pixel
        if isinstance(a, np.ndarray) and a.shape == base.SHAPE and k.rsplit('/', 1)[-1].startswith('g'):
            assert not a[~v.numpy()].any(), k
    meta = dict(name=NAME, shape=base.SHAPE, seed=base.SEED, mask_seed=MASK_SEED, mask_keep=MASK_KEEP,
                valid_per_sample=PER_SAMPLE, alpha=base.ALPHA, kinds=list(crit), loss_bar=base.LOSS_BAR,
                grad_bar=base.GRAD_BAR,
                generator='reference utils/loss_functions.py on gathered elements (CPU fp32 and fp64, torch '
                          + torch.__version__ + ')')
    rec['meta'] = np.array(json.dumps(meta))
    path = os.path.join(HERE, f'{NAME}.npz')
    np.savez_compressed(path, **rec)
    print(f'{NAME}: {len(rec)} arrays -> {os.path.getsize(path) / 1024:.0f} KiB')


if __name__ == '__main__':
    main()
