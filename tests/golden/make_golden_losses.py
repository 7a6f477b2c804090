"""Generate tests/golden/losses_t5-11x13.npz by running the REFERENCE loss functions themselves (build container only).

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_golden_losses.py  [--ref /root/reference]

Loads the reference's utils/loss_functions.py by path (it imports only torch) and evaluates, on the CPU, once in fp32
and once in fp64 (the functions are dtype-agnostic), every single-channel criterion `get_criterion` registers, the
MMCR `L2` consistency term (train_semisupervised.py:101-102) and two MMCR compositions (train_semisupervised.py:78-113,
alpha = 0.5).  Only data is written; no reference source travels.

Inputs: logits x (stream 1), z (stream 2) and f (fusion) of shape (5, 1, 11, 13) -- 143 pixels per sample, 715
elements: no multiple of 4 or 64, so a sample boundary falls inside a 16-byte vector and inside a wave -- drawn
N(0, 1) * 3, six cells of x overwritten with -100, -40, -17, 17, 40, 100; a hard target t with about 20 % ones;
is_labeled = [1, 0, 1, 1, 0].

Per kind K and target form F in {hard: t, soft: sigmoid(z), not detached}:
    K/F/loss64 (float64), K/F/loss32 (float32), K/F/gx (d loss / d x, fp64 rounded to float32), soft: K/F/gz
l2cons/...: MSE(sigmoid(x), sigmoid(z)).   mmcr/<sup>_<cons>/<mask>/{loss64, loss32, gf, gs1, gs2}.

Before anything is written the reference's own fp32 run is asserted to sit within the bars the GPU tests use, measured
against its fp64 run:  |loss32 - loss64| <= 1e-5 max(1, |loss64|),  max|g32 - g64| <= 1e-5 max|g64| per tensor.
"""
from __future__ import annotations

import argparse
import importlib.util
import json
import os

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
NAME = 'losses_t5-11x13'
SHAPE = (5, 1, 11, 13)
SEED = 11
SCALE = 3.0
EXTREMES = (-100.0, -40.0, -17.0, 17.0, 40.0, 100.0)
LABELED = [1, 0, 1, 1, 0]
MASKS = {'mixed': LABELED, 'all': [1, 1, 1, 1, 1], 'none': [0, 0, 0, 0, 0]}
ALPHA = 0.5
LOSS_BAR = 1e-5
GRAD_BAR = 1e-5


def load_reference(ref):
    spec = importlib.util.spec_from_file_location('ref_loss_functions', os.path.join(ref, 'utils', 'loss_functions.py'))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def inputs():
    """The seeded recipe (tests/test_losses_gpu.py draws its larger shape the same way)."""
    g = torch.Generator().manual_seed(SEED)
    x = torch.randn(SHAPE, generator=g, dtype=torch.float64) * SCALE
    z = torch.randn(SHAPE, generator=g, dtype=torch.float64) * SCALE
    f = torch.randn(SHAPE, generator=g, dtype=torch.float64) * SCALE
    t = (torch.rand(SHAPE, generator=g, dtype=torch.float64) < 0.2).double()
    flat = x.view(-1)
    n = flat.numel()
    for k, v in enumerate(EXTREMES):  # spread over the five samples
        flat[(k * n) // len(EXTREMES) + 5 * k + 1] = v
    # the values every consumer sees are the float32 ones
    return tuple(a.float().double() for a in (x, z, f, t))


def criteria(ref):
    return {
        'soft_dice': ref.get_criterion('SoftDiceLoss'),
        'soft_dice_balanced': ref.get_criterion('SoftDiceBalancedLoss'),
        'iou': ref.get_criterion('IoULoss'),
        'dice_like': ref.get_criterion('DiceLikeLoss'),
        'power_jaccard': ref.get_criterion('PowerJaccardLoss'),
        'bce': ref.get_criterion('BCEWithLogitsLoss'),
        'mse': ref.get_criterion('MeanSquareErrorLoss'),
    }


def run(fn, tensors, dtype):
    """fn over fresh leaves of `dtype`; the loss and the gradient of every leaf (zeros where it is unused)."""
    leaves = [a.to(dtype).clone().requires_grad_(True) for a in tensors]
    loss = fn(*leaves)
    grads = torch.autograd.grad(loss, leaves, allow_unused=True)
    return loss.detach(), [torch.zeros_like(a) if g is None else g for a, g in zip(leaves, grads)]


def record(rec, key, names, fn, tensors):
    l64, g64 = run(fn, tensors, torch.float64)
    l32, g32 = run(fn, tensors, torch.float32)
    err = abs(float(l32) - float(l64)) / max(1.0, abs(float(l64)))
    assert err <= LOSS_BAR, f'{key}: the reference fp32 loss is {err:.2e} off its fp64 run'
    worst = 0.0
    for nm, a, b in zip(names, g32, g64):
        if float(b.abs().max()) == 0.0:
            assert float(a.abs().max()) == 0.0, f'{key}/{nm}'
            continue
        e = float((a.double() - b).abs().max() / b.abs().max())
        assert e <= GRAD_BAR, f'{key}/{nm}: the reference fp32 gradient is {e:.2e} of max off its fp64 run'
        worst = max(worst, e)
    rec[f'{key}/loss64'] = np.float64(float(l64))
    rec[f'{key}/loss32'] = np.float32(float(l32))
    for nm, b in zip(names, g64):
        rec[f'{key}/{nm}'] = b.float().numpy()
    print(f'{key}: loss64={float(l64):.9f} fp32 loss err {err:.1e} grad err {worst:.1e}')


def mmcr(sup, cons, l2, lab):
    """train_semisupervised.py:78-113 with LOSS_FACTOR = ALPHA."""
    lab = torch.tensor(lab, dtype=torch.bool)

    def fn(f, s1, s2, y):
        loss = None
        if lab.any():
            loss = ALPHA * ((sup(f[lab], y[lab]) + sup(s1[lab], y[lab]) + sup(s2[lab], y[lab])) / 3)
        if not lab.all():
            nl = torch.logical_not(lab)
            p1, p2 = torch.sigmoid(s1), torch.sigmoid(s2)
            c = cons(p1[nl], p2[nl]) if l2 else cons(s1[nl], p2[nl])
            c = (1 - ALPHA) * c
            loss = c if loss is None else loss + c
        return loss
    return fn


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--ref', default='/root/reference')
    args = ap.parse_args()
    ref = load_reference(args.ref)
    torch.set_num_threads(1)
    x, z, f, t = inputs()
    rec = {'x': x.float().numpy(), 'z': z.float().numpy(), 'f': f.float().numpy(), 't': t.float().numpy(),
           'is_labeled': np.array(LABELED, dtype=np.uint8)}
    crit = criteria(ref)
    for kind, fn in crit.items():
        # hard target: only x is a leaf
        record(rec, f'{kind}/hard', ['gx'], lambda a, fn=fn: fn(a, t.to(a.dtype)), [x])
        record(rec, f'{kind}/soft', ['gx', 'gz'], lambda a, b, fn=fn: fn(a, torch.sigmoid(b)), [x, z])
    l2 = ref.get_criterion('L2')
    record(rec, 'l2cons', ['gx', 'gz'], lambda a, b: l2(torch.sigmoid(a), torch.sigmoid(b)), [x, z])
    for name, sup, cons, is_l2 in (('bce_l2', crit['bce'], l2, True),
                                   ('dicelike_pj', crit['dice_like'], crit['power_jaccard'], False)):
        for mname, lab in MASKS.items():
            fn = mmcr(sup, cons, is_l2, lab)
            record(rec, f'mmcr/{name}/{mname}', ['gf', 'gs1', 'gs2'],
                   lambda a, b, c, fn=fn: fn(a, b, c, t.to(a.dtype)), [f, x, z])
            rec[f'mmcr/{name}/{mname}/mask'] = np.array(lab, dtype=np.uint8)
    meta = dict(name=NAME, shape=SHAPE, seed=SEED, scale=SCALE, extremes=EXTREMES, alpha=ALPHA,
                kinds=list(crit), loss_bar=LOSS_BAR, grad_bar=GRAD_BAR,
                generator='reference utils/loss_functions.py (CPU fp32 and fp64, torch ' + torch.__version__ + ')')
    rec['meta'] = np.array(json.dumps(meta))
    path = os.path.join(HERE, f'{NAME}.npz')
    np.savez_compressed(path, **rec)
    print(f'{NAME}: {len(rec)} arrays -> {os.path.getsize(path) / 1024:.0f} KiB')


if __name__ == '__main__':
    main()
