"""The masked loss kernels beside the unmasked ones, for a kernel-trace run of their own:

    rocprofv3 --kernel-trace --stats --output-format csv -d <dir> -o <name> -- \
        python tools/perf_masked_loss.py --kind iou --mask cloud [--batch 32] [--size 256] [--iters 200]

One process launches, for ONE kind and ONE mask, `iters` times each: scd_loss_multi_fwd / _bwd (kernels
loss_multi_partial, loss_multi_finalize, loss_multi_bwd_kernel) and scd_loss_masked_fwd / _bwd (loss_masked_partial,
loss_masked_finalize, loss_masked_bwd_kernel) on the same logits and target, single term, every sample selected, the
bench shape (32 x 1 x 256 x 256) by default.  The stats' AverageNs per kernel name is then one kind's time; run it once
per kind and mask.  Masks: `ones` (every pixel valid: the vector path throughout), `cloud` (each sample loses a
rectangle of about a quarter of its pixels: whole invalid vectors, and mixed ones on the rectangle's edges), `speckle`
(rand < 0.7: nearly every vector of mixed validity).

Bytes per pixel the kernels must move (fp32 logits and target, one mask byte): forward 8 unmasked, 9 masked; backward
(hard target: logits, target in, glogits out) 12 unmasked, 13 masked.  The line printed at the end carries the host
timing of the same loops (device-synchronised), for orientation only; the kernel times are the trace's.
"""
import argparse
import json
import os
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from multimodal_siamese_cd_amd import hip  # noqa: E402

KINDS = {'iou': hip.LOSS_IOU, 'bce': hip.LOSS_BCE_LOGITS, 'power_jaccard': hip.LOSS_POWER_JACCARD,
         'soft_dice_balanced': hip.LOSS_SOFT_DICE_BALANCED, 'mse': hip.LOSS_MSE}


def make_mask(kind, shape, gen, dev):
    b, _, h, w = shape
    if kind == 'ones':
        return torch.ones(shape, dtype=torch.uint8, device=dev)
    if kind == 'speckle':
        return (torch.rand(shape, generator=gen) < 0.7).to(torch.uint8).to(dev)
    v = torch.ones(shape, dtype=torch.uint8)
    for i in range(b):
        y0 = int(torch.randint(0, h // 2, (1,), generator=gen))
        x0 = int(torch.randint(0, w // 2, (1,), generator=gen))
        v[i, :, y0:y0 + h // 2, x0 + 1:x0 + 1 + w // 2] = 0  # an odd left edge: mixed vectors along both sides
    return v.to(dev)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--kind', default='iou', choices=sorted(KINDS))
    ap.add_argument('--mask', default='cloud', choices=['ones', 'cloud', 'speckle'])
    ap.add_argument('--batch', type=int, default=32)
    ap.add_argument('--size', type=int, default=256)
    ap.add_argument('--iters', type=int, default=200)
    ap.add_argument('--warmup', type=int, default=20)
    a = ap.parse_args()
    hip.load_library()
    dev = torch.device('cuda:0')
    gen = torch.Generator().manual_seed(0)
    shape = (a.batch, 1, a.size, a.size)
    x = (torch.randn(shape, generator=gen) * 3).to(dev)
    t = (torch.rand(shape, generator=gen) < 0.2).float().to(dev)
    v = make_mask(a.mask, shape, gen, dev)
    gx = torch.empty_like(x)
    n, pixels = a.batch, a.size * a.size
    sums = torch.empty((1, hip.LOSS_ROW), device=dev)
    counts = torch.empty(1, dtype=torch.int64, device=dev)
    loss = torch.empty((), device=dev)
    term = dict(logits=x, target=t, coef=1.0, select=0, soft=0, kind=KINDS[a.kind])
    bterm = dict(term, glogits=gx)
    loops = {
        'unmasked_fwd': lambda: hip.loss_multi_fwd([term], None, n, pixels, sums, loss),
        'unmasked_bwd': lambda: hip.loss_multi_bwd([bterm], None, n, pixels, sums, None),
        'masked_fwd': lambda: hip.loss_masked_fwd([term], None, [v], n, pixels, sums, counts, loss),
        'masked_bwd': lambda: hip.loss_masked_bwd([bterm], None, [v], n, pixels, sums, None),
    }
    out = dict(kind=a.kind, mask=a.mask, shape=list(shape), iters=a.iters, valid_fraction=float(v.float().mean()))
    for rep in range(2):  # the second pass repeats every loop: the spread on this box
        for name, fn in loops.items():
            for _ in range(a.warmup):
                fn()
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(a.iters):
                fn()
            torch.cuda.synchronize()
            out[f'{name}_host_us_{rep}'] = round((time.perf_counter() - t0) / a.iters * 1e6, 2)
    out['count'] = int(counts[0])
    print(json.dumps(out), flush=True)


if __name__ == '__main__':
    main()
