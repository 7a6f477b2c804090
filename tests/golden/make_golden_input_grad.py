"""Generate the input-gradient fixtures by running the REFERENCE implementation itself (build container only).

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_golden_input_grad.py  [--ref /root/reference]

The reference is imported as tests/golden/make_golden.py imports it.  For each base fixture (tests/golden/<name>.npz)
the reference model takes the base's parameters `p0/*`, is put in train mode and runs the base's own first step --
forward, the trainer's loss recipe, backward (CPU fp32) -- with both inputs requiring grad.  The parameter gradients of
that step must equal the base fixture's `g/*` bit for bit (asserted here): asking for the input gradients changes
nothing else.

tests/golden/inputgrad_<name>.npz holds only `gx/x_t1`, `gx/x_t2`, `loss` and `meta`; inputs and parameters come from
the base fixture at test time.  inputgrad_eval_siamese_t8-16.npz is the saliency-on-a-checkpoint case: module.eval(),
the buffers `r1/*` of the base, the loss on the one eval output.  Only data is written; no reference source travels.
"""
from __future__ import annotations

import argparse
import json
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
sys.path.insert(0, HERE)

import make_golden as G  # noqa: E402
from oracle.golden import Fixture  # noqa: E402

BASES = ['siamese_t8-16', 'siamese_t8-16-32_odd', 'siamese_t32-64', 'siamese_t12-20', 'unet_t8-16',
         'dualstream_t8-16', 'dtsiamese_t8-16', 'whatevernet_t8-16', 'whatevernet2_t8-16']
EVAL = ('eval_siamese_t8-16', 'siamese_t8-16')


def input_grad_step(networks, pj, base: str, eval_mode: bool):
    fx = Fixture(base)
    net = networks.create_network(G.ns_cfg(fx.cfg))
    module = net.module
    with torch.no_grad():
        for k, p in module.named_parameters():
            p.copy_(torch.from_numpy(fx.params0[k]))
        if eval_mode:
            r1 = fx.prefixed('r1/')
            for k, b in module.named_buffers():
                b.copy_(torch.from_numpy(r1[k]))
    module.train(not eval_mode)
    batch = fx.batch()
    x1 = batch['x_t1'].clone().requires_grad_()
    x2 = batch['x_t2'].clone().requires_grad_()
    out = net(x1, x2)
    if eval_mode:
        outs = G.outputs_list(out)
        assert len(outs) == 1, 'the eval fixture takes the loss on the one eval output'
        loss = pj(outs[0], batch['y_change'])
    else:
        loss = G._ref_step_loss(fx.model_type, out, batch, pj)
    loss.backward()
    if not eval_mode:  # the same step as the base fixture's: its parameter gradients, bit for bit
        assert np.float32(loss.item()) == fx.z['loss0'], base
        for k, p in module.named_parameters():
            if p.grad is not None:
                assert np.array_equal(p.grad.numpy(), fx.grads[k]), f'{base}: {k}'
    rec = {'gx/x_t1': x1.grad.numpy().copy(), 'gx/x_t2': x2.grad.numpy().copy(), 'loss': np.float32(loss.item())}
    meta = dict(base=base, mode='eval' if eval_mode else 'train',
                buffers='r1/* of the base fixture' if eval_mode else 'initial',
                generator='reference utils/networks.py + utils/loss_functions.py, x_t1 and x_t2 requiring grad '
                          '(CPU fp32, torch ' + torch.__version__ + ')')
    rec['meta'] = np.array(json.dumps(meta))
    return rec, loss.item()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--ref', default='/root/reference')
    ap.add_argument('--only', default=None)
    args = ap.parse_args()
    networks, loss_functions = G.import_reference(args.ref)
    pj = loss_functions.get_criterion('PowerJaccardLoss')
    torch.set_num_threads(min(8, os.cpu_count() or 1))
    jobs = [(b, b, False) for b in BASES] + [(EVAL[0], EVAL[1], True)]
    for name, base, eval_mode in jobs:
        if args.only and args.only != name:
            continue
        rec, loss = input_grad_step(networks, pj, base, eval_mode)
        path = os.path.join(HERE, f'inputgrad_{name}.npz')
        np.savez_compressed(path, **rec)
        size = os.path.getsize(path)
        assert size < 1_000_000, f'{path}: {size} bytes'
        print(f'inputgrad_{name}: loss={loss:.6f} -> {size / 1024:.0f} KiB')


if __name__ == '__main__':
    main()
