"""Generate the frozen-BatchNorm fixtures by running the REFERENCE implementation itself (build container only).

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_golden_frozen_bn.py  [--ref /root/reference]

The reference is imported as tests/golden/make_golden.py imports it.  For each base fixture (tests/golden/<name>.npz)
the reference model takes the base's parameters `p0/*` and the running statistics `r1/*` (the base's buffers after
its train-mode step: far from their initial 0 / 1 and different from this batch's statistics), is put in train mode
with its BatchNorm2d modules in eval mode -- the torch idiom of fine-tuning with frozen BatchNorm -- and runs one
forward, the trainer's loss recipe and backward on the base's own inputs (CPU fp32).

tests/golden/frozenbn_<name>.npz holds only `out/i`, `loss`, every `g/<param>` and `meta`; inputs, parameters and
buffers come from the base fixture at test time.  frozenbn_enc_siamese_t8-16.npz is the mixed case: only the BatchNorms
under `inc.` and `encoder.` are frozen; it also holds the buffers after the step as `r/*` (encoder: unchanged,
decoder: updated once).  Only data is written; no reference source travels.
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

BASES = ['siamese_t8-16', 'siamese_t8-16-32_odd', 'siamese_t32-64', 'dtsiamese_t8-16', 'dualstream_t8-16',
         'unet_t8-16', 'whatevernet_t8-16', 'whatevernet2_t8-16']
MIXED = ('enc_siamese_t8-16', 'siamese_t8-16', ['inc.', 'encoder.'])


def frozen_step(networks, pj, base: str, prefixes):
    fx = Fixture(base)
    cfgd = fx.cfg
    net = networks.create_network(G.ns_cfg(cfgd))
    module = net.module
    with torch.no_grad():
        for k, p in module.named_parameters():
            p.copy_(torch.from_numpy(fx.params0[k]))
        r1 = fx.prefixed('r1/')
        for k, b in module.named_buffers():
            b.copy_(torch.from_numpy(r1[k]))
    module.train()
    frozen = []
    for name, m in module.named_modules():
        if isinstance(m, torch.nn.BatchNorm2d) and (prefixes is None or name.startswith(tuple(prefixes))):
            m.eval()
            frozen.append(name)
    batch = fx.batch()
    out = net(batch['x_t1'], batch['x_t2'])
    loss = G._ref_step_loss(fx.model_type, out, batch, pj)
    loss.backward()
    rec = {f'out/{i}': o.detach().numpy() for i, o in enumerate(G.outputs_list(out))}
    rec['loss'] = np.float32(loss.item())
    for k, p in module.named_parameters():
        if p.grad is not None:
            rec['g/' + k] = p.grad.detach().numpy().copy()
    if prefixes is not None:
        for k, b in module.named_buffers():
            rec['r/' + k] = b.detach().numpy().copy()
    for k, b in module.named_buffers():  # a frozen BatchNorm leaves its statistics and its counter alone
        if k.rpartition('.')[0] in frozen:
            assert np.array_equal(b.numpy(), r1[k]), k
    meta = dict(base=base, frozen_prefixes=prefixes, frozen=frozen, buffers='r1/* of the base fixture',
                generator='reference utils/networks.py + utils/loss_functions.py, module.train() with the listed '
                          'BatchNorm2d modules in eval mode (CPU fp32, torch ' + torch.__version__ + ')')
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
    jobs = [(b, b, None) for b in BASES] + [MIXED]
    for name, base, prefixes in jobs:
        if args.only and args.only != name:
            continue
        rec, loss = frozen_step(networks, pj, base, prefixes)
        path = os.path.join(HERE, f'frozenbn_{name}.npz')
        np.savez_compressed(path, **rec)
        size = os.path.getsize(path)
        assert size < 1_000_000, f'{path}: {size} bytes'
        print(f'frozenbn_{name}: loss={loss:.6f} -> {size / 1024:.0f} KiB')


if __name__ == '__main__':
    main()
