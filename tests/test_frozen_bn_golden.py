"""Frozen BatchNorm (modules in eval mode inside a training step) on the CPU: the oracle's eval-mode backward pinned
against fixtures the reference itself produced (tests/golden/make_golden_frozen_bn.py), and the public surface
(networks.freeze_batchnorm, TRAINER.FREEZE_BN).  The GPU tests (tests/test_frozen_bn_gpu.py) lean on this oracle."""
import json
import os

import numpy as np
import pytest
import torch

from oracle import siamese_oracle as O
from oracle.golden import GOLDEN_DIR, Fixture, rel_err

FROZEN = ['siamese_t8-16', 'siamese_t8-16-32_odd', 'siamese_t32-64', 'dtsiamese_t8-16', 'dualstream_t8-16',
          'unet_t8-16', 'whatevernet_t8-16', 'whatevernet2_t8-16']
WHATEVER = ('whatevernet', 'whatevernet2')


def load_frozen(name):
    z = np.load(os.path.join(GOLDEN_DIR, f'frozenbn_{name}.npz'), allow_pickle=False)
    z = {k: z[k] for k in z.files}
    return z, json.loads(str(z['meta']))


def r1_buffers(fx):
    return {k: torch.from_numpy(v.copy()) for k, v in fx.prefixed('r1/').items()}


@pytest.mark.parametrize('name', FROZEN)
def test_oracle_frozen_step_matches_reference(name):
    """The bars of tests/test_oracle_golden.py's train-mode step: outputs 1e-5, loss 1e-6, gradients 1e-4 -- here
    for every tensor: the conv biases in front of a frozen BatchNorm have true gradients."""
    z, meta = load_frozen(name)
    fx = Fixture(meta['base'])
    assert set(z) - {'loss', 'meta'} == {k for k in z if k.startswith(('out/', 'g/'))}
    P = {k: torch.from_numpy(v.copy()).requires_grad_(True) for k, v in fx.params0.items()}
    B = r1_buffers(fx)
    B0 = {k: v.clone() for k, v in B.items()}
    batch = fx.batch()
    out = O.forward(fx.model_type, P, B, batch['x_t1'], batch['x_t2'], fx.cfg, training=False)
    for k, v in B.items():
        assert torch.equal(v, B0[k]), k
    if fx.model_type in WHATEVER:  # the oracle's eval mode returns the fusion output alone
        assert rel_err(out.detach().numpy(), z['out/0']) < 1e-5
        return
    outs = list(out) if isinstance(out, tuple) else [out]
    assert len(outs) == sum(k.startswith('out/') for k in z)
    for i, o in enumerate(outs):
        assert rel_err(o.detach().numpy(), z[f'out/{i}']) < 1e-5
    loss = O.step_loss(fx.model_type, out, batch, fx.meta['alpha'])
    assert abs(loss.item() - float(z['loss'])) < 1e-6
    loss.backward()
    for k, p in P.items():
        if 'g/' + k not in z:
            assert p.grad is None, k
            continue
        assert rel_err(p.grad.numpy(), z['g/' + k]) < 1e-4, k


@pytest.mark.parametrize('name', ['siamese_t8-16', 'siamese_t32-64', 'dtsiamese_t8-16', 'dualstream_t8-16'])
def test_reference_frozen_step_has_no_zero_gradient(name):
    """No parameter of the reference's frozen step has an all-zero gradient, the conv biases in front of a BatchNorm
    included (in train mode theirs is a true zero).  (siamese_t8-16-32_odd is left out: at its deepest level both
    branches take the same ReLU decisions, so the +g / -g of the difference cancel exactly in two bias gradients.)"""
    z, _ = load_frozen(name)
    for k, v in z.items():
        if k.startswith('g/'):
            assert np.abs(v).max() > 0, k


def test_mixed_fixture_buffers():
    """The reference's mixed step: frozen (inc., encoder.) BatchNorms keep r1/*, the decoder's update once."""
    z, meta = load_frozen('enc_siamese_t8-16')
    fx = Fixture(meta['base'])
    r1 = fx.prefixed('r1/')
    assert meta['frozen_prefixes'] == ['inc.', 'encoder.']
    for k, v in r1.items():
        after = z['r/' + k]
        if k.startswith(('inc.', 'encoder.')):
            assert np.array_equal(after, v), k
        elif k.endswith('num_batches_tracked'):
            assert int(after) == int(v) + 1, k
        else:
            assert not np.array_equal(after, v), k


def _net(name='siamese_t8-16'):
    from multimodal_siamese_cd_amd.utils import networks
    fx = Fixture(name)
    return networks, networks.create_network(fx.package_cfg()), fx


def test_freeze_batchnorm_selects_batchnorm_modules():
    networks, net, _ = _net()
    net.train()
    assert networks.freeze_batchnorm(net) is net
    n_bn = 0
    for name, m in net.module.named_modules():
        if isinstance(m, torch.nn.BatchNorm2d):
            assert not m.training, name
            n_bn += 1
        else:
            assert m.training, name
    assert n_bn == sum(k.endswith('running_mean') for k in net.module.state_dict()) > 0
    assert net.training


def test_freeze_batchnorm_prefixes():
    networks, net, _ = _net()
    net.train()
    networks.freeze_batchnorm(net, ['inc.', 'encoder.'])
    for name, m in net.module.named_modules():
        if isinstance(m, torch.nn.BatchNorm2d):
            assert m.training == (not name.startswith(('inc.', 'encoder.'))), name
    net.train()  # torch semantics: train() unfreezes
    assert all(m.training for m in net.module.modules())
    networks.freeze_batchnorm(net.module, 'decoder.up_seq.up1.conv.conv.1')  # a bare module, one full name
    frozen = [n for n, m in net.module.named_modules() if isinstance(m, torch.nn.BatchNorm2d) and not m.training]
    assert frozen == ['decoder.up_seq.up1.conv.conv.1']


def test_trainer_freeze_bn_setting():
    networks, net, fx = _net()
    cfg = fx.package_cfg()
    assert 'FREEZE_BN' not in cfg.TRAINER  # shipped configs carry no such key: absent means False
    assert networks.freeze_bn_setting(cfg) is False
    net.train()
    networks.apply_freeze_bn(net, cfg)
    assert all(m.training for m in net.module.modules())
    cfg.TRAINER.FREEZE_BN = True
    assert networks.freeze_bn_setting(cfg) is True
    networks.apply_freeze_bn(net.train(), cfg)
    assert not any(m.training for m in net.module.modules() if isinstance(m, torch.nn.BatchNorm2d))
    cfg.TRAINER.FREEZE_BN = ['encoder.']
    assert networks.freeze_bn_setting(cfg) == ['encoder.']
    networks.apply_freeze_bn(net.train(), cfg)
    for name, m in net.module.named_modules():
        if isinstance(m, torch.nn.BatchNorm2d):
            assert m.training == (not name.startswith('encoder.')), name
    for bad in ('encoder.', [], [1], 3):
        cfg.TRAINER.FREEZE_BN = bad
        with pytest.raises(ValueError):
            networks.freeze_bn_setting(cfg)
