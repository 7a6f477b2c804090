"""CPU-side checks of networks.freeze_parameters and TRAINER.FREEZE_PARAMS (the GPU behaviour:
tests/test_frozen_params_gpu.py)."""
import pytest
import torch

from oracle.golden import Fixture


def _net(name='siamese_t8-16'):
    from multimodal_siamese_cd_amd.utils import networks
    fx = Fixture(name)
    return networks, networks.create_network(fx.package_cfg()), fx


def test_freeze_parameters_all_and_by_prefix():
    networks, net, _ = _net()
    net.train()
    names = [k for k, _ in net.module.named_parameters()]
    frozen = networks.freeze_parameters(net, ['inc.', 'encoder.'])
    assert frozen == [k for k in names if k.startswith(('inc.', 'encoder.'))] and frozen
    assert not any(k.startswith('module.') for k in frozen)  # names as freeze_batchnorm's: wrappers aside
    for k, p in net.module.named_parameters():
        assert p.requires_grad == (k not in frozen), k
    assert all(m.training for m in net.module.modules())  # .training is not touched
    assert networks.freeze_parameters(net.module, 'outc.conv.bias') == ['outc.conv.bias']  # a bare module, one name
    assert networks.freeze_parameters(net) == names
    assert not any(p.requires_grad for p in net.parameters())


def test_freeze_parameters_composes_with_freeze_batchnorm():
    networks, net, _ = _net()
    networks.freeze_parameters(net, ['encoder.'])
    networks.freeze_batchnorm(net.train(), ['encoder.'])
    for name, m in net.module.named_modules():
        if isinstance(m, torch.nn.BatchNorm2d):
            assert m.training == (not name.startswith('encoder.')), name
            assert m.weight.requires_grad == (not name.startswith('encoder.')), name
    net.train()  # unfreezes the BatchNorms' mode, not the parameters
    assert not any(p.requires_grad for k, p in net.module.named_parameters() if k.startswith('encoder.'))


def test_trainer_freeze_params_setting():
    networks, net, fx = _net()
    cfg = fx.package_cfg()
    assert 'FREEZE_PARAMS' not in cfg.TRAINER  # shipped configs carry no such key: absent means False
    assert networks.freeze_params_setting(cfg) is False
    assert networks.apply_freeze_params(net, cfg) is net
    assert all(p.requires_grad for p in net.parameters())
    cfg.TRAINER.FREEZE_PARAMS = ['encoder.']
    assert networks.freeze_params_setting(cfg) == ['encoder.']
    networks.apply_freeze_params(net, cfg)
    for k, p in net.module.named_parameters():
        assert p.requires_grad == (not k.startswith('encoder.')), k
    cfg.TRAINER.FREEZE_PARAMS = True
    assert networks.freeze_params_setting(cfg) is True
    networks.apply_freeze_params(net, cfg)
    assert not any(p.requires_grad for p in net.parameters())
    for bad in ('encoder.', [], [1], 3):
        cfg.TRAINER.FREEZE_PARAMS = bad
        with pytest.raises(ValueError):
            networks.freeze_params_setting(cfg)


def test_skip_frozen_grads_is_an_engine_option():
    from multimodal_siamese_cd_amd import engine
    assert engine.option('skip_frozen_grads') is True
    prev = engine.set_options(skip_frozen_grads=False)
    try:
        assert prev['skip_frozen_grads'] is True and engine.option('skip_frozen_grads') is False
    finally:
        engine.set_options(**prev)
    assert 'skip_frozen_grads' in engine.set_options.__doc__
