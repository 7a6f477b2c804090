"""networks.convert_sync_batchnorm and TRAINER.SYNC_BN on the CPU: what is marked, what stays as it was, and how the
setting is validated (as TRAINER.FREEZE_BN is)."""
import pytest
import torch
from torch import nn


def _net():
    from multimodal_siamese_cd_amd.utils import networks
    from oracle.golden import Fixture
    return networks.create_network(Fixture('siamese_t8-16').package_cfg())


def _marked(net):
    from multimodal_siamese_cd_amd import engine
    return {n for n, m in net.module.named_modules() if isinstance(m, nn.BatchNorm2d) and engine.bn_sync_mark(m)[0]}


def test_convert_marks_in_place():
    from multimodal_siamese_cd_amd.utils import networks
    net = _net()
    keys = list(net.state_dict())
    ids = {k: id(v) for k, v in list(net.named_parameters()) + list(net.named_buffers())}
    all_bn = {n for n, m in net.module.named_modules() if isinstance(m, nn.BatchNorm2d)}
    assert all_bn and not _marked(net)
    assert networks.convert_sync_batchnorm(net) is net
    assert _marked(net) == all_bn
    assert all(type(m) is nn.BatchNorm2d for m in net.modules() if isinstance(m, nn.BatchNorm2d))
    assert list(net.state_dict()) == keys
    assert ids == {k: id(v) for k, v in list(net.named_parameters()) + list(net.named_buffers())}
    # a checkpoint of the converted model loads into an unconverted one and back
    _net().load_state_dict(net.state_dict())
    net.load_state_dict(_net().state_dict())
    # the stock isinstance idiom and freeze_batchnorm keep working
    networks.freeze_batchnorm(net.train())
    assert not any(m.training for m in net.modules() if isinstance(m, nn.BatchNorm2d))


def test_convert_by_prefix_and_group():
    from multimodal_siamese_cd_amd import engine
    from multimodal_siamese_cd_amd.utils import networks
    net = _net()
    group = object()
    networks.convert_sync_batchnorm(net, ['encoder.'], process_group=group)
    marked = _marked(net)
    assert marked and all(n.startswith('encoder.') for n in marked)
    assert {n for n, m in net.module.named_modules() if isinstance(m, nn.BatchNorm2d) and n.startswith('encoder.')} \
        == marked
    assert all(engine.bn_sync_mark(net.module.get_submodule(n)) == (True, group) for n in marked)
    assert _marked(networks.convert_sync_batchnorm(_net(), 'inc.')) == {'inc.conv.conv.1', 'inc.conv.conv.4'}


def test_stock_conversion_is_recognised_and_frozen():
    from multimodal_siamese_cd_amd import engine
    from multimodal_siamese_cd_amd.utils import networks
    net = nn.SyncBatchNorm.convert_sync_batchnorm(_net())
    bns = [m for m in net.modules() if isinstance(m, nn.SyncBatchNorm)]
    assert bns and all(engine.bn_sync_mark(m) == (True, None) for m in bns)
    networks.freeze_batchnorm(net.train(), ['inc.'])
    frozen = {n for n, m in net.module.named_modules() if isinstance(m, nn.SyncBatchNorm) and not m.training}
    assert frozen == {'inc.conv.conv.1', 'inc.conv.conv.4'}


def test_single_process_is_not_synchronized():
    """Outside a process group a marked BatchNorm takes the existing path: no collective can be issued."""
    from multimodal_siamese_cd_amd import engine
    from multimodal_siamese_cd_amd.utils import networks
    net = networks.convert_sync_batchnorm(_net())
    assert not torch.distributed.is_initialized()
    assert all(engine._bn_sync_of(m) is None for m in net.modules() if isinstance(m, nn.BatchNorm2d))


def test_trainer_sync_bn_setting():
    from multimodal_siamese_cd_amd.utils import experiment_manager as em, networks
    cfg = em.load_cfg('debug')
    assert 'SYNC_BN' not in cfg.TRAINER  # shipped configs carry no such key: absent means False
    assert networks.sync_bn_setting(cfg) is False
    net = _net()
    assert networks.apply_sync_bn(net, cfg) is net and not _marked(net)
    cfg.TRAINER.SYNC_BN = True
    assert networks.sync_bn_setting(cfg) is True
    assert _marked(networks.apply_sync_bn(_net(), cfg)) == {n for n, m in net.module.named_modules()
                                                            if isinstance(m, nn.BatchNorm2d)}
    cfg.TRAINER.SYNC_BN = ['encoder.']
    assert networks.sync_bn_setting(cfg) == ['encoder.']
    assert all(n.startswith('encoder.') for n in _marked(networks.apply_sync_bn(_net(), cfg)))
    for bad in ('encoder.', 1, [], [1], ['inc.', 2]):
        cfg.TRAINER.SYNC_BN = bad
        with pytest.raises(ValueError, match='TRAINER.SYNC_BN'):
            networks.sync_bn_setting(cfg)
