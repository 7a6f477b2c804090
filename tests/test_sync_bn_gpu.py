"""BatchNorm synchronized over ranks at model level (MI355X): two ranks on one GPU (gloo carries the collectives of the
rehearsal; on a node the same code runs over RCCL), as tests/test_exact_dp_gpu.py runs them.

With networks.convert_sync_batchnorm and parallel.wrap_ddp(exact_dataparallel=True) a step of two ranks is the step of
one device on the global batch, so two ranks holding ONE sample each must reproduce the reference's own full-batch
fixtures (tests/golden/*.npz, batch 2) -- which per-rank statistics cannot: a batch of one against a batch of two.
Bars, those of tests/test_exact_dp_gpu.py: concatenated logits 1e-4, loss 1e-5 on every rank, every gradient 1e-3
under tests/_parity.py's kink rule (kinks recorded on the full batch), running statistics 1e-5 and num_batches_tracked
against the post-step buffers; the running statistics of the two ranks are bit-equal.

Further cases run against ONE process that takes the whole batch with plain BatchNorm, at the same bars: DDP's default
mode (gradient averaging: the mean of the two shards' losses; the model converted by torch's own
nn.SyncBatchNorm.convert_sync_batchnorm), an uneven 3 + 1 split, and a bf16 model (baseline_dualstream), whose bars are
those tests/test_bf16_gpu.py holds a bf16 model step to (logits 3e-2, loss 1e-2, every weight gradient's cosine
similarity > 0.95): in bf16 storage a last-bit difference of a statistic becomes one bf16 step of an activation.
"""
import os
import socket
import tempfile

import numpy as np
import pytest
import torch
import torch.multiprocessing as mp

pytestmark = pytest.mark.gpu

FIXTURES = ['siamese_t8-16', 'siamese_t32-64', 'dtsiamese_t32-64', 'dualstream_t32-64', 'whatevernet_t8-16',
            'siamese_t12-20']
# id: (config, model, topology, tile, images per rank, exact_dataparallel, conversion)
SYNTHETIC = {
    'uneven': ('baseline_siamese', 'siameseunet', [32, 64], 32, (3, 1), True, 'ours'),
    'bf16': ('baseline_dualstream', 'dualstreamunet', [64, 128], 64, (2, 2), True, 'ours'),
}


def _free_port():
    with socket.socket() as s:
        s.bind(('127.0.0.1', 0))
        return s.getsockname()[1]


def _outs(o):
    return list(o) if isinstance(o, (tuple, list)) else [o]


def _setup(case):
    """(cfg, oracle cfg, model type, parameters, whole batch, images per rank, exact_dataparallel, conversion)."""
    from oracle import siamese_oracle as O
    from oracle.golden import Fixture
    if case in SYNTHETIC:
        from multimodal_siamese_cd_amd.utils import experiment_manager as em
        config, model, topo, size, counts, exact, conv = SYNTHETIC[case]
        cfg = em.load_cfg(config)
        cfg.MODEL.TYPE, cfg.MODEL.TOPOLOGY = model, list(topo)
        ocfg = dict(TYPE=model, TOPOLOGY=list(topo), IN_CHANNELS=cfg.MODEL.IN_CHANNELS,
                    OUT_CHANNELS=cfg.MODEL.OUT_CHANNELS, S1_BANDS=list(cfg.DATALOADER.S1_BANDS),
                    S2_BANDS=list(cfg.DATALOADER.S2_BANDS))
        P = O.deterministic_params(O.param_shapes(model, ocfg), 21)
        return cfg, ocfg, model, P, O.synthetic_batch(ocfg, sum(counts), size, 22), counts, exact, conv
    fx = Fixture('siamese_t8-16' if case == 'avg' else case)
    P = {k: torch.from_numpy(v.copy()) for k, v in fx.params0.items()}
    assert fx.meta['batch'] == 2
    return fx.package_cfg(), fx.cfg, fx.model_type, P, fx.batch(), (1, 1), case != 'avg', \
        'torch' if case == 'avg' else 'ours'


def _net(cfg, P, dev):
    from multimodal_siamese_cd_amd.utils import networks
    net = networks.create_network(cfg)
    with torch.no_grad():
        for k, p in net.module.named_parameters():
            p.copy_(P[k])
    return net.to(dev).train()


def _shard(batch, counts, r):
    lo = sum(counts[:r])
    return {k: v[lo:lo + counts[r]] for k, v in batch.items()}


def _result(net, loss, out):
    from multimodal_siamese_cd_amd.utils import networks
    m = networks._unwrapped(net)
    return {'loss': loss.item(), 'outs': [o.detach().cpu() for o in _outs(out)],
            'grads': {n: p.grad.detach().cpu() for n, p in m.named_parameters() if p.grad is not None},
            'buffers': {n: v.detach().cpu() for n, v in m.named_buffers()}}


def _worker(rank, world, port, out_dir, case):
    os.environ.update(RANK=str(rank), LOCAL_RANK=str(rank), WORLD_SIZE=str(world), MASTER_ADDR='127.0.0.1',
                      MASTER_PORT=str(port), SCD_RANKS_SHARE_GPU='1')
    from multimodal_siamese_cd_amd import hip, parallel, trainers
    from multimodal_siamese_cd_amd.utils import networks
    parallel.init_distributed('gloo')
    dev = torch.device('cuda', parallel.device_index(rank))
    torch.cuda.set_device(dev)
    hip.load_library()
    cfg, _, _, P, batch, counts, exact, conv = _setup(case)
    net = _net(cfg, P, dev)
    if conv == 'torch':
        net = torch.nn.SyncBatchNorm.convert_sync_batchnorm(net)
        assert any(isinstance(m, torch.nn.SyncBatchNorm) for m in net.modules())
    else:
        assert networks.convert_sync_batchnorm(net) is net
    net = parallel.wrap_ddp(net, dev, exact_dataparallel=exact)
    b = {k: v.to(dev) for k, v in _shard(batch, counts, rank).items()}
    out = net(b['x_t1'], b['x_t2'])
    loss = trainers.step_loss(cfg, out, b, net)
    loss.backward()
    torch.cuda.synchronize()
    torch.save(_result(net, loss, out), os.path.join(out_dir, f'rank{rank}.pt'))
    torch.distributed.destroy_process_group()


def _two_ranks(case):
    with tempfile.TemporaryDirectory() as d:
        mp.spawn(_worker, args=(2, _free_port(), d, case), nprocs=2, join=True)
        res = [torch.load(os.path.join(d, f'rank{r}.pt'), weights_only=True) for r in range(2)]
    for n, v in res[0]['buffers'].items():  # replicas must not drift: the same bits on both ranks
        assert torch.equal(v, res[1]['buffers'][n]), n
    return res


def _kinks(model, P, batch, ocfg):
    from _parity import record_kinks
    from oracle import siamese_oracle as O
    return record_kinks(model, P, O.fresh_buffers(O.param_shapes(model, ocfg)), batch, ocfg, torch.float32, 1e-6)


def _check(res, ref_outs, ref_losses, ref_grads, ref_buffers, kinks):
    """The bars of tests/test_exact_dp_gpu.py; ref_losses: per rank."""
    from _parity import KINK_MAX_ERR, check_gradients
    from oracle.golden import rel_err
    for i, ref in enumerate(ref_outs):
        got = np.concatenate([r['outs'][i].numpy() for r in res])
        e = rel_err(got, ref)
        print(f'output {i}: rel err {e:.2e}')
        assert e < 1e-4
    for r, ref in zip(res, ref_losses):
        print(f"loss {r['loss']:.7f} ref {ref:.7f}")
        assert abs(r['loss'] - ref) < 1e-5
    order = [k for k in res[0]['grads'] if k in ref_grads]
    assert set(order) == set(ref_grads)
    # check_gradients places a kink at its BatchNorm's `.weight`, so that module's own `.bias`, next in the order, counts
    # as downstream of it.  It is not: dbeta is the sum of dz = da * [z > 0] over exactly the kink-ambiguous outputs z.
    # Such a beta is held to the rule's bar for a tensor upstream of a kink (dtsiamese_t32-64:
    # decoder_sem.up_seq.up1.conv.conv.4, |z| 2.5e-7 of its maximum, beta 1.957e-3 from the fixture -- and 1.957e-3 too
    # when ONE process takes the whole batch through plain BatchNorm: the ReLU decision, not the synchronization)
    own_beta = {kk[0] + '.bias' for kk in kinks}
    for r in res:
        bad = check_gradients(r['grads'], ref_grads, order, {k: 1e-3 for k in order}, kinks)
        assert not [(k, e) for k, e in bad if not (k in own_beta and e < KINK_MAX_ERR)], bad
    for n, v in ref_buffers.items():
        got = res[0]['buffers'][n].numpy()
        if n.endswith('num_batches_tracked'):
            assert int(got) == int(v), n
        else:
            assert rel_err(got, v) < 1e-5, n


@pytest.mark.timeout(300)
@pytest.mark.parametrize('name', FIXTURES)
def test_two_ranks_of_one_sample_match_the_full_batch_fixture(name):
    from oracle.golden import Fixture
    fx = Fixture(name)
    res = _two_ranks(name)
    _, ocfg, model, P, batch, _, _, _ = _setup(name)
    _check(res, fx.outputs, [float(fx.z['loss0'])] * 2, {k: torch.from_numpy(v) for k, v in fx.grads.items()},
           fx.prefixed('r1/'), _kinks(model, P, batch, ocfg))


def _one_process(case):
    """The whole batch in one process with plain BatchNorm: (outputs, per-rank losses, gradients, buffers)."""
    from multimodal_siamese_cd_amd import hip, trainers
    hip.load_library()
    dev = torch.device('cuda:0')
    cfg, _, _, P, batch, counts, exact, _ = _setup(case)
    net = _net(cfg, P, dev)
    b = {k: v.to(dev) for k, v in batch.items()}
    out = net(b['x_t1'], b['x_t2'])
    if exact:
        loss = trainers.step_loss(cfg, out, b)
        losses = [loss.item()] * len(counts)
    else:  # DDP's default: every rank's own loss, gradients averaged -- the gradient of the mean of the losses
        parts = []
        for r in range(len(counts)):
            lo = sum(counts[:r])
            o = [t[lo:lo + counts[r]] for t in _outs(out)]
            parts.append(trainers.step_loss(cfg, o if len(o) > 1 else o[0], {k: v.to(dev) for k, v in
                                                                             _shard(batch, counts, r).items()}))
        loss = sum(parts) / len(parts)
        losses = [p.item() for p in parts]
    loss.backward()
    torch.cuda.synchronize()
    r = _result(net, loss, out)
    return r['outs'], losses, r['grads'], r['buffers']


@pytest.mark.timeout(300)
@pytest.mark.parametrize('case', ['avg', 'uneven'])
def test_two_ranks_match_one_process_on_the_whole_batch(case):
    res = _two_ranks(case)
    outs, losses, grads, buffers = _one_process(case)
    _, ocfg, model, P, batch, _, _, _ = _setup(case)
    _check(res, [o.numpy() for o in outs], losses, grads, {n: v.numpy() for n, v in buffers.items()},
           _kinks(model, P, batch, ocfg))


@pytest.mark.timeout(300)
def test_bf16_two_ranks_match_one_process_on_the_whole_batch():
    from oracle.golden import rel_err
    res = _two_ranks('bf16')
    outs, losses, grads, buffers = _one_process('bf16')
    worst_out = max(rel_err(np.concatenate([r['outs'][i].numpy() for r in res]), o.numpy()) for i, o in enumerate(outs))
    worst_loss = max(abs(r['loss'] - ref) for r, ref in zip(res, losses))
    worst_cos = 1.0
    for r in res:
        for k, g in grads.items():
            if k.endswith(('conv.0.bias', 'conv.3.bias')):
                continue
            a, b = r['grads'][k].double().flatten(), g.double().flatten()
            worst_cos = min(worst_cos, float(torch.dot(a, b) / (a.norm() * b.norm())))
    worst_stat = max(rel_err(res[0]['buffers'][n].numpy(), v.numpy()) for n, v in buffers.items()
                     if not n.endswith('num_batches_tracked'))
    print(f'bf16 sync BN, 2 ranks vs one process: outputs {worst_out:.2e}, loss {worst_loss:.2e}, worst gradient '
          f'cosine {worst_cos:.5f}, running statistics {worst_stat:.2e}')
    assert worst_out < 3e-2 and worst_loss < 1e-2 and worst_cos > 0.95


# ---------------------------------------------------------------------------------------------------------------------
# one process: a converted model runs exactly as before
# ---------------------------------------------------------------------------------------------------------------------
def _step(net, cfg, batch, dev):
    from multimodal_siamese_cd_amd import trainers
    b = {k: v.to(dev) for k, v in batch.items()}
    out = net(b['x_t1'], b['x_t2'])
    loss = trainers.step_loss(cfg, out, b)
    loss.backward()
    torch.cuda.synchronize()
    return _result(net, loss, out)


def _same(a, b):
    assert a['loss'] == b['loss']
    for x, y in zip(a['outs'], b['outs']):
        assert torch.equal(x, y)
    for key in ('grads', 'buffers'):
        assert set(a[key]) == set(b[key])
        for n, v in a[key].items():
            assert torch.equal(v, b[key][n]), n


def _converted(cfg, P, dev, conv):
    from multimodal_siamese_cd_amd.utils import networks
    net = _net(cfg, P, dev)
    keys, ids = list(net.state_dict()), {k: id(p) for k, p in net.named_parameters()}
    if conv == 'torch':
        net = torch.nn.SyncBatchNorm.convert_sync_batchnorm(net)
        assert any(isinstance(m, torch.nn.SyncBatchNorm) for m in net.modules())
    else:
        assert networks.convert_sync_batchnorm(net) is net
        marked = [m for m in net.modules() if getattr(m, 'scd_sync', False)]
        assert marked and all(type(m) is torch.nn.BatchNorm2d for m in marked)
        assert len(marked) == sum(isinstance(m, torch.nn.BatchNorm2d) for m in net.modules())
    # in place: parameters keep their identity, state_dict keys (checkpoints) do not change
    assert ids == {k: id(p) for k, p in net.named_parameters()} and list(net.state_dict()) == keys
    return net


@pytest.mark.parametrize('conv', ['ours', 'torch'])
@pytest.mark.parametrize('name', ['siamese_t8-16', 'siamese_t12-20'])
def test_converted_model_is_bit_identical_in_one_process(name, conv):
    """Not distributed: the existing path, with or without freeze_batchnorm (which reaches torch's SyncBatchNorm too)."""
    from multimodal_siamese_cd_amd import hip
    from multimodal_siamese_cd_amd.utils import networks
    hip.load_library()
    dev = torch.device('cuda:0')
    cfg, _, _, P, batch, _, _, _ = _setup(name)
    plain = _step(_net(cfg, P, dev), cfg, batch, dev)
    _same(plain, _step(_converted(cfg, P, dev, conv), cfg, batch, dev))
    frozen = _step(networks.freeze_batchnorm(_net(cfg, P, dev)), cfg, batch, dev)
    net = networks.freeze_batchnorm(_converted(cfg, P, dev, conv))
    assert not any(m.training for m in net.modules() if isinstance(m, torch.nn.modules.batchnorm._BatchNorm))
    _same(frozen, _step(net, cfg, batch, dev))
    assert frozen['loss'] != plain['loss']


def test_frozen_converted_model_matches_the_frozen_fixture():
    """freeze_batchnorm on a converted model gives the frozen path the reference's frozen fixture pins."""
    from multimodal_siamese_cd_amd import hip
    from multimodal_siamese_cd_amd.utils import networks
    from oracle.golden import Fixture, rel_err
    from test_frozen_bn_golden import load_frozen
    hip.load_library()
    dev = torch.device('cuda:0')
    z, meta = load_frozen('siamese_t8-16')
    fx = Fixture(meta['base'])
    cfg = fx.package_cfg()
    net = _net(cfg, {k: torch.from_numpy(v.copy()) for k, v in fx.params0.items()}, dev)
    with torch.no_grad():
        bufs = dict(net.module.named_buffers())
        for k, v in fx.prefixed('r1/').items():
            bufs[k].copy_(torch.from_numpy(v))
    networks.freeze_batchnorm(networks.convert_sync_batchnorm(net))
    r = _step(net, cfg, fx.batch(), dev)
    assert rel_err(r['outs'][0].numpy(), z['out/0']) < 1e-4
    assert abs(r['loss'] - float(z['loss'])) < 1e-5
