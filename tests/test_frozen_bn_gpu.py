"""Model-level parity of the frozen-BatchNorm training step on MI355X: BatchNorm2d modules in eval mode inside a model
in train mode (networks.freeze_batchnorm), against fixtures the reference itself produced that way
(tests/golden/make_golden_frozen_bn.py) and against the fp64 oracle following the GPU forward's own branches.

Bars as tests/test_model_gpu.py: logits 1e-4 (masks bit-exact outside the band), loss 1e-5, every gradient within
GRAD_TOL = 1e-3 (max-relative) of the branch-matched fp64 oracle run with training=False on the same running
statistics, and within FIXTURE_L2 = 2e-2 (norm-wise) of the reference's fp32 gradients.  The conv biases in front of a
frozen BatchNorm have true gradients and are held to the same bars as every other tensor.

Two bias gradients of siamese_t8-16-32_odd (CANCELLING) are exactly zero in the reference and have no scale of their
own: at its deepest level both dates take the same ReLU decisions, so the +g / -g of the feature difference cancel
term by term.  Their error is measured against the largest gradient of the same DoubleConv, the scale of the terms
that cancel.  Every other tensor is measured against its own maximum, as everywhere else, and a zero reference for any
other tensor fails.
"""
import numpy as np
import pytest
import torch

from _parity import branch_matched_reference
from oracle.golden import Fixture, rel_err
from test_frozen_bn_golden import FROZEN, WHATEVER, load_frozen

pytestmark = pytest.mark.gpu

LOGIT_TOL = 1e-4
GRAD_TOL = 1e-3
FIXTURE_L2 = 2e-2


@pytest.fixture(scope='module')
def dev():
    from multimodal_siamese_cd_amd import hip
    hip.load_library()
    return torch.device('cuda:0')


def _outs(o):
    return list(o) if isinstance(o, (tuple, list)) else [o]


def check_logits(out, ref):
    out = out.detach().cpu().numpy()
    assert out.shape == ref.shape
    assert rel_err(out, ref) < LOGIT_TOL
    band = np.abs(ref) < LOGIT_TOL * np.abs(ref).max()
    mism = ((out > 0) != (ref > 0)) & ~band
    assert not mism.any(), f'{mism.sum()} mask pixels differ outside the tolerance band'


def _build(fx, dev, precision=None):
    """The fixture's model with its parameters p0/* and the running statistics r1/*."""
    from multimodal_siamese_cd_amd.utils import networks
    cfg = fx.package_cfg()
    if precision is not None:
        cfg.MODEL.PRECISION = precision
    net = networks.create_network(cfg)
    r1 = fx.prefixed('r1/')
    with torch.no_grad():
        for k, p in net.module.named_parameters():
            p.copy_(torch.from_numpy(fx.params0[k]))
        for k, b in net.module.named_buffers():
            b.copy_(torch.from_numpy(r1[k]))
    return cfg, net.to(dev)


def _buffers(net):
    return {k: v.detach().cpu().clone() for k, v in net.module.named_buffers()}


# the reference gradients that cancel to exactly zero (module docstring), by fixture parameter name
CANCELLING = ('encoder.down_seq.down3.mpconv.1.conv.3.bias', 'encoder.down_seq.down3.mpconv.1.conv.4.bias')


def _scale_of(k, ref: dict, norm):
    """norm(ref[k]); for the CANCELLING tensors, all zero in the reference, the largest norm among the gradients of
    the same DoubleConv.  Any other all-zero reference is an error."""
    s = norm(ref[k])
    if s > 0:
        return s
    assert k in CANCELLING, f'{k}: the reference gradient is all zero'
    pre = k[:k.rindex('conv.') + len('conv.')]
    return max(norm(v) for kk, v in ref.items() if kk.startswith(pre))


def compare_gradients(got: dict, ref: dict, bar: float, l2: bool = False, skip=()):
    """Every tensor of `ref` (pre-BatchNorm conv biases included) within `bar`; max-relative, or norm-wise."""
    norm = (lambda t: float(torch.as_tensor(t).double().norm())) if l2 else \
        (lambda t: float(torch.as_tensor(t).double().abs().max()))
    bad, worst = [], (None, 0.0)
    for k, r in ref.items():
        if k in skip:
            continue
        d = torch.as_tensor(got[k]).double().cpu() - torch.as_tensor(r).double().cpu()
        e = norm(d) / _scale_of(k, ref, norm)
        worst = max(worst, (k, e), key=lambda t: t[1])
        if not e <= bar:
            bad.append((k, e))
    print(f'gradients {"rel-L2" if l2 else "max-rel"}: worst {worst[1]:.2e} ({worst[0]}), bar {bar:.0e}')
    return bad


def _frozen_step(fx, dev, prefixes=None, precision=None):
    from multimodal_siamese_cd_amd import engine, trainers
    from multimodal_siamese_cd_amd.utils import networks
    cfg, net = _build(fx, dev, precision)
    networks.freeze_batchnorm(net.train(), prefixes)
    before = _buffers(net)
    batch = {k: v.to(dev) for k, v in fx.batch().items()}
    with engine.trace_bn() as trace:
        out = net(batch['x_t1'], batch['x_t2'])
    loss = trainers.step_loss(cfg, out, batch)
    loss.backward()
    torch.cuda.synchronize()
    got = {k: p.grad.cpu() for k, p in net.module.named_parameters() if p.grad is not None}
    return net, out, loss, got, trace, before


def _step_loss(model_type, alpha):
    from oracle import siamese_oracle as O
    return lambda out, batch: O.step_loss(model_type, out, batch, alpha)


@pytest.mark.parametrize('name', FROZEN)
def test_frozen_step_matches_reference(dev, name):
    z, meta = load_frozen(name)
    fx = Fixture(meta['base'])
    net, out, loss, got, trace, before = _frozen_step(fx, dev)
    outs = _outs(out)
    assert len(outs) == sum(k.startswith('out/') for k in z)
    for i, o in enumerate(outs):
        check_logits(o, z[f'out/{i}'])
    print(f'loss {loss.item():.7f} reference {float(z["loss"]):.7f}')
    assert abs(loss.item() - float(z['loss'])) < 1e-5
    grads = {k[2:]: torch.from_numpy(v) for k, v in z.items() if k.startswith('g/')}
    assert set(got) == set(grads)
    after = _buffers(net)
    for k, v in before.items():  # a frozen BatchNorm reads its statistics and leaves its counter alone
        assert torch.equal(after[k], v), k
        assert torch.equal(v, torch.from_numpy(fx.prefixed('r1/')[k])), k
    if fx.model_type not in WHATEVER:  # (their eval-mode oracle has one output: the branch-matched bar is below)
        P = {k: torch.from_numpy(v.copy()) for k, v in fx.params0.items()}
        B = {k: torch.from_numpy(v.copy()) for k, v in fx.prefixed('r1/').items()}
        _, lref, ref = branch_matched_reference(fx.model_type, P, fx.batch(), fx.cfg, trace, net.module,
                                                _step_loss(fx.model_type, fx.meta['alpha']), training=False, buffers=B)
        assert abs(loss.item() - lref.item()) < 1e-5
        assert set(ref) == set(got)
        assert not compare_gradients(got, ref, GRAD_TOL)
    assert not compare_gradients(got, grads, FIXTURE_L2, l2=True)


@pytest.mark.parametrize('name', ['whatevernet_t8-16', 'whatevernet2_t8-16'])
def test_whatevernet_eval_mode_backward(dev, name):
    """Whole-model net.eval(): one output (the fusion head), every BatchNorm on its running statistics; the
    supervised loss on it, differentiated, at the branch-matched bar."""
    from multimodal_siamese_cd_amd import engine
    from multimodal_siamese_cd_amd.utils import loss_functions
    from oracle import siamese_oracle as O
    fx = Fixture(name)
    _, net = _build(fx, dev)
    net.eval()
    before = _buffers(net)
    batch = {k: v.to(dev) for k, v in fx.batch().items()}
    with engine.trace_bn() as trace:
        out = net(batch['x_t1'], batch['x_t2'])
    assert isinstance(out, torch.Tensor)
    loss = loss_functions.get_criterion('PowerJaccardLoss')(out, batch['y_change'])
    loss.backward()
    got = {k: p.grad.cpu() for k, p in net.module.named_parameters() if p.grad is not None}
    P = {k: torch.from_numpy(v.copy()) for k, v in fx.params0.items()}
    B = {k: torch.from_numpy(v.copy()) for k, v in fx.prefixed('r1/').items()}
    oref, lref, ref = branch_matched_reference(fx.model_type, P, fx.batch(), fx.cfg, trace, net.module,
                                               lambda o, b: O.power_jaccard_loss(o, b['y_change']), training=False,
                                               buffers=B)
    check_logits(out, oref.detach().float().numpy())
    assert abs(loss.item() - lref.item()) < 1e-5
    # the two stream heads are not part of eval mode's output: as in torch, their gradients stay None
    assert {f'outc_stream{s}.conv.{p}' for s in (1, 2) for p in ('weight', 'bias')}.isdisjoint(got)
    assert set(ref) == set(got)
    assert not compare_gradients(got, ref, GRAD_TOL)
    for k, v in _buffers(net).items():
        assert torch.equal(v, before[k]), k


def test_heads_only_fine_tuning(dev):
    """Only the heads train (every other parameter requires_grad False) over frozen BatchNorms: the decoder stages
    save nothing for a backward of their own, yet the heads' backward finds their last BatchNorm's state, and the
    heads' gradients are the full frozen step's (the fixture's, at its bar)."""
    from multimodal_siamese_cd_amd import trainers
    from multimodal_siamese_cd_amd.utils import networks
    z, meta = load_frozen('whatevernet_t8-16')
    fx = Fixture(meta['base'])
    cfg, net = _build(fx, dev)
    for k, p in net.module.named_parameters():
        p.requires_grad_(k.startswith('outc_'))
    networks.freeze_batchnorm(net.train())
    batch = {k: v.to(dev) for k, v in fx.batch().items()}
    trainers.step_loss(cfg, net(batch['x_t1'], batch['x_t2']), batch).backward()
    got = {k: p.grad.cpu() for k, p in net.module.named_parameters() if p.grad is not None}
    grads = {k[2:]: torch.from_numpy(v) for k, v in z.items() if k.startswith('g/outc_')}
    assert set(got) == set(grads) and len(grads) == 6
    assert not compare_gradients(got, grads, FIXTURE_L2, l2=True)


def test_mixed_frozen_encoder_training_decoder(dev):
    """Only the BatchNorms under inc. / encoder. frozen: their buffers stay, the decoder's are updated once.  The
    fixture bars; the conv biases in front of the decoder's train-mode BatchNorms have a true gradient of zero (float
    noise on both sides) and are checked for being ~0, as tests/test_model_gpu.py does."""
    z, meta = load_frozen('enc_siamese_t8-16')
    fx = Fixture(meta['base'])
    net, out, loss, got, _, before = _frozen_step(fx, dev, meta['frozen_prefixes'])
    check_logits(out, z['out/0'])
    assert abs(loss.item() - float(z['loss'])) < 1e-5
    grads = {k[2:]: torch.from_numpy(v) for k, v in z.items() if k.startswith('g/')}
    assert set(got) == set(grads)
    noise = [k for k in grads if k.startswith('decoder.') and k.endswith(('conv.0.bias', 'conv.3.bias'))]
    assert len(noise) == 2 * sum(k.endswith('.up.weight') for k in grads)  # two per Up's DoubleConv
    for k in noise:
        wmax = float(grads[k.replace('.bias', '.weight')].abs().max())
        assert float(got[k].abs().max()) < 1e-4 * max(wmax, 1e-3), k
    assert not compare_gradients(got, grads, FIXTURE_L2, l2=True, skip=noise)
    after = _buffers(net)
    for k, v in after.items():
        ref = z['r/' + k]
        if k.startswith(('inc.', 'encoder.')):
            assert torch.equal(v, before[k]), k
        if k.endswith('num_batches_tracked'):
            assert int(v) == int(ref), k
        else:
            assert rel_err(v.numpy(), ref) < 1e-5, k


def _launches(net, cfg, batch, monkeypatch, dev):
    """One step's conv launches: (record_arith's list, per weight grad whether it forms a BatchNorm backward's dy
    (scd_wgrad_t.rows_y), per igemm whether it records BatchNorm statistics / BatchNorm-backward sums)."""
    from _parity import record_arith
    from multimodal_siamese_cd_amd import hip, trainers
    seen = record_arith(monkeypatch, dev)
    fused_wgrad, stat_rec, bn_bwd_rec = [], [], []
    inner_wgrad, inner_igemm = hip.conv_wgrad, hip.conv_igemm

    def wgrad(d, slabs):
        fused_wgrad.append(bool(d.rows_y.data))
        return inner_wgrad(d, slabs)

    def igemm(*a, **kw):
        stat_rec.append(kw.get('stat_rec') is not None)
        bn_bwd_rec.append(kw.get('bn_bwd') is not None)
        return inner_igemm(*a, **kw)

    monkeypatch.setattr(hip, 'conv_wgrad', wgrad)
    monkeypatch.setattr(hip, 'conv_igemm', igemm)
    net.zero_grad(set_to_none=True)
    trainers.step_loss(cfg, net(batch['x_t1'], batch['x_t2']), batch).backward()
    monkeypatch.undo()
    return seen, fused_wgrad, stat_rec, bn_bwd_rec


@pytest.mark.parametrize('topology', [[32, 64], [64, 128]])
def test_frozen_step_reaches_the_h2_and_fused_kernels(dev, monkeypatch, topology):
    """The frozen step takes the production kernels wherever the train-mode step does -- a silent fallback to the
    generic ones must not pass unnoticed.  On siamese_t32-64 ([32, 64]) and on the same model at [64, 128]:
      - every conv launch runs the arithmetic it would with bounds on all operands, and the 3x3 convs with
        32-channel-multiple sources and >= 64 outputs run h2;
      - the weight grads that form a BatchNorm backward's dy themselves (scd_wgrad_t.rows_y) and the data grads that
        record its tile sums are the train-mode step's, launch for launch, and the arithmetic of every launch is too;
      - no conv records statistics for a frozen BatchNorm (train mode: one per BatchNorm).
    At least one data grad records the sums on both; at least one weight grad forms dy at [64, 128].  At [32, 64]
    none can, frozen or not (measured: 0 of 12 in both modes): under h2 that weight grad needs 128 rows
    (wgrad_halo_rbn_ok), the widest layer has 64, and the 16-channel input-layer kernel needs 64 (wgrad_halo_shape)
    where inc has 32 -- which is why the second topology is here."""
    from multimodal_siamese_cd_amd.utils import networks
    fx = Fixture('siamese_t32-64')
    if topology == fx.cfg['TOPOLOGY']:
        cfg, net = _build(fx, dev)
    else:
        cfg = fx.package_cfg()
        cfg.MODEL.TOPOLOGY = topology
        torch.manual_seed(3)
        net = networks.create_network(cfg).to(dev)
    assert net.module.conv_math == 'h2'
    batch = {k: v.to(dev) for k, v in fx.batch().items()}
    networks.freeze_batchnorm(net.train())
    seen, fused_wgrad, stat_rec, bn_bwd_rec = _launches(net, cfg, batch, monkeypatch, dev)
    assert all(torch.isfinite(p.grad).all() for p in net.parameters())
    seen_t, fused_wgrad_t, stat_rec_t, bn_bwd_rec_t = _launches(net.train(), cfg, batch, monkeypatch, dev)
    print(f'{topology}: {sum(s[4] == "h2" for s in seen)} of {len(seen)} conv launches run h2; weight grads forming a '
          f'BatchNorm backward: frozen {sum(fused_wgrad)} of {len(fused_wgrad)}, train {sum(fused_wgrad_t)} of '
          f'{len(fused_wgrad_t)}; data grads recording its sums: frozen {sum(bn_bwd_rec)}, train {sum(bn_bwd_rec_t)}; '
          f'convs recording statistics: frozen {sum(stat_rec)}, train {sum(stat_rec_t)}')
    assert all(s[4] == s[5] for s in seen), [s for s in seen if s[4] != s[5]]
    h2 = [s for s in seen if s[3] == 9 and s[1] % 32 == 0 and s[2] % 64 == 0]
    assert h2 and all(s[4] == 'h2' for s in h2), [s for s in h2 if s[4] != 'h2']
    assert seen == seen_t
    assert fused_wgrad == fused_wgrad_t and bn_bwd_rec == bn_bwd_rec_t
    assert any(bn_bwd_rec)
    assert any(stat_rec_t) and not any(stat_rec)
    if topology == [64, 128]:
        assert any(fused_wgrad)


def _bf16_oracle_forward(fx, P, B, bf16_convs: set):
    """The fp32 oracle's eval-mode forward with the bf16 kernels' arithmetic in the 3x3 convs that ran it, as
    tests/test_bf16_gpu.py emulates it (_Conv16: bf16-rounded operands, exact products; convT_bf16); fp32 storage, which
    is what a TOPOLOGY off the 64-channel granule runs in (engine.act_storage_for).  `bf16_convs`: the (source
    channels as read, outputs) of the 3x3 launches that reported bf16 -- at [32, 64] not every conv with a
    32-channel-multiple source has a bf16 kernel, and the emulation follows the launches, not a rule of its own."""
    import torch.nn.functional as F
    import test_bf16_gpu as T
    from oracle import siamese_oracle as O

    def conv(x, w, b=None, stride=1, padding=0, *a, **k):
        cin = 16 if w.shape[1] <= 16 else w.shape[1]  # the input layer's bands, zero-padded to the 16-channel kernel
        if w.shape[2:] == (3, 3) and (cin, w.shape[0]) in bf16_convs and stride == 1 and padding == 1:
            return T._Conv16.apply(x, w, b)
        return T._CONV2D(x, w, b, stride, padding, *a, **k)

    b = fx.batch()
    F.conv2d, F.conv_transpose2d = conv, T.convT_bf16
    try:
        with torch.no_grad():
            return O.forward(fx.model_type, P, B, b['x_t1'], b['x_t2'], fx.cfg, training=False)
    finally:
        F.conv2d, F.conv_transpose2d = T._CONV2D, T._CONVT2D


def test_frozen_step_bf16(dev, monkeypatch):
    """siamese_t32-64 under MODEL.PRECISION bf16, at the bars of tests/test_bf16_gpu.py's model step: logits within
    3e-2 of the fp32 reference and closer to the oracle with the bf16 arithmetic emulated in its convs, loss within
    1e-2, every gradient with cosine similarity > 0.95 to the fp32 one -- the pre-BatchNorm conv biases included."""
    from _parity import record_arith, rel
    z, meta = load_frozen('siamese_t32-64')
    fx = Fixture(meta['base'])
    seen = record_arith(monkeypatch, dev)
    net, out, loss, got, _, before = _frozen_step(fx, dev, precision='bf16')
    monkeypatch.undo()
    assert net.module.conv_math == 'bf16'
    bf16_convs = {(s[1], s[2]) for s in seen if s[0] == 'igemm' and s[3] == 9 and s[4] == 'bf16'}
    print('3x3 launches by arithmetic:', sorted({(s[1], s[2], s[4]) for s in seen if s[0] == 'igemm' and s[3] == 9}))
    assert bf16_convs
    P = {k: torch.from_numpy(v.copy()) for k, v in fx.params0.items()}
    B = {k: torch.from_numpy(v.copy()) for k, v in fx.prefixed('r1/').items()}
    out16 = _bf16_oracle_forward(fx, P, B, bf16_convs)
    e16, e32 = rel(out, out16), rel(out, z['out/0'])
    print(f'bf16 logits rel err vs emulated {e16:.2e}, vs fp32 {e32:.2e}; loss {loss.item():.6f} fp32 '
          f'{float(z["loss"]):.6f}')
    worst = (None, 1.0)
    for k, v in z.items():
        if not k.startswith('g/'):
            continue
        a, r = got[k[2:]].double().flatten(), torch.from_numpy(v).double().flatten()
        cs = float(torch.dot(a, r) / (a.norm() * r.norm()))
        worst = min(worst, (k[2:], cs), key=lambda t: t[1])
    print(f'bf16 worst gradient cosine similarity {worst[1]:.4f} ({worst[0]})')
    assert e32 < 3e-2
    assert e16 < e32
    assert abs(loss.item() - float(z['loss'])) < 1e-2
    assert worst[1] > 0.95, worst
    for k, v in _buffers(net).items():
        assert torch.equal(v, before[k]), k


def test_training_loop_freeze_bn(dev, monkeypatch):
    """Two steps of train_supervised.run_training with TRAINER.FREEZE_BN: True (an evaluation, hence a net.eval() /
    net.train() round trip, between them): every BatchNorm buffer bit-identical, the weights moved."""
    from multimodal_siamese_cd_amd import train_supervised
    from multimodal_siamese_cd_amd.utils import experiment_manager as em, networks
    cfg = em.load_cfg('debug')
    cfg.DEBUG = False
    cfg.TRAINER.EPOCHS = 1
    cfg.TRAINER.STEPS_PER_EPOCH = 2
    cfg.TRAINER.FREEZE_BN = True
    cfg.LOG_FREQ = 1
    cfg.EVAL_SAMPLES = 1
    cfg.SAVE_CHECKPOINTS = []
    start = {}
    create = networks.create_network

    def create_and_record(c):
        net = create(c)
        # statistics a train-mode step would visibly move; a mean below the freshly initialised convs' outputs keeps
        # the ReLUs alive (above them every gradient is zero and only weight decay moves anything)
        with torch.no_grad():
            for k, b in net.named_buffers():
                if k.endswith('running_mean'):
                    b.fill_(-0.25)
                elif k.endswith('running_var'):
                    b.fill_(1.5)
        start.update({k: v.detach().clone() for k, v in net.state_dict().items()})
        return net

    monkeypatch.setattr(networks, 'create_network', create_and_record)
    net, _, steps = train_supervised.run_training(cfg, dev)
    assert steps == 2
    buffers = {k for k, _ in net.named_buffers()}
    assert buffers
    moved = 0
    for k, v in net.state_dict().items():
        if k in buffers:
            assert torch.equal(v.cpu(), start[k].cpu()), k
        else:
            moved += int(not torch.equal(v.cpu(), start[k].cpu()))
    assert moved == len(start) - len(buffers)
