"""A frozen parameter (requires_grad False) costs nothing in the backward: the stage Functions read
ctx.needs_input_grad per parameter, so no weight grad and no reduction is launched for a gradient without a reader, a
frozen BatchNorm whose gamma, beta and conv bias in front are frozen runs the reduction-free scd_bn_relu_through, and
the walk stops where the last reader is (engine option skip_frozen_grads, default on).

No result changes, so every number here is held to the bar the same fixture already has elsewhere:
  GRAD_TOL 1e-3 (max-relative) against the fp64 oracle following the GPU forward's own branches and FIXTURE_L2 2e-2
  (norm-wise) against the reference's fp32 fixtures (tests/test_model_gpu.py, tests/test_input_grad_gpu.py,
  tests/test_frozen_bn_gpu.py); BF16_L2 / BF16_COS for the bf16 config (tests/test_input_grad_gpu.py).
The launches are counted by spies on the hip bindings, in the style of test_frozen_bn_gpu._launches."""
import pytest
import torch

import test_frozen_bn_gpu as FB
import test_input_grad_gpu as IG
from _parity import branch_matched_reference, check_branch_matched, record_arith, rel, rel_l2
from oracle.golden import Fixture
from test_frozen_bn_golden import load_frozen
from test_input_grad_golden import EVAL, load_input_grad, oracle_input_grads

pytestmark = pytest.mark.gpu

GRAD_TOL = IG.GRAD_TOL
FIXTURE_L2 = IG.FIXTURE_L2
REDUCING = ('bn_relu_backward', 'bn_relu_backward_pooled', 'bn_relu_backward_pooled2', 'bn_relu_backward_head',
            'bn_relu_backward_tiles', 'bn_relu_backward_coef')
OTHER = ('bn_relu_through', 'wgrad_finalize', 'wgrad_colsum_finalize', 'channel_sum', 'conv1x1_bwd_bn', 'conv1x1_bwd')


@pytest.fixture(scope='module')
def dev():
    from multimodal_siamese_cd_amd import hip
    hip.load_library()
    return torch.device('cuda:0')


class Spy:
    """record_arith's conv launch list (`seen`) and, in order, the name of every call of the bindings a backward's
    gradient work goes through (`calls`).  `mark()` after the forward: `bwd_*` are the backward's."""

    def __init__(self, monkeypatch, dev):
        from multimodal_siamese_cd_amd import hip
        self.mp = monkeypatch
        self.seen = record_arith(monkeypatch, dev)
        self.calls = []
        for name in ('conv_igemm', 'conv_wgrad') + REDUCING + OTHER:
            monkeypatch.setattr(hip, name, self._wrap(name, getattr(hip, name)))
        self.n_seen = self.n_calls = 0

    def _wrap(self, name, inner):
        def call(*a, **kw):
            if name == 'conv_igemm':
                self.calls.append(('conv_igemm', kw.get('bn_bwd') is not None))
            else:
                self.calls.append(name)
            return inner(*a, **kw)
        return call

    def mark(self):
        self.n_seen, self.n_calls = len(self.seen), len(self.calls)

    def done(self):
        torch.cuda.synchronize()
        self.mp.undo()
        return self

    @property
    def bwd_seen(self):
        return self.seen[self.n_seen:]

    @property
    def bwd_calls(self):
        return self.calls[self.n_calls:]

    def count(self, *names, bwd=True):
        return sum(c in names for c in (self.bwd_calls if bwd else self.calls))

    def wgrads(self):
        return self.count('conv_wgrad', bwd=False)

    def summary(self):
        names = ('conv_wgrad', 'wgrad_finalize', 'bn_relu_through') + REDUCING
        return {n: self.count(n, bwd=False) for n in names if self.count(n, bwd=False)}


def _n_bn(net):
    return sum(isinstance(m, torch.nn.BatchNorm2d) for m in net.modules())


def _params(net):
    return dict(net.module.named_parameters())


def _cpu_params(net):
    return {k: p.detach().cpu().clone() for k, p in net.module.named_parameters()}


def _cpu_buffers(net):
    return {k: b.detach().cpu().clone() for k, b in net.module.named_buffers()}


def _loss(cfg, out, batch):
    from multimodal_siamese_cd_amd import trainers
    from multimodal_siamese_cd_amd.utils import loss_functions
    if isinstance(out, torch.Tensor):
        return loss_functions.get_criterion('PowerJaccardLoss')(out, batch['y_change'])
    return trainers.step_loss(cfg, out, batch)


def _oracle_loss(fx):
    from oracle import siamese_oracle as O

    def loss(out, batch):
        if isinstance(out, torch.Tensor):
            return O.power_jaccard_loss(out, batch['y_change'])
        return O.step_loss(fx.model_type, out, batch, fx.meta['alpha'])
    return loss


def _saliency(fx, dev, net, cfg, monkeypatch):
    """net.eval(), every parameter frozen, both inputs requiring grad; one forward + torch.autograd.grad under the
    spies.  (loss, g1, g2, trace, spy)."""
    from multimodal_siamese_cd_amd import engine
    from multimodal_siamese_cd_amd.utils import networks
    net.eval()
    frozen = networks.freeze_parameters(net)
    assert len(frozen) == len(list(net.module.parameters()))
    batch = {k: v.to(dev) for k, v in fx.batch().items()}
    x1 = batch['x_t1'].clone().requires_grad_()
    x2 = batch['x_t2'].clone().requires_grad_()
    spy = Spy(monkeypatch, dev)
    with engine.trace_bn() as trace:
        out = net(x1, x2)
    loss = _loss(cfg, out, batch)
    spy.mark()
    g1, g2 = torch.autograd.grad(loss, [x1, x2])
    spy.done()
    assert all(p.grad is None for p in net.module.parameters())
    return loss, g1, g2, trace, spy


def _assert_saliency_launches(spy, net):
    print('launches:', spy.summary())
    assert spy.count('conv_wgrad', 'wgrad_finalize', 'wgrad_colsum_finalize', 'channel_sum', bwd=False) == 0
    assert spy.count(*REDUCING, bwd=False) == 0
    assert spy.count('conv1x1_bwd_bn') == 0  # no head weight or bias grad
    assert spy.count('bn_relu_through') == _n_bn(net)  # one per BatchNorm on the path
    assert not any(c[1] for c in spy.bwd_calls if isinstance(c, tuple))  # no data grad records sums nobody reads


def _oracle_inputs(fx, net, trace, P, B, ocfg=None):
    return IG.branch_matched_input_reference(fx.model_type, P, fx.batch(), ocfg or fx.cfg, trace, net.module,
                                             _oracle_loss(fx), training=False, buffers=B)


def test_saliency_launches_no_weight_grad_and_no_reduction(dev, monkeypatch):
    """1. inputgrad_eval_siamese_t8-16: the input gradients at that fixture's bars, from a backward without a single
    weight grad, finalize or reducing BatchNorm backward."""
    z, meta = load_input_grad(EVAL)
    fx = Fixture(meta['base'])
    cfg, net = IG._build(fx, dev, eval_buffers=True)
    loss, g1, g2, trace, spy = _saliency(fx, dev, net, cfg, monkeypatch)
    _assert_saliency_launches(spy, net)
    assert abs(loss.item() - float(z['loss'])) < 1e-5
    P = {k: torch.from_numpy(v.copy()) for k, v in fx.params0.items()}
    B = {k: torch.from_numpy(v.copy()) for k, v in fx.prefixed('r1/').items()}
    lref, _, r1, r2 = _oracle_inputs(fx, net, trace, P, B)
    assert abs(loss.item() - lref.item()) < 1e-5
    for name, g, r in (('x_t1', g1, r1), ('x_t2', g2, r2)):
        e, e2 = rel(g, r), rel_l2(g, z['gx/' + name])
        print(f'{name}: max-relative vs the branch-matched oracle {e:.2e}, rel-L2 vs the reference fixture {e2:.2e}')
        assert e <= GRAD_TOL and e2 <= FIXTURE_L2


@pytest.mark.parametrize('topology', [[32, 64], [64, 128]])
def test_saliency_on_the_production_kernels(dev, monkeypatch, topology):
    """2. siamese_t32-64 and the same model at [64, 128] (built as test_frozen_step_reaches_the_h2_and_fused_kernels
    builds it), eval mode on the model's buffers: the backward's 3x3 data grads with 32-channel-multiple sources and
    >= 64 outputs run h2 -- they read the through pass' dy by its dy_bound, and an understated one would overflow
    fp16 -- every gradient is finite and within GRAD_TOL of the branch-matched oracle."""
    from multimodal_siamese_cd_amd.utils import networks
    fx = Fixture('siamese_t32-64')
    if topology == fx.cfg['TOPOLOGY']:
        cfg, net = IG._build(fx, dev, eval_buffers=True)
        ocfg = fx.cfg
    else:
        cfg = fx.package_cfg()
        cfg.MODEL.TOPOLOGY = topology
        torch.manual_seed(3)
        net = networks.create_network(cfg).to(dev)
        ocfg = dict(fx.cfg, TOPOLOGY=topology)
    assert net.module.conv_math == 'h2'
    P, B = _cpu_params(net), _cpu_buffers(net)
    loss, g1, g2, trace, spy = _saliency(fx, dev, net, cfg, monkeypatch)
    _assert_saliency_launches(spy, net)
    dgrads = [s for s in spy.bwd_seen if s[0] == 'igemm' and s[3] == 9]
    h2 = [s for s in dgrads if s[1] % 32 == 0 and s[2] >= 64]
    print(f'{topology}: backward 3x3 data grads {[(s[1], s[2], s[4]) for s in dgrads]}')
    assert h2 and all(s[4] == 'h2' for s in h2), [s for s in h2 if s[4] != 'h2']
    assert all(s[4] == s[5] for s in spy.bwd_seen), [s for s in spy.bwd_seen if s[4] != s[5]]
    assert torch.isfinite(g1).all() and torch.isfinite(g2).all() and float(g1.abs().max()) > 0
    lref, _, r1, r2 = _oracle_inputs(fx, net, trace, P, B, ocfg)
    assert abs(loss.item() - lref.item()) < 1e-5
    for name, g, r in (('x_t1', g1, r1), ('x_t2', g2, r2)):
        e = rel(g, r)
        print(f'{topology} {name}: max-relative vs the branch-matched oracle {e:.2e}, bar {GRAD_TOL:.0e}')
        assert e <= GRAD_TOL


def _train_step(net, cfg, batch, monkeypatch, dev, trace=False):
    """zero_grad, forward, step loss, backward under the spies: (out, loss, {name: grad}, BatchNorm trace, spy)."""
    from multimodal_siamese_cd_amd import engine
    net.zero_grad(set_to_none=True)
    spy = Spy(monkeypatch, dev)
    with engine.trace_bn() as tr:
        out = net(batch['x_t1'], batch['x_t2'])
    loss = _loss(cfg, out, batch)
    spy.mark()
    loss.backward()
    spy.done()
    got = {k: p.grad.cpu() for k, p in net.module.named_parameters() if p.grad is not None}
    return out, loss, got, (tr if trace else None), spy


def _conv_weights(net, trainable_only=True):
    """The weights whose gradient is a conv_wgrad launch: every 3x3 Conv2d's and every ConvTranspose2d's."""
    ws = [m.weight for m in net.modules()
          if (isinstance(m, torch.nn.Conv2d) and m.kernel_size == (3, 3)) or isinstance(m, torch.nn.ConvTranspose2d)]
    return [w for w in ws if w.requires_grad or not trainable_only]


def test_frozen_encoder_training_decoder(dev, monkeypatch):
    """3. freeze_parameters + freeze_batchnorm on inc. / encoder. (frozenbn_enc_siamese_t8-16): the decoder's and the
    head's gradients at test_mixed_frozen_encoder_training_decoder's bars, one weight grad per trainable conv / ConvT
    weight, and no ConvT data grad into the deepest feature, which nobody reads."""
    from multimodal_siamese_cd_amd.utils import networks
    z, meta = load_frozen('enc_siamese_t8-16')
    fx = Fixture(meta['base'])
    prefixes = meta['frozen_prefixes']
    assert sorted(prefixes) == ['encoder.', 'inc.']
    cfg, net = FB._build(fx, dev)
    frozen = networks.freeze_parameters(net, prefixes)
    assert frozen and all(k.startswith(tuple(prefixes)) for k in frozen)
    assert set(frozen) == {k for k in _params(net) if k.startswith(tuple(prefixes))}
    networks.freeze_batchnorm(net.train(), prefixes)
    batch = {k: v.to(dev) for k, v in fx.batch().items()}
    out, loss, got, _, spy = _train_step(net, cfg, batch, monkeypatch, dev)
    FB.check_logits(out, z['out/0'])
    assert abs(loss.item() - float(z['loss'])) < 1e-5
    grads = {k[2:]: torch.from_numpy(v) for k, v in z.items()
             if k.startswith('g/') and not k[2:].startswith(tuple(prefixes))}
    assert set(got) == set(grads)  # the encoder's stay None
    noise = [k for k in grads if k.startswith('decoder.') and k.endswith(('conv.0.bias', 'conv.3.bias'))]
    assert len(noise) == 2 * sum(k.endswith('.up.weight') for k in grads)
    for k in noise:  # true gradient zero in front of a train-mode BatchNorm: ~0, as tests/test_model_gpu.py checks
        wmax = float(grads[k.replace('.bias', '.weight')].abs().max())
        assert float(got[k].abs().max()) < 1e-4 * max(wmax, 1e-3), k
    assert not FB.compare_gradients(got, grads, FIXTURE_L2, l2=True, skip=noise)
    print('launches:', spy.summary())
    n_ups = len(net.module.decoder.up_seq)
    assert spy.wgrads() == len(_conv_weights(net)) == 3 * n_ups
    convT_dgrads = [s for s in spy.bwd_seen if s[0] == 'igemm' and s[3] == 4]
    assert len(convT_dgrads) == n_ups - 1  # every Up's but the deepest
    assert spy.count('bn_relu_through') == 0  # the decoder's BatchNorms train; the encoder's stages never run backward


def _base_step(dev):
    fx = Fixture('siamese_t8-16')
    cfg, net = IG._build(fx, dev)
    net.train()
    batch = {k: v.to(dev) for k, v in fx.batch().items()}
    return fx, cfg, net, batch


def _check_base_bars(fx, net, got, trace, expect_none=()):
    """The base fixture's bars (tests/test_model_gpu.py) for every gradient but `expect_none`, which must be absent."""
    assert set(got) == set(fx.grads) - set(expect_none)
    order = [k for k, _ in net.module.named_parameters() if k in got]
    P = {k: torch.from_numpy(v.copy()) for k, v in fx.params0.items()}
    _, _, ref = branch_matched_reference(fx.model_type, P, fx.batch(), fx.cfg, trace, net.module,
                                         FB._step_loss(fx.model_type, fx.meta['alpha']))
    assert not check_branch_matched(got, ref, order, GRAD_TOL)
    l2 = {k: rel_l2(got[k], fx.grads[k]) for k in order if not k.endswith(('conv.0.bias', 'conv.3.bias'))}
    worst = max(l2.items(), key=lambda kv: kv[1])
    print(f'gradients vs the reference fixture: worst rel-L2 {worst[1]:.2e} ({worst[0]})')
    assert worst[1] < FIXTURE_L2, worst


@pytest.mark.parametrize('frozen', [('encoder.down_seq.down1.mpconv.1.conv.3.weight',),
                                    ('decoder.up_seq.up1.conv.conv.3.weight',),
                                    ('encoder.down_seq.down1.mpconv.1.conv.1.weight',
                                     'encoder.down_seq.down1.mpconv.1.conv.1.bias')])
def test_one_parameter_frozen_inside_a_stage(dev, monkeypatch, frozen):
    """4. Train mode, siamese_t8-16: a single conv.3.weight frozen (one weight grad fewer), or one BatchNorm's gamma and
    beta (a train-mode BatchNorm keeps its route: dy needs the gradient's statistics).  That gradient is None, every
    other one at the base fixture's bars."""
    fx, cfg, net, batch = _base_step(dev)
    _, _, _, _, base = _train_step(net, cfg, batch, monkeypatch, dev)
    # the running statistics moved in the baseline step: a fresh model for the step the oracle follows
    cfg, net2 = IG._build(fx, dev)
    for k in frozen:
        _params(net2)[k].requires_grad_(False)
    out, loss, got, trace, spy = _train_step(net2.train(), cfg, batch, monkeypatch, dev, trace=True)
    assert abs(loss.item() - float(fx.z['loss0'])) < 1e-5
    assert all(_params(net2)[k].grad is None for k in frozen)
    print('launches:', spy.summary(), 'all trainable:', base.summary())
    if frozen[0].endswith('.weight') and 'conv.3' in frozen[0]:
        assert spy.wgrads() == base.wgrads() - 1
        assert spy.count('wgrad_finalize') == base.count('wgrad_finalize') - 1
    else:
        assert spy.calls == base.calls  # the same routes, launch for launch
        assert spy.seen == base.seen
    _check_base_bars(fx, net2, got, trace, expect_none=frozen)


def test_walk_stops_inside_the_first_stage(dev, monkeypatch):
    """4b. The first DoubleConv's conv0 weight and bias and its BatchNorm's gamma and beta frozen, the input without a
    gradient: nothing reads the second conv's data grad, so it and the first BatchNorm's backward are not launched
    (one 3x3 data grad, one reducing backward, one weight grad fewer).  Every other gradient at the base bars."""
    fx, cfg, net, batch = _base_step(dev)
    _, _, _, _, base = _train_step(net, cfg, batch, monkeypatch, dev)
    frozen = tuple(f'inc.conv.conv.{i}.{p}' for i in (0, 1) for p in ('weight', 'bias'))
    cfg, net2 = IG._build(fx, dev)
    for k in frozen:
        _params(net2)[k].requires_grad_(False)
    out, loss, got, trace, spy = _train_step(net2.train(), cfg, batch, monkeypatch, dev, trace=True)
    assert abs(loss.item() - float(fx.z['loss0'])) < 1e-5
    dgrads = lambda s: sum(1 for c in s.bwd_seen if c[0] == 'igemm' and c[3] == 9)  # noqa: E731
    print('launches:', spy.summary(), 'all trainable:', base.summary(), '3x3 data grads', dgrads(spy), dgrads(base))
    assert dgrads(spy) == dgrads(base) - 1
    assert spy.count(*REDUCING) == base.count(*REDUCING) - 1
    assert spy.wgrads() == base.wgrads() - 1
    _check_base_bars(fx, net2, got, trace, expect_none=frozen)


@pytest.mark.parametrize('name,frozen_bn', [('siamese_t8-16', False), ('siamese_t8-16', True),
                                            ('dtsiamese_t8-16', False), ('unet_t8-16', False)])
def test_only_the_fused_head_trains(dev, monkeypatch, name, frozen_bn):
    """4c. Heads-only fine-tuning of a model whose head runs inside the decoder stage: only outc* trainable.  The
    head's weight grad is formed by the last BatchNorm's backward pass (scd_bn_relu_backward_head w_grad), so that one
    pass still runs, on the reducing route, and the walk stops after it: no conv launch at all in the backward.  The
    head's gradients at the fixture's bars (train mode: the base fixture and the branch-matched oracle; frozen
    BatchNorm: frozenbn_*), so a gradient nobody wrote fails."""
    from multimodal_siamese_cd_amd.utils import networks
    fx = Fixture(name)
    if frozen_bn:
        z, _ = load_frozen(name)
        cfg, net = FB._build(fx, dev)
        ref = {k[2:]: torch.from_numpy(v) for k, v in z.items() if k.startswith('g/outc')}
    else:
        cfg, net = IG._build(fx, dev)
        ref = {k: torch.from_numpy(v) for k, v in fx.grads.items() if k.startswith('outc')}
    for k, p in net.module.named_parameters():
        p.requires_grad_(k.startswith('outc'))
    net.train()
    if frozen_bn:
        networks.freeze_batchnorm(net)
    batch = {k: v.to(dev) for k, v in fx.batch().items()}
    out, loss, got, trace, spy = _train_step(net, cfg, batch, monkeypatch, dev, trace=True)
    print('launches:', spy.summary(), [c for c in spy.bwd_calls])
    assert set(got) == set(ref) and len(ref) >= 2
    for k in ref:
        e2 = rel_l2(got[k], ref[k])
        print(f'{k}: rel-L2 vs the reference fixture {e2:.2e}, bar {FIXTURE_L2:.0e}')
        assert e2 <= FIXTURE_L2, k
    if not frozen_bn:
        P = {k: torch.from_numpy(v.copy()) for k, v in fx.params0.items()}
        _, _, oref = branch_matched_reference(fx.model_type, P, fx.batch(), fx.cfg, trace, net.module,
                                              FB._step_loss(fx.model_type, fx.meta['alpha']))
        assert not check_branch_matched(got, oref, list(ref), GRAD_TOL)
    n_heads = spy.count('bn_relu_backward_head')
    assert n_heads >= 1 and spy.count(*REDUCING) == n_heads  # the head's BatchNorm only
    assert spy.count('conv1x1_bwd_bn') == n_heads  # the head's bias grad
    assert spy.count('bn_relu_through') == 0
    assert spy.wgrads() == 0 and not [c for c in spy.bwd_seen]  # no conv launch in the backward


def test_frozen_decoder_training_encoder(dev, monkeypatch):
    """5. decoder. frozen under train-mode BatchNorm: the reducing route throughout, no decoder weight grad, the
    encoder's and the head's gradients at the base fixture's bars."""
    from multimodal_siamese_cd_amd.utils import networks
    fx, cfg, net, batch = _base_step(dev)
    frozen = networks.freeze_parameters(net, ['decoder.'])
    assert frozen and all(k.startswith('decoder.') for k in frozen)
    out, loss, got, trace, spy = _train_step(net, cfg, batch, monkeypatch, dev, trace=True)
    assert abs(loss.item() - float(fx.z['loss0'])) < 1e-5
    print('launches:', spy.summary())
    assert spy.wgrads() == len(_conv_weights(net))  # the encoder's 3x3 convs
    assert len(_conv_weights(net, False)) - len(_conv_weights(net)) == 3 * len(net.module.decoder.up_seq)
    assert spy.count('bn_relu_through') == 0
    assert spy.count('channel_sum', 'wgrad_colsum_finalize') == 0  # no ConvT bias grad either
    assert spy.count(*REDUCING) == _n_bn(net)  # train mode: dy needs the gradient's statistics whatever trains
    _check_base_bars(fx, net, got, trace, expect_none=frozen)


def test_frozen_decoder_and_its_batchnorm_training_encoder(dev, monkeypatch):
    """5b. The through route inside a training step: every BatchNorm frozen (frozenbn_siamese_t8-16) and decoder.
    frozen, so the decoder's BatchNorms pass the gradient on without a reduction while the encoder's, whose parameters
    train, keep the reducing frozen route.  The encoder's and the head's gradients at that fixture's bar."""
    from multimodal_siamese_cd_amd.utils import networks
    z, meta = load_frozen('siamese_t8-16')
    fx = Fixture(meta['base'])
    cfg, net = FB._build(fx, dev)
    frozen = networks.freeze_parameters(net, ['decoder.'])
    networks.freeze_batchnorm(net.train())
    batch = {k: v.to(dev) for k, v in fx.batch().items()}
    out, loss, got, _, spy = _train_step(net, cfg, batch, monkeypatch, dev)
    FB.check_logits(out, z['out/0'])
    assert abs(loss.item() - float(z['loss'])) < 1e-5
    grads = {k[2:]: torch.from_numpy(v) for k, v in z.items() if k.startswith('g/') and k[2:] not in frozen}
    assert set(got) == set(grads)
    assert not FB.compare_gradients(got, grads, FIXTURE_L2, l2=True)
    print('launches:', spy.summary())
    n_dec = sum(isinstance(m, torch.nn.BatchNorm2d) for m in net.module.decoder.modules())
    # the last decoder BatchNorm also forms the trainable head's weight grad in its pass: it keeps the reducing route
    assert spy.count('bn_relu_through') == n_dec - 1
    assert spy.count(*REDUCING) == _n_bn(net) - (n_dec - 1)
    assert spy.wgrads() == len(_conv_weights(net))


@pytest.mark.parametrize('name', ['dtsiamese_t8-16', 'whatevernet2_t8-16'])
def test_saliency_other_families(dev, monkeypatch, name):
    """6. All frozen + eval on the dual-task model (the pooled2 form and the pair walk) and WhateverNet2 (HeadsFn):
    input gradients against the branch-matched oracle, launch counts as in test 1."""
    fx = Fixture(name)
    cfg, net = IG._build(fx, dev, eval_buffers=True)
    P = {k: torch.from_numpy(v.copy()) for k, v in fx.params0.items()}
    B = {k: torch.from_numpy(v.copy()) for k, v in fx.prefixed('r1/').items()}
    loss, g1, g2, trace, spy = _saliency(fx, dev, net, cfg, monkeypatch)
    _assert_saliency_launches(spy, net)
    assert spy.count('conv1x1_bwd') == 0
    lref, _, r1, r2 = _oracle_inputs(fx, net, trace, P, B)
    assert abs(loss.item() - lref.item()) < 1e-5
    for n_, g, r in (('x_t1', g1, r1), ('x_t2', g2, r2)):
        e = rel(g, r)
        print(f'{name} {n_}: max-relative vs the branch-matched oracle {e:.2e}, bar {GRAD_TOL:.0e}')
        assert e <= GRAD_TOL


def test_saliency_bf16_config(dev, monkeypatch):
    """7. siamese_t32-64 under MODEL.PRECISION bf16, all frozen + eval, at test_input_grad_gpu.test_bf16_config's bar
    against the fp32 oracle: cosine similarity > BF16_COS and rel-L2 <= BF16_L2, loss within 1e-2."""
    fx = Fixture('siamese_t32-64')
    cfg, net = IG._build(fx, dev, eval_buffers=True, precision='bf16')
    assert net.module.conv_math == 'bf16'
    loss, g1, g2, _, spy = _saliency(fx, dev, net, cfg, monkeypatch)
    _assert_saliency_launches(spy, net)
    lref, r1, r2 = oracle_input_grads(fx, eval_mode=True)
    assert abs(loss.item() - lref.item()) < 1e-2
    for name, g, r in (('x_t1', g1, r1), ('x_t2', g2, r2)):
        a, b = g.detach().double().cpu().flatten(), r.double().flatten()
        cs = float(torch.dot(a, b) / (a.norm() * b.norm()))
        e2 = rel_l2(g, r)
        print(f'bf16 {name}.grad vs the fp32 oracle: cosine {cs:.6f} (bar {IG.BF16_COS}), rel-L2 {e2:.2e} '
              f'(bar {IG.BF16_L2:.3f})')
        assert cs > IG.BF16_COS and e2 <= IG.BF16_L2


@pytest.mark.parametrize('mode', ['train', 'frozen_bn'])
def test_no_change_when_everything_trains(dev, monkeypatch, mode):
    """8. With every parameter requiring grad, skip_frozen_grads on and off are the same step: the same launch list
    (record_arith's and the spies') and bit-equal gradients.  With parameters frozen (every first conv weight of a
    DoubleConv, so that every stage still runs its backward) the off arm runs the all-trainable launch list again, the
    weight grads included, and the on arm drops exactly those."""
    from multimodal_siamese_cd_amd import engine
    from multimodal_siamese_cd_amd.utils import networks
    fx = Fixture('siamese_t8-16')
    batch = {k: v.to(dev) for k, v in fx.batch().items()}

    def step(on, freeze=()):
        cfg, net = IG._build(fx, dev, eval_buffers=True)
        net.train()
        if mode == 'frozen_bn':
            networks.freeze_batchnorm(net)
        for k in freeze:
            _params(net)[k].requires_grad_(False)
        prev = engine.set_options(skip_frozen_grads=on)
        try:
            _, loss, got, _, spy = _train_step(net, cfg, batch, monkeypatch, dev)
        finally:
            engine.set_options(**prev)
        return loss, got, spy

    l_on, g_on, s_on = step(True)
    l_off, g_off, s_off = step(False)
    assert s_on.calls == s_off.calls and s_on.seen == s_off.seen
    assert torch.equal(l_on, l_off) and set(g_on) == set(g_off) == set(fx.grads)
    assert all(torch.equal(g_on[k], g_off[k]) for k in g_on)
    frozen = [k for k in fx.grads if k.endswith('conv.0.weight')]
    assert frozen
    l_f_off, g_f_off, s_f_off = step(False, frozen)
    l_f_on, g_f_on, s_f_on = step(True, frozen)
    assert s_f_off.calls == s_off.calls and s_f_off.seen == s_off.seen  # everything computed, autograd discards
    assert s_f_off.wgrads() == len(_conv_weights_of(fx, dev))
    assert s_f_on.wgrads() == s_f_off.wgrads() - len(frozen)
    assert set(g_f_on) == set(g_f_off) == set(fx.grads) - set(frozen)
    bad = {k: rel(g_f_on[k], g_off[k]) for k in g_f_on if not k.endswith(('conv.0.bias', 'conv.3.bias'))}
    print('frozen first convs, on vs all-trainable: worst max-relative', max(bad.values()))
    # the same function; a stand-alone BatchNorm backward may replace one formed inside the dropped weight grad, whose
    # h2 operand bound differs: GRAD_TOL, the bar of two correct evaluations of one gradient
    assert max(bad.values()) <= GRAD_TOL
    assert all(torch.equal(g_f_off[k], g_off[k]) for k in g_f_off)


def _conv_weights_of(fx, dev):
    _, net = IG._build(fx, dev)
    return _conv_weights(net, False)


def test_training_loop_freeze_params(dev, monkeypatch):
    """9. Two steps of train_supervised.run_training with TRAINER.FREEZE_PARAMS and FREEZE_BN ['inc.', 'encoder.']:
    the frozen parameters and their BatchNorm buffers bit-unchanged, every decoder / head parameter moved, the loss
    finite (run_training raises on a non-finite one)."""
    from multimodal_siamese_cd_amd import train_supervised
    from multimodal_siamese_cd_amd.utils import experiment_manager as em, networks
    cfg = em.load_cfg('debug')
    assert 'FREEZE_PARAMS' not in cfg.TRAINER and networks.freeze_params_setting(cfg) is False
    cfg.DEBUG = False
    cfg.TRAINER.EPOCHS = 1
    cfg.TRAINER.STEPS_PER_EPOCH = 2
    cfg.TRAINER.FREEZE_BN = ['inc.', 'encoder.']
    cfg.TRAINER.FREEZE_PARAMS = ['inc.', 'encoder.']
    cfg.LOG_FREQ = 1
    cfg.EVAL_SAMPLES = 1
    cfg.SAVE_CHECKPOINTS = []
    start = {}
    create = networks.create_network

    def create_and_record(c):
        net = create(c)
        with torch.no_grad():  # as test_training_loop_freeze_bn: statistics a train-mode step would visibly move
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
    frozen_side = lambda k: k.replace('module.', '').startswith(('inc.', 'encoder.'))  # noqa: E731
    buffers = {k for k, _ in net.named_buffers()}
    n_frozen = n_moved = 0
    for k, v in net.state_dict().items():
        same = torch.equal(v.cpu(), start[k].cpu())
        if frozen_side(k):
            assert same, k
            n_frozen += 1
        elif k not in buffers:
            assert not same, k
            assert torch.isfinite(v).all(), k
            n_moved += 1
    assert n_frozen and n_moved
    assert all(not p.requires_grad for k, p in net.named_parameters() if frozen_side(k))
    assert all(p.requires_grad for k, p in net.named_parameters() if not frozen_side(k))
