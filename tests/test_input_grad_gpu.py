"""Input gradients of the six model families on MI355X: x_t1.requires_grad_() / x_t2.requires_grad_() through the HIP
path, against fixtures the reference itself produced that way (tests/golden/make_golden_input_grad.py) and against the
fp64 oracle following the GPU forward's own branches.

Bars as tests/test_model_gpu.py: every gradient -- the inputs' and, in the same backward, the parameters' -- within
GRAD_TOL = 1e-3 (max-relative) of the branch-matched fp64 oracle, and the input gradients within FIXTURE_L2 = 2e-2
(norm-wise) of the reference's fp32 ones (which took their own ReLU / MaxPool branches: tests/_parity.py).
"""
import pytest
import torch

from _parity import BranchMatch, check_branch_matched, rel, rel_l2
from oracle.golden import Fixture
from test_input_grad_golden import EVAL, TRAIN, load_input_grad, oracle_input_grads

pytestmark = pytest.mark.gpu

GRAD_TOL = 1e-3
FIXTURE_L2 = 2e-2
# tests/test_bf16_gpu.py holds every weight gradient of a bf16 step, the first layer's included, to a cosine
# similarity > 0.95 with the fp32 oracle's; two vectors of one norm at that cosine are sqrt(2 - 2 * 0.95) apart
BF16_COS = 0.95
BF16_L2 = (2 - 2 * BF16_COS) ** 0.5


@pytest.fixture(scope='module')
def dev():
    from multimodal_siamese_cd_amd import hip
    hip.load_library()
    return torch.device('cuda:0')


def _build(fx, dev, eval_buffers=False, precision=None):
    from multimodal_siamese_cd_amd.utils import networks
    cfg = fx.package_cfg()
    if precision is not None:
        cfg.MODEL.PRECISION = precision
    net = networks.create_network(cfg)
    with torch.no_grad():
        for k, p in net.module.named_parameters():
            p.copy_(torch.from_numpy(fx.params0[k]))
        if eval_buffers:
            r1 = fx.prefixed('r1/')
            for k, b in net.module.named_buffers():
                b.copy_(torch.from_numpy(r1[k]))
    return cfg, net.to(dev)


def branch_matched_input_reference(model_type, P, batch, ocfg, trace, module, loss_fn, training=True, buffers=None):
    """_parity.branch_matched_reference with the inputs as leaves: (loss, {name: parameter grad}, dL/dx_t1, dL/dx_t2)
    of the fp64 oracle following the branches of the GPU forward recorded in `trace`."""
    from oracle import siamese_oracle as O
    Pd = {k: v.detach().double().clone().requires_grad_(True) for k, v in P.items()}
    if buffers is None:
        buffers = O.fresh_buffers(O.param_shapes(model_type, ocfg))
    Bd = {k: (v.double() if v.is_floating_point() else v.clone()) for k, v in buffers.items()}
    bt = {k: (v.detach().cpu().double() if v.is_floating_point() else v.detach().cpu()) for k, v in batch.items()}
    x1, x2 = bt['x_t1'].clone().requires_grad_(), bt['x_t2'].clone().requires_grad_()
    bm = BranchMatch(trace, module)
    O.BRANCH = bm
    try:
        out = O.forward(model_type, Pd, Bd, x1, x2, ocfg, training)
    finally:
        O.BRANCH = None
    loss = loss_fn(out, bt)
    loss.backward()
    print(f'branch matching: {bm.summary()}')
    return loss, {k: v.grad for k, v in Pd.items() if v.grad is not None}, x1.grad, x2.grad


def _step_loss(fx):
    from oracle import siamese_oracle as O
    return lambda out, batch: O.step_loss(fx.model_type, out, batch, fx.meta['alpha'])


def _gpu_step(fx, dev, net, cfg, needs=(True, True), eval_loss=False):
    """One forward + backward with the inputs requiring grad; (x1, x2, loss, parameter grads, BatchNorm trace)."""
    from multimodal_siamese_cd_amd import engine, trainers
    from multimodal_siamese_cd_amd.utils import loss_functions
    batch = {k: v.to(dev) for k, v in fx.batch().items()}
    x1 = batch['x_t1'].clone().requires_grad_(needs[0])
    x2 = batch['x_t2'].clone().requires_grad_(needs[1])
    with engine.trace_bn() as trace:
        out = net(x1, x2)
    if eval_loss:
        assert isinstance(out, torch.Tensor)
        loss = loss_functions.get_criterion('PowerJaccardLoss')(out, batch['y_change'])
    else:
        loss = trainers.step_loss(cfg, out, batch)
    loss.backward()
    torch.cuda.synchronize()
    got = {k: p.grad.cpu() for k, p in net.module.named_parameters() if p.grad is not None}
    return x1, x2, loss, got, trace


def _check_inputs(x1, x2, r1, r2, z=None):
    for name, x, r in (('x_t1', x1, r1), ('x_t2', x2, r2)):
        assert x.grad is not None and x.grad.dtype == x.dtype and x.grad.shape == x.shape
        assert x.grad.device == x.device
        e = rel(x.grad, r)
        print(f'{name}.grad vs the branch-matched fp64 oracle: max-relative {e:.2e}, bar {GRAD_TOL:.0e}')
        assert e <= GRAD_TOL
        if z is not None:
            e2 = rel_l2(x.grad, z['gx/' + name])
            print(f'{name}.grad vs the reference fixture: rel-L2 {e2:.2e}, bar {FIXTURE_L2:.0e}')
            assert e2 <= FIXTURE_L2


@pytest.mark.parametrize('name', TRAIN)
def test_input_gradients_match_reference(dev, name):
    z, meta = load_input_grad(name)
    fx = Fixture(meta['base'])
    cfg, net = _build(fx, dev)
    net.train()
    x1, x2, loss, got, trace = _gpu_step(fx, dev, net, cfg)
    assert abs(loss.item() - float(z['loss'])) < 1e-5
    P = {k: torch.from_numpy(v.copy()) for k, v in fx.params0.items()}
    lref, ref, r1, r2 = branch_matched_input_reference(fx.model_type, P, fx.batch(), fx.cfg, trace, net.module,
                                                       _step_loss(fx))
    assert abs(loss.item() - lref.item()) < 1e-5
    _check_inputs(x1, x2, r1, r2, z)
    # the parameter gradients of the same backward
    assert set(got) == set(fx.grads)
    order = [k for k, _ in net.module.named_parameters() if k in got]
    assert not check_branch_matched(got, ref, order, GRAD_TOL)


def test_only_one_input_requires_grad(dev):
    z, meta = load_input_grad('siamese_t8-16')
    fx = Fixture(meta['base'])
    cfg, net = _build(fx, dev)
    net.train()
    x1, x2, _, _, trace = _gpu_step(fx, dev, net, cfg, needs=(True, False))
    assert x2.grad is None
    assert rel_l2(x1.grad, z['gx/x_t1']) <= FIXTURE_L2
    P = {k: torch.from_numpy(v.copy()) for k, v in fx.params0.items()}
    _, _, r1, _ = branch_matched_input_reference(fx.model_type, P, fx.batch(), fx.cfg, trace, net.module, _step_loss(fx))
    assert rel(x1.grad, r1) <= GRAD_TOL


@pytest.mark.parametrize('name', ['dualstream_t8-16', 'unet_t8-16'])
def test_only_second_input_of_a_stream_packing(dev, name):
    """pack_stream with a NULL first record: only x_t2's channel ranges are written."""
    z, meta = load_input_grad(name)
    fx = Fixture(meta['base'])
    cfg, net = _build(fx, dev)
    net.train()
    x1, x2, _, _, _ = _gpu_step(fx, dev, net, cfg, needs=(False, True))
    assert x1.grad is None
    assert x2.grad.shape == x2.shape and rel_l2(x2.grad, z['gx/x_t2']) <= FIXTURE_L2


def test_second_backward_accumulates(dev):
    from multimodal_siamese_cd_amd import trainers
    z, meta = load_input_grad('dualstream_t8-16')
    fx = Fixture(meta['base'])
    cfg, net = _build(fx, dev)
    net.eval()  # the same function twice: no running statistics move
    batch = {k: v.to(dev) for k, v in fx.batch().items()}
    x1 = batch['x_t1'].clone().requires_grad_()
    x2 = batch['x_t2'].clone().requires_grad_()
    trainers.step_loss(cfg, net(x1, x2), batch).backward()
    g1, g2 = x1.grad.clone(), x2.grad.clone()
    assert float(g1.abs().max()) > 0 and float(g2.abs().max()) > 0
    trainers.step_loss(cfg, net(x1, x2), batch).backward()
    assert torch.equal(x1.grad, 2 * g1) and torch.equal(x2.grad, 2 * g2)  # deterministic kernels: the same bits twice


def test_gradient_takes_the_inputs_dtype(dev):
    """A float64 input: the packing reads it as fp32, its gradient comes back as float64 of its shape and device."""
    z, meta = load_input_grad('siamese_t8-16')
    fx = Fixture(meta['base'])
    cfg, net = _build(fx, dev)
    net.train()
    from multimodal_siamese_cd_amd import trainers
    batch = {k: v.to(dev) for k, v in fx.batch().items()}
    x1 = batch['x_t1'].double().requires_grad_()
    x2 = batch['x_t2'].clone().requires_grad_()
    trainers.step_loss(cfg, net(x1, x2), batch).backward()
    assert x1.grad.dtype == torch.float64 and x1.grad.shape == x1.shape and x1.grad.device == x1.device
    assert x2.grad.dtype == torch.float32
    assert rel_l2(x1.grad, z['gx/x_t1']) <= FIXTURE_L2 and rel_l2(x2.grad, z['gx/x_t2']) <= FIXTURE_L2


def test_frozen_batchnorm(dev):
    """freeze_batchnorm(net): train mode, every BatchNorm on its running statistics (r1/* of the fixture)."""
    from multimodal_siamese_cd_amd.utils import networks
    fx = Fixture('siamese_t8-16')
    cfg, net = _build(fx, dev, eval_buffers=True)
    networks.freeze_batchnorm(net.train())
    x1, x2, loss, got, trace = _gpu_step(fx, dev, net, cfg)
    P = {k: torch.from_numpy(v.copy()) for k, v in fx.params0.items()}
    B = {k: torch.from_numpy(v.copy()) for k, v in fx.prefixed('r1/').items()}
    lref, ref, r1, r2 = branch_matched_input_reference(fx.model_type, P, fx.batch(), fx.cfg, trace, net.module,
                                                       _step_loss(fx), training=False, buffers=B)
    assert abs(loss.item() - lref.item()) < 1e-5
    _check_inputs(x1, x2, r1, r2)
    assert set(got) == set(ref)
    for k, r in ref.items():  # (conv biases in front of a frozen BatchNorm have true gradients)
        assert rel(got[k], r) <= GRAD_TOL, k


def test_eval_mode_with_every_parameter_frozen(dev):
    """Saliency on a checkpoint: net.eval(), every parameter requires_grad False, torch.autograd.grad on the inputs."""
    from multimodal_siamese_cd_amd import engine
    from multimodal_siamese_cd_amd.utils import loss_functions
    from oracle import siamese_oracle as O
    z, meta = load_input_grad(EVAL)
    fx = Fixture(meta['base'])
    cfg, net = _build(fx, dev, eval_buffers=True)
    net.eval()
    for p in net.module.parameters():
        p.requires_grad_(False)
    batch = {k: v.to(dev) for k, v in fx.batch().items()}
    x1 = batch['x_t1'].clone().requires_grad_()
    x2 = batch['x_t2'].clone().requires_grad_()
    with engine.trace_bn() as trace:
        out = net(x1, x2)
    loss = loss_functions.get_criterion('PowerJaccardLoss')(out, batch['y_change'])
    g1, g2 = torch.autograd.grad(loss, [x1, x2])
    assert abs(loss.item() - float(z['loss'])) < 1e-5
    assert all(p.grad is None for p in net.module.parameters())
    P = {k: torch.from_numpy(v.copy()) for k, v in fx.params0.items()}
    B = {k: torch.from_numpy(v.copy()) for k, v in fx.prefixed('r1/').items()}
    lref, _, r1, r2 = branch_matched_input_reference(fx.model_type, P, fx.batch(), fx.cfg, trace, net.module,
                                                     lambda o, b: O.power_jaccard_loss(o, b['y_change']),
                                                     training=False, buffers=B)
    assert abs(loss.item() - lref.item()) < 1e-5
    for name, g, r in (('x_t1', g1, r1), ('x_t2', g2, r2)):
        e, e2 = rel(g, r), rel_l2(g, z['gx/' + name])
        print(f'{name}: max-relative vs the branch-matched oracle {e:.2e}, rel-L2 vs the reference fixture {e2:.2e}')
        assert e <= GRAD_TOL and e2 <= FIXTURE_L2


def test_bf16_config(dev):
    """dualstream_t8-16 under MODEL.PRECISION 'bf16'.  _parity.bf16_conv_oracle emulates the bf16 kernels' convs by
    shape rules written for the 64-channel topologies; at TOPOLOGY [8, 16] the library takes other kernels for them,
    so there is no emulation of this path and the input gradients are held to the bar tests/test_bf16_gpu.py holds a
    bf16 step's first-layer gradients to against the fp32 oracle: cosine similarity > 0.95 (BF16_COS), and the
    rel-L2 distance that cosine allows at equal norms, sqrt(2 - 2 * 0.95) = 0.316 (BF16_L2)."""
    fx = Fixture('dualstream_t8-16')
    cfg, net = _build(fx, dev, precision='bf16')
    assert net.module.conv_math == 'bf16'
    net.train()
    x1, x2, loss, _, _ = _gpu_step(fx, dev, net, cfg)
    lref, r1, r2 = oracle_input_grads(fx)
    assert abs(loss.item() - lref.item()) < 1e-2  # the loss bar of tests/test_bf16_gpu.py
    for name, x, r in (('x_t1', x1, r1), ('x_t2', x2, r2)):
        a, b = x.grad.detach().double().cpu().flatten(), r.double().flatten()
        cs = float(torch.dot(a, b) / (a.norm() * b.norm()))
        e2 = rel_l2(x.grad, r)
        print(f'bf16 {name}.grad vs the fp32 oracle: cosine {cs:.6f} (bar {BF16_COS}), rel-L2 {e2:.2e} (bar {BF16_L2:.3f})')
        assert cs > BF16_COS and e2 <= BF16_L2


def test_standalone_inconv_returns_its_input_gradient(dev):
    """InConv on its 5 bands, called on its own with the input requiring grad, against O.double_conv in fp64."""
    from multimodal_siamese_cd_amd import hip
    from multimodal_siamese_cd_amd.utils import networks
    from oracle import siamese_oracle as O
    fx = Fixture('dtsiamese_t32-64')
    net = networks.create_network(fx.package_cfg())
    with torch.no_grad():
        for k, p in net.module.named_parameters():
            p.copy_(torch.from_numpy(fx.params0[k]))
    inc = net.to(dev).train().module.inc
    P = {k: p.detach().cpu().double().clone().requires_grad_(True) for k, p in inc.named_parameters()}
    B = {k: (v.detach().cpu().double().clone() if v.is_floating_point() else v.detach().cpu().clone())
         for k, v in inc.named_buffers()}
    g = torch.Generator().manual_seed(2)
    x = torch.randn((2, 5, 32, 48), generator=g)
    xd = x.to(dev).requires_grad_()
    with hip.conv_scope('h2'):
        out = inc(xd)
        G = torch.randn(out.shape, generator=torch.Generator().manual_seed(20))
        (out * G.to(dev)).sum().backward()
    xr = x.double().requires_grad_()
    ref = O.double_conv(xr, P, B, 'conv.', True)
    (ref * G.double()).sum().backward()
    assert rel(out, ref) < 1e-4
    assert xd.grad is not None and xd.grad.shape == xd.shape and xd.grad.dtype == xd.dtype
    e = rel(xd.grad, xr.grad)
    print(f'stand-alone InConv input gradient: max-relative {e:.2e}')
    assert e <= GRAD_TOL
    for k, p in inc.named_parameters():
        if k.endswith('conv.0.bias') or k.endswith('conv.3.bias'):
            continue
        assert rel(p.grad, P[k].grad) <= GRAD_TOL, k
