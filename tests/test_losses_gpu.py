"""The loss family on MI355X (scd_loss_multi_fwd / _loss_from_sums / _bwd): every criterion against the reference's
own fp64 results (tests/golden/losses_t5-11x13.npz, written by tests/golden/make_golden_losses.py), the subset,
exact-DataParallel and determinism properties of the fused multi-term form, and the trainers on top of it.

Bars, both taken from this project's existing loss tests:
  loss       |gpu - fp64| <= 1e-5 * max(1, |fp64|)           (tests/test_model_gpu.py's loss bar, made relative for
                                                              the unbounded MSE / BCE values)
  gradients  max|gpu - fp64| <= 1e-5 * max|fp64| per tensor   (the form in tests/test_exact_dp_gpu.py)
"""
import json
import os

import numpy as np
import pytest
import torch

from multimodal_siamese_cd_amd import hip

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LOSS_BAR = 1e-5
GRAD_BAR = 1e-5
KINDS = {'soft_dice': hip.LOSS_SOFT_DICE, 'soft_dice_balanced': hip.LOSS_SOFT_DICE_BALANCED, 'iou': hip.LOSS_IOU,
         'dice_like': hip.LOSS_DICE_LIKE, 'power_jaccard': hip.LOSS_POWER_JACCARD, 'bce': hip.LOSS_BCE_LOGITS,
         'mse': hip.LOSS_MSE}
# The forward sweeps at most 1024 blocks x 256 threads x 4 elements = 1048576 elements per grid-stride pass (the
# backward twice that), so (3, 1, 160, 150) would be one pass of a partly filled grid; (3, 1, 591, 593) = 1051389
# elements is about the smallest three-sample shape with an odd pixel count (350463 per sample: sample boundaries
# inside vectors) that fills the forward's grid and makes its loop run a second time.
BIG = (3, 1, 591, 593)


def loss_ok(got, ref):
    return abs(float(got) - float(ref)) <= LOSS_BAR * max(1.0, abs(float(ref)))


def grad_err(got, ref):
    """max|got - ref| / max|ref|; a reference of all zeros demands exact zeros (0.0, else inf)."""
    got = torch.as_tensor(got).detach().double().cpu()
    ref = torch.as_tensor(ref).detach().double().cpu()
    assert got.shape == ref.shape
    den = float(ref.abs().max())
    if den == 0.0:
        return 0.0 if float(got.abs().max()) == 0.0 else float('inf')
    return float((got - ref).abs().max()) / den


@pytest.fixture(scope='module')
def dev():
    hip.load_library()
    return torch.device('cuda:0')


@pytest.fixture(scope='module')
def fx(dev):
    z = np.load(os.path.join(ROOT, 'tests', 'golden', 'losses_t5-11x13.npz'), allow_pickle=False)
    d = {k: z[k] for k in z.files}
    d['meta'] = json.loads(str(d['meta']))
    for k in ('x', 'z', 'f', 't'):
        d['dev/' + k] = torch.from_numpy(d[k]).to(dev)
    return d


def run(spec, labeled, tensors, grad_on):
    """engine.multi_loss forward + backward on fresh leaves; (loss, [gradient per tensor or None])."""
    from multimodal_siamese_cd_amd import engine
    leaves = [t.detach().clone().requires_grad_(i in grad_on) for i, t in enumerate(tensors)]
    loss = engine.multi_loss(spec, labeled, *leaves)
    loss.backward()
    return loss.detach(), [t.grad for t in leaves]


def single(kind, x, tgt, soft, sigmoid_input=0):
    loss, (gx, gz) = run([(0, 1, 1.0, 0, int(soft), kind, sigmoid_input)], None, [x, tgt], {0, 1} if soft else {0})
    return loss, gx, gz


# ---------------------------------------------------------------------------------------------------------------------
# fp64 references in plain torch (the reference's expressions; its utils/loss_functions.py lines in brackets)
# ---------------------------------------------------------------------------------------------------------------------
def ref_expr(name, x, t):
    e = 1e-6
    if name == 'bce':  # nn.BCEWithLogitsLoss [7-8]
        return (x.clamp(min=0) - x * t + torch.log1p(torch.exp(-x.abs()))).mean()
    if name == 'mse':  # nn.MSELoss on the raw logits [22-23]
        return ((x - t) ** 2).mean()
    p = torch.sigmoid(x).flatten()
    t = t.flatten()
    i = (p * t).sum()
    if name == 'soft_dice':  # [36-44]
        return 1 - (2 * i + e) / (p.sum() + t.sum() + e)
    if name == 'soft_dice_balanced':  # [184-198]
        ni = ((1 - p) * (1 - t)).sum()
        return 1 - 2 * i / (p.sum() + t.sum() + e) - 2 * ni / ((1 - p).sum() + (1 - t).sum() + e)
    if name == 'iou':  # [153-162]
        return 1 - i / ((p + t).sum() - i + e)
    if name == 'dice_like':  # [129-138]
        return 1 - 2 * i / ((p ** 2 + t ** 2).sum() + e)
    if name == 'power_jaccard':  # [141-150]
        return 1 - i / ((p ** 2 + t ** 2).sum() - i + e)
    raise KeyError(name)


@pytest.fixture(scope='module')
def big(dev):
    """Inputs of shape BIG drawn by the fixture generator's seeded recipe, and their fp64 references (computed once)."""
    g = torch.Generator().manual_seed(12)
    x = torch.randn(BIG, generator=g, dtype=torch.float64) * 3
    z = torch.randn(BIG, generator=g, dtype=torch.float64) * 3
    t = (torch.rand(BIG, generator=g, dtype=torch.float64) < 0.2).double()
    flat = x.view(-1)
    for k, v in enumerate((-100.0, -40.0, -17.0, 17.0, 40.0, 100.0)):
        flat[(k * flat.numel()) // 6 + 5 * k + 1] = v
    x, z = x.float().double(), z.float().double()
    ref = {}
    for name in list(KINDS) + ['l2cons']:
        for form in ('hard', 'soft'):
            if name == 'l2cons' and form == 'hard':
                continue
            a, b = x.clone().requires_grad_(True), z.clone().requires_grad_(True)
            if name == 'l2cons':  # train_semisupervised.py:101-102
                loss = ((torch.sigmoid(a) - torch.sigmoid(b)) ** 2).mean()
            else:
                loss = ref_expr(name, a, torch.sigmoid(b) if form == 'soft' else t)
            loss.backward()
            ref[name, form] = (float(loss.detach()), a.grad.clone(), b.grad.clone() if b.grad is not None else None)
    return dict(x=x.float().to(dev), z=z.float().to(dev), t=t.float().to(dev), ref=ref)


CASES = [(k, f) for k in KINDS for f in ('hard', 'soft')] + [('l2cons', 'soft')]


def _case(name, form, x, z, t):
    if name == 'l2cons':
        return single(hip.LOSS_MSE, x, z, True, 1)
    return single(KINDS[name], x, z if form == 'soft' else t, form == 'soft')


@pytest.mark.parametrize('name,form', CASES)
def test_fixture_parity(fx, name, form):
    loss, gx, gz = _case(name, form, fx['dev/x'], fx['dev/z'], fx['dev/t'])
    key = 'l2cons' if name == 'l2cons' else f'{name}/{form}'
    eg = grad_err(gx, fx[key + '/gx'])
    ez = grad_err(gz, fx[key + '/gz']) if form == 'soft' else 0.0
    print(f'{key}: loss {float(loss):.9f} vs {float(fx[key + "/loss64"]):.9f}, gx {eg:.2e}, gz {ez:.2e}')
    assert torch.isfinite(loss)
    assert loss_ok(loss, fx[key + '/loss64'])
    assert eg <= GRAD_BAR and ez <= GRAD_BAR


@pytest.mark.parametrize('name,form', CASES)
def test_grid_stride_loop_shape(big, name, form):
    loss, gx, gz = _case(name, form, big['x'], big['z'], big['t'])
    rl, rgx, rgz = big['ref'][name, form]
    eg = grad_err(gx, rgx)
    ez = grad_err(gz, rgz) if form == 'soft' else 0.0
    print(f'{name}/{form}: loss {float(loss):.9f} vs {rl:.9f}, gx {eg:.2e}, gz {ez:.2e}')
    assert loss_ok(loss, rl)
    assert eg <= GRAD_BAR and ez <= GRAD_BAR


# ---------------------------------------------------------------------------------------------------------------------
# subsets
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('name', list(KINDS))
def test_subset_terms_equal_masked_single_term_calls(fx, dev, name):
    kind = KINDS[name]
    x, z, t = fx['dev/x'], fx['dev/z'], fx['dev/t']
    lab = torch.tensor([1, 0, 1, 1, 0], dtype=torch.uint8, device=dev)
    m = lab.bool()
    # a labelled-only hard-target term, then an unlabelled-only soft-target term, each alone: a single partial writer
    # must zero the unselected samples exactly
    l1, (g1, _) = run([(0, 1, 1.0, 1, 0, kind, 0)], lab, [x, t], {0})
    r1, rg1, _ = single(kind, x[m].contiguous(), t[m].contiguous(), False)
    assert loss_ok(l1, r1) and grad_err(g1[m], rg1) <= GRAD_BAR
    assert float(g1[~m].abs().max()) == 0.0
    l2, (g2, gz2) = run([(0, 1, 1.0, 2, 1, kind, 0)], lab, [x, z], {0, 1})
    r2, rg2, rgz2 = single(kind, x[~m].contiguous(), z[~m].contiguous(), True)
    assert loss_ok(l2, r2) and grad_err(g2[~m], rg2) <= GRAD_BAR and grad_err(gz2[~m], rgz2) <= GRAD_BAR
    assert float(g2[m].abs().max()) == 0.0 and float(gz2[m].abs().max()) == 0.0
    # both in one call: x is written by two terms over disjoint samples
    l12, (g12, _, gz12) = run([(0, 1, 0.7, 1, 0, kind, 0), (0, 2, 0.3, 2, 1, kind, 0)], lab, [x, t, z], {0, 2})
    assert loss_ok(l12, 0.7 * float(r1) + 0.3 * float(r2))
    want = torch.zeros_like(x)
    want[m], want[~m] = 0.7 * rg1, 0.3 * rg2
    assert grad_err(g12, want) <= GRAD_BAR
    assert grad_err(gz12[~m], 0.3 * rgz2) <= GRAD_BAR and float(gz12[m].abs().max()) == 0.0


@pytest.mark.parametrize('name', list(KINDS))
def test_empty_subset_contributes_exactly_nothing(fx, dev, name):
    kind = KINDS[name]
    x, z, t = fx['dev/x'], fx['dev/z'], fx['dev/t']
    two = [(0, 1, 0.7, 1, 0, kind, 0), (0, 2, 0.3, 2, 1, kind, 0)]
    ones = torch.ones(5, dtype=torch.uint8, device=dev)
    # the same call without the empty term gives the same bits
    la, (ga, _, gza) = run(two, ones, [x, t, z], {0, 2})
    lr, (gr, _) = run(two[:1], ones, [x, t], {0})
    assert torch.isfinite(la) and torch.equal(la, lr) and torch.equal(ga, gr)
    assert float(gza.abs().max()) == 0.0
    zeros = torch.zeros(5, dtype=torch.uint8, device=dev)
    lb, (gb, _, gzb) = run(two, zeros, [x, t, z], {0, 2})
    lr, (gr, _, gzr) = run(two[1:], zeros, [x, t, z], {0, 2})
    assert torch.isfinite(lb) and torch.equal(lb, lr) and torch.equal(gb, gr) and torch.equal(gzb, gzr)
    # and the whole-batch single-term call agrees within the bars
    lw, gw, _ = single(kind, x, t, False)
    assert loss_ok(la, 0.7 * float(lw)) and grad_err(ga, 0.7 * gw) <= GRAD_BAR
    # nothing selected at all: the loss is exactly 0 and so is every gradient
    l0, (g0, _) = run([(0, 1, 1.0, 1, 0, kind, 0)], zeros, [x, t], {0})
    assert float(l0) == 0.0 and float(g0.abs().max()) == 0.0


# ---------------------------------------------------------------------------------------------------------------------
# exact-DataParallel form and determinism, at the binding level
# ---------------------------------------------------------------------------------------------------------------------
def _terms(kind, x, t, z, gx=None, gz=None):
    """A labelled hard-target term and an unlabelled soft-target term (MSE: the L2 consistency form) on one x."""
    return [dict(logits=x, target=t, coef=0.5, select=1, soft=0, kind=kind, glogits=gx),
            dict(logits=x, target=z, coef=0.5, select=2, soft=1, kind=kind, sigmoid_input=int(kind == hip.LOSS_MSE),
                 glogits=gx, gtarget=gz, zero=2)]


def _fwd_bwd(kind, x, t, z, lab, sums=None):
    n, pixels = x.shape[0], x[0].numel()
    loss = torch.empty((), device=x.device)
    if sums is None:
        sums = torch.empty((2, hip.LOSS_ROW), device=x.device)
        hip.loss_multi_fwd(_terms(kind, x, t, z), lab, n, pixels, sums, loss)
    gx, gz = torch.full_like(x, float('nan')), torch.full_like(z, float('nan'))
    hip.loss_multi_bwd(_terms(kind, x, t, z, gx, gz), lab, n, pixels, sums, None)
    return loss, sums, gx, gz


@pytest.mark.parametrize('name', list(KINDS))
def test_loss_from_global_sums(fx, dev, name):
    kind = KINDS[name]
    x, z, t = fx['dev/x'], fx['dev/z'], fx['dev/t']
    lab = torch.tensor([1, 0, 1, 1, 0], dtype=torch.uint8, device=dev)
    loss_all, sums_all, gx_all, gz_all = _fwd_bwd(kind, x, t, z, lab)
    assert not torch.isnan(gx_all).any() and not torch.isnan(gz_all).any()
    shards = [slice(0, 2), slice(2, 5)]  # the second shard starts off 16-byte alignment (143 pixels per sample)
    acc = torch.zeros((2, hip.LOSS_ROW), device=dev)
    for sl in shards:
        acc += _fwd_bwd(kind, x[sl], t[sl], z[sl], lab[sl].contiguous())[1]
    assert torch.equal(acc[:, 4], sums_all[:, 4]) and acc[:, 4].tolist() == [3.0, 2.0]
    loss = torch.empty((), device=dev)
    hip.loss_multi_loss_from_sums(_terms(kind, x, t, z), x[0].numel(), acc, loss)
    assert loss_ok(loss, loss_all)
    for sl in shards:
        _, _, gx, gz = _fwd_bwd(kind, x[sl], t[sl], z[sl], lab[sl].contiguous(), sums=acc)
        assert grad_err(gx, gx_all[sl]) <= GRAD_BAR and grad_err(gz, gz_all[sl]) <= GRAD_BAR


@pytest.mark.parametrize('name', list(KINDS))
def test_two_runs_are_bit_identical(big, dev, name):
    kind = KINDS[name]
    lab = torch.tensor([1, 0, 1], dtype=torch.uint8, device=dev)
    a = _fwd_bwd(kind, big['x'], big['t'], big['z'], lab)
    b = _fwd_bwd(kind, big['x'], big['t'], big['z'], lab)
    for u, v in zip(a, b):
        assert torch.equal(u, v)
    assert torch.isfinite(a[0]) and torch.isfinite(a[1]).all()


# ---------------------------------------------------------------------------------------------------------------------
# trainers
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('mask', ['mixed', 'all', 'none'])
@pytest.mark.parametrize('combo,sup,cons', [('bce_l2', 'BCEWithLogitsLoss', 'L2'),
                                            ('dicelike_pj', 'DiceLikeLoss', 'PowerJaccardLoss')])
def test_mmcr_loss_matches_the_reference_composition(fx, dev, combo, sup, cons, mask):
    from multimodal_siamese_cd_amd import trainers
    from multimodal_siamese_cd_amd.utils import loss_functions as L
    key = f'mmcr/{combo}/{mask}'
    outs = [fx['dev/' + k].clone().requires_grad_(True) for k in ('f', 'x', 'z')]
    batch = dict(is_labeled=torch.from_numpy(fx[key + '/mask']).bool(), y_change=fx['dev/t'])
    loss = trainers.mmcr_loss(L.get_criterion(sup), L.get_criterion(cons), outs, batch, fx['meta']['alpha'], cons)
    loss.backward()
    errs = [grad_err(o.grad, fx[f'{key}/{g}']) for o, g in zip(outs, ('gf', 'gs1', 'gs2'))]
    print(f'{key}: loss {loss.item():.9f} vs {float(fx[key + "/loss64"]):.9f}, gradients {errs}')
    assert loss_ok(loss, fx[key + '/loss64'])
    assert max(errs) <= GRAD_BAR


def test_dualtask_loss_with_iou(fx):
    from multimodal_siamese_cd_amd import trainers
    from multimodal_siamese_cd_amd.utils import loss_functions as L
    crit = L.get_criterion('IoULoss')
    t = fx['dev/t']
    ys = [t, 1 - t, t.flip(0).contiguous()]
    outs = [fx['dev/' + k].clone().requires_grad_(True) for k in ('f', 'x', 'z')]
    batch = dict(y_change=ys[0], y_sem_t1=ys[1], y_sem_t2=ys[2])
    loss = trainers.dualtask_loss(crit, crit, outs, batch)
    loss.backward()
    parts = [single(hip.LOSS_IOU, o.detach(), y, False) for o, y in zip(outs, ys)]
    want = (float(parts[0][0]) + (float(parts[1][0]) + float(parts[2][0])) / 2) / 2
    assert loss_ok(loss, want)
    for o, (_, g, _), c in zip(outs, parts, (0.5, 0.25, 0.25)):
        assert grad_err(o.grad, c * g) <= GRAD_BAR


def test_power_jaccard_recipes_keep_their_kernels(fx, dev):
    """With PowerJaccardLoss everywhere the trainers still call engine.multi_jaccard with the specs they had before
    the loss family: bit-identical loss and gradients."""
    from multimodal_siamese_cd_amd import engine, trainers
    from multimodal_siamese_cd_amd.utils import loss_functions as L
    pj = L.get_criterion('PowerJaccardLoss')
    t = fx['dev/t']
    lab = torch.tensor([1, 0, 1, 1, 0], dtype=torch.bool)

    def leaves():
        return [fx['dev/' + k].clone().requires_grad_(True) for k in ('f', 'x', 'z')]
    a, b = leaves(), leaves()
    la = trainers.mmcr_loss(pj, pj, a, dict(is_labeled=lab, y_change=t), 0.5, 'PowerJaccardLoss')
    spec = [(0, 3, 0.5 / 3, 1, 0), (1, 3, 0.5 / 3, 1, 0), (2, 3, 0.5 / 3, 1, 0), (1, 2, 0.5, 2, 1)]
    lb = engine.multi_jaccard(spec, lab.to(dev), *b, t)
    la.backward()
    lb.backward()
    assert torch.equal(la, lb) and all(torch.equal(u.grad, v.grad) for u, v in zip(a, b))
    a, b = leaves(), leaves()
    ys = [t, 1 - t, t.flip(0).contiguous()]
    la = trainers.dualtask_loss(pj, pj, a, dict(y_change=ys[0], y_sem_t1=ys[1], y_sem_t2=ys[2]))
    spec = [(0, 1, 0.5, 0, 0), (2, 3, 0.25, 0, 0), (4, 5, 0.25, 0, 0)]
    lb = engine.multi_jaccard(spec, torch.ones(5, dtype=torch.uint8, device=dev), b[0], ys[0], b[1], ys[1], b[2], ys[2])
    la.backward()
    lb.backward()
    assert torch.equal(la, lb) and all(torch.equal(u.grad, v.grad) for u, v in zip(a, b))


def test_model_step_with_soft_dice_balanced(dev):
    """One training step of the siamese_t8-16 fixture model with MODEL.LOSS_TYPE = SoftDiceBalancedLoss through
    trainers.step_loss: the network receives the single-term kernel's logit gradient, and every parameter gradient
    is finite and non-zero (conv biases feeding a train-mode BatchNorm have a true gradient of 0 and are only checked
    for being finite, as in tests/test_model_gpu.py)."""
    from multimodal_siamese_cd_amd import trainers
    from multimodal_siamese_cd_amd.utils import networks
    from oracle.golden import Fixture
    mfx = Fixture('siamese_t8-16')
    cfg = mfx.package_cfg()
    cfg.MODEL.LOSS_TYPE = 'SoftDiceBalancedLoss'
    net = networks.create_network(cfg)
    with torch.no_grad():
        for k, p in net.module.named_parameters():
            p.copy_(torch.from_numpy(mfx.params0[k]))
    net = net.to(dev).train()
    batch = {k: v.to(dev) for k, v in mfx.batch().items()}
    out = net(batch['x_t1'], batch['x_t2'])
    out.retain_grad()
    loss = trainers.step_loss(cfg, out, batch)
    loss.backward()
    rl, rg, _ = single(hip.LOSS_SOFT_DICE_BALANCED, out.detach(), batch['y_change'], False)
    assert torch.isfinite(loss) and torch.equal(loss.detach(), rl)
    assert torch.equal(out.grad, rg.reshape(out.grad.shape))
    for k, p in net.module.named_parameters():
        assert p.grad is not None and torch.isfinite(p.grad).all(), k
        if not (k.endswith('conv.0.bias') or k.endswith('conv.3.bias')):
            assert float(p.grad.abs().max()) > 0.0, k
