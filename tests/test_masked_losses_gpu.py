"""The per-pixel validity mask of the loss family on MI355X (scd_loss_masked_fwd / _loss_from_sums / _bwd):
`criterion(logits, target, valid=v)` against the reference's own fp64 results on `logits[v], target[v]`
(tests/golden/masked_losses_t5-11x13.npz, written by tests/golden/make_golden_masked_losses.py), and the properties
the contract names: +0.0 gradients at invalid pixels, NaN / Inf there never entering the arithmetic, an all-ones mask
bit-identical to the unmasked call, an exact integer element count, empty terms contributing nothing, the
exact-DataParallel form with int64 counts, and the trainers' recipes on top.

Bars, those of tests/test_losses_gpu.py:
  loss       |gpu - fp64| <= 1e-5 * max(1, |fp64|)
  gradients  max|gpu - fp64| <= 1e-5 * max|fp64| per tensor
"""
import json
import os
import socket
import tempfile

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
CASES = [(k, f) for k in KINDS for f in ('hard', 'soft')]
# 1052651 pixels per sample (not a multiple of 4: sample boundaries inside vectors), 3157953 elements: more than
# 2 * 1024 blocks * 256 threads * 4, so the unmasked sweep's two-vectors-in-flight loop and its remainder loop both
# iterate, and the masked sweep's single loop runs four times
BIG = (3, 1, 1021, 1031)


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


def same_bits(a, b):
    """Bit-identical, -0.0 and +0.0 told apart."""
    return a.shape == b.shape and torch.equal(a.contiguous().view(torch.int32), b.contiguous().view(torch.int32))


@pytest.fixture(scope='module')
def dev():
    hip.load_library()
    return torch.device('cuda:0')


@pytest.fixture(scope='module')
def fx(dev):
    z = np.load(os.path.join(ROOT, 'tests', 'golden', 'masked_losses_t5-11x13.npz'), allow_pickle=False)
    d = {k: z[k] for k in z.files}
    d['meta'] = json.loads(str(d['meta']))
    for k in ('x', 'z', 'f', 't', 'valid'):
        d['dev/' + k] = torch.from_numpy(d[k]).to(dev)
    return d


def run(spec, labeled, tensors, grad_on, valid):
    """engine.multi_loss forward + backward on fresh leaves; (loss, [gradient per tensor or None])."""
    from multimodal_siamese_cd_amd import engine
    leaves = [t.detach().clone().requires_grad_(i in grad_on) for i, t in enumerate(tensors)]
    loss = engine.multi_loss(spec, labeled, *leaves, valid=valid)
    loss.backward()
    return loss.detach(), [t.grad for t in leaves]


def single(kind, x, tgt, soft, valid, sigmoid_input=0):
    loss, (gx, gz) = run([(0, 1, 1.0, 0, int(soft), kind, sigmoid_input)], None, [x, tgt], {0, 1} if soft else {0},
                         valid)
    return loss, gx, gz


def _case(name, form, x, z, t, valid):
    return single(KINDS[name], x, z if form == 'soft' else t, form == 'soft', valid)


def ref_expr(name, x, t):
    """The reference's expressions on flat gathered elements, in the dtype given (utils/loss_functions.py)."""
    e = 1e-6
    if name == 'bce':
        return (x.clamp(min=0) - x * t + torch.log1p(torch.exp(-x.abs()))).mean()
    if name == 'mse':
        return ((x - t) ** 2).mean()
    p = torch.sigmoid(x)
    i = (p * t).sum()
    if name == 'soft_dice':
        return 1 - (2 * i + e) / (p.sum() + t.sum() + e)
    if name == 'soft_dice_balanced':
        ni = ((1 - p) * (1 - t)).sum()
        return 1 - 2 * i / (p.sum() + t.sum() + e) - 2 * ni / ((1 - p).sum() + (1 - t).sum() + e)
    if name == 'iou':
        return 1 - i / ((p + t).sum() - i + e)
    if name == 'dice_like':
        return 1 - 2 * i / ((p ** 2 + t ** 2).sum() + e)
    if name == 'power_jaccard':
        return 1 - i / ((p ** 2 + t ** 2).sum() - i + e)
    raise KeyError(name)


def check_against_fixture(fx, name, form, loss, gx, gz):
    key = f'{name}/{form}'
    inv = fx['dev/valid'] == 0
    eg = grad_err(gx, fx[key + '/gx'])
    ez = grad_err(gz, fx[key + '/gz']) if form == 'soft' else 0.0
    print(f'{key}: loss {float(loss):.9f} vs {float(fx[key + "/loss64"]):.9f}, gx {eg:.2e}, gz {ez:.2e}')
    assert torch.isfinite(loss)
    assert loss_ok(loss, fx[key + '/loss64'])
    assert eg <= GRAD_BAR and ez <= GRAD_BAR
    for g in (gx, gz) if form == 'soft' else (gx,):
        assert not torch.isnan(g).any()
        assert same_bits(g[inv], torch.zeros_like(g[inv]))  # exactly +0.0


# ---------------------------------------------------------------------------------------------------------------------
# 1. fixture parity, 2. poison, 4. unaligned pointers
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('name,form', CASES)
def test_fixture_parity(fx, name, form):
    loss, gx, gz = _case(name, form, fx['dev/x'], fx['dev/z'], fx['dev/t'], fx['dev/valid'])
    check_against_fixture(fx, name, form, loss, gx, gz)
    # a bool mask is the same call
    lb, gxb, _ = _case(name, form, fx['dev/x'], fx['dev/z'], fx['dev/t'], fx['dev/valid'].bool())
    assert torch.equal(loss, lb) and same_bits(gx, gxb)


def test_criteria_take_valid(fx):
    """The public surface: every registered criterion with valid= is its single-term kernel call."""
    from multimodal_siamese_cd_amd.utils import loss_functions as L
    names = {'PowerJaccardLoss': 'power_jaccard', 'BCEWithLogitsLoss': 'bce', 'SoftDiceSquaredSumLoss': 'soft_dice',
             'SoftDiceBalancedLoss': 'soft_dice_balanced', 'MeanSquareErrorLoss': 'mse', 'IoULoss': 'iou',
             'DiceLikeLoss': 'dice_like', 'L2': 'mse'}
    assert set(names) == set(L._REGISTRY)
    for reg, name in names.items():
        x = fx['dev/x'].clone().requires_grad_(True)
        loss = L.get_criterion(reg)(x, fx['dev/t'], valid=fx['dev/valid'])
        loss.backward()
        check_against_fixture(fx, name, 'hard', loss.detach(), x.grad, None)


@pytest.mark.parametrize('name,form', CASES)
def test_poison_at_invalid_pixels_changes_no_bit(fx, dev, name, form):
    x, z, t, v = fx['dev/x'], fx['dev/z'], fx['dev/t'], fx['dev/valid']
    clean = _case(name, form, x, z, t, v)
    inv = (v == 0).flatten().nonzero().flatten()
    px, pz, pt = x.clone(), z.clone(), t.clone()
    for a in (px, pz, pt):
        a.view(-1)[inv] = float('nan')
        a.view(-1)[inv[3]] = float('inf')     # inside a vector of mixed validity or not, as the mask falls
        a.view(-1)[inv[-2]] = float('inf')
    poisoned = _case(name, form, px, pz, pt, v)
    assert torch.isfinite(poisoned[0]) and torch.equal(clean[0], poisoned[0])
    assert same_bits(clean[1], poisoned[1])
    if form == 'soft':
        assert same_bits(clean[2], poisoned[2])


def _offset_view(t, offset):
    """A contiguous copy of t whose data pointer is `offset` elements past a fresh allocation's start."""
    buf = torch.empty(t.numel() + offset + 8, dtype=t.dtype, device=t.device)
    view = buf[offset:offset + t.numel()].view(t.shape)
    view.copy_(t)
    return view


@pytest.mark.parametrize('name,form', CASES)
def test_unaligned_pointers_take_the_scalar_path(fx, name, form):
    x, z, t, v = fx['dev/x'], fx['dev/z'], fx['dev/t'], fx['dev/valid']
    for what in ('mask', 'logits'):
        xs = _offset_view(x, 1) if what == 'logits' else x
        vs = _offset_view(v, 1) if what == 'mask' else v
        assert (vs.data_ptr() % 4 != 0) if what == 'mask' else (xs.data_ptr() % 16 == 4)
        # at the binding: engine.multi_loss would clone the leaves into aligned storage
        soft = form == 'soft'
        tgt = z if soft else t
        term = dict(logits=xs, target=tgt, coef=1.0, select=0, soft=int(soft), kind=KINDS[name])
        sums = torch.empty((1, hip.LOSS_ROW), device=x.device)
        counts = torch.empty(1, dtype=torch.int64, device=x.device)
        loss = torch.empty((), device=x.device)
        hip.loss_masked_fwd([term], None, [vs], 5, 143, sums, counts, loss)
        gx = _offset_view(torch.full_like(x, float('nan')), 1) if what == 'logits' else torch.full_like(x, float('nan'))
        gz = torch.full_like(z, float('nan')) if soft else None
        hip.loss_masked_bwd([dict(term, glogits=gx, gtarget=gz)], None, [vs], 5, 143, sums, None)
        assert int(counts[0]) == 449
        check_against_fixture(fx, name, form, loss, gx, gz)


# ---------------------------------------------------------------------------------------------------------------------
# 3. an all-ones mask is the unmasked call, bit for bit
# ---------------------------------------------------------------------------------------------------------------------
def _two_terms(kind, x, t, z, gx=None, gz=None):
    """A labelled hard-target term and an unlabelled soft-target term (MSE: the L2 consistency form) on one x."""
    return [dict(logits=x, target=t, coef=0.5, select=1, soft=0, kind=kind, glogits=gx),
            dict(logits=x, target=z, coef=0.5, select=2, soft=1, kind=kind, sigmoid_input=int(kind == hip.LOSS_MSE),
                 glogits=gx, gtarget=gz, zero=2)]


def _binding_fwd_bwd(kind, x, t, z, lab, valid, sums=None, counts=None):
    """valid None: the unmasked trio; else the masked one with that per-term list.  NaN-filled gradient buffers."""
    n, pixels = x.shape[0], x[0].numel()
    loss = torch.empty((), device=x.device)
    if sums is None:
        sums = torch.empty((2, hip.LOSS_ROW), device=x.device)
        if valid is None:
            hip.loss_multi_fwd(_two_terms(kind, x, t, z), lab, n, pixels, sums, loss)
        else:
            counts = torch.empty(2, dtype=torch.int64, device=x.device)
            hip.loss_masked_fwd(_two_terms(kind, x, t, z), lab, valid, n, pixels, sums, counts, loss)
    gx, gz = torch.full_like(x, float('nan')), torch.full_like(z, float('nan'))
    if valid is None:
        hip.loss_multi_bwd(_two_terms(kind, x, t, z, gx, gz), lab, n, pixels, sums, None)
    else:
        hip.loss_masked_bwd(_two_terms(kind, x, t, z, gx, gz), lab, valid, n, pixels, sums, None)
    return loss, sums, gx, gz, counts


@pytest.fixture(scope='module')
def big(dev):
    """Inputs of shape BIG by the fixture generator's seeded recipe, a mask of rand < 0.5 with one 64-row band invalid,
    and the fp64 references over the gathered elements (computed once, on the CPU)."""
    g = torch.Generator().manual_seed(12)
    x = torch.randn(BIG, generator=g, dtype=torch.float64) * 3
    z = torch.randn(BIG, generator=g, dtype=torch.float64) * 3
    t = (torch.rand(BIG, generator=g, dtype=torch.float64) < 0.2).double()
    v = torch.rand(BIG, generator=g) < 0.5
    v[:, :, 300:364, :] = False
    flat = x.view(-1)
    for k, val in enumerate((-100.0, -40.0, -17.0, 17.0, 40.0, 100.0)):
        flat[(k * flat.numel()) // 6 + 5 * k + 1] = val
    x, z = x.float().double(), z.float().double()
    ref = {}
    for name, form in CASES:
        a, b = x.clone().requires_grad_(True), z.clone().requires_grad_(True)
        loss = ref_expr(name, a[v], torch.sigmoid(b)[v] if form == 'soft' else t[v])
        loss.backward()
        ref[name, form] = (float(loss.detach()), a.grad.clone(), b.grad.clone() if b.grad is not None else None)
    return dict(x=x.float().to(dev), z=z.float().to(dev), t=t.float().to(dev), v=v.to(dev), ref=ref)


@pytest.mark.parametrize('size', ['fixture', 'big'])
@pytest.mark.parametrize('name', list(KINDS))
def test_all_ones_mask_is_the_unmasked_call_bit_for_bit(fx, big, dev, name, size):
    kind = KINDS[name]
    if size == 'fixture':
        x, z, t = fx['dev/x'], fx['dev/z'], fx['dev/t']
        lab = torch.tensor([1, 0, 1, 1, 0], dtype=torch.uint8, device=dev)
    else:
        x, z, t = big['x'], big['z'], big['t']
        lab = torch.tensor([1, 0, 1], dtype=torch.uint8, device=dev)
    ones = torch.ones(x.shape, dtype=torch.uint8, device=dev)
    pixels = x[0].numel()
    plain = _binding_fwd_bwd(kind, x, t, z, lab, None)
    for valid in ([ones, ones], [ones, None], [None, ones]):  # a NULL entry: that term is unmasked
        masked = _binding_fwd_bwd(kind, x, t, z, lab, valid)
        assert torch.equal(plain[0], masked[0]) and torch.isfinite(masked[0])
        assert same_bits(plain[1], masked[1])  # the rows, coefficients included
        assert same_bits(plain[2], masked[2]) and same_bits(plain[3], masked[3])
        assert masked[4].tolist() == [int(lab.sum()) * pixels, int((lab == 0).sum()) * pixels]
    # and through autograd, every sample selected (the unmasked sweep's two-vectors-in-flight loop)
    a = single(kind, x, t, False, None)
    b = single(kind, x, t, False, ones)
    assert torch.equal(a[0], b[0]) and same_bits(a[1], b[1])


# ---------------------------------------------------------------------------------------------------------------------
# 5. grid stride
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('name,form', CASES)
def test_grid_stride_shape_against_fp64_on_gathered_elements(big, name, form):
    loss, gx, gz = _case(name, form, big['x'], big['z'], big['t'], big['v'])
    rl, rgx, rgz = big['ref'][name, form]
    eg = grad_err(gx, rgx)
    ez = grad_err(gz, rgz) if form == 'soft' else 0.0
    print(f'{name}/{form}: loss {float(loss):.9f} vs {rl:.9f}, gx {eg:.2e}, gz {ez:.2e}')
    assert loss_ok(loss, rl)
    assert eg <= GRAD_BAR and ez <= GRAD_BAR
    inv = ~big['v']
    assert same_bits(gx[inv], torch.zeros_like(gx[inv]))
    again = _case(name, form, big['x'], big['z'], big['t'], big['v'])
    assert torch.equal(loss, again[0]) and same_bits(gx, again[1])
    if form == 'soft':
        assert same_bits(gz[inv], torch.zeros_like(gz[inv])) and same_bits(gz, again[2])


# ---------------------------------------------------------------------------------------------------------------------
# 6. the element count is an integer
# ---------------------------------------------------------------------------------------------------------------------
def test_count_is_exact_past_2_to_24(dev):
    """2^24 + 1 valid elements: an fp32 count would read 2^24 (the mean's denominator off by one part in 2^24 is far
    inside the bar; the count itself is what is pinned)."""
    n = (1 << 24) + 4
    g = torch.Generator().manual_seed(5)
    x = (torch.randn(n, generator=g) * 3).view(1, 1, 4, n // 4)
    t = (torch.rand(n, generator=g) < 0.2).float().view(1, 1, 4, n // 4)
    v = torch.ones(n, dtype=torch.uint8)
    v[[7, n // 2 + 1, n - 1]] = 0
    xd, td, vd = x.to(dev), t.to(dev), v.view(x.shape).to(dev)
    term = dict(logits=xd, target=td, coef=1.0, select=0, soft=0, kind=hip.LOSS_BCE_LOGITS)
    sums = torch.empty((1, hip.LOSS_ROW), device=dev)
    counts = torch.empty(1, dtype=torch.int64, device=dev)
    loss = torch.empty((), device=dev)
    hip.loss_masked_fwd([term], None, [vd], 1, n, sums, counts, loss)
    assert counts.tolist() == [(1 << 24) + 1]
    assert float(sums[0, 4]) == 1.0  # slot 4 keeps meaning "selected samples"
    keep = v.bool()
    ref = ref_expr('bce', x.view(-1)[keep].double(), t.view(-1)[keep].double())
    print(f'bce over 2^24 + 1 elements: {float(loss):.9f} vs {float(ref):.9f}')
    assert loss_ok(loss, ref)
    assert float(sums[0, 5]) == float(np.float32(1.0 / ((1 << 24) + 1)))  # a = 1 / N from the integer count


# ---------------------------------------------------------------------------------------------------------------------
# 7. empty terms
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('name', list(KINDS))
def test_empty_terms_contribute_exactly_nothing(fx, dev, name):
    kind = KINDS[name]
    x, z, f, t, v = fx['dev/x'], fx['dev/z'], fx['dev/f'], fx['dev/t'], fx['dev/valid']
    none = torch.zeros_like(v)
    loss, gx, gz = single(kind, x, z, True, none)
    assert float(loss) == 0.0
    assert same_bits(gx, torch.zeros_like(gx)) and same_bits(gz, torch.zeros_like(gz))
    # a labelled-only term whose labelled samples are all invalid is empty too (sample 1 of the fixture's mask)
    lab = torch.tensor([0, 1, 0, 0, 0], dtype=torch.uint8, device=dev)
    l1, (g1, _) = run([(0, 1, 1.0, 1, 0, kind, 0)], lab, [x, t], {0}, v)
    assert float(l1) == 0.0 and same_bits(g1, torch.zeros_like(g1))
    # beside a live term: that term's bits are those of its single-term call
    two = [(0, 1, 0.7, 0, 0, kind, 0), (2, 3, 0.3, 0, 1, kind, 0)]
    la, (ga, _, gza, gfa) = run(two, None, [x, t, z, f], {0, 2, 3}, [v, none])
    lr, (gr, _) = run(two[:1], None, [x, t], {0}, [v])
    assert torch.isfinite(la) and torch.equal(la, lr) and same_bits(ga, gr)
    assert same_bits(gza, torch.zeros_like(gza)) and same_bits(gfa, torch.zeros_like(gfa))


# ---------------------------------------------------------------------------------------------------------------------
# 8. exact-DataParallel form
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('name', list(KINDS))
def test_masked_loss_from_global_sums(fx, dev, name):
    kind = KINDS[name]
    x, z, t, v = fx['dev/x'], fx['dev/z'], fx['dev/t'], fx['dev/valid']
    lab = torch.tensor([1, 0, 1, 1, 0], dtype=torch.uint8, device=dev)
    loss_all, sums_all, gx_all, gz_all, counts_all = _binding_fwd_bwd(kind, x, t, z, lab, [v, v])
    assert not torch.isnan(gx_all).any() and not torch.isnan(gz_all).any()
    assert counts_all.tolist() == [103 + 105 + 143, 0 + 98]
    shards = [slice(0, 2), slice(2, 5)]  # the second shard starts off 16-byte (and its mask off 4-byte) alignment
    acc = torch.zeros((2, hip.LOSS_ROW), device=dev)
    cnt = torch.zeros(2, dtype=torch.int64, device=dev)
    for sl in shards:
        out = _binding_fwd_bwd(kind, x[sl], t[sl], z[sl], lab[sl].contiguous(), [v[sl], v[sl]])
        acc += out[1]
        cnt += out[4]
    assert torch.equal(cnt, counts_all) and acc[:, 4].tolist() == [3.0, 2.0]
    loss = torch.empty((), device=dev)
    hip.loss_masked_loss_from_sums(_two_terms(kind, x, t, z), acc, cnt, loss)
    assert loss_ok(loss, loss_all)
    for sl in shards:
        _, _, gx, gz, _ = _binding_fwd_bwd(kind, x[sl], t[sl], z[sl], lab[sl].contiguous(), [v[sl], v[sl]], sums=acc)
        assert grad_err(gx, gx_all[sl]) <= GRAD_BAR and grad_err(gz, gz_all[sl]) <= GRAD_BAR


def test_loss_reduction_reduces_counts_as_int64(fx, dev):
    """Under engine.loss_reduction the rows and the int64 counts both go through the collective, then the masked
    from-sums: with two "ranks" holding the same shard, every sum and count doubles."""
    from multimodal_siamese_cd_amd import engine
    seen = []

    def double(buf):
        seen.append(buf.dtype)
        buf.mul_(2)
    x, t, v = fx['dev/x'], fx['dev/t'], fx['dev/valid']
    for name in ('soft_dice_balanced', 'bce', 'power_jaccard'):
        with engine.loss_reduction(double):
            a = x.clone().requires_grad_(True)
            loss = engine.single_loss(KINDS[name], a, t, valid=v)
            loss.backward()
        # the batch twice over: the same loss, half the gradient per copy
        x2, t2, v2 = torch.cat([x, x]), torch.cat([t, t]), torch.cat([v, v])
        rl, rg, _ = single(KINDS[name], x2, t2, False, v2)
        assert loss_ok(loss.detach(), rl) and grad_err(a.grad, rg[:5]) <= GRAD_BAR
    assert seen == [torch.float32, torch.int64] * 3


def _free_port():
    with socket.socket() as s:
        s.bind(('127.0.0.1', 0))
        return s.getsockname()[1]


def _ddp_worker(rank, port, out_dir):
    os.environ.update(RANK='0', LOCAL_RANK='0', WORLD_SIZE='1', MASTER_ADDR='127.0.0.1', MASTER_PORT=str(port))
    import torch.distributed as dist
    from multimodal_siamese_cd_amd import parallel, trainers
    from multimodal_siamese_cd_amd.utils import networks
    from oracle.golden import Fixture
    dev = torch.device('cuda', 0)
    torch.cuda.set_device(dev)
    dist.init_process_group('nccl', rank=0, world_size=1, device_id=dev)
    hip.load_library()
    mfx = Fixture('siamese_t8-16')
    cfg = mfx.package_cfg()
    cfg.MODEL.LOSS_TYPE = 'SoftDiceBalancedLoss'
    b = {k: v.to(dev) for k, v in mfx.batch().items()}
    b['valid'] = (torch.rand(b['y_change'].shape, generator=torch.Generator().manual_seed(3)) < 0.7).to(dev)
    out, grads = {}, []
    for use_ddp in (False, True):
        net = networks.create_network(cfg)
        with torch.no_grad():
            for k, p in net.module.named_parameters():
                p.copy_(torch.from_numpy(mfx.params0[k]))
        net = net.to(dev).train()
        if use_ddp:
            net = parallel.wrap_ddp(net, dev, exact_dataparallel=True, single_rank=True)
            out['wrapped'] = type(net).__name__
        y = net(b['x_t1'], b['x_t2'])
        loss = trainers.step_loss(cfg, y, b, net)
        loss.backward()
        torch.cuda.synchronize()
        grads.append({n: p.grad.detach().cpu() for n, p in net.module.named_parameters() if p.grad is not None})
        out[f'loss_{int(use_ddp)}'] = loss.item()
    out['same_grads'] = sorted(grads[0]) == sorted(grads[1]) and all(torch.equal(grads[0][n], grads[1][n])
                                                                    for n in grads[0])
    out['n_grads'] = len(grads[0])
    torch.save(out, os.path.join(out_dir, 'masked_ddp.pt'))
    dist.destroy_process_group()


@pytest.mark.timeout(300)
def test_masked_step_through_exact_dataparallel_one_rank():
    """The masked loss under parallel.wrap_ddp(single_rank=True, exact_dataparallel=True): rows and counts through the
    one-rank collective and the masked from-sums, equal to the same step without DDP bit for bit."""
    import torch.multiprocessing as mp
    with tempfile.TemporaryDirectory() as d:
        mp.spawn(_ddp_worker, args=(_free_port(), d), nprocs=1, join=True)
        out = torch.load(os.path.join(d, 'masked_ddp.pt'), weights_only=True)
    assert out['wrapped'] == 'DistributedDataParallel'
    assert np.isfinite(out['loss_0']) and out['loss_0'] == out['loss_1']
    assert out['n_grads'] > 0 and out['same_grads']


# ---------------------------------------------------------------------------------------------------------------------
# 9. recipes, 10. a model step
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('mask', ['mixed', 'all'])
@pytest.mark.parametrize('combo,sup,cons', [('bce_l2', 'BCEWithLogitsLoss', 'L2'),
                                            ('dicelike_pj', 'DiceLikeLoss', 'PowerJaccardLoss')])
def test_mmcr_loss_with_valid_matches_the_reference_composition(fx, dev, combo, sup, cons, mask):
    from multimodal_siamese_cd_amd import trainers
    from multimodal_siamese_cd_amd.utils import loss_functions as L
    key = f'mmcr/{combo}/{mask}'
    outs = [fx['dev/' + k].clone().requires_grad_(True) for k in ('f', 'x', 'z')]
    batch = dict(is_labeled=torch.from_numpy(fx[key + '/mask']).bool(), y_change=fx['dev/t'], valid=fx['dev/valid'])
    loss = trainers.mmcr_loss(L.get_criterion(sup), L.get_criterion(cons), outs, batch, fx['meta']['alpha'], cons)
    loss.backward()
    errs = [grad_err(o.grad, fx[f'{key}/{g}']) for o, g in zip(outs, ('gf', 'gs1', 'gs2'))]
    print(f'{key}: loss {loss.item():.9f} vs {float(fx[key + "/loss64"]):.9f}, gradients {errs}')
    assert loss_ok(loss, fx[key + '/loss64'])
    assert max(errs) <= GRAD_BAR
    inv = fx['dev/valid'] == 0
    for o in outs:
        assert same_bits(o.grad[inv], torch.zeros_like(o.grad[inv]))


def test_mmcr_foreign_criterion_takes_the_gather_idiom(fx, dev):
    """A callable without a kernel kind: the recipe gathers, and agrees with the fused call within the bars."""
    from multimodal_siamese_cd_amd import trainers
    from multimodal_siamese_cd_amd.utils import loss_functions as L

    def foreign(logits, target):
        return L.dice_like_loss(logits.reshape(1, 1, 1, -1), target.reshape(1, 1, 1, -1))
    key = 'mmcr/dicelike_pj/mixed'
    outs = [fx['dev/' + k].clone().requires_grad_(True) for k in ('f', 'x', 'z')]
    batch = dict(is_labeled=torch.from_numpy(fx[key + '/mask']).bool(), y_change=fx['dev/t'], valid=fx['dev/valid'])

    def foreign_pj(logits, target):  # the consistency target arrives as probabilities here; only the value is checked
        return L.power_jaccard_loss(logits.reshape(1, 1, 1, -1), target.detach().reshape(1, 1, 1, -1))
    loss = trainers.mmcr_loss(foreign, foreign_pj, outs, batch, fx['meta']['alpha'], 'PowerJaccardLoss')
    assert loss_ok(loss, fx[key + '/loss64'])


def test_dualtask_loss_with_valid(fx):
    from multimodal_siamese_cd_amd import trainers
    from multimodal_siamese_cd_amd.utils import loss_functions as L
    crit = L.get_criterion('IoULoss')
    t, v = fx['dev/t'], fx['dev/valid']
    ys = [t, 1 - t, t.flip(0).contiguous()]
    outs = [fx['dev/' + k].clone().requires_grad_(True) for k in ('f', 'x', 'z')]
    batch = dict(y_change=ys[0], y_sem_t1=ys[1], y_sem_t2=ys[2], valid=v)
    loss = trainers.dualtask_loss(crit, crit, outs, batch)
    loss.backward()
    parts = [single(hip.LOSS_IOU, o.detach(), y, False, v) for o, y in zip(outs, ys)]
    want = (float(parts[0][0]) + (float(parts[1][0]) + float(parts[2][0])) / 2) / 2
    assert loss_ok(loss, want)
    for o, (_, g, _), c in zip(outs, parts, (0.5, 0.25, 0.25)):
        assert grad_err(o.grad, c * g) <= GRAD_BAR
        assert same_bits(o.grad[v == 0], torch.zeros_like(o.grad[v == 0]))
    # and the single call is the gathered expression
    assert loss_ok(parts[0][0], ref_expr('iou', fx['dev/f'].double()[v.bool()], t.double()[v.bool()]))


def test_power_jaccard_recipes_without_valid_keep_their_kernels(fx, dev, monkeypatch):
    """No `valid` key: the PowerJaccard recipes still reach engine.multi_jaccard (bit-identical to its direct call)
    and never the loss family; with one they run as kind 0 of the family and match the gathered reference."""
    from multimodal_siamese_cd_amd import engine, trainers
    from multimodal_siamese_cd_amd.utils import loss_functions as L
    pj = L.get_criterion('PowerJaccardLoss')
    t, v = fx['dev/t'], fx['dev/valid']
    lab = torch.tensor([1, 0, 1, 1, 0], dtype=torch.bool)
    calls = []
    real_jaccard, real_loss = engine.multi_jaccard, engine.multi_loss
    monkeypatch.setattr(engine, 'multi_jaccard', lambda *a, **k: (calls.append('jaccard'), real_jaccard(*a, **k))[1])
    monkeypatch.setattr(engine, 'multi_loss', lambda *a, **k: (calls.append('loss'), real_loss(*a, **k))[1])

    def leaves():
        return [fx['dev/' + k].clone().requires_grad_(True) for k in ('f', 'x', 'z')]
    a, b = leaves(), leaves()
    la = trainers.mmcr_loss(pj, pj, a, dict(is_labeled=lab, y_change=t), 0.5, 'PowerJaccardLoss')
    assert calls == ['jaccard']
    spec = [(0, 3, 0.5 / 3, 1, 0), (1, 3, 0.5 / 3, 1, 0), (2, 3, 0.5 / 3, 1, 0), (1, 2, 0.5, 2, 1)]
    lb = real_jaccard(spec, lab.to(dev), *b, t)
    la.backward()
    lb.backward()
    assert torch.equal(la, lb) and all(torch.equal(p.grad, q.grad) for p, q in zip(a, b))
    ys = [t, 1 - t, t.flip(0).contiguous()]
    del calls[:]
    trainers.dualtask_loss(pj, pj, leaves(), dict(y_change=ys[0], y_sem_t1=ys[1], y_sem_t2=ys[2]))
    assert calls == ['jaccard']
    # with a mask: the loss family, kind 0
    del calls[:]
    c = leaves()
    lc = trainers.mmcr_loss(pj, pj, c, dict(is_labeled=lab, y_change=t, valid=v), 0.5, 'PowerJaccardLoss')
    assert calls == ['loss']
    vb, m = v.bool(), lab.to(dev).view(-1, 1, 1, 1)
    f64, x64, z64, t64 = (fx['dev/' + k].double() for k in ('f', 'x', 'z', 't'))
    sel, uns = vb & m, vb & ~m
    want = 0.5 / 3 * sum(ref_expr('power_jaccard', o[sel], t64[sel]) for o in (f64, x64, z64)) \
        + 0.5 * ref_expr('power_jaccard', x64[uns], torch.sigmoid(z64)[uns])
    assert loss_ok(lc, want)
    del calls[:]
    trainers.supervised_loss(pj, c[0], dict(y_change=t, valid=v))
    assert calls == ['loss']


def test_model_step_with_a_mask(dev):
    """One training step of a small siameseunet (TOPOLOGY [8, 16], 2 x 5 x 32 x 32) with batch['valid'] through
    trainers.step_loss: the logit gradient is the single-loss kernel's, +0.0 at invalid pixels, and every parameter
    gradient is finite."""
    from multimodal_siamese_cd_amd import trainers
    from multimodal_siamese_cd_amd.utils import networks
    from oracle.golden import Fixture
    mfx = Fixture('siamese_t8-16')
    cfg = mfx.package_cfg()
    net = networks.create_network(cfg)
    with torch.no_grad():
        for k, p in net.module.named_parameters():
            p.copy_(torch.from_numpy(mfx.params0[k]))
    net = net.to(dev).train()
    batch = {k: (v[..., :32, :32].contiguous() if v.dim() == 4 else v).to(dev) for k, v in mfx.batch().items()}
    assert tuple(batch['x_t1'].shape) == (2, 5, 32, 32) and tuple(batch['y_change'].shape) == (2, 1, 32, 32)
    valid = torch.rand(batch['y_change'].shape, generator=torch.Generator().manual_seed(3)) < 0.7
    valid[0, :, 8:16] = False
    batch['valid'] = valid.to(dev)
    batch['y_change'] = torch.where(batch['valid'], batch['y_change'], torch.full_like(batch['y_change'], float('nan')))
    out = net(batch['x_t1'], batch['x_t2'])
    out.retain_grad()
    loss = trainers.step_loss(cfg, out, batch)  # PowerJaccardLoss: kind 0 of the family with a mask
    loss.backward()
    rl, rg, _ = single(hip.LOSS_POWER_JACCARD, out.detach(), batch['y_change'], False, batch['valid'])
    assert torch.isfinite(loss) and torch.equal(loss.detach(), rl)
    assert same_bits(out.grad, rg.reshape(out.grad.shape))
    inv = ~batch['valid']
    assert same_bits(out.grad[inv], torch.zeros_like(out.grad[inv])) and float(out.grad.abs().max()) > 0.0
    for k, p in net.module.named_parameters():
        assert p.grad is not None and torch.isfinite(p.grad).all(), k
