"""The BatchNorm + ReLU backward in frozen mode (scd_bn_relu_backward_desc with SCD_BN_BWD_FROZEN, coefficients from
scd_bn_frozen_coeffs), every form, against a direct fp64 evaluation of the formula:

    m, v the running statistics, r = 1/sqrt(v + eps), scale = gamma*r, shift = beta - m*scale
    dz = da * [scale*y + shift > 0];  dy = scale*dz;  dbeta = sum dz;  dgamma = sum dz*(y - m)*r
    conv bias in front: sum dy = scale*dbeta

The running statistics are far from the batch's, so a kernel that silently used batch statistics fails.  The ReLU
decisions of the reference are the kernels' own (the fp32 scale / shift formed in fp64, where the product is exact).

Bars: those of the train-mode tests of the same kernels (tests/test_kernels_gpu.py): dy 1e-4, dgamma / dbeta 1e-5
(test_batchnorm_relu_train_forward_backward), the head's weight grad 1e-5 (test_head_conv1x1), an h2 weight grad
2e-6 of the fp64 one (test_wgrad_c16_deferred_bn_backward), a bf16 weight grad 2e-2.  The conv-bias grad is a sum
like dbeta and takes its bar (in train mode it is a true zero and was only checked for being small).  Under bf16
storage dy is rounded once as it is stored (2^-9 of the element) and the conv-bias grad sums the stored values:
both take 2^-8 there.
"""
import pytest
import torch

pytestmark = pytest.mark.gpu

EPS = 1e-5
DY_TOL = 1e-4
SUM_TOL = 1e-5
BF16_TOL = 2.0 ** -8


@pytest.fixture(scope='module')
def dev():
    from multimodal_siamese_cd_amd import hip
    hip.load_library()
    d = torch.device('cuda:0')
    hip.ensure_device(torch.empty(1, device=d))
    return d


def rel(a, b):
    a = a.detach().double().cpu()
    b = b.detach().double().cpu()
    return ((a - b).abs().max() / b.abs().max().clamp_min(1e-30)).item()


class Case:
    """One BatchNorm's tensors on the device, its frozen coefficients, and the fp64 reference of a backward."""

    def __init__(self, dev, n, h, w, c, nseg, seed, dtype=torch.float32):
        from multimodal_siamese_cd_amd import hip
        g = torch.Generator().manual_seed(seed)
        self.dev, self.shape, self.c, self.nseg, self.dtype = dev, (n, h, w, c), c, nseg, dtype
        self.y = (torch.randn(n, h, w, c, generator=g) * 2 + 0.3).to(dev).to(dtype)
        self.gamma = (torch.rand(c, generator=g) + 0.5).to(dev)
        self.beta = torch.randn(c, generator=g).to(dev)
        self.rm = (torch.randn(c, generator=g) * 1.5 + 2.0).to(dev)  # the batch: mean 0.3, variance 4
        self.rv = (torch.rand(c, generator=g) * 3 + 0.5).to(dev)
        self.gen = g
        rm0, rv0 = self.rm.clone(), self.rv.clone()
        self.smean, self.sinv, self.scale, self.shift = (torch.full((nseg * c,), float('nan'), device=dev)
                                                         for _ in range(4))
        hip.bn_frozen_coeffs(c, nseg, self.gamma, self.beta, self.rm, self.rv, EPS, self.smean, self.sinv, self.scale,
                             self.shift)
        assert torch.equal(self.rm, rm0) and torch.equal(self.rv, rv0)
        m, v = self.rm.double().cpu(), self.rv.double().cpu()
        self.m, self.r = m, 1 / torch.sqrt(v + EPS)
        sc = self.gamma.double().cpu() * self.r
        sh = self.beta.double().cpu() - m * sc
        for got, want in ((self.smean, m), (self.sinv, self.r), (self.scale, sc), (self.shift, sh)):
            got = got.cpu().reshape(nseg, c)
            assert all(torch.equal(got[s], got[0]) for s in range(nseg))  # one coefficient set for all segments
            assert rel(got[0], want) < 1e-6
        self.ws = torch.empty(hip.bn_workspace_bytes(n, h, w, c, nseg), dtype=torch.uint8, device=dev)

    def rand(self, *shape):
        return torch.randn(*shape, generator=self.gen).to(self.dev).to(self.dtype)

    def reference(self, da):
        """fp64 (dy, dgamma, dbeta, conv-bias grad, a) for the incoming gradient da (NHWC, any float type)."""
        y = self.y.double().cpu()
        sc32, sh32 = self.scale[:self.c].double().cpu(), self.shift[:self.c].double().cpu()
        z = y * sc32 + sh32  # the kernels' decision fmaf(y, scale, shift) > 0: same sign as the exact value
        mask = z > 0
        sc = self.gamma.double().cpu() * self.r
        dz = torch.where(mask, da.double().cpu(), torch.zeros((), dtype=torch.float64))
        dbeta = dz.sum((0, 1, 2))
        dgamma = (dz * (y - self.m) * self.r).sum((0, 1, 2))
        return sc * dz, dgamma, dbeta, sc * dbeta, torch.relu(z)

    def outputs(self):
        dy = torch.full_like(self.y, float('nan'))
        return dy, [torch.full((self.c,), float('nan'), device=self.dev) for _ in range(3)]

    def args(self):
        return (self.nseg, self.smean, self.sinv, self.gamma, self.scale, self.shift)

    def check(self, da, dy, sums, bound):
        dy_tol = DY_TOL if self.dtype == torch.float32 else BF16_TOL
        ry, rg, rb, rbias, _ = self.reference(da)
        errs = dict(dy=rel(dy, ry), dgamma=rel(sums[0], rg), dbeta=rel(sums[1], rb), dbias=rel(sums[2], rbias))
        print(errs, 'dy_bound', None if bound is None else bound.item(), 'max|dy|', ry.abs().max().item())
        assert errs['dy'] < dy_tol, errs
        assert errs['dgamma'] < SUM_TOL and errs['dbeta'] < SUM_TOL, errs
        assert errs['dbias'] < (SUM_TOL if self.dtype == torch.float32 else BF16_TOL), errs
        if bound is not None:
            assert bound.item() >= dy.float().abs().max().item() > 0
            assert bound.item() >= ry.abs().max().item() * (1 - dy_tol)


@pytest.mark.parametrize('nseg', [1, 2])
def test_frozen_plain(dev, nseg):
    """The plain walk on an odd map, (n, h, w, c) = (2, 5, 7, 8)."""
    from multimodal_siamese_cd_amd import hip
    k = Case(dev, 2, 5, 7, 8, nseg, 11 + nseg)
    da = k.rand(2, 5, 7, 8)
    dy, sums = k.outputs()
    bound = torch.zeros(1, device=dev)
    hip.bn_relu_backward(hip.nhwc(k.y), hip.nhwc(da), *k.args(), *sums, hip.nhwc(dy), k.ws, bound, frozen=True)
    k.check(da, dy, sums, bound)


def test_frozen_differs_from_train_mode(dev):
    """The same call without the flag is the train-mode formula on the handed statistics: another dy.  (Guards the
    test above against a flag that does nothing.)"""
    from multimodal_siamese_cd_amd import hip
    k = Case(dev, 2, 5, 7, 8, 1, 5)
    da = k.rand(2, 5, 7, 8)
    outs = []
    for frozen in (True, False):
        dy, sums = k.outputs()
        hip.bn_relu_backward(hip.nhwc(k.y), hip.nhwc(da), *k.args(), *sums, hip.nhwc(dy), k.ws, None, frozen=frozen)
        outs.append((dy, sums))
    assert torch.equal(outs[0][1][0], outs[1][1][0]) and torch.equal(outs[0][1][1], outs[1][1][1])  # the sums
    assert rel(outs[1][0], outs[0][0]) > 1e-2


def _host_tile_records(k, da, tile_px=128):
    """The partial sums a data-grad conv epilogue records per tile of `tile_px` pixels and channel: {sum dz,
    sum dz*xhat}, xhat from the handed (running) mean / invstd; rec[c][tile][2]."""
    n, h, w, c = k.shape
    y = k.y.double().cpu()
    z = y * k.scale[:c].double().cpu() + k.shift[:c].double().cpu()
    dz = torch.where(z > 0, da.double().cpu(), torch.zeros((), dtype=torch.float64)).reshape(-1, tile_px, c)
    xh = ((y - k.smean[:c].double().cpu()) * k.sinv[:c].double().cpu()).reshape(-1, tile_px, c)
    rec = torch.stack([dz.sum(1), (dz * xh).sum(1)], -1).permute(1, 0, 2).contiguous().float().to(k.dev)
    return rec, dz.shape[0]


@pytest.mark.parametrize('dtype', [torch.float32, torch.bfloat16])
def test_frozen_tile_records(dev, dtype):
    """Partial sums from tile records (as the data-grad conv's epilogue leaves them), then the apply pass:
    (2, 16, 16, 64), fp32 and bf16 storage."""
    from multimodal_siamese_cd_amd import hip
    k = Case(dev, 2, 16, 16, 64, 2, 21, dtype)
    da = k.rand(2, 16, 16, 64)
    rec, ntiles = _host_tile_records(k, da)
    dy, sums = k.outputs()
    bound = torch.zeros(1, device=dev)
    hip.bn_relu_backward_tiles(hip.nhwc(k.y), hip.nhwc(da), *k.args(), rec, ntiles, *sums, hip.nhwc(dy), k.ws, bound,
                               frozen=True)
    k.check(da, dy, sums, bound)


@pytest.mark.parametrize('tiles', [False, True])
@pytest.mark.parametrize('math,dtype,co', [('h2', torch.float32, 128), ('bf16', torch.bfloat16, 64)])
def test_frozen_coef_and_weight_grad_forms_dy(dev, math, dtype, co, tiles):
    """The coefficient-only form and its consumer, the halo weight grad that forms dy while staging and stores it
    (scd_wgrad_t.rows_y / rows_out), on a (2, 16, 16) map with a 64-channel source: zero coefficients, the sums and the
    conv-bias grad from them, the h2 operand bound from the statistics, the stored dy, its exact bound, and the weight
    grad of that dy.  h2 takes 128 rows (its kernel has no 64-row block), bf16 storage 64."""
    from multimodal_siamese_cd_amd import hip
    n, h, w, ci = 2, 16, 16, 64
    k = Case(dev, n, h, w, co, 2, 31 + co, dtype)
    da = k.rand(n, h, w, co)
    x = k.rand(n, h, w, ci)
    h2 = math == 'h2'
    rec, ntiles = _host_tile_records(k, da) if tiles else (None, 0)
    prev = hip.set_conv_math(math)
    try:
        da_bound = da.float().abs().max().reshape(1) if h2 else None
        rows_bound = torch.zeros(1, device=dev) if h2 else None
        x_bound = x.float().abs().max().reshape(1) if h2 else None
        assert hip.wgrad_rows_bn_supported(hip.nhwc(da), hip.nhwc(x), 1, hip.TAPS_3X3, None, rows_bound, x_bound)
        coef = torch.full((2 * co * 2,), float('nan'), device=dev)
        _, sums = k.outputs()
        hip.bn_relu_backward_coef(hip.nhwc(k.y), hip.nhwc(da), *k.args(), rec, ntiles, coef, *sums, k.ws, da_bound,
                                  rows_bound, frozen=True)
        assert (coef == 0).all()
        dy = torch.full_like(k.y, float('nan'))
        out_bound = torch.zeros(1, device=dev)
        rows_bn = (hip.nhwc(k.y), 2, k.smean, k.sinv, k.gamma, k.scale, k.shift, coef)
        d, nsplit, nbytes = hip.wgrad_plan(hip.nhwc(da), hip.nhwc(x), 1, hip.TAPS_3X3, None, rows_bound, x_bound,
                                           rows_bn=rows_bn, rows_out=hip.nhwc(dy), rows_out_bound=out_bound)
        assert hip.wgrad_arith(d) == math
        slabs = torch.empty(nbytes // 4, device=dev)
        hip.conv_wgrad(d, slabs)
        dw = torch.empty(co, ci, 3, 3, device=dev)
        hip.wgrad_finalize(slabs, nsplit, co, 9, ci, 0, ci, dw)
        torch.cuda.synchronize()
    finally:
        hip.set_conv_math(prev)
    ry, rg, rb, rbias, _ = k.reference(da)
    errs = dict(dy=rel(dy, ry), dgamma=rel(sums[0], rg), dbeta=rel(sums[1], rb), dbias=rel(sums[2], rbias))
    exact = torch.nn.grad.conv2d_weight(x.double().cpu().permute(0, 3, 1, 2), (co, ci, 3, 3),
                                        dy.double().cpu().permute(0, 3, 1, 2), padding=1)
    errs['dw'] = rel(dw, exact)
    print(errs, 'rows bound', None if rows_bound is None else rows_bound.item(), 'max|dy|', ry.abs().max().item())
    assert errs['dy'] < (DY_TOL if dtype == torch.float32 else BF16_TOL), errs
    # the sums and the conv-bias grad come from the records alone (fp32 sums, no stored value): the fp32 bar
    assert errs['dgamma'] < SUM_TOL and errs['dbeta'] < SUM_TOL and errs['dbias'] < SUM_TOL, errs
    assert errs['dw'] < (2e-6 if h2 else 2e-2), errs
    assert out_bound.item() == dy.float().abs().max().item()
    if h2:
        assert rows_bound.item() >= ry.abs().max().item()


def _pool_idx(k, n, h, w, c):
    from multimodal_siamese_cd_amd import hip
    src = k.rand(n, h, w, c)
    idx = torch.empty(n, h // 2, w // 2, c, dtype=torch.uint8, device=k.dev)
    hip.maxpool2_fwd(hip.nhwc(src), hip.nhwc(torch.empty(n, h // 2, w // 2, c, device=k.dev, dtype=k.dtype)), idx)
    return idx


@pytest.mark.parametrize('mode', [0, 1, 2])
def test_frozen_pooled(dev, mode):
    """The pooled forms on (4, 8, 8, 64) with a 2x2-pooled gradient: a plain skip over all images (mode 0), the
    Siamese pair walk (mode 1: the shared difference gradient, t1 images subtract) and the second, swapped skip of
    the dual-task encoder (mode 2, scd_bn_relu_backward_pooled2).  The incoming gradient of the reference is
    materialised by scd_feature_grad, which the pooled forms state they reproduce."""
    from multimodal_siamese_cd_amd import hip
    n, h, w, c = 4, 8, 8, 64
    k = Case(dev, n, h, w, c, 2, 41 + mode)
    gy = k.rand(n, h // 2, w // 2, c)
    idx = _pool_idx(k, n, h, w, c)
    gs = k.rand(n if mode == 0 else n // 2, h, w, c)
    da = torch.empty_like(k.y)
    hip.feature_grad(hip.nhwc(gy), idx, hip.nhwc(gs), min(mode, 1), hip.nhwc(da))
    dy, sums = k.outputs()
    bound = torch.zeros(1, device=dev)
    if mode == 2:
        gs2 = k.rand(n, h, w, c)
        da = da + torch.cat([gs2[n // 2:], gs2[:n // 2]])  # image i takes gskip2 of the other date
        hip.bn_relu_backward_pooled2(hip.nhwc(k.y), hip.nhwc(gy), idx, hip.nhwc(gs), 2, hip.nhwc(gs2), *k.args(),
                                     *sums, hip.nhwc(dy), k.ws, bound, frozen=True)
    else:
        hip.bn_relu_backward_pooled(hip.nhwc(k.y), hip.nhwc(gy), idx, hip.nhwc(gs), mode, *k.args(), *sums,
                                    hip.nhwc(dy), k.ws, bound, frozen=True)
    k.check(da, dy, sums, bound)


@pytest.mark.parametrize('with_wgrad', [True, False])
@pytest.mark.parametrize('n_out', [1, 3])
def test_frozen_head(dev, n_out, with_wgrad):
    """The head form: dL/da = gout . w_head formed on the fly, and the head's weight grad from the same pass."""
    from multimodal_siamese_cd_amd import hip
    n, h, w, c = 2, 5, 7, 8
    k = Case(dev, n, h, w, c, 1, 51 + n_out)
    gout = k.rand(n, n_out, h, w)
    w_head = k.rand(n_out, c)
    da = torch.einsum('nohw,oc->nhwc', gout.double().cpu(), w_head.double().cpu())
    dy, sums = k.outputs()
    bound = torch.zeros(1, device=dev)
    wg = torch.full((n_out, c), float('nan'), device=dev) if with_wgrad else None
    ws = torch.empty(hip.bn_head_workspace_bytes(n, h, w, c, 1, n_out), dtype=torch.uint8, device=dev)
    hip.bn_relu_backward_head(hip.nhwc(k.y), gout, w_head, n_out, *k.args(), *sums, hip.nhwc(dy), ws, bound, wg,
                              frozen=True)
    k.check(da, dy, sums, bound)
    if with_wgrad:
        a = k.reference(da)[4]
        ref = torch.einsum('nohw,nhwc->oc', gout.double().cpu(), a)
        print('head weight grad', rel(wg, ref))
        assert rel(wg, ref) < SUM_TOL
