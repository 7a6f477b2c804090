"""scd_bn_relu_through, the reduction-free backward through a frozen BatchNorm + ReLU (dy = gamma*invstd * g*[relu']),
every accepted form in the cases of tests/test_frozen_bn_kernels_gpu.py.

Bars: that file's, because this is the same formula: dy against the fp64 reference within DY_TOL 1e-4 (fp32) or 2^-8
(bf16 storage, one rounding of the stored element).  Against the frozen form of scd_bn_relu_backward_desc the stored dy
is bit-equal: with k1 = k2 = 0 and finite y that form stores mul*(dz - 0 - xhat*0) = mul*dz with the same mul
(torch.equal ignores the sign of a zero).  dy_bound is the max of the stored |dy| (an integer atomic max of the float's
bits), so it is >= that maximum and, the gradients being random, > 0.  What is not passed is not written: NaN-filled
dgamma / dbeta / conv-bias buffers stay NaN, and a 1-byte workspace is accepted because none is read."""
import pytest
import torch

from test_frozen_bn_kernels_gpu import BF16_TOL, DY_TOL, Case, _pool_idx, dev, rel  # noqa: F401  (dev: the fixture)

pytestmark = pytest.mark.gpu

DTYPES = [torch.float32, torch.bfloat16]


def _run_both(k, form, da_ref, frozen_call, **fields):
    """The through pass and the frozen reducing form on the same inputs; checks the properties every form shares and
    returns the through dy."""
    from multimodal_siamese_cd_amd import hip
    dev_ = k.dev
    dy, sums = k.outputs()
    bound = torch.zeros(1, device=dev_)
    ws1 = torch.empty(1, dtype=torch.uint8, device=dev_)
    hip.bn_relu_through(form, hip.nhwc(k.y), *k.args(), hip.nhwc(dy), bound, ws=ws1.data_ptr(), ws_bytes=1, **fields)
    dy_f, sums_f = k.outputs()
    bound_f = torch.zeros(1, device=dev_)
    frozen_call(dy_f, sums_f, bound_f)
    torch.cuda.synchronize()
    tol = DY_TOL if k.dtype == torch.float32 else BF16_TOL
    ref = k.reference(da_ref)[0]
    err = rel(dy, ref)
    print('form', form, 'dy err', err, 'dy_bound', bound.item(), 'max|dy|', dy.float().abs().max().item(),
          'frozen dy_bound', bound_f.item())
    assert err < tol
    assert torch.equal(dy, dy_f)
    assert bound.item() >= dy.float().abs().max().item() > 0
    assert bound.item() == bound_f.item()
    assert all(torch.isnan(t).all() for t in sums)  # never passed: never written
    assert all(torch.isfinite(t).all() for t in sums_f)
    return dy


@pytest.mark.parametrize('dtype', DTYPES)
@pytest.mark.parametrize('nseg', [1, 2])
def test_through_plain(dev, nseg, dtype):
    """The plain walk on an odd map, (n, h, w, c) = (2, 5, 7, 8)."""
    from multimodal_siamese_cd_amd import hip
    k = Case(dev, 2, 5, 7, 8, nseg, 11 + nseg, dtype)
    da = k.rand(2, 5, 7, 8)
    _run_both(k, hip.BN_BWD_PLAIN, da,
              lambda dy, sums, b: hip.bn_relu_backward(hip.nhwc(k.y), hip.nhwc(da), *k.args(), *sums, hip.nhwc(dy),
                                                       k.ws, b, frozen=True), da=hip.nhwc(da))


@pytest.mark.parametrize('dtype', DTYPES)
def test_through_plain_multi_block(dev, dtype):
    """(2, 16, 16, 64): several chunks per segment and the four-pixel main loop (test_frozen_tile_records' shape)."""
    from multimodal_siamese_cd_amd import hip
    k = Case(dev, 2, 16, 16, 64, 2, 21, dtype)
    da = k.rand(2, 16, 16, 64)
    _run_both(k, hip.BN_BWD_PLAIN, da,
              lambda dy, sums, b: hip.bn_relu_backward(hip.nhwc(k.y), hip.nhwc(da), *k.args(), *sums, hip.nhwc(dy),
                                                       k.ws, b, frozen=True), da=hip.nhwc(da))


@pytest.mark.parametrize('dtype', DTYPES)
@pytest.mark.parametrize('shape', [(4, 8, 8, 64), (4, 7, 5, 64)])
@pytest.mark.parametrize('mode', [0, 1, 2])
def test_through_pooled(dev, mode, shape, dtype):
    """The pooled forms with a 2x2-pooled gradient, on an even and an odd map: a plain skip over all images (mode 0),
    the Siamese pair walk (mode 1, two segments) and pooled2 (mode 2).  The reference's incoming gradient is
    materialised by scd_feature_grad, which the pooled forms state they reproduce."""
    from multimodal_siamese_cd_amd import hip
    n, h, w, c = shape
    k = Case(dev, n, h, w, c, 2, 41 + mode, dtype)
    gy = k.rand(n, h // 2, w // 2, c)
    idx = _pool_idx(k, n, h, w, c)
    gs = k.rand(n if mode == 0 else n // 2, h, w, c)
    # the reference's gradient in fp32 whatever the storage: bf16 operands are exact in fp32, and the kernel adds them
    # in fp32 too, so no rounding of a stored bf16 sum enters the reference
    da = torch.empty(n, h, w, c, device=dev)
    hip.feature_grad(hip.nhwc(gy.float()), idx, hip.nhwc(gs.float()), min(mode, 1), hip.nhwc(da))
    fields = dict(gy=hip.nhwc(gy), idx=idx.data_ptr(), gskip=hip.nhwc(gs), skip_mode=mode)
    if mode == 2:
        gs2 = k.rand(n, h, w, c)
        # image i takes gskip2 of the other date; the kernel adds the two skip terms first (one rounding each way)
        da = da + torch.cat([gs2[n // 2:], gs2[:n // 2]]).float()
        _run_both(k, hip.BN_BWD_POOLED2, da,
                  lambda dy, sums, b: hip.bn_relu_backward_pooled2(hip.nhwc(k.y), hip.nhwc(gy), idx, hip.nhwc(gs), 2,
                                                                   hip.nhwc(gs2), *k.args(), *sums, hip.nhwc(dy), k.ws,
                                                                   b, frozen=True), gskip2=hip.nhwc(gs2), **fields)
    else:
        _run_both(k, hip.BN_BWD_POOLED, da,
                  lambda dy, sums, b: hip.bn_relu_backward_pooled(hip.nhwc(k.y), hip.nhwc(gy), idx, hip.nhwc(gs), mode,
                                                                  *k.args(), *sums, hip.nhwc(dy), k.ws, b,
                                                                  frozen=True), **fields)


def test_through_pooled_without_pooled_gradient(dev):
    """The deepest level: only the Siamese difference gradient (gy null), the pair walk."""
    from multimodal_siamese_cd_amd import hip
    n, h, w, c = 4, 5, 7, 8
    k = Case(dev, n, h, w, c, 2, 47)
    gs = k.rand(n // 2, h, w, c)
    da = torch.cat([-gs, gs])
    _run_both(k, hip.BN_BWD_POOLED, da,
              lambda dy, sums, b: hip.bn_relu_backward_pooled(hip.nhwc(k.y), hip._NULL, None, hip.nhwc(gs), 1,
                                                              *k.args(), *sums, hip.nhwc(dy), k.ws, b, frozen=True),
              gskip=hip.nhwc(gs), skip_mode=1)


@pytest.mark.parametrize('dtype', DTYPES)
@pytest.mark.parametrize('n_out', [1, 3])
def test_through_head(dev, n_out, dtype):
    """The head form: dL/da = gout . w_head formed on the fly (fp32 gradient and weights in either storage)."""
    from multimodal_siamese_cd_amd import hip
    n, h, w, c = 2, 5, 7, 8
    k = Case(dev, n, h, w, c, 1, 51 + n_out, dtype)
    gout = k.rand(n, n_out, h, w).float()
    w_head = k.rand(n_out, c).float()
    da = torch.einsum('nohw,oc->nhwc', gout.double().cpu(), w_head.double().cpu())
    _run_both(k, hip.BN_BWD_HEAD, da,
              lambda dy, sums, b: hip.bn_relu_backward_head(hip.nhwc(k.y), gout, w_head, n_out, *k.args(), *sums,
                                                            hip.nhwc(dy), k.ws, b, None, frozen=True),
              gout=gout.data_ptr(), w_head=w_head.data_ptr(), n_out=n_out)


@pytest.mark.parametrize('dtype', DTYPES)
def test_through_channel_slice(dev, dtype):
    """y and dy as channel slices of wider buffers (ldc > c), as the concat buffers produce; the channels outside the
    slice keep their contents."""
    from multimodal_siamese_cd_amd import hip
    n, h, w, c, wide = 2, 5, 7, 8, 24
    k = Case(dev, n, h, w, c, 2, 61, dtype)
    ybuf = k.rand(n, h, w, wide)
    ybuf[..., 8:16] = k.y
    da = k.rand(n, h, w, c)
    dybuf = torch.full((n, h, w, wide), 7.0, device=dev, dtype=dtype)
    bound = torch.zeros(1, device=dev)
    hip.bn_relu_through(hip.BN_BWD_PLAIN, hip.nhwc(ybuf, 8, c), *k.args(), hip.nhwc(dybuf, 4, c), bound,
                        da=hip.nhwc(da))
    dense, _ = k.outputs()
    hip.bn_relu_through(hip.BN_BWD_PLAIN, hip.nhwc(k.y), *k.args(), hip.nhwc(dense), None, da=hip.nhwc(da))
    torch.cuda.synchronize()
    got = dybuf[..., 4:12]
    err = rel(got, k.reference(da)[0])
    print('slice dy err', err, 'bound', bound.item())
    assert err < (DY_TOL if dtype == torch.float32 else BF16_TOL)
    assert torch.equal(got, dense)
    assert (dybuf[..., :4] == 7).all() and (dybuf[..., 12:] == 7).all()
    assert bound.item() == got.float().abs().max().item() > 0


def test_through_refuses_before_launch(dev):
    """A shape mismatch on real device tensors is refused on the host with `through:`, dy untouched."""
    from multimodal_siamese_cd_amd import hip
    k = Case(dev, 2, 5, 7, 8, 1, 71)
    da = k.rand(2, 5, 7, 4)
    dy, _ = k.outputs()
    with pytest.raises(RuntimeError, match='through:'):
        hip.bn_relu_through(hip.BN_BWD_PLAIN, hip.nhwc(k.y), *k.args(), hip.nhwc(dy), None, da=hip.nhwc(da))
    torch.cuda.synchronize()
    assert torch.isnan(dy).all()
