"""The six positional BatchNorm + ReLU backward exports, which hip.py no longer calls, raw through hip.lib(), against
the named wrappers (the descriptor path) on the same inputs: every output is bit-equal (torch.equal).  Both are the
same kernels on the same arguments, so there is no tolerance.  The written outputs start as NaN (a value left unwritten
fails the comparison); dy_bound starts at zero, as its callers hand it, because the kernels raise it by an integer
atomic max of the float's bits.

Shapes are the smallest at which each walk's branches are live, as in tests/test_frozen_bn_kernels_gpu.py, whose Case
supplies the tensors (its statistics are merely some statistics here: train mode takes them as handed)."""
import pytest
import torch

from test_bn_bwd_positional_abi import EXPORTS
from test_frozen_bn_kernels_gpu import Case, _host_tile_records, _pool_idx, dev  # noqa: F401  (dev: the fixture)

pytestmark = pytest.mark.gpu

VIEWS = ('y', 'dy', 'da', 'gy', 'gskip', 'gskip2')
OUTPUTS = ('dy', 'dgamma', 'dbeta', 'dbias_prev', 'dy_bound', 'w_grad', 'coef')

# the named wrapper of each form on a dict t of descriptor field -> tensor (None: absent) or int
WRAPPERS = {
    'plain': lambda hip, v, t: hip.bn_relu_backward(
        v('y'), v('da'), t['nseg'], t['mean'], t['invstd'], t['gamma'], t['scale'], t['shift'], t['dgamma'],
        t['dbeta'], t['dbias_prev'], v('dy'), t['ws'], t['dy_bound']),
    'tiles': lambda hip, v, t: hip.bn_relu_backward_tiles(
        v('y'), v('da'), t['nseg'], t['mean'], t['invstd'], t['gamma'], t['scale'], t['shift'], t['tile_rec'],
        t['ntiles'], t['dgamma'], t['dbeta'], t['dbias_prev'], v('dy'), t['ws'], t['dy_bound']),
    'pooled': lambda hip, v, t: hip.bn_relu_backward_pooled(
        v('y'), v('gy'), t['idx'], v('gskip'), t['skip_mode'], t['nseg'], t['mean'], t['invstd'], t['gamma'],
        t['scale'], t['shift'], t['dgamma'], t['dbeta'], t['dbias_prev'], v('dy'), t['ws'], t['dy_bound']),
    'pooled2': lambda hip, v, t: hip.bn_relu_backward_pooled2(
        v('y'), v('gy'), t['idx'], v('gskip'), t['skip_mode'], v('gskip2'), t['nseg'], t['mean'], t['invstd'],
        t['gamma'], t['scale'], t['shift'], t['dgamma'], t['dbeta'], t['dbias_prev'], v('dy'), t['ws'], t['dy_bound']),
    'head': lambda hip, v, t: hip.bn_relu_backward_head(
        v('y'), t['gout'], t['w_head'], t['n_out'], t['nseg'], t['mean'], t['invstd'], t['gamma'], t['scale'],
        t['shift'], t['dgamma'], t['dbeta'], t['dbias_prev'], v('dy'), t['ws'], t['dy_bound'], t['w_grad']),
    'coef': lambda hip, v, t: hip.bn_relu_backward_coef(
        v('y'), v('da'), t['nseg'], t['mean'], t['invstd'], t['gamma'], t['scale'], t['shift'], t['tile_rec'],
        t['ntiles'], t['coef'], t['dgamma'], t['dbeta'], t['dbias_prev'], t['ws'], t['da_bound'], t['dy_bound']),
}


def _inputs(k, **form_fields):
    return dict(y=k.y, nseg=k.nseg, mean=k.smean, invstd=k.sinv, gamma=k.gamma, scale=k.scale, shift=k.shift,
                ws=k.ws, **form_fields)


def _fresh_outputs(k, t, want):
    """t with the outputs named in `want` as new buffers: NaN, dy_bound zero."""
    c, nan = k.c, float('nan')
    new = dict(dy=lambda: torch.full_like(k.y, nan), dy_bound=lambda: torch.zeros(1, device=k.dev),
               w_grad=lambda: torch.full((t.get('n_out', 0), c), nan, device=k.dev),
               coef=lambda: torch.full((k.nseg * c * 2,), nan, device=k.dev))
    vec = lambda: torch.full((c,), nan, device=k.dev)  # noqa: E731
    return dict(t, **{o: new.get(o, vec)() if o in want else None for o in OUTPUTS})


def _positional(hip, form, t):
    """The raw export of `form` on t: views by value, tensors by pointer, the workspace with its size."""
    def arg(name):
        x = t.get(name)
        if name in VIEWS:
            return hip.nhwc(x)
        if name == 'ws_bytes':
            return t['ws'].numel()
        return x.data_ptr() if isinstance(x, torch.Tensor) else x

    symbol, order = EXPORTS[form]
    rc = getattr(hip.lib(), symbol)(*(arg(n) for n in order.split()), torch.cuda.current_stream().cuda_stream)
    assert rc == 0, hip.lib().scd_last_error()


def _compare(k, form, t, want, wrapper=None):
    """The positional export of `form` and the named wrapper (of `wrapper`, where that is another form) on the same
    inputs t, each with its own outputs `want`."""
    from multimodal_siamese_cd_amd import hip
    a, b = _fresh_outputs(k, t, want), _fresh_outputs(k, t, want)
    _positional(hip, form, a)
    WRAPPERS[wrapper or form](hip, lambda name: hip.nhwc(b.get(name)), b)
    torch.cuda.synchronize()
    for o in want:
        assert not torch.isnan(a[o].float()).any(), o
        assert torch.equal(a[o], b[o]), o
    if 'dy_bound' in want and 'dy' in want:
        assert a['dy_bound'].item() >= a['dy'].float().abs().max().item() > 0


SUMS = ('dgamma', 'dbeta', 'dbias_prev')
APPLY = ('dy', 'dy_bound') + SUMS


@pytest.mark.parametrize('dtype', [torch.float32, torch.bfloat16])
@pytest.mark.parametrize('nseg', [1, 2])
def test_plain(dev, nseg, dtype):
    k = Case(dev, 2, 5, 7, 8, nseg, 11 + nseg, dtype)
    _compare(k, 'plain', _inputs(k, da=k.rand(2, 5, 7, 8)), APPLY)


def test_pooled_plain_skip_on_an_odd_map(dev):
    """skip_mode 0 on (2, 5, 7, 8): the edge cells of an odd map."""
    n, h, w, c = 2, 5, 7, 8
    k = Case(dev, n, h, w, c, 2, 41)
    t = _inputs(k, gy=k.rand(n, h // 2, w // 2, c), idx=_pool_idx(k, n, h, w, c), gskip=k.rand(n, h, w, c),
                skip_mode=0)
    _compare(k, 'pooled', t, APPLY)


@pytest.mark.parametrize('absent', [None, 'gy', 'gskip'])
def test_pooled_siamese_pair(dev, absent):
    """skip_mode 1 with two segments on (4, 6, 10, 8): the pair walk; then without the pooled gradient (the deepest
    level) and without the skip gradient."""
    n, h, w, c = 4, 6, 10, 8
    k = Case(dev, n, h, w, c, 2, 42)
    t = _inputs(k, gy=k.rand(n, h // 2, w // 2, c), idx=_pool_idx(k, n, h, w, c), gskip=k.rand(n // 2, h, w, c),
                skip_mode=1)
    if absent == 'gy':
        t.update(gy=None, idx=None)
    elif absent == 'gskip':
        t['gskip'] = None
    _compare(k, 'pooled', t, APPLY)


@pytest.mark.parametrize('skip_mode', [2, 1])
def test_pooled2(dev, skip_mode):
    """The second skip gradient on (4, 6, 10, 8); and the positional export with skip_mode 1 and no second skip, which
    is scd_bn_relu_backward_pooled."""
    n, h, w, c = 4, 6, 10, 8
    k = Case(dev, n, h, w, c, 2, 43)
    t = _inputs(k, gy=k.rand(n, h // 2, w // 2, c), idx=_pool_idx(k, n, h, w, c), gskip=k.rand(n // 2, h, w, c),
                skip_mode=skip_mode, gskip2=k.rand(n, h, w, c) if skip_mode == 2 else None)
    _compare(k, 'pooled2', t, APPLY, wrapper='pooled2' if skip_mode == 2 else 'pooled')


@pytest.mark.parametrize('with_wgrad', [True, False])
@pytest.mark.parametrize('n_out', [1, 3])
def test_head(dev, n_out, with_wgrad):
    from multimodal_siamese_cd_amd import hip
    n, h, w, c = 2, 5, 7, 8
    k = Case(dev, n, h, w, c, 1, 51 + n_out)
    t = _inputs(k, gout=k.rand(n, n_out, h, w), w_head=k.rand(n_out, c), n_out=n_out)
    t['ws'] = torch.empty(hip.bn_head_workspace_bytes(n, h, w, c, 1, n_out), dtype=torch.uint8, device=dev)
    _compare(k, 'head', t, APPLY + (('w_grad',) if with_wgrad else ()))


@pytest.mark.parametrize('dtype', [torch.float32, torch.bfloat16])
def test_tiles(dev, dtype):
    """Tile records as test_frozen_tile_records builds them, (2, 16, 16, 64)."""
    k = Case(dev, 2, 16, 16, 64, 2, 21, dtype)
    da = k.rand(2, 16, 16, 64)
    rec, ntiles = _host_tile_records(k, da)
    _compare(k, 'tiles', _inputs(k, da=da, tile_rec=rec, ntiles=ntiles), APPLY)


@pytest.mark.parametrize('tiles', [False, True])
def test_coef(dev, tiles):
    """The coefficient-only form on (2, 16, 16, 64), from a pass over (y, da) and from tile records, with the bound of
    the dy its consumer forms."""
    k = Case(dev, 2, 16, 16, 64, 2, 31)
    da = k.rand(2, 16, 16, 64)
    rec, ntiles = _host_tile_records(k, da) if tiles else (None, 0)
    t = _inputs(k, da=da, tile_rec=rec, ntiles=ntiles, da_bound=da.float().abs().max().reshape(1))
    _compare(k, 'coef', t, ('coef', 'dy_bound') + SUMS)
