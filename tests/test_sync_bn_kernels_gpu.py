"""The synchronized-BatchNorm kernels in one process: the statistics and every backward form cut in two around the
gather of the ranks' records (scd_bn_stats_local / _from_ranks, scd_bn_relu_backward_sums / _from_sums).

1. One rank: each pair is bit-identical (torch.equal) to the entry point it was cut from, in every output.
2. Shards of one batch as ranks (even 2+2 and uneven 1+3 images per segment; shard r holds its images of every segment):
   - statistics against an fp64 BatchNorm of the whole batch, 2e-6 relative, the bar tests/test_kernels_gpu.py holds
     the statistics to.  The entry point takes no rank, so its outputs cannot depend on one;
   - backward, with the whole batch run through scd_bn_relu_backward on the SAME coefficients (the synchronized ones,
     so that only the backward is compared): each shard's dy against its slice, the shards' dgamma / dbeta summed against
     the whole batch's, each shard's conv-bias grad against the sum of its dy -- all at 2e-6 of the tensor's maximum,
     that file's bar for a different order of the per-chunk sums.  bf16 storage: a stored dy element is rounded once to
     8 significant bits, and a last-bit difference in k1 / k2 can move it by one such step, so stored dy is held to
     2^-8 (the bar of tests/test_frozen_bn_kernels_gpu.py for one rounding of a stored element); the fp32 outputs
     (dgamma, dbeta, the bias grad of the applying forms, which sum the stored values) keep 2e-6.  The deferred form's
     bias grad is a closed form of the sums, judged against the fp64 sum of the dy its coefficients define.
"""
import types

import pytest
import torch

pytestmark = pytest.mark.gpu

DTYPES = [torch.float32, torch.bfloat16]
CHANNELS = [16, 64, 24]  # 24: six channel quads in blocks of four, a ragged second channel group
PER_SEG = 4  # images per segment
SPLITS = {'2+2': (2, 2), '1+3': (1, 3)}
TOL, BF16_TOL = 2e-6, 2.0 ** -8
FORMS = ['plain', 'tiles', 'pooled', 'pooled2', 'head', 'coef', 'coef_tiles']


@pytest.fixture(scope='module')
def dev():
    from multimodal_siamese_cd_amd import hip
    hip.load_library()
    d = torch.device('cuda:0')
    hip.ensure_device(torch.empty(1, device=d))
    return d


def rel(a, b):
    a, b = a.detach().double().cpu(), b.detach().double().cpu()
    return ((a - b).abs().max() / b.abs().max().clamp_min(1e-30)).item()


def _ws(nbytes, dev):
    return torch.empty(nbytes, dtype=torch.uint8, device=dev)


class Data:
    """A conv output y (n = PER_SEG * nseg images), BatchNorm parameters and one backward form's gradient sources."""

    def __init__(self, dev, h, w, c, nseg, dtype, seed):
        self.dev, self.h, self.w, self.c, self.nseg, self.dtype = dev, h, w, c, nseg, dtype
        self.n = PER_SEG * nseg
        self.g = torch.Generator().manual_seed(seed)
        self.y = self.rand(self.n, h, w, c, scale=2.0, shift=0.3)
        self.gamma = (torch.rand(c, generator=self.g) + 0.5).to(dev)
        self.beta = torch.randn(c, generator=self.g).to(dev)

    def rand(self, *shape, scale=1.0, shift=0.0, dtype=None):
        return (torch.randn(*shape, generator=self.g) * scale + shift).to(self.dev).to(dtype or self.dtype)

    def images(self, counts, r):
        """Image indices of shard r: its counts[r] images of every segment, segment-major."""
        lo = sum(counts[:r])
        return [s * PER_SEG + lo + i for s in range(self.nseg) for i in range(counts[r])]


def row_tile_stats(y, nseg):
    """Conv-epilogue statistics records with one tile per image row: rec[tile][c] = {mean, M2}, fp32."""
    n, h, w, c = y.shape
    t = y.float().reshape(n * h, w, c)
    mean = t.mean(1)
    return torch.stack([mean, ((t - mean[:, None]) ** 2).sum(1)], -1).contiguous(), n * h, w


def stats_whole(hip, d, y, tiles):
    """scd_bn_train_stats / scd_bn_stats_from_tiles with the running update: the 7 outputs."""
    c, nseg, dev = d.c, d.nseg, d.dev
    o = [torch.empty(nseg * c, device=dev) for _ in range(4)]
    rm, rv, bound = torch.full((c,), 0.25, device=dev), torch.full((c,), 1.5, device=dev), torch.zeros(1, device=dev)
    if tiles is not None:
        hip.bn_stats_from_tiles(tiles[0], tiles[1], tiles[2], c, nseg, d.gamma, d.beta, 1e-5, 0.1, True, rm, rv, *o,
                                _ws(hip.bn_tile_stats_workspace_bytes(tiles[1], c, nseg), dev), act_bound=bound)
    else:
        hip.bn_train_stats(hip.nhwc(y), nseg, d.gamma, d.beta, 1e-5, 0.1, True, rm, rv, *o,
                           _ws(hip.bn_workspace_bytes(*y.shape, nseg), dev), act_bound=bound)
    return o + [rm, rv, bound]


def stats_sync(hip, d, shards, tiles=None):
    """local per shard, stacked as the gather would, from_ranks: (the 7 outputs, the gathered records)."""
    c, nseg, dev = d.c, d.nseg, d.dev
    stats = torch.zeros((len(shards), nseg * c * 3), dtype=torch.float64, device=dev)
    for r, ys in enumerate(shards):
        tl = tiles[r] if tiles is not None else None
        ws = _ws(hip.bn_tile_stats_workspace_bytes(tl[1], c, nseg) if tl is not None else
                 hip.bn_workspace_bytes(*ys.shape, nseg), dev)
        hip.bn_stats_local(hip.nhwc(ys), nseg, stats[r], ws, tl)
    o = [torch.empty(nseg * c, device=dev) for _ in range(4)]
    rm, rv, bound = torch.full((c,), 0.25, device=dev), torch.full((c,), 1.5, device=dev), torch.zeros(1, device=dev)
    hip.bn_stats_from_ranks(stats, len(shards), c, nseg, d.gamma, d.beta, 1e-5, 0.1, True, rm, rv, *o, act_bound=bound)
    return o + [rm, rv, bound], stats


@pytest.mark.parametrize('dtype', DTYPES, ids=['f32', 'bf16'])
@pytest.mark.parametrize('nseg', [1, 2])
@pytest.mark.parametrize('c', CHANNELS)
def test_statistics_one_rank_bit_identical(dev, c, nseg, dtype):
    from multimodal_siamese_cd_amd import hip
    d = Data(dev, 18, 22, c, nseg, dtype, 100 + c + nseg)
    for tiles in (None, row_tile_stats(d.y, nseg)):
        whole = stats_whole(hip, d, d.y, tiles)
        sync, stats = stats_sync(hip, d, [d.y], None if tiles is None else [tiles])
        torch.cuda.synchronize()
        assert all(torch.equal(a, b) for a, b in zip(whole, sync)), 'tiles' if tiles else 'pass'
        assert whole[6].item() > 0
        assert torch.equal(stats.reshape(nseg, c, 3)[..., 0],
                           torch.full((nseg, c), float(PER_SEG * 18 * 22), dtype=torch.float64, device=dev))


@pytest.mark.parametrize('dtype', DTYPES, ids=['f32', 'bf16'])
@pytest.mark.parametrize('nseg', [1, 2])
@pytest.mark.parametrize('c', CHANNELS)
@pytest.mark.parametrize('split', list(SPLITS))
def test_statistics_of_shards(dev, split, c, nseg, dtype):
    from multimodal_siamese_cd_amd import hip
    d = Data(dev, 18, 22, c, nseg, dtype, 200 + c + nseg)
    counts = SPLITS[split]
    shards = [d.y[d.images(counts, r)].contiguous() for r in range(2)]
    y64 = d.y.double().cpu().reshape(nseg, -1, c)
    mean, var = y64.mean(1), y64.var(1, unbiased=False)
    inv = 1 / torch.sqrt(var + 1e-5)
    gamma, beta = d.gamma.double().cpu(), d.beta.double().cpu()
    rm, rv = torch.full((c,), 0.25, dtype=torch.float64), torch.full((c,), 1.5, dtype=torch.float64)
    for s in range(nseg):  # one update per segment, in order
        rm, rv = 0.9 * rm + 0.1 * mean[s], 0.9 * rv + 0.1 * y64[s].var(0, unbiased=True)
    ref = [mean, inv, gamma * inv, beta - mean * gamma * inv, rm, rv]
    for tiled in (False, True):
        got, _ = stats_sync(hip, d, shards, [row_tile_stats(ys, nseg) for ys in shards] if tiled else None)
        torch.cuda.synchronize()
        errs = [rel(a.reshape(b.shape), b) for a, b in zip(got, ref)]
        print(split, c, nseg, dtype, 'tiles' if tiled else 'pass', ['%.1e' % e for e in errs])
        assert max(errs) < TOL


# ---------------------------------------------------------------------------------------------------------------------
# backward
# ---------------------------------------------------------------------------------------------------------------------
class Form:
    """One backward form on data d (or on a shard of it): `call(sync)` runs hip's wrapper and returns its outputs
    {dy, dgamma, dbeta, dbias, dy_bound, coef, w_grad} (those the form has)."""

    def __init__(self, hip, d, form, st, src=None, images=None):
        """st: (smean, sinv, scale, shift); src: the gradient sources of the whole batch (made on first use, then
        sliced by `images` for a shard)."""
        self.hip, self.d, self.form, self.st = hip, d, form, st
        n, h, w, c, nseg = d.n, d.h, d.w, d.c, d.nseg
        if src is None:
            src = {}
            if form in ('plain', 'tiles', 'coef', 'coef_tiles'):
                src['da'] = d.rand(n, h, w, c)
            elif form in ('pooled', 'pooled2'):
                src['gy'] = d.rand(n, h // 2, w // 2, c)
                src['idx'] = torch.empty(n, h // 2, w // 2, c, dtype=torch.uint8, device=d.dev)
                hip.maxpool2_fwd(hip.nhwc(d.rand(n, h, w, c)), hip.nhwc(torch.empty_like(src['gy'])), src['idx'])
                # one segment: a plain skip over all images; two: the Siamese difference gradient (the pair walk)
                src['gs'] = d.rand(n if nseg == 1 else n // 2, h, w, c)
                if form == 'pooled2':
                    src['gs2'] = d.rand(n, h, w, c)
            else:
                src['gout'] = d.rand(n, 2, h, w, dtype=torch.float32)
                src['w_head'] = d.rand(2, c, dtype=torch.float32)
        self.src = src
        pick = (lambda t: t) if images is None else (lambda t: t[images].contiguous())
        self.y = pick(d.y)
        self.t = {k: (v if k == 'w_head' else pick(v) if v.shape[0] == d.n else
                      pick(torch.cat([v, v]))[:len(images) // 2].contiguous() if images is not None else v)
                  for k, v in src.items()}

    def tile_sums(self):
        """Data-grad-epilogue records with one tile per image row: rec[c][tile] = {sum dz, sum dz*xhat}, fp32."""
        d, y, da = self.d, self.y.float(), self.t['da'].float()
        n, h, w, c = y.shape
        seg = torch.arange(n, device=d.dev) // (n // d.nseg)
        mu, iv, sc, sf = (t.reshape(d.nseg, c)[seg][:, None, None, :] for t in self.st)
        dz = da * (y.double() * sc.double() + sf.double() > 0)  # the sign fma(y, sc, sf) has: the product is exact
        rec = torch.stack([dz.sum(2), (dz * ((y - mu) * iv)).sum(2)], -1)  # [n][h][c][2]
        return rec.reshape(n * h, c, 2).permute(1, 0, 2).contiguous(), n * h

    def call(self, sync=None):
        hip, d, t, y = self.hip, self.d, self.t, self.y
        n, h, w, c = y.shape
        nseg, dev = d.nseg, d.dev
        o = dict(dgamma=torch.empty(c, device=dev), dbeta=torch.empty(c, device=dev),
                 dbias=torch.empty(c, device=dev), dy_bound=torch.zeros(1, device=dev))
        ws = _ws(hip.bn_head_workspace_bytes(n, h, w, c, nseg, 2), dev)
        st, sums = self.st, (o['dgamma'], o['dbeta'], o['dbias'])
        if self.form.startswith('coef'):
            o['coef'] = torch.empty(nseg * c * 2, device=dev)
            da_bound = t['da'].float().abs().max().reshape(1)
            rec, ntiles = self.tile_sums() if self.form == 'coef_tiles' else (None, 0)
            hip.bn_relu_backward_coef(hip.nhwc(y), hip.nhwc(t['da']), nseg, st[0], st[1], d.gamma, st[2], st[3], rec,
                                      ntiles, o['coef'], *sums, ws, da_bound, o['dy_bound'], sync=sync)
            return o
        o['dy'] = torch.full_like(y, float('nan'))
        args = (nseg, st[0], st[1], d.gamma, st[2], st[3], *sums, hip.nhwc(o['dy']), ws, o['dy_bound'])
        if self.form == 'plain':
            hip.bn_relu_backward(hip.nhwc(y), hip.nhwc(t['da']), *args, sync=sync)
        elif self.form == 'tiles':
            rec, ntiles = self.tile_sums()
            hip.bn_relu_backward_tiles(hip.nhwc(y), hip.nhwc(t['da']), *args[:6], rec, ntiles, *args[6:], sync=sync)
        elif self.form == 'pooled':
            hip.bn_relu_backward_pooled(hip.nhwc(y), hip.nhwc(t['gy']), t['idx'], hip.nhwc(t['gs']),
                                        0 if nseg == 1 else 1, *args, sync=sync)
        elif self.form == 'pooled2':
            hip.bn_relu_backward_pooled2(hip.nhwc(y), hip.nhwc(t['gy']), t['idx'], hip.nhwc(t['gs']), 2,
                                         hip.nhwc(t['gs2']), *args, sync=sync)
        else:
            o['w_grad'] = torch.empty(2, c, device=dev)
            hip.bn_relu_backward_head(hip.nhwc(y), t['gout'], t['w_head'], 2, *args, w_grad=o['w_grad'], sync=sync)
        return o


def _sync(stats, rank, log=None):
    """What engine._BNSync is to hip's wrappers, with the gather done by the test: `fill(buf)` puts the other ranks'
    slots in (nothing for one rank)."""
    def gather(buf):
        if log is not None:
            log(buf)
        return buf
    return types.SimpleNamespace(world=stats.shape[0], rank=rank, stats=stats, gather=gather)


def _cases(forms):
    for form in forms:
        for nseg in (1, 2):
            if form == 'pooled2' and nseg == 1:
                continue  # the dual-task form has two segments by definition
            for c in CHANNELS:
                yield pytest.param(form, nseg, c, id=f'{form}-nseg{nseg}-c{c}')


@pytest.mark.parametrize('dtype', DTYPES, ids=['f32', 'bf16'])
@pytest.mark.parametrize('form,nseg,c', _cases(FORMS))
def test_backward_one_rank_bit_identical(dev, form, nseg, c, dtype):
    from multimodal_siamese_cd_amd import hip
    h, w = (16, 24) if form.startswith('pooled') else (18, 22)
    d = Data(dev, h, w, c, nseg, dtype, 300 + c + nseg)
    out, stats = stats_sync(hip, d, [d.y])
    f = Form(hip, d, form, out[:4])
    whole = f.call()
    sync = f.call(_sync(stats, 0))
    torch.cuda.synchronize()
    assert set(whole) == set(sync)
    for k in whole:
        assert torch.isfinite(whole[k].float()).all(), k
        assert torch.equal(whole[k], sync[k]), k
    assert whole['dy_bound'].item() > 0


def _dy_from_coef(f, o):
    """fp64 dy = gamma*invstd*(dz - k1 - xhat*k2) of form f's (y, da) with the kernel's statistics and coefficients."""
    d = f.d
    y, da = f.y.double(), f.t['da'].double()
    n, _, _, c = y.shape
    seg = torch.arange(n, device=d.dev) // (n // d.nseg)
    mu, iv, sc, sf = (t.double().reshape(d.nseg, c)[seg][:, None, None, :] for t in f.st)
    k = o['coef'].double().reshape(d.nseg, c, 2)[seg][:, None, None]
    dz = da * (y * sc + sf > 0)  # the sign fma(y, sc, sf) has: the product of two floats is exact in double
    return d.gamma.double() * iv * (dz - k[..., 0] - (y - mu) * iv * k[..., 1])


@pytest.mark.parametrize('dtype', DTYPES, ids=['f32', 'bf16'])
@pytest.mark.parametrize('split', list(SPLITS))
@pytest.mark.parametrize('form,nseg,c', _cases(FORMS))
def test_backward_of_shards(dev, form, nseg, c, split, dtype):
    from multimodal_siamese_cd_amd import hip
    h, w = (16, 24) if form.startswith('pooled') else (18, 22)
    d = Data(dev, h, w, c, nseg, dtype, 400 + c + nseg)
    counts = SPLITS[split]
    images = [d.images(counts, r) for r in range(2)]
    out, stats = stats_sync(hip, d, [d.y[im].contiguous() for im in images])
    st = out[:4]
    whole_form = 'plain' if form in ('tiles', 'coef', 'coef_tiles') else form
    fw = Form(hip, d, whole_form, st)
    whole = fw.call()  # the whole batch in one piece, on the synchronized coefficients
    forms = [Form(hip, d, form, st, fw.src, im) for im in images]
    # the gather, by hand: both ranks' sums calls first (a throw-away from_sums follows each, on a half-filled buffer),
    # then each rank's real call with both slots
    slots = {}
    for r, f in enumerate(forms):
        f.call(_sync(stats, r, lambda buf, r=r: slots.__setitem__(r, buf[r].clone())))
    res = [f.call(_sync(stats, r, lambda buf, r=r: buf[1 - r].copy_(slots[1 - r]))) for r, f in enumerate(forms)]
    torch.cuda.synchronize()
    dy_tol = TOL if dtype == torch.float32 else BF16_TOL
    errs = {}
    for k in ('dgamma', 'dbeta'):
        errs[k] = rel(res[0][k].double() + res[1][k].double(), whole[k])
    for r, (f, o) in enumerate(zip(forms, res)):
        if 'dy' in o:
            errs[f'dy{r}'] = rel(o['dy'], whole['dy'][images[r]]) / (dy_tol / TOL)
            errs[f'dbias{r}'] = rel(o['dbias'], o['dy'].double().sum((0, 1, 2)))
            assert o['dy_bound'].item() >= o['dy'].float().abs().max().item() > 0
        else:
            dy64 = _dy_from_coef(f, o)
            errs[f'dy{r}'] = rel(dy64, whole['dy'][images[r]]) / (dy_tol / TOL)
            errs[f'dbias{r}'] = rel(o['dbias'], dy64.sum((0, 1, 2)))
            assert o['dy_bound'].item() >= dy64.abs().max().item() > 0
        if 'w_grad' in o:
            errs[f'w_grad{r}'] = 0.0
    if form == 'head':
        errs['w_grad'] = rel(res[0]['w_grad'].double() + res[1]['w_grad'].double(), whole['w_grad'])
    print(form, nseg, c, split, dtype, {k: '%.1e' % v for k, v in errs.items()})
    assert max(errs.values()) < TOL, errs
    if 'coef' in res[0]:  # the coefficients are global: the same bits on both ranks
        assert torch.equal(res[0]['coef'], res[1]['coef'])
