"""Every shipped instance of igemm_halo16_x3 / igemm_halo16_c16 against an fp64 CPU reference.

One table (tests/_conv_matrix.py): the h2 1 x N tiles (kLayout rows 3, 4, 5 and the 256 -> 128 pixel fallback), the
bf16 2 x 2 tiles with fp32 storage (rows 0, 1), the bf16-storage tiles (rows 6, 7, 8 and the 128 x 256 block, row 9)
and the 16-channel input-layer kernel in the three arithmetics; each at tile widths 16, 32 and 64 on maps with at
least two tiles per image in each direction, forward (mode-0 pack) and data grad (mode-1 pack), 1 to 4 source chunks
of 32 channels, full, half-empty and ragged (136) output blocks; and each epilogue form (bias, per-tile statistics,
BatchNorm-backward records, fused input BatchNorm, output bound, concat-slice destination and source) once per row at
a width other than 16.  Automatic tile choice, default tune bits: what the shipped configs run.

Each case first asks scd_igemm_kernel which instance the launch will run and asserts it is the one the row names, so a
dispatcher change cannot quietly move a case onto another kernel.  Then every element of the output is compared with
the definition in double.  No exclusions.

Bars.  A = the fp64 conv of |x| with |w| (plus |bias|): the sum of the absolute terms of that output.  K = 9 c (plus
one with a bias): the terms.  Kv = the in-range products of that pixel.

1. Elementwise ceiling, derived, not measured:
   bf16 (inputs and weights bf16-representable, so every product is exact and only the fp32 accumulation is under
   test): |got - ref| <= K 2^-24 A, the bound of a K-term fp32 sum in any order (each of at most K roundings is at most
   2^-24 of a partial sum, and no partial sum exceeds A).
   h2: each operand is split into two fp16 terms to 2^-22 of its scale (x3_common.h): the activation's
   scale is the bound handed to the kernel, the weight's its row maximum.  A product is then off by at most
   2 x 2^-22 bound_x rowmax|w| to first order; with a factor 2 of margin the Kv products add
   2^-20 Kv bound_x rowmax|w|[channel] to the fp32 accumulation ceiling above.
   bf16 storage: one rounding of the result to bf16, 2^-8 |ref|: half a unit in the last of bf16's 8 significant
   bits, the most one round-to-nearest can move a value (so the measured ratio of a large output sits just below 1;
   the accumulation term, met at under 0.02 of itself, is the slack for the fp32 value not being the reference).
   A dropped tap, a wrong halo row, a missing low-order product or a mis-scaled channel breaks this at c <= 128.
2. h2 also meets the project's single-op bar max|got - ref| / max|ref| <= 1e-5 (TOL of tests/test_kernels_gpu.py).

Records are compared with their definition over the kernel's own stored output, at the bars test_conv_halo16_tiles
holds them to: 2e-6 for first-order sums (tile mean, sum dz), 2e-5 for second-order ones (M2, sum dz xhat).  Their
tiles are laid out from the query's tile width and block pixels.  Record buffers and slice surroundings start as NaN,
so an unwritten record or a write outside the slice fails.

Under bf16 the fused input BatchNorm uses quarter-integer inputs and coefficients whose transform relu(y s + t) is
exact in bf16 (at most 7 significant bits), so that the products stay exact there too.
"""
import pytest
import torch
import torch.nn.functional as F

from _conv_matrix import (CASES, DST_SLICE_EXTRA, DST_SLICE_OFF, FORM_FIELDS, IDS, SRC_SLICE_EXTRA, SRC_SLICE_OFF,
                          case_key, instance_key)

pytestmark = pytest.mark.gpu

TOL = 1e-5                    # the single-op bar of tests/test_kernels_gpu.py (h2)
REC1, REC2 = 2e-6, 2e-5       # record bars of test_conv_halo16_tiles
WORST: dict = {}              # family tag -> {metric: worst measured}


@pytest.fixture(scope='module')
def dev():
    from multimodal_siamese_cd_amd import hip
    hip.load_library()
    d = torch.device('cuda:0')
    hip.ensure_device(torch.empty(1, device=d))
    return d


def nchw(t):
    return t.permute(0, 3, 1, 2).contiguous()


def nhwc_t(t):
    return t.permute(0, 2, 3, 1).contiguous()


def rel(a, b):
    a, b = a.detach().double().cpu(), b.detach().double().cpu()
    return ((a - b).abs().max() / b.abs().max().clamp_min(1e-30)).item()


def r16(t):
    return t.to(torch.bfloat16).float()


def note(tag, **kv):
    w = WORST.setdefault(tag, {})
    for k, v in kv.items():
        w[k] = max(w.get(k, 0.0), float(v))


def make_data(case, g):
    """(x or the BatchNorm input y0, weights OIHW of the underlying conv, in_bn coefficients or None), fp32 on the
    CPU.  h2: spread over 10^+-1; bf16: bf16-representable."""
    n, h, w, c, no = case.n, case.h, case.w, case.c, case.n_out
    wshape = (no, c, 3, 3) if case.direction == 'fwd' else (c, no, 3, 3)
    coef = None
    if case.math == 'h2':
        spread = lambda *s: (torch.randn(*s, generator=g, dtype=torch.float64)
                             * 10 ** (2 * torch.rand(*s, generator=g, dtype=torch.float64) - 1)).float()
        x = spread(n, h, w, c)
        wt = (spread(*wshape).double() / (3 * c ** 0.5)).float()
        if case.form == 'in_bn':
            coef = ((torch.rand(2 * c, generator=g) * 2 - 0.5), torch.randn(2 * c, generator=g))  # some negative scales
    else:
        x = r16(torch.randn(n, h, w, c, generator=g))
        wt = r16(torch.randn(*wshape, generator=g) / (3 * c ** 0.5))
        if case.form == 'in_bn':  # relu(y s + t) a multiple of 1/8 below 16: exact in fp32 and in bf16
            x = torch.randint(-16, 17, (n, h, w, c), generator=g).float() / 4
            sc = torch.tensor([-1.0, -0.5, 0.5, 1.0, 2.0])[torch.randint(0, 5, (2 * c,), generator=g)]
            coef = (sc, torch.randint(-8, 9, (2 * c,), generator=g).float() / 4)
    return x, wt, coef


def reference(case, x, wt, coef, bias):
    """ref, A (sum of absolute terms), Kv (in-range products), row maxima of |w| per output channel; fp64 NHWC."""
    n, h, w, c = x.shape
    xd = x.double()
    if coef is not None:
        sc, sh = (t.double().reshape(2, 1, 1, c) for t in coef)
        xd = torch.relu(xd.reshape(2, n // 2, h, w, c) * sc[:, None] + sh[:, None]).reshape(n, h, w, c)
    wd = wt.double()
    if case.direction == 'fwd':
        op = lambda a, b: F.conv2d(a, b, None, padding=1)
        rowmax = wd.abs().amax(dim=(1, 2, 3))
    else:
        op = lambda a, b: F.conv_transpose2d(a, b, None, padding=1)
        rowmax = wd.abs().amax(dim=(0, 2, 3))
    ref = nhwc_t(op(nchw(xd), wd))
    A = nhwc_t(op(nchw(xd.abs()), wd.abs()))
    taps = F.conv2d(torch.ones(1, 1, h, w, dtype=torch.float64), torch.ones(1, 1, 3, 3, dtype=torch.float64), padding=1)
    Kv = (taps[0, 0] * c).reshape(1, h, w, 1)
    if bias is not None:
        ref = ref + bias.double()
        A = A + bias.double().abs()
    return ref, A, Kv, rowmax, xd


def tiles_of(t, bm, tw):
    """[n, h, w, c] -> [tiles, bm, c], tiles image-major, then tile rows, then tile columns."""
    n, h, w, c = t.shape
    tr = bm // tw
    return t.reshape(n, h // tr, tr, w // tw, tw, c).permute(0, 1, 3, 2, 4, 5).reshape(-1, bm, c)


@pytest.mark.parametrize('case', CASES, ids=IDS)
def test_instance_vs_fp64(dev, case):
    from multimodal_siamese_cd_amd import hip
    tag = case.name.split('-')[0]
    n, h, w, c, no = case.n, case.h, case.w, case.c, case.n_out
    fields = FORM_FIELDS[case.form]
    sb = case.store == 'bf16'
    sdt = torch.bfloat16 if sb else torch.float32
    g = torch.Generator().manual_seed(sum(map(ord, case.name)))
    x, wt, coef = make_data(case, g)
    bias = (torch.randn(no, generator=g) + 0.5) if 'bias' in fields else None
    ref, A, Kv, rowmax, x_read = reference(case, x, wt, coef, bias)

    with hip.conv_scope(case.math, 0):
        # source: contiguous, or channels [8, 8 + c) of a wider NaN buffer
        if case.form == 'src_slice':
            xbuf = torch.full((n, h, w, c + SRC_SLICE_EXTRA), float('nan'), dtype=sdt, device=dev)
            xbuf[..., SRC_SLICE_OFF:SRC_SLICE_OFF + c] = x.to(dev).to(sdt)
            src = hip.nhwc(xbuf, SRC_SLICE_OFF, c)
        else:
            xbuf = x.to(dev).to(sdt)
            src = hip.nhwc(xbuf)
        stored_x = xbuf[..., SRC_SLICE_OFF:SRC_SLICE_OFF + c] if case.form == 'src_slice' else xbuf
        assert torch.equal(stored_x.float().cpu(), x)  # the stored source is exactly the data (bf16: representable)
        wd = wt.to(dev)
        wpk = hip.pack_conv3x3(wd, 0, ci_pad=c) if case.direction == 'fwd' else hip.pack_conv3x3(wd, 1)
        in_bn = None
        if coef is not None:
            in_bn = (coef[0].to(dev), coef[1].to(dev), 2)
        bound, bx = None, 0.0
        if case.math == 'h2':
            bound = torch.zeros(1, device=dev)
            if in_bn is None:
                hip.absmax_bound(src, bound)
            else:
                hip.absmax_bound(src, bound, 2, in_bn[0], in_bn[1])  # covers the transformed activation
            bx = bound.item()
            assert bx >= x_read.abs().max().item() * (1 - 1e-6)
        # destination: contiguous, or channels [32, 32 + n_out) of a NaN buffer 32 + n_out + 8 wide
        if case.form == 'dst_slice':
            ybuf = torch.full((n, h, w, no + DST_SLICE_EXTRA), float('nan'), dtype=sdt, device=dev)
            dst = hip.nhwc(ybuf, DST_SLICE_OFF, no)
            y = ybuf[..., DST_SLICE_OFF:DST_SLICE_OFF + no]
        else:
            ybuf = y = torch.full((n, h, w, no), float('nan'), dtype=sdt, device=dev)
            dst = hip.nhwc(ybuf)
        kw = dict(src=src, out_h=h, out_w=w, stride=1, taps=hip.TAPS_3X3, wpk=wpk, n_out=no,
                  bias=None if bias is None else bias.to(dev), dst=dst, in_bn=in_bn, src_bound=bound)
        bm, tw = case.inst.block_pixels, case.inst.tile_width
        ntiles = n * h * w // bm
        rec = None
        if 'stat_rec' in fields:
            assert hip.igemm_stat_tiles(src, h, w, 1, hip.TAPS_3X3, wpk, no, dst, src_bound=bound) == (ntiles, bm)
            rec = kw['stat_rec'] = torch.full((ntiles * no * 2,), float('nan'), device=dev)
        bb = None
        if 'bn_bwd' in fields:
            assert hip.igemm_bn_bwd_tiles(src, h, w, 1, hip.TAPS_3X3, wpk, no, dst, bound) == (ntiles, bm)
            y0 = torch.randn(n, h, w, no, generator=g)
            y0 = r16(y0) if sb else y0
            mu, iv = torch.randn(2 * no, generator=g) * 0.1, torch.rand(2 * no, generator=g) + 0.5
            bsc, bsh = torch.rand(2 * no, generator=g) * 2 - 0.5, torch.randn(2 * no, generator=g) * 0.2
            bb = torch.full((no * ntiles * 2,), float('nan'), device=dev)
            kw['bn_bwd'] = (y0.to(dev).to(sdt), 2, mu.to(dev), iv.to(dev), bsc.to(dev), bsh.to(dev), bb)
        db = None
        if 'dst_bound' in fields:
            db = kw['dst_bound'] = torch.zeros(1, device=dev)

        # 1. the instance this launch runs is the one the row names
        assert hip.igemm_kernel(**kw) == case.inst
        # 2. the launch
        hip.conv_igemm(**kw)
        torch.cuda.synchronize()
        got = y.double().cpu()

        # 3. against the definition, every element
        diff = (got - ref).abs()
        K = 9 * c + (1 if bias is not None else 0)
        ceil = K * 2.0 ** -24 * A
        if case.math == 'h2':
            ceil = ceil + 2.0 ** -20 * Kv * bx * rowmax.reshape(1, 1, 1, no)
        if sb:
            ceil = ceil + 2.0 ** -8 * ref.abs()
        e_ceil = (diff / ceil.clamp_min(1e-300)).max().item()
        e_rel = (diff.max() / ref.abs().max()).item()
        note(tag, ceiling=e_ceil, **({'rel': e_rel} if case.math == 'h2' else {}))
        print(f'{case.name}: |got - ref| / ceiling {e_ceil:.3f}, max-relative {e_rel:.2e}')
        assert torch.isfinite(got).all()
        assert bool((diff <= ceil).all()), (case.name, e_ceil)
        if case.math == 'h2':
            assert e_rel <= TOL, (case.name, e_rel)

        if case.form == 'dst_slice':  # nothing outside the slice was written
            assert torch.isnan(ybuf[..., :DST_SLICE_OFF]).all() and torch.isnan(ybuf[..., DST_SLICE_OFF + no:]).all()

        if rec is not None:  # per-tile mean and M2 of the stored output
            r = rec.double().cpu().reshape(ntiles, no, 2)
            yy = tiles_of(got, bm, tw)
            e1 = rel(r[..., 0], yy.mean(1))
            e2 = rel(r[..., 1], ((yy - yy.mean(1, keepdim=True)) ** 2).sum(1))
            note(tag, stat_mean=e1, stat_m2=e2)
            print(f'{case.name}: tile mean {e1:.2e}, M2 {e2:.2e}')
            assert torch.isfinite(r).all() and e1 < REC1 and e2 < REC2, (case.name, e1, e2)

        if bb is not None:  # per (channel, tile) sum dz, sum dz xhat over the kernel's own stored output
            r = bb.double().cpu().reshape(no, ntiles, 2)
            seg = lambda t: t.double().reshape(2, 1, 1, 1, no).expand(2, n // 2, 1, 1, no).reshape(n, 1, 1, no)
            yd = y0.double()
            dz = torch.where(yd * seg(bsc) + seg(bsh) > 0, got, torch.zeros_like(got))  # fma's sign, exact in double
            xhat = (yd - seg(mu)) * seg(iv)
            e1 = rel(r[..., 0], tiles_of(dz, bm, tw).sum(1).t())
            e2 = rel(r[..., 1], tiles_of(dz * xhat, bm, tw).sum(1).t())
            note(tag, bn_bwd_dz=e1, bn_bwd_dzx=e2)
            print(f'{case.name}: sum dz {e1:.2e}, sum dz xhat {e2:.2e}')
            assert torch.isfinite(r).all() and e1 < REC1 and e2 < REC2, (case.name, e1, e2)
            # the records do not touch the stored output: bit-equal to the launch without them
            plain = torch.full_like(ybuf, float('nan'))
            kw2 = {k: v for k, v in kw.items() if k not in ('bn_bwd', 'dst_bound')}
            kw2['dst'] = hip.nhwc(plain)
            hip.conv_igemm(**kw2)
            assert torch.equal(plain, ybuf)

        if db is not None:  # exactly max |stored output|; a larger value already there stays
            m = y.float().abs().max()
            assert db.item() == m.item(), (case.name, db.item(), m.item())
            hi = torch.full((1,), 2.0 * m.item() + 1.0, device=dev)
            hi0 = hi.item()
            kw3 = dict(kw, dst_bound=hi)
            if bb is not None:
                kw3['bn_bwd'] = kw['bn_bwd'][:6] + (torch.empty_like(bb),)
            hip.conv_igemm(**kw3)
            assert hi.item() == hi0


@pytest.mark.parametrize('config', ['baseline_siamese', 'baseline_dualstream'])
def test_matrix_covers_shipped_instances(dev, monkeypatch, config):
    """The matrix above checks what ships: one small training step of the h2 Siamese config and of a bf16-storage
    config (batch 2, the configs' own 256 x 256 crops), every 3x3 conv launch recorded.  Each launch must run one of the
    two 16x16x32 halo kernels, and its instance key -- family, layout row, NP, DB, SB, IN_BN, WL and the epilogue fields
    set; the tile width is left out, production maps all take 16 -- must be a key of some matrix row.  So must the key
    of the same descriptor at the config's shipped batch (the 128 x 256 bf16 block depends on the grid; the query is
    host-only, nothing of that size is allocated).  A dispatcher or kernel change that introduces an instance no row
    checks fails here and names it."""
    import ctypes
    from multimodal_siamese_cd_amd import hip, trainers
    from multimodal_siamese_cd_amd.utils import datasets, experiment_manager as em, networks
    cfg = em.load_cfg(config)
    batch = 2
    assert int(cfg.TRAINER.BATCH_SIZE) % batch == 0
    scale = int(cfg.TRAINER.BATCH_SIZE) // batch
    net = networks.create_network(cfg).to(dev).train()
    seen = {}
    orig = hip.conv_igemm

    def spy(src, out_h, out_w, stride, taps, wpk, n_out, bias, dst, store_mode=0, **kw):
        if len(taps[0]) == 9:
            d = hip._igemm_desc(src, out_h, out_w, stride, taps, wpk, n_out, bias, dst, store_mode,
                                kw.get('stat_rec'), kw.get('in_bn'), kw.get('bn_bwd'), kw.get('src_bound'),
                                kw.get('dst_bound'), kw.get('dst_bound_seed'))
            fields = [f for f, v in (('bias', bias), ('stat_rec', kw.get('stat_rec')), ('bn_bwd', kw.get('bn_bwd')),
                                     ('dst_bound', kw.get('dst_bound'))) if v is not None]
            what = f'c={src.c} n_out={n_out} {out_h}x{out_w}'
            for n in (src.n, src.n * scale):  # as launched, and at the shipped batch
                d.src.n = d.dst.n = n
                if d.bn_bwd:
                    d.bn_bwd.contents.y.n = n
                seen.setdefault(instance_key(hip.igemm_kernel_of(d), fields), f'{what} n={n}')
            d.src.n = d.dst.n = src.n
        return orig(src, out_h, out_w, stride, taps, wpk, n_out, bias, dst, store_mode, **kw)

    monkeypatch.setattr(hip, 'conv_igemm', spy)
    gen = torch.Generator(device=dev).manual_seed(1)
    b = datasets.synthetic_batch(cfg, batch, dev, gen)
    loss = trainers.step_loss(cfg, net(b['x_t1'], b['x_t2']), b, net)
    loss.backward()
    torch.cuda.synchronize()
    monkeypatch.undo()
    assert torch.isfinite(loss)
    covered = {case_key(c) for c in CASES}
    print(f'{config}: {len(seen)} instance keys over the 3x3 launches')
    for k, what in sorted(seen.items(), key=str):
        print(('  ' if k in covered else '  UNCHECKED ') + f'{k}  ({what})')
    assert seen
    assert all(k[0] in ('halo16', 'halo16_c16') for k in seen), [k for k in seen if k[0] not in ('halo16', 'halo16_c16')]
    missing = {k: v for k, v in seen.items() if k not in covered}
    assert not missing, missing


def test_report_worst_measured():
    """Prints the worst measured value per family (the table of DESIGN.md 4); asserts nothing new."""
    keys = ['ceiling', 'rel', 'stat_mean', 'stat_m2', 'bn_bwd_dz', 'bn_bwd_dzx']
    print('\nfamily       ' + ' '.join(f'{k:>11s}' for k in keys))
    for tag in sorted(WORST):
        print(f'{tag:12s} ' + ' '.join(f'{WORST[tag][k]:11.3e}' if k in WORST[tag] else f'{"-":>11s}' for k in keys))
