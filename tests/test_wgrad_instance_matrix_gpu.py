"""Every shipped weight-grad instance against an fp64 CPU reference, the kernel and the finalize each on their own.

One table (tests/_wgrad_matrix.py): wgrad_halo16_x3 in h2 (128- and 64-row blocks), x3, x5 and bf16 (fp32 storage),
wgrad_halo16_dma and its register-staged fallback on bf16 storage, wgrad_halo16_c16 in the five arithmetics, and the
generic wgrad_x3 tiles / wgrad_f32 on ConvTranspose weight grads and on 3x3 shapes the halo kernels refuse; each in the
forms its instance supports (plain, fused source transform with two and three segments, rows formed through the
BatchNorm backward with and without the source transform, channel slices of wider buffers on either side, column
sums) on the smallest shapes at which the mechanism can go wrong (one patch, ragged K splits that cut through images
and coefficient segments, splits shorter than the DMA ring, three row and channel tiles, K tails).

Each case first asks scd_wgrad_kernel which instance the launch will run and asserts it is the one the row names, and,
where the row is there for an awkward K cut, that the plan cuts there (nsplit >= 2, a ragged last split, a cut inside an
image / a coefficient segment).  The slabs start as NaN: every element must be finite afterwards.

The kernel alone.  S = the fp64 sum of the slabs over the splits; ref = the definition in fp64
(torch.nn.grad.conv2d_weight for 3x3; for the ConvTranspose weight grad the definition of scd.h, rows = X and src = dOut
at stride 2, slab[r][(i 2 + j) C + c] = sum X[n, y, x, r] dOut[n, 2y + i, 2x + j, c]).  Operands of ref: the source after
its transform evaluated in fp64; with rows_bn the kernel's own stored rows_out (the 16-channel kernel stores none: the
stand-alone scd_bn_relu_backward's dY, which the contract of scd.h makes the same values).  Under bf16 arithmetic with
fp32 storage those rows are rounded to bf16, round-to-nearest-even, as the kernel does: the staging code hands the
formed fp32 dY to stage_bits<false>, i.e. cvt_pk_bf16 (v_cvt_pk_bf16_f32, RNE), the same conversion every fp32-stored
bf16 operand takes.  Every element of S is compared, no exclusions.

Ceilings, derived, not measured.  A = the same weight grad of |rows| and |src|, K = n h w terms, Kv = the in-range
pixels of the element's tap, b_r and b_s the bounds handed to the kernel.
  bf16   K 2^-24 A.  Operands are bf16-representable (asserted on the stored buffers), so products are exact and only
         the fp32 accumulation is under test: at most K roundings, each at most 2^-24 of a partial sum, none of which
         exceeds A.  The fused source transform uses quarter-integer inputs, scales from {-1, -0.5, 0.5, 1, 2} and
         shifts that are multiples of 1/4, so relu(x s + t) is a multiple of 1/8 below 16: exact in fp32 and in bf16.
  h2     + 2^-20 Kv b_r b_s.  A power-of-two scale brings a bound to [2^14, 2^15); the scaled operand is split into
         h = fp16(x) and m = fp16(x - h) (rows, and both operands of the generic kernel: m pre-scaled by 2^11).  fp16
         carries 11 significant bits, so |m| <= 2^-11 |x| and h + m is x to 2^-22 |x| (absolute floors 2^-25 / 2^-36 of
         the scaled unit, below 2^-39 of the bound).  The kernels keep hh + hm + mh.  Per product, relative to
         b_r b_s: two operand representations 2 x 2^-22, the dropped m m <= 2^-22 (x3_common.h calls it 2^-24; with
         |m| <= 2^-11 |x| the code's arithmetic gives 2^-22), the fp32 rounding of a fused source transform 2^-24:
         3.25 x 2^-22 < 2^-20, the rest is margin.
  x3     + 2^-22 A.  split3 is exact (h + m + l = x: three bf16 terms of 8 bits cover fp32's 24).  Of the nine
         products the kernel keeps six; dropped are m l, l m (2^-8 2^-16 = 2^-24 each) and l l (2^-32); a fused source
         transform adds one fp32 rounding, 2^-24: under 2^-22 together.
  x5     + (2^-16 + 2^-22) A.  x5 keeps two planes of the source: it also drops x_l dy_h, and |x_l| <= 2^-16 |x|, plus
         x_l dy_m (2^-24); the x3 terms stay.  (DESIGN.md's 1e-5 for x5 is this 2^-16 = 1.5e-5 met on average data.)
  f32    (K + 1) 2^-24 A.  wgrad_f32 feeds v_mfma_f32_32x32x2f32 the fp32 operands as loaded: no input rounding.  The
         K accumulations round as above; should the instruction round its products before adding them, that is one
         more 2^-24 per term, 2^-24 A in all.
h2 (both bounds) also meets the project's single-op bar max|S - ref| / max|ref| <= 1e-5 (TOL of test_kernels_gpu.py).

The finalize alone (on a copy's worth of care: scd_wgrad_finalize overwrites the slabs, S is taken first): every element
of its output within nsplit 2^-24 sum_s |slab_s| of S, at its place in the parameter layout (OIHW with c_valid <= C,
ConvT [R][C][2][2]); a stand-alone test runs it on synthetic slabs through every reduction plan.

rows_bn: rows_out bit-equal to a stand-alone scd_bn_relu_backward, every element written once (NaN-prefilled),
rows_out_bound exactly max |rows_out| and a larger value left alone, and the slabs bit-equal to a launch reading that
stored dY as plain rows.  colsum: after scd_wgrad_colsum_finalize within M 2^-24 sum |dOut| of the fp64 channel sum.
Slices: the buffers around them start as NaN and stay NaN.  On failure the worst element's split, row block and channel
tile are printed (the query's kchunk maps pixels to splits).
"""
import pytest
import torch

from _wgrad_matrix import (CASES, FORM_FIELDS, IDS, SLICE_EXTRA, asserts_split, case_key, instance_key, less_split,
                           nseg_of)

pytestmark = pytest.mark.gpu

TOL = 1e-5     # the single-op bar of tests/test_kernels_gpu.py (h2)
WORST: dict = {}   # family tag -> {metric: worst measured}
NAN = float('nan')


@pytest.fixture(scope='module')
def dev():
    from multimodal_siamese_cd_amd import hip
    hip.load_library()
    d = torch.device('cuda:0')
    hip.ensure_device(torch.empty(1, device=d))
    return d


def nchw(t):
    return t.permute(0, 3, 1, 2).contiguous()


def r16(t):
    return t.to(torch.bfloat16).float()


def note(tag, **kv):
    w = WORST.setdefault(tag, {})
    for k, v in kv.items():
        w[k] = max(w.get(k, 0.0), float(v))


def spread(g, *s):
    return (torch.randn(*s, generator=g, dtype=torch.float64)
            * 10 ** (2 * torch.rand(*s, generator=g, dtype=torch.float64) - 1)).float()


def per_image(t, n, nseg):
    """[nseg * c] coefficients -> [n, 1, 1, c] in double."""
    c = t.numel() // nseg
    return t.double().reshape(nseg, c).repeat_interleave(n // nseg, 0).reshape(n, 1, 1, c)


def weight_grad(kind, rows, src):
    """The slab layout [R][ntaps * C] of the definition, fp64."""
    n, h, w, R = rows.shape
    C = src.shape[3]
    if kind == '3x3':
        gw = torch.nn.grad.conv2d_weight(nchw(src), (R, C, 3, 3), nchw(rows), padding=1)  # [R][C][3][3]
        return gw.permute(0, 2, 3, 1).reshape(R, 9 * C)
    return torch.einsum('nyxr,nyixjc->rijc', rows, src.reshape(n, h, 2, w, 2, C)).reshape(R, 4 * C)


def patch_split(n, h, w, kchunk):
    """[n, h, w] split index of every pixel under the halo kernels' patch walk: image-major, inside an image down the
    patch rows first (patch_y0 / patch_x0 of conv_halo16.hip), kchunk patches per split."""
    ph_n = h // 2
    y, x = torch.meshgrid(torch.arange(h), torch.arange(w), indexing='ij')
    pr = (x // 16) * ph_n + y // 2
    pi = torch.arange(n).reshape(n, 1, 1) * (ph_n * (w // 16)) + pr
    return pi // kchunk


def explain(case, k, slabs, rows, src, S, ref, ceil):
    """The worst element of a failing case: its split, row block and channel tile."""
    n, h, w, R = rows.shape
    C = src.shape[3]
    ratio = (S - ref).abs() / ceil.clamp_min(1e-300)
    r, col = divmod(int(ratio.argmax()), S.shape[1])
    t, c = divmod(col, C)
    msg = (f'{case.name}: worst element r={r} (row block {r // k.block_rows}) tap={t} c={c} (channel tile '
           f'{c // k.block_channels if case.kind == "3x3" else col // k.block_channels}) S={S[r, col].item():.9g} '
           f'ref={ref[r, col].item():.9g} ratio={ratio[r, col].item():.3g}')
    if case.kind == '3x3':
        dy, dx = t // 3 - 1, t % 3 - 1
        sp = torch.nn.functional.pad(src[..., c], (1, 1, 1, 1))[:, 1 + dy:1 + dy + h, 1 + dx:1 + dx + w]
        prod, split = rows[..., r] * sp, patch_split(n, h, w, k.kchunk)
    else:
        i, j = t // 2, t % 2
        prod = rows[..., r] * src[:, i::2, j::2, c]
        split = (torch.arange(n * h * w) // k.kchunk).reshape(n, h, w)
    per = [(s, slabs[s, r, col].item(), prod[split == s].sum().item()) for s in range(k.nsplit)]
    s, got, want = max(per, key=lambda p: abs(p[1] - p[2]))
    return msg + f'; worst split {s} of {k.nsplit} (kchunk {k.kchunk}): slab {got:.9g} vs {want:.9g}'


def sliced(t, dev, sdt, off, extra):
    """t as channels [off, off + c) of a NaN buffer `extra` channels wider; returns (buffer, view of t)."""
    c = t.shape[3]
    buf = torch.full(t.shape[:3] + (c + extra,), NAN, dtype=sdt, device=dev)
    buf[..., off:off + c] = t.to(dev).to(sdt)
    return buf, buf[..., off:off + c]


def assert_surroundings_nan(buf, off, c):
    assert torch.isnan(buf[..., :off]).all() and torch.isnan(buf[..., off + c:]).all()


@pytest.mark.parametrize('case', CASES, ids=IDS)
def test_instance_vs_fp64(dev, case):
    from multimodal_siamese_cd_amd import hip
    tag = case.name.split('-')[0]
    n, h, w, R, C = case.n, case.h, case.w, case.R, case.C
    fields = FORM_FIELDS[case.form]
    conv = case.kind == '3x3'
    hs, ws, ntaps, stride, taps = (h, w, 9, 1, hip.TAPS_3X3) if conv else (2 * h, 2 * w, 4, 2, hip.TAPS_2X2)
    math, bounded = ('h2', False) if case.math == 'h2u' else (case.math, case.math == 'h2')
    exact = math == 'bf16'
    sb = case.store == 'bf16'
    sdt = torch.bfloat16 if sb else torch.float32
    g = torch.Generator().manual_seed(sum(map(ord, case.name)))
    val = (lambda *s: r16(torch.randn(*s, generator=g))) if exact else (lambda *s: spread(g, *s))

    # ---- data, fp32 on the CPU
    src = val(n, hs, ws, C)
    coef = None
    if 'src_bn' in fields:
        sn = nseg_of(n, case.form)
        if exact:
            src = torch.randint(-16, 17, (n, hs, ws, C), generator=g).float() / 4
            coef = (torch.tensor([-1.0, -0.5, 0.5, 1.0, 2.0])[torch.randint(0, 5, (sn * C,), generator=g)],
                    torch.randint(-8, 9, (sn * C,), generator=g).float() / 4, sn)
        else:  # some negative scales, shifts of both signs
            coef = (torch.rand(sn * C, generator=g) * 2 - 0.5, torch.randn(sn * C, generator=g), sn)
    rows_bn = 'rows_y' in fields
    if rows_bn:
        rn = nseg_of(n, 'rows_bn')
        y = torch.randn(n, h, w, R, generator=g) * 2 + 0.3
        rows = val(n, h, w, R)  # dL/da
        if sb:
            y = r16(y)
        gamma, beta = torch.rand(R, generator=g) + 0.5, torch.randn(R, generator=g)
    else:
        rows = val(n, h, w, R)

    with hip.conv_scope(math, 0):
        # ---- device operands: contiguous, or channel slices of wider NaN buffers
        if 'rows_slice' in fields:
            rbuf, rdev = sliced(rows, dev, sdt, SLICE_EXTRA, SLICE_EXTRA)
            rview = hip.nhwc(rbuf, SLICE_EXTRA, R)
        else:
            rbuf = rdev = rows.to(dev).to(sdt)
            rview = hip.nhwc(rbuf)
        if 'src_slice' in fields:
            sbuf, sdev = sliced(src, dev, sdt, 0, SLICE_EXTRA)
            sview = hip.nhwc(sbuf, 0, C)
        else:
            sbuf = sdev = src.to(dev).to(sdt)
            sview = hip.nhwc(sbuf)
        if exact:  # the stored operands are exactly the data: bf16-representable
            assert torch.equal(sdev.float().cpu(), src)
            if not rows_bn or sb:
                assert torch.equal(rdev.float().cpu(), rows)
        src_bn = None if coef is None else (coef[0].to(dev), coef[1].to(dev), coef[2])
        src_read = src.double()
        if coef is not None:
            src_read = torch.relu(src_read * per_image(coef[0], n, coef[2]) + per_image(coef[1], n, coef[2]))

        kw = dict(rows=rview, src=sview, stride=stride, taps=taps, src_bn=src_bn)
        b_r = b_s = 0.0
        if bounded:
            kw['src_bound'] = torch.zeros(1, device=dev)
            if src_bn is None:
                hip.absmax_bound(sview, kw['src_bound'])
            else:
                hip.absmax_bound(sview, kw['src_bound'], src_bn[2], src_bn[0], src_bn[1])
            b_s = kw['src_bound'].item()
            assert b_s >= src_read.abs().max().item() * (1 - 1e-6)
            kw['rows_bound'] = torch.zeros(1, device=dev)
            if not rows_bn:
                hip.absmax_bound(rview, kw['rows_bound'])
        dy_ref = rows_out = out_bound = None
        if rows_bn:
            yd = y.to(dev).to(sdt)
            gd = gamma.to(dev)
            smean, sinv, scale, shift = (torch.empty(rn * R, device=dev) for _ in range(4))
            wsb = torch.empty(hip.bn_workspace_bytes(n, h, w, R, rn), dtype=torch.uint8, device=dev)
            hip.bn_train_stats(hip.nhwc(yd), rn, gd, beta.to(dev), 1e-5, 0.1, False, None, None, smean, sinv, scale,
                               shift, wsb)
            dy_ref = torch.empty_like(yd)
            o = [torch.empty(R, device=dev) for _ in range(3)]
            hip.bn_relu_backward(hip.nhwc(yd), rview, rn, smean, sinv, gd, scale, shift, *o, hip.nhwc(dy_ref), wsb)
            bn_coef = torch.empty(rn * R * 2, device=dev)
            da_bound = rdev.float().abs().max().reshape(1) if bounded else None
            hip.bn_relu_backward_coef(hip.nhwc(yd), rview, rn, smean, sinv, gd, scale, shift, None, 0, bn_coef, *o, wsb,
                                      da_bound, kw.get('rows_bound'))
            kw['rows_bn'] = (hip.nhwc(yd), rn, smean, sinv, gd, scale, shift, bn_coef)
            if 'rows_out' in fields:
                rows_out = torch.full_like(yd, NAN)
                kw['rows_out'] = hip.nhwc(rows_out)
                if 'rows_out_bound' in fields:
                    out_bound = kw['rows_out_bound'] = torch.zeros(1, device=dev)
        if bounded:
            b_r = kw['rows_bound'].item()

        # ---- 1. the instance and the split this launch runs
        d, nsplit, nbytes = hip.wgrad_plan(**kw)
        k = hip.wgrad_kernel(**kw)
        assert less_split(k) == case.inst, (case.name, k)
        assert k == hip.wgrad_kernel_of(d) and k.nsplit == nsplit and nbytes == nsplit * R * ntaps * C * 4
        assert hip.wgrad_rows_per_block(d) == (0 if k.family.startswith('generic') else k.block_rows)
        units, per_img = (n * h * w // 32, h * w // 32) if conv else (n * h * w, h * w)
        assert (k.nsplit - 1) * k.kchunk < units <= k.nsplit * k.kchunk
        cut = asserts_split(case)
        if cut:
            assert k.nsplit >= 2, (case.name, k)
        if cut in ('ragged', 'seg'):  # a ragged last split; no split boundary on an image boundary
            assert units % k.kchunk != 0 and k.kchunk % per_img != 0, (case.name, k)
        if cut == 'seg':  # the segment boundary, image n / 2, lies inside a split's patch range
            assert (n // 2 * per_img) % k.kchunk != 0, (case.name, k)
        if cut == 'convT':
            assert units % 16 != 0, (case.name, units)
        colsum = None
        if 'colsum' in fields:
            assert hip.wgrad_colsum_supported(d)
            colsum = torch.full((nsplit * ntaps * C,), NAN, device=dev)
            d.src_colsum = colsum.data_ptr()
            assert hip.wgrad_kernel_of(d) == k

        # ---- 2. the launch, into NaN slabs
        slabs = torch.full((nbytes // 4,), NAN, device=dev)
        hip.conv_wgrad(d, slabs)
        torch.cuda.synchronize()
        sl = slabs.double().cpu().reshape(nsplit, R, ntaps * C)
        assert torch.isfinite(sl).all(), f'{case.name}: {int((~torch.isfinite(sl)).sum())} slab elements not written'
        if 'rows_slice' in fields:
            assert_surroundings_nan(rbuf, SLICE_EXTRA, R)
            assert torch.equal(rdev.float().cpu(), rows)
        if 'src_slice' in fields:
            assert_surroundings_nan(sbuf, 0, C)
            assert torch.equal(sdev.float().cpu(), src)

        # ---- 3. the kernel alone: the fp64 sum of the slabs against the definition
        S = sl.sum(0)
        if rows_bn:
            formed = rows_out if rows_out is not None else dy_ref
            rows_read = formed.float().cpu()
            if exact and not sb:
                rows_read = r16(rows_read)
            rows_read = rows_read.double()
        else:
            rows_read = rows.double()
        ref = weight_grad(case.kind, rows_read, src_read)
        A = weight_grad(case.kind, rows_read.abs(), src_read.abs())
        K = n * h * w
        ceil = K * 2.0 ** -24 * A
        if k.np in (2, 4):
            if conv:
                Kv = torch.tensor([n * (h - abs(t // 3 - 1)) * (w - abs(t % 3 - 1)) for t in range(9)], dtype=torch.float64)
                Kv = Kv.repeat_interleave(C).reshape(1, 9 * C)
            else:
                Kv = float(K)
            ceil = ceil + 2.0 ** -20 * Kv * b_r * b_s
        elif k.np == 3:
            ceil = ceil + 2.0 ** -22 * A
        elif k.np == 5:
            ceil = ceil + (2.0 ** -16 + 2.0 ** -22) * A
        elif k.np == 0:
            ceil = ceil + 2.0 ** -24 * A
        diff = (S - ref).abs()
        e_ceil = (diff / ceil.clamp_min(1e-300)).max().item()
        e_rel = (diff.max() / ref.abs().max()).item()
        note(tag, ceiling=e_ceil, **({'rel': e_rel} if k.np == 4 else {}))
        print(f'{case.name}: {k.family} np {k.np} {k.nsplit} x {k.kchunk}: |S - ref| / ceiling {e_ceil:.3f}, '
              f'max-relative {e_rel:.2e}')
        if not bool((diff <= ceil).all()):
            pytest.fail(explain(case, k, sl, rows_read, src_read, S, ref, ceil))
        if k.np == 4:
            assert e_rel <= TOL, (case.name, e_rel)

        # ---- 4. the finalize alone: within nsplit 2^-24 sum |slab| of S, at its place in the parameter layout
        if conv:
            cv = C - 3 if C == 16 else C  # the input layer's padded channels are cut
            out = torch.full((R, cv, 3, 3), NAN, device=dev)
            hip.wgrad_finalize(slabs, nsplit, R, 9, C, 0, cv, out)
            lay = lambda t: t.reshape(R, 9, C).permute(0, 2, 1)[:, :cv].reshape(R, cv, 3, 3)
        else:
            out = torch.full((R, C, 2, 2), NAN, device=dev)
            hip.wgrad_finalize(slabs, nsplit, R, 4, C, 1, C, out)
            lay = lambda t: t.reshape(R, 4, C).permute(0, 2, 1).reshape(R, C, 2, 2)
        fd = (out.double().cpu() - lay(S)).abs()
        fceil = nsplit * 2.0 ** -24 * lay(sl.abs().sum(0))
        e_fin = (fd / fceil.clamp_min(1e-300)).max().item()
        note(tag, finalize=e_fin)
        assert torch.isfinite(out).all() and bool((fd <= fceil).all()), (case.name, e_fin)

        # ---- 5. the rows transform
        if rows_bn:
            plain = dict(kw, rows=hip.nhwc(dy_ref))
            for f in ('rows_bn', 'rows_out', 'rows_out_bound'):
                plain.pop(f, None)
            d2, ns2, nb2 = hip.wgrad_plan(**plain)
            k2 = hip.wgrad_kernel_of(d2)
            assert (k2.np, k2.block_rows, k2.layout, k2.sb, k2.src_xform) == (k.np, k.block_rows, k.layout, k.sb, k.src_xform)
            assert (ns2, k2.kchunk) == (nsplit, k.kchunk)
            slabs2 = torch.full((nb2 // 4,), NAN, device=dev)
            hip.conv_wgrad(d2, slabs2)
            assert torch.equal(slabs2.cpu().reshape(sl.shape).double(), sl), f'{case.name}: slabs differ from the plain launch'
        if rows_out is not None:
            assert not torch.isnan(rows_out.float()).any(), f'{case.name}: rows_out not fully written'
            assert torch.equal(rows_out, dy_ref), f'{case.name}: rows_out differs from scd_bn_relu_backward'
            m = rows_out.float().abs().max().item()
            if bounded:
                assert m <= b_r
        if out_bound is not None:
            assert out_bound.item() == m, (case.name, out_bound.item(), m)
            hi = torch.full((1,), 2.0 * m + 1.0, device=dev)
            hi0 = hi.item()
            d3, _, _ = hip.wgrad_plan(**dict(kw, rows_out=hip.nhwc(torch.empty_like(rows_out)), rows_out_bound=hi))
            hip.conv_wgrad(d3, torch.empty_like(slabs))
            assert hi.item() == hi0

        # ---- 6. the column sums
        if colsum is not None:
            assert torch.isfinite(colsum).all(), f'{case.name}: column sums not fully written'
            gb = torch.full((C,), NAN, device=dev)
            hip.wgrad_colsum_finalize(colsum, nsplit, ntaps, C, gb)
            M = n * hs * ws
            cd = (gb.double().cpu() - src.double().sum((0, 1, 2))).abs()
            cceil = M * 2.0 ** -24 * src.double().abs().sum((0, 1, 2))
            note(tag, colsum=(cd / cceil).max().item())
            assert bool((cd <= cceil).all()), (case.name, (cd / cceil).max().item())


@pytest.mark.parametrize('mode,R,C,cv', [(0, 16, 8, 5), (0, 6, 48, 33), (0, 5, 64, 63), (0, 3, 192, 130), (0, 5, 7, 6),
                                         (1, 6, 48, 48), (1, 5, 64, 64), (1, 3, 7, 7)])
@pytest.mark.parametrize('nsplit', [1, 3, 4, 5, 7, 16, 33])
def test_finalize_alone(dev, nsplit, mode, R, C, cv):
    """scd_wgrad_finalize on synthetic slabs, no conv: one slab, the ungrouped path (up to 4), the first grouped plan
    (5: groups of 3 + 2), a ragged last group (7), many groups (16, 33); OIHW with c_valid < C (a partial and several
    64-channel blocks) and the ConvTranspose layout.  Every element within nsplit 2^-24 sum_s |slab_s| of the fp64 sum,
    at its place.  The same data 4 bytes off 16-byte alignment (and R ntaps C % 4 != 0 at C = 7) takes wgrad_group_sum
    instead of wgrad_group_sum4: bit-identical."""
    from multimodal_siamese_cd_amd import hip
    ntaps = 9 if mode == 0 else 4
    g = torch.Generator().manual_seed(nsplit * 131 + C + mode)
    data = spread(g, nsplit, R, ntaps, C)
    S = data.double().sum(0)
    ceil = nsplit * 2.0 ** -24 * data.double().abs().sum(0)
    shape = (R, cv, 3, 3) if mode == 0 else (R, C, 2, 2)
    lay = lambda t: t.permute(0, 2, 1)[:, :cv].reshape(shape)
    outs = []
    for off in (0, 1):  # 16-byte aligned; 4 bytes off
        buf = torch.empty(data.numel() + 4, device=dev)
        assert buf.data_ptr() % 16 == 0
        sl = buf[off:off + data.numel()]
        sl.copy_(data.reshape(-1))
        out = torch.full(shape, NAN, device=dev)
        hip.wgrad_finalize(sl, nsplit, R, ntaps, C, mode, cv, out)
        outs.append(out.cpu())
        fd = (outs[-1].double() - lay(S)).abs()
        e = (fd / lay(ceil).clamp_min(1e-300)).max().item()
        note('finalize_alone', finalize=e)
        assert torch.isfinite(outs[-1]).all() and bool((fd <= lay(ceil)).all()), (off, e)
    assert torch.equal(outs[0], outs[1])


STEPS = [('baseline_siamese', 'train'), ('baseline_dualstream', 'train'), ('baseline_siamese', 'frozen_bn'),
         ('baseline_siamese', 'input_grad')]


@pytest.mark.parametrize('config,step', STEPS, ids=[f'{c}-{s}' for c, s in STEPS])
def test_matrix_covers_shipped_weight_grads(dev, monkeypatch, config, step):
    """The matrix above checks what ships: one small training step of the h2 Siamese config and of the bf16-storage
    config (batch 2, the configs' own 256 x 256 crops), and of the Siamese config with every BatchNorm frozen and with
    input gradients asked for (those change which weight grads carry the rows transform), every weight-grad launch
    recorded.  Its key -- family, NP, tile id or rows and channels per block, wave layout, SB, rows_bn, source
    transform, ring depth, and the optional fields set (source transform, rows_y, rows_out, rows_out_bound, column sums,
    a slice on either side) -- must be a key of some matrix row.  So must the key of the same descriptor at the config's
    shipped batch (the query is host-only, nothing of that size is allocated).  A dispatcher or kernel change that
    introduces an instance no row checks fails here and names it with its shape."""
    from multimodal_siamese_cd_amd import hip, trainers
    from multimodal_siamese_cd_amd.utils import datasets, experiment_manager as em, networks
    cfg = em.load_cfg(config)
    batch = 2
    assert int(cfg.TRAINER.BATCH_SIZE) % batch == 0
    scale = int(cfg.TRAINER.BATCH_SIZE) // batch
    net = networks.create_network(cfg).to(dev).train()
    if step == 'frozen_bn':
        networks.freeze_batchnorm(net, None)
    seen = {}
    orig = hip.conv_wgrad

    def spy(d, slabs):
        fields = [f for f, on in (('src_bn', d.src_scale), ('rows_y', d.rows_y.data), ('rows_out', d.rows_out.data),
                                  ('rows_out_bound', d.rows_out_bound), ('colsum', d.src_colsum),
                                  ('rows_slice', d.rows.ldc != d.rows.c), ('src_slice', d.src.ldc != d.src.c)) if on]
        what = f'ntaps={d.ntaps} R={d.rows.c} C={d.src.c} {d.rows.h}x{d.rows.w}'
        q = type(d).from_buffer_copy(d)
        for m in (1, scale):  # as launched, and at the shipped batch
            for v in (q.rows, q.src, q.rows_y, q.rows_out):
                v.n = d.rows.n * m
            seen.setdefault(instance_key(hip.wgrad_kernel_of(q), fields), f'{what} n={d.rows.n * m}')
        return orig(d, slabs)

    monkeypatch.setattr(hip, 'conv_wgrad', spy)
    gen = torch.Generator(device=dev).manual_seed(1)
    b = datasets.synthetic_batch(cfg, batch, dev, gen)
    x1, x2 = b['x_t1'], b['x_t2']
    if step == 'input_grad':
        x1, x2 = x1.clone().requires_grad_(), x2.clone().requires_grad_()
    loss = trainers.step_loss(cfg, net(x1, x2), b, net)
    loss.backward()
    torch.cuda.synchronize()
    monkeypatch.undo()
    assert torch.isfinite(loss)
    covered = {case_key(c) for c in CASES}
    print(f'{config} / {step}: {len(seen)} instance keys over the weight-grad launches')
    for key, what in sorted(seen.items(), key=str):
        print(('  ' if key in covered else '  UNCHECKED ') + f'{key}  ({what})')
    assert seen
    missing = {key: v for key, v in seen.items() if key not in covered}
    assert not missing, missing


def test_report_worst_measured():
    """Prints the worst measured ratio per family (the table of DESIGN.md 4); asserts nothing."""
    keys = ['ceiling', 'rel', 'finalize', 'colsum']
    print('\nfamily         ' + ' '.join(f'{k:>11s}' for k in keys))
    for tag in sorted(WORST):
        print(f'{tag:14s} ' + ' '.join(f'{WORST[tag][k]:11.3e}' if k in WORST[tag] else f'{"-":>11s}' for k in keys))
