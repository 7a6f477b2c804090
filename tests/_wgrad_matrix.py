"""The instance matrix of the weight-grad kernels (wgrad_halo16_x3, wgrad_halo16_dma, wgrad_halo16_c16, the generic
wgrad_x3 tiles and wgrad_f32): the cases tests/test_wgrad_instance_matrix_gpu.py runs against fp64 and
tests/test_wgrad_instances.py walks through the host query (scd_wgrad_kernel) on a machine without a GPU.  Test
infrastructure.

Every case names the instance it is there to check.  The expected instances are written down here from the dispatcher's
comments (wgrad16_choose and wgrad16_c16_choose in csrc/conv_halo16.hip, wgrad_generic_choose and kWgradTiles in
csrc/conv_f32.hip), by hand, not read back from the query:

  halo16 family (3x3, stride 1, R and C multiples of 64, h even, w a multiple of 16); C = 16 runs halo16_c16
  arithmetic / storage          halo16                                                    C = 16
  h2, both bounds               np 4, along c; 128 rows (512 threads) when R % 128 == 0,  np 4, 64 rows, rows_bn on / off
                                else 64; rows_bn only on the 128-row block
  h2 without both bounds, x3    np 3, 2x2 waves, 64 rows                                  np 3
  x5                            np 5, 2x2 waves, 64 rows                                  np 5
  bf16, fp32 storage            np 1, along c, 64 / 128 rows, through registers;          np 1
                                rows_bn on both
  bf16, bf16 storage, plain     halo16_dma, ring 4, 64 / 128 rows                         np 1, SB
  ... source transform          ring 4 (64 rows), ring 5 (128 rows); more than two source
                                segments: halo16 SB through registers
  ... rows_bn                   ring 3 (64 rows), ring 5 (128 rows), with and without the
                                source transform

  Everything else runs the generic kernel -- the ConvTranspose weight grad (4 taps, stride 2) and the 3x3 shapes the
  halo kernels refuse -- on the kWgradTiles entry of least padded work for (R, ntaps C) (ties: the larger tile, then the
  first): 0 128x128, 1 64x256, 2 64x192, 3 64x96 (128 threads), 4 32x128.  h2 (np 4) where both bounds are set, bf16
  (np 1) for 4 taps under bf16, x3 (np 3) otherwise; SCD_MATH_F32 runs wgrad_f32 (np 0).

Shapes, the smallest at which each mechanism can go wrong (K units: 2x16 patches for the halo kernels):
  one_patch     h 2, w 16, n 1 and n 3: the whole halo out of range on three sides; with n 3 neighbouring patches are
                different images.  1 and 3 patches in total, `two_patch` (1 x 2 x 32) 2: shorter than every DMA ring.
  ragged        3 x 10 x 32: 30 patches, 10 per image.  With four splits of 8 the last holds 6 and no split boundary is
                an image boundary (the GPU test asserts nsplit >= 2, npatch % kchunk and kchunk % 10 from the query).
                The plan cuts the K range only from about 11 blocks per split at 64 rows (6 at 128 rows), so these rows
                have C 256 (192): 12 (9) blocks.  On the MI355X: 4 splits of 8 patches, as without a device.
  seg           2 x 10 x 48: 30 patches, 15 per image; the segment boundary (patch 15) lies inside split [8, 16).  The
                forms with two coefficient segments run here; shifts of both signs, some source scales negative.
                The 16-channel kernel has one channel tile and the MI355X holds four (bf16: five) of its blocks per CU:
                R 384 (six blocks per split) on 3 x 34 x 16 (51 patches, 17 per image: 5 splits of 11, bf16 6 of 9)
                and 2 x 22 x 32 (44 patches, 22 per image: 5 of 9, bf16 6 of 8), ragged at either capacity and at
                the constants used without a device.
  row tiles     R 192 = three 64-row blocks (R % 128 != 0 keeps h2 / bf16 off the 128-row block), R 384 = three 128-row
                blocks, C 192 = three channel tiles (only tile 0 writes rows_out).
  ConvT         3 x 10 x 18: M = 540 pixels, not a multiple of 16 (the K step leaves a tail); R 256 / C 128 is cut into
                3 splits of 192 pixels there (asserted from the query); R 96 / C 48: neither a multiple of the tile.
"""
from __future__ import annotations

from collections import namedtuple

from multimodal_siamese_cd_amd import hip

# kind: '3x3' (rows = dY, src = X) or 'convT' (rows = X, src = dOut at stride 2); R rows channels, C source channels
# rbn / colsum: what scd_wgrad_rows_bn_supported / scd_wgrad_colsum_supported answer for the row's descriptor, written per
# row from the table above (rows transform: h2 on 128-row blocks, bf16, the 16-channel kernel; column sums: the generic
# split-arithmetic kernel), not computed from the queried instance
Case = namedtuple('Case', 'name math store kind n h w R C form inst rbn colsum')

# What each form sets in the descriptor (the coverage test keys a production launch by the same set)
FORM_FIELDS = {
    'plain': (), 'src_bn': ('src_bn',), 'src_bn3': ('src_bn',),
    'rows_bn': ('rows_y', 'rows_out', 'rows_out_bound'), 'rows_bn+src_bn': ('src_bn', 'rows_y', 'rows_out', 'rows_out_bound'),
    'rows_dy': ('rows_y', 'rows_out'), 'rows_dy+src_bn': ('src_bn', 'rows_y', 'rows_out'),  # no bound: the bf16 configs
    'rows_y': ('rows_y',), 'rows_y+src_bn': ('src_bn', 'rows_y'),   # the 16-channel kernel forms dY and stores none
    'rows_slice': ('rows_slice',), 'src_slice': ('src_slice',), 'colsum': ('colsum',),
    'colsum+src_slice': ('colsum', 'src_slice'),
}

ONE, ONE3, TWO, RAGGED, SEG = (1, 2, 16), (3, 2, 16), (1, 2, 32), (3, 10, 32), (2, 10, 48)
RAGGED17, SEG22 = (3, 34, 16), (2, 22, 32)  # the 16-channel kernel: 17 / 22 patches per image (see `seg` above)
CONVT = (3, 10, 18)

TILES = {0: (128, 128, 256), 1: (64, 256, 256), 2: (64, 192, 256), 3: (64, 96, 128), 4: (32, 128, 256)}


def _halo(np_, rows, layout, sb=False, rows_bn=False, src_xform=False, ring=0):
    return hip.WgradKernel('halo16_dma' if ring else 'halo16', np_, -1, rows, 64, layout, sb, rows_bn, src_xform, ring,
                           4 * rows, None, None)


def _c16(np_, sb=False, rows_bn=False, src_xform=False):
    return hip.WgradKernel('halo16_c16', np_, -1, 64, 16, None, sb, rows_bn, src_xform, 0, 256, None, None)


def _generic(np_, tile, sb=False):
    bm, bn, threads = TILES[tile]
    return hip.WgradKernel('generic_split' if np_ else 'generic_f32', np_, tile, bm, bn, None, sb, False, False, 0,
                           threads, None, None)


def less_split(k):
    """A queried instance without its split (what a row pins; the split depends on the device's capacity)."""
    return k._replace(nsplit=None, kchunk=None)


# tag, arithmetic, storage, both bounds, np, layout, R, rows per block, whether the instance has the rows transform
_HALO16 = [
    ('h2_r128', 'h2', 'f32', True, 4, 'along_c', 384, 128, True),
    ('h2_r64', 'h2', 'f32', True, 4, 'along_c', 192, 64, False),
    ('x3', 'x3', 'f32', False, 3, '2x2', 192, 64, False),
    ('x5', 'x5', 'f32', False, 5, '2x2', 192, 64, False),
    ('bf16_r128', 'bf16', 'f32', False, 1, 'along_c', 384, 128, True),
    ('bf16_r64', 'bf16', 'f32', False, 1, 'along_c', 192, 64, True),
    ('sb_r128', 'bf16', 'bf16', False, 1, 'along_c', 384, 128, True),
    ('sb_r64', 'bf16', 'bf16', False, 1, 'along_c', 192, 64, True),
]
# the DMA ring depth by (rows per block, source transform, rows transform)
_RING = {(64, False, False): 4, (128, False, False): 4, (64, True, False): 4, (128, True, False): 5,
         (64, False, True): 3, (128, False, True): 5, (64, True, True): 3, (128, True, True): 5}
_C16 = [('c16_h2', 'h2', 'f32', 4), ('c16_x3', 'x3', 'f32', 3), ('c16_x5', 'x5', 'f32', 5), ('c16_bf16', 'bf16', 'f32', 1),
        ('c16_sb', 'bf16', 'bf16', 1)]


def _cases():
    out = []

    def add(name, math, store, kind, shape, R, C, form, inst, rbn=False, colsum=False):
        out.append(Case(name, math, store, kind, *shape, R, C, form, inst, rbn, colsum))

    for tag, math, store, _, np_, lay, R, rb, rbn in _HALO16:
        sb = store == 'bf16'

        def inst(form, sb=sb, np_=np_, lay=lay, rb=rb):
            xf, rt = 'src_bn' in form, form.split('+')[0] in ('rows_bn', 'rows_dy')
            ring = 0
            if sb and form != 'src_bn3':  # bf16 storage: the ring, but three source segments stage through registers
                ring = _RING[rb, xf, rt]
            return _halo(np_, rb, lay, sb, rt, xf, ring)

        def row(name, shape, C, form, rbn=rbn):
            add(f'{tag}-{name}', math, store, '3x3', shape, R, C, form, inst(form), rbn)
        cw = 192 if rb == 128 else 256  # channel tiles enough for the split plan to cut the K range (`ragged` above)
        row('one_patch', ONE, 64, 'plain')
        row('one_patch_n3', ONE3, 192, 'plain')
        row('ragged-plain', RAGGED, cw, 'plain')
        row('seg-src_bn', SEG, cw, 'src_bn')
        row('ragged-src_bn3', RAGGED, 64, 'src_bn3')
        row('ragged-rows_slice', RAGGED, 64, 'rows_slice')
        row('ragged-src_slice', RAGGED, 128, 'src_slice')
        if rbn:
            row('seg-rows_bn', SEG, cw, 'rows_bn')
            row('seg-rows_bn+src_bn', SEG, cw, 'rows_bn+src_bn')
        if sb:  # short rings: 1, 2 and 3 patches in total are the one_patch rows and two_patch; with the transforms
            row('two_patch', TWO, 64, 'plain')
            row('one_patch_n3-rows_bn', ONE3, 64, 'rows_bn')
            row('one_patch-rows_bn+src_bn', ONE, 64, 'rows_bn+src_bn')
            # as the bf16 configs launch it: dY stored, no bound asked for
            row('seg-rows_dy', SEG, cw, 'rows_dy')
            row('seg-rows_dy+src_bn', SEG, cw, 'rows_dy+src_bn')
    # h2 with one bound missing runs the x3 instance
    add('h2_unbounded-plain', 'h2u', 'f32', '3x3', RAGGED, 128, 64, 'plain', _halo(3, 64, '2x2'), False)
    add('h2_unbounded-src_bn', 'h2u', 'f32', '3x3', SEG, 128, 64, 'src_bn', _halo(3, 64, '2x2', False, False, True))

    for tag, math, store, np_ in _C16:  # every arithmetic has the rows transform (rows_y: no dY is stored) and the source's
        sb = store == 'bf16'

        def row(name, shape, R, form, tag=tag, math=math, store=store, np_=np_, sb=sb):
            add(f'{tag}-{name}', math, store, '3x3', shape, R, 16, form,
                _c16(np_, sb, 'rows_y' in form, 'src_bn' in form), True)
        row('one_patch', ONE, 64, 'plain')
        row('one_patch_n3', ONE3, 64, 'plain')
        row('ragged-plain', RAGGED17, 384, 'plain')
        row('seg-src_bn', SEG22, 384, 'src_bn')
        row('ragged-src_bn3', RAGGED, 64, 'src_bn3')
        row('seg-rows_y', SEG22, 384, 'rows_y')
        row('seg-rows_y+src_bn', SEG22, 384, 'rows_y+src_bn')
        row('ragged-rows_slice', RAGGED, 64, 'rows_slice')
        row('ragged-src_slice', RAGGED, 128, 'src_slice')

    # the generic kernels.  Tile by least padded work over (R, Ng = ntaps C):
    #   ConvT R 96, C 48 (Ng 192): 128x256 on tiles 0 / 1, 128x192 on 2 / 3, 96x256 on 4 -- a three-way tie, largest tile: 2
    #   ConvT R 256, C 128 (Ng 512): exact on tiles 0 and 1, equal areas, the first: 0   (the shipped ConvT levels: 0)
    #   ConvT R 64, C 64 (Ng 256): exact on tiles 1 and 4, the larger: 1
    #   ConvT R 64, C 32 (Ng 128): exact on tile 4 only: 4
    #   ConvT R 64, C 24 (Ng 96): exact on tile 3 only: 3
    for tag, math, store, np_ in [('gen_h2', 'h2', 'f32', 4), ('gen_x3', 'x3', 'f32', 3), ('gen_bf16', 'bf16', 'f32', 1),
                                  ('gen_sb', 'bf16', 'bf16', 1), ('gen_f32', 'f32', 'f32', 0)]:
        sb = store == 'bf16'
        cs = math != 'f32'  # the column sums: every split arithmetic, not wgrad_f32
        add(f'{tag}-convT-plain', math, store, 'convT', CONVT, 96, 48, 'plain', _generic(np_, 2, sb), False, cs)
        add(f'{tag}-convT-t0-split', math, store, 'convT', CONVT, 256, 128, 'plain', _generic(np_, 0, sb), False, cs)
        if math != 'x3':
            add(f'{tag}-convT-src_slice', math, store, 'convT', CONVT, 64, 64, 'src_slice', _generic(np_, 1, sb), False, cs)
        if np_:  # the column sums: the split arithmetics only
            add(f'{tag}-convT-t0-split-colsum', math, store, 'convT', CONVT, 256, 128, 'colsum', _generic(np_, 0, sb), False, cs)
            add(f'{tag}-convT-colsum+src_slice', math, store, 'convT', CONVT, 96, 48, 'colsum+src_slice',
                _generic(np_, 2, sb), False, cs)
    # the shipped ConvT levels: g_up is a slice of the concat gradient and the bias grad comes from the column sums, on
    # tile 0 (R >= 128) and tile 1 (R 64, C 64)
    for tag, math, store, np_ in [('gen_h2', 'h2', 'f32', 4), ('gen_sb', 'bf16', 'bf16', 1)]:
        add(f'{tag}-convT-t0-colsum+src_slice', math, store, 'convT', CONVT, 128, 64, 'colsum+src_slice',
            _generic(np_, 0, store == 'bf16'), False, True)
        add(f'{tag}-convT-t1-colsum+src_slice', math, store, 'convT', CONVT, 64, 64, 'colsum+src_slice',
            _generic(np_, 1, store == 'bf16'), False, True)
    add('gen_h2-convT-t4', 'h2', 'f32', 'convT', CONVT, 64, 32, 'plain', _generic(4, 4), False, True)
    add('gen_h2-convT-t3', 'h2', 'f32', 'convT', CONVT, 64, 24, 'plain', _generic(4, 3), False, True)
    add('gen_sb-convT-t4', 'bf16', 'bf16', 'convT', CONVT, 64, 32, 'plain', _generic(1, 4, True), False, True)
    # 3x3 shapes the halo kernels refuse: w = 24 is no multiple of 16; R = 96 no multiple of 64.  bf16 keeps x3 there.
    #   R 64, C 64 (Ng 576): 64x768 on tile 1, 64x576 exact on tiles 2 and 3, the larger: 2
    #   R 96, C 32 (Ng 288): 128x384 on 0, 128x512 on 1, 128x384 on 2, 128x288 on 3, 96x384 on 4: tiles 3 and 4 tie, 64x96: 3
    add('gen_x3-3x3-w24', 'x3', 'f32', '3x3', (2, 10, 24), 64, 64, 'plain', _generic(3, 2), False, True)
    add('gen_h2-3x3-w24', 'h2', 'f32', '3x3', (2, 10, 24), 64, 64, 'plain', _generic(4, 2), False, True)
    add('gen_bf16-3x3-w24', 'bf16', 'f32', '3x3', (2, 10, 24), 64, 64, 'plain', _generic(3, 2), False, True)
    add('gen_x3-3x3-R96', 'x3', 'f32', '3x3', (2, 10, 32), 96, 32, 'plain', _generic(3, 3), False, True)
    add('gen_f32-3x3-R96', 'f32', 'f32', '3x3', (2, 10, 32), 96, 32, 'plain', _generic(0, 3), False, False)
    return out


CASES = _cases()
IDS = [c.name for c in CASES]


def asserts_split(c: Case) -> str | None:
    """'ragged' / 'seg' / 'convT' where the row is there for a K range cut at an awkward place: the GPU test asserts
    the cut from the query, it does not assume it."""
    if c.name.endswith('-ragged-plain'):
        return 'ragged'
    if '-seg-' in c.name:
        return 'seg'
    return 'convT' if '-split' in c.name else None

# slices of wider buffers, the offsets of test_weight_grad_dma_ring_bit_identical's concat views: the rows at channel 64
# of a buffer 64 + R wide, the source at channel 0 of a buffer C + 64 wide
SLICE_EXTRA = 64


def instance_key(k, fields) -> tuple:
    """What the coverage test compares: the instance less its split, and the optional fields set."""
    return (k.family, k.np, k.tile, k.block_rows, k.block_channels, k.layout, k.sb, k.rows_bn, k.src_xform, k.ring,
            tuple(sorted(fields)))


def case_key(c: Case) -> tuple:
    return instance_key(c.inst, FORM_FIELDS[c.form])


# ------------------------------------------------------------------------------------------------
# Descriptors without a device: fake, suitably aligned, non-null pointers (the query reads their alignment only)
# ------------------------------------------------------------------------------------------------
FAKE = 0x7F0000100000  # 1 MiB aligned


def nseg_of(n: int, form: str) -> int:
    """Coefficient segments of a case's transforms: three for src_bn3, else two where n is even, else one."""
    return 3 if form == 'src_bn3' else 2 if n % 2 == 0 else 1


def fake_wgrad_desc(math: str, store: str, kind: str, n: int, h: int, w: int, R: int, C: int, form: str = 'plain',
                    tune: int = 0, bound: bool | None = None, src_nseg: int | None = None,
                    rows_nseg: int | None = None) -> 'hip.WGRAD':
    """An scd_wgrad_t as the GPU matrix builds it for `form`, on fake pointers.  math 'h2u': h2 without its bounds."""
    dt, eb = (hip.DT_BF16, 2) if store == 'bf16' else (hip.DT_F32, 4)
    f = FORM_FIELDS[form]
    r_off, r_ldc = (SLICE_EXTRA, R + SLICE_EXTRA) if 'rows_slice' in f else (0, R)
    s_ldc = C + SLICE_EXTRA if 'src_slice' in f else C
    p = lambda i, on=True: (3 + i) * FAKE if on else None
    rows = hip.NHWC(FAKE + eb * r_off, n, h, w, R, r_ldc, dt)
    if kind == '3x3':
        src, stride, taps = hip.NHWC(2 * FAKE, n, h, w, C, s_ldc, dt), 1, hip.TAPS_3X3
    else:
        src, stride, taps = hip.NHWC(2 * FAKE, n, 2 * h, 2 * w, C, s_ldc, dt), 2, hip.TAPS_2X2
    nt, dy, dx = hip._taps(taps)
    bound = math == 'h2' if bound is None else bound
    xf = 'src_bn' in f
    src_nseg = nseg_of(n, form) if src_nseg is None else src_nseg
    rows_nseg = nseg_of(n, 'rows_bn') if rows_nseg is None else rows_nseg
    d = hip.WGRAD(rows, src, stride, nt, dy, dx, p(0, xf), p(1, xf), src_nseg if xf else 0, p(2, bound), p(3, bound))
    d.math, d.tune = hip._MATH_NAMES['h2' if math == 'h2u' else math], tune
    if 'rows_y' in f:
        d.rows_y = hip.NHWC(p(4), n, h, w, R, R, dt)
        d.rows_nseg = rows_nseg
        d.rows_mean, d.rows_invstd, d.rows_gamma = p(5), p(6), p(7)
        d.rows_scale, d.rows_shift, d.rows_coef = p(8), p(9), p(10)
    if 'rows_out' in f:
        d.rows_out = hip.NHWC(p(11), n, h, w, R, R, dt)
        d.rows_out_bound = p(12, 'rows_out_bound' in f)
    if 'colsum' in f:
        d.src_colsum = p(13)
    return d
