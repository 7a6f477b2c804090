"""Which kernel instance a weight-grad descriptor runs and how its K range is split, pinned on the host (no GPU:
scd_wgrad_kernel reads only the alignment of the descriptor's pointers, so the descriptors here carry fake ones; its
one device call, the cached occupancy query of the split plan, falls back to constants without a device).

The query goes through the launch's own decision (wgrad_choose -> wgrad16_choose / wgrad16_c16_choose /
wgrad_generic_choose, then wgrad_split and wgrad_prepare), so what is pinned here is what scd_conv_wgrad launches.
Expected values are taken from the comments of csrc/conv_halo16.hip and csrc/conv_f32.hip, not from the function under
test.
"""
import ctypes
import itertools

import pytest

from _wgrad_matrix import CASES, FORM_FIELDS, IDS, fake_wgrad_desc, less_split

ARITH = {0: 'f32', 1: 'bf16', 3: 'x3', 5: 'x5', 4: 'h2', 2: 'h2'}


@pytest.fixture(scope='module')
def hip():
    from multimodal_siamese_cd_amd import build, hip
    build.build_lib()
    hip.load_library()
    return hip


def query(hip, *a, **k):
    return hip.wgrad_kernel_of(fake_wgrad_desc(*a, **k))


@pytest.mark.parametrize('case', CASES, ids=IDS)
def test_ladder_walk(hip, case):
    """Every row of the GPU matrix runs the instance it claims, and the older queries agree with it."""
    d = fake_wgrad_desc(case.math, case.store, case.kind, case.n, case.h, case.w, case.R, case.C, case.form)
    k = hip.wgrad_kernel_of(d)
    assert less_split(k) == case.inst
    halo = k.family in ('halo16', 'halo16_dma', 'halo16_c16')
    assert hip.wgrad_rows_per_block(d) == (k.block_rows if halo else 0)
    assert hip.wgrad_arith(d) == ARITH[k.np]
    assert hip.lib().scd_wgrad_src_bn_supported(ctypes.byref(d)) == int(halo)
    # what the row says, written per row in the table, not derived from the queried instance
    assert hip.lib().scd_wgrad_rows_bn_supported(ctypes.byref(d)) == int(case.rbn)
    assert hip.wgrad_colsum_supported(d) == case.colsum
    ns, nb = ctypes.c_int32(0), ctypes.c_size_t(0)
    assert hip.lib().scd_wgrad_plan(ctypes.byref(d), ctypes.byref(ns), ctypes.byref(nb)) == 0
    ntaps = 9 if case.kind == '3x3' else 4
    assert ns.value == k.nsplit and nb.value == k.nsplit * case.R * ntaps * case.C * 4


def test_matrix_is_complete():
    """Every row of the table in _wgrad_matrix.py appears in every form its instance supports; names are unique."""
    have = {(c.inst.family, c.inst.np, c.inst.block_rows, c.inst.sb, c.form) for c in CASES}
    base = ['plain', 'src_bn', 'src_slice', 'rows_slice']
    more = base + ['src_bn3']
    rbn = ['rows_bn', 'rows_bn+src_bn']
    c16 = more + ['rows_y', 'rows_y+src_bn']
    want = {
        ('halo16', 4, 128, False): more + rbn, ('halo16', 4, 64, False): more, ('halo16', 3, 64, False): more,
        ('halo16', 5, 64, False): more, ('halo16', 1, 128, False): more + rbn, ('halo16', 1, 64, False): more + rbn,
        # bf16 storage: the ring, and its register-staged fallback for three source segments
        ('halo16_dma', 1, 128, True): base + rbn, ('halo16_dma', 1, 64, True): base + rbn,
        ('halo16', 1, 128, True): ['src_bn3'], ('halo16', 1, 64, True): ['src_bn3'],
        ('halo16_c16', 4, 64, False): c16, ('halo16_c16', 3, 64, False): c16, ('halo16_c16', 5, 64, False): c16,
        ('halo16_c16', 1, 64, False): c16, ('halo16_c16', 1, 64, True): c16,
    }
    for row, forms in want.items():
        for f in forms:
            assert row[:4] + (f,) in have, (row, f)
        # one patch with one image and with three, on every row
        fam = [c for c in CASES if (c.inst.family, c.inst.np, c.inst.block_rows, c.inst.sb) == row and c.form == 'plain']
        if row[0] != 'halo16' or not row[3]:
            assert {(c.n, c.h, c.w) for c in fam} >= {(1, 2, 16), (3, 2, 16)}, row
    # the ring depths: 4 plain and transformed at 64 rows, 5 transformed at 128 rows, 3 / 5 with the rows transform
    rings = {(c.inst.block_rows, c.inst.src_xform, c.inst.rows_bn, c.inst.ring) for c in CASES if c.inst.family == 'halo16_dma'}
    assert rings == {(64, False, False, 4), (128, False, False, 4), (64, True, False, 4), (128, True, False, 5),
                     (64, False, True, 3), (128, False, True, 5), (64, True, True, 3), (128, True, True, 5)}
    # the DMA instances also on 1, 2 and 3 patches in total (shorter than every ring)
    for rb in (64, 128):
        assert {c.n * c.h * c.w // 32 for c in CASES if c.inst.family == 'halo16_dma' and c.inst.block_rows == rb} >= {1, 2, 3}
    # ConvT: plain, column sums and a source slice per arithmetic; every tile id
    convt = {(c.inst.np, c.inst.sb, c.form) for c in CASES if c.kind == 'convT'}
    for np_, sb in ((4, False), (3, False), (1, False), (1, True)):
        assert {(np_, sb, 'plain'), (np_, sb, 'colsum'), (np_, sb, 'colsum+src_slice')} <= convt
    assert (0, False, 'plain') in convt and (0, False, 'src_slice') in convt
    assert {c.inst.tile for c in CASES if c.inst.family == 'generic_split'} == {0, 1, 2, 3, 4}
    assert all(c.form in FORM_FIELDS for c in CASES)
    assert len(set(IDS)) == len(CASES)


def _units(kind, n, h, w):
    return (n * h * w // 32, 8) if kind == 'halo' else (n * h * w, 16)


PRIMES = (1, 2, 3, 5, 7, 11, 13)


@pytest.mark.parametrize('math,store,kind,C', [('h2', 'f32', 'halo', 64), ('x3', 'f32', 'halo', 128),
                                               ('bf16', 'bf16', 'halo', 192), ('h2', 'f32', 'halo', 16),
                                               ('h2', 'f32', 'convT', 64), ('bf16', 'bf16', 'convT', 48),
                                               ('f32', 'f32', 'convT', 32)])
def test_plan_invariants(hip, math, store, kind, C):
    """Over a sweep of (n, h, w, R) with prime n and odd unit counts: the splits tile the K range exactly and the plan
    and the query agree.  U units (2x16 patches on the halo kernels, pixels on the generic ones):
      (nsplit - 1) kchunk < U <= nsplit kchunk, nsplit >= 1, slab_bytes = nsplit R ntaps C 4, plan nsplit = query nsplit;
      generic: kchunk % 16 == 0 (the K step of the kernel);
      halo: split_units is called with a granule of one patch and 8 patches as the unit that bounds the split count,
      so what holds, and is asserted, is nsplit <= ceil(U / 8) -- not kchunk % 8 == 0: 8 patches cap how finely the
      range is cut, they are no step (21 patches are planned as 3 x 7, and the kernels walk any patch range); the
      generic kernels likewise cut no finer than ceil(U / 256).
    The capacity comes from the occupancy query, or its fallback constants without a device; the invariants hold for
    any capacity."""
    count = 0
    for n, (h, w), R in itertools.product(PRIMES, [(2, 16), (6, 16), (10, 32), (14, 48), (26, 32), (18, 80)],
                                          (64, 128, 192, 384)):
        if kind == 'convT':
            h, w = h + 1, w + 2  # odd sizes: pixels no multiple of 16
        d = fake_wgrad_desc(math, store, '3x3' if kind == 'halo' else 'convT', n, h, w, R, C)
        k = hip.wgrad_kernel_of(d)
        U, g = _units(kind, n, h, w)
        assert (k.family in ('halo16', 'halo16_dma', 'halo16_c16')) == (kind == 'halo'), k
        assert k.nsplit >= 1 and (k.nsplit - 1) * k.kchunk < U <= k.nsplit * k.kchunk, (n, h, w, R, k)
        if kind == 'halo':
            assert k.nsplit <= (U + g - 1) // g, (n, h, w, R, k)
        else:
            assert k.kchunk % g == 0 and k.nsplit <= (U + 255) // 256, (n, h, w, R, k)
        ns, nb = ctypes.c_int32(0), ctypes.c_size_t(0)
        assert hip.lib().scd_wgrad_plan(ctypes.byref(d), ctypes.byref(ns), ctypes.byref(nb)) == 0
        assert ns.value == k.nsplit and nb.value == k.nsplit * R * (9 if kind == 'halo' else 4) * C * 4
        count += 1
    assert count == len(PRIMES) * 6 * 4  # 168 shapes per family


def test_row_block_by_r(hip):
    """R % 128 decides the row block of the h2 / bf16 along-c variants; x3 / x5 stay at 64; SCD_TUNE_WGRAD_R64 keeps 64."""
    for math, store in (('h2', 'f32'), ('bf16', 'f32'), ('bf16', 'bf16')):
        for R, rb in ((64, 64), (128, 128), (192, 64), (256, 128), (320, 64), (384, 128)):
            k = query(hip, math, store, '3x3', 2, 16, 32, R, 64)
            assert (k.block_rows, k.threads, k.layout) == (rb, 4 * rb, 'along_c'), (math, R, k)
        k = query(hip, math, store, '3x3', 2, 16, 32, 256, 64, tune=hip.TUNE_WGRAD_R64)
        assert (k.block_rows, k.threads) == (64, 256)
    for math in ('x3', 'x5'):
        k = query(hip, math, 'f32', '3x3', 2, 16, 32, 256, 64)
        assert (k.block_rows, k.layout, k.np) == (64, '2x2', {'x3': 3, 'x5': 5}[math])


def test_tune_bits_move_the_instance(hip):
    # SCD_TUNE_W16_LAYOUT_2X2: h2 / bf16 back on 2x2 waves, which has no 128-row block, no rows transform and no ring
    for math, store, np_ in (('h2', 'f32', 4), ('bf16', 'f32', 1), ('bf16', 'bf16', 1)):
        d = fake_wgrad_desc(math, store, '3x3', 2, 16, 32, 256, 64, tune=hip.TUNE_W16_LAYOUT_2X2)
        k = hip.wgrad_kernel_of(d)
        assert (k.family, k.np, k.layout, k.block_rows, k.ring) == ('halo16', np_, '2x2', 64, 0), k
        assert hip.lib().scd_wgrad_rows_bn_supported(ctypes.byref(d)) == 0
    # SCD_TUNE_WGRAD16_REGSTAGE: bf16 storage through registers, same block
    for form in ('plain', 'src_bn', 'rows_bn', 'rows_bn+src_bn'):
        k = query(hip, 'bf16', 'bf16', '3x3', 2, 16, 32, 256, 64, form, tune=hip.TUNE_WGRAD16_REGSTAGE)
        assert (k.family, k.ring, k.sb, k.block_rows, k.layout) == ('halo16', 0, True, 128, 'along_c'), (form, k)
        assert query(hip, 'bf16', 'bf16', '3x3', 2, 16, 32, 256, 64, form).family == 'halo16_dma'
    # SCD_TUNE_NO_WGRAD_C16: the input layer on the generic x3 kernel (R 64, Ng 144: tile 2 and 3 tie at 64 x 192)
    k = query(hip, 'h2', 'f32', '3x3', 2, 16, 32, 64, 16, tune=hip.TUNE_NO_WGRAD_C16)
    assert (k.family, k.np, k.tile) == ('generic_split', 4, 2), k
    k = query(hip, 'x3', 'f32', '3x3', 2, 16, 32, 64, 16, tune=hip.TUNE_NO_WGRAD_C16)
    assert (k.family, k.np, k.tile) == ('generic_split', 3, 2), k
    # SCD_TUNE_NO_WGRAD_H2: the ConvTranspose weight grad on x3 (the halo kernels are not affected)
    assert query(hip, 'h2', 'f32', 'convT', 2, 8, 8, 128, 64).np == 4
    assert query(hip, 'h2', 'f32', 'convT', 2, 8, 8, 128, 64, tune=hip.TUNE_NO_WGRAD_H2).np == 3
    assert query(hip, 'h2', 'f32', '3x3', 2, 16, 32, 128, 64, tune=hip.TUNE_NO_WGRAD_H2).np == 4
    # SCD_TUNE_H2_NO_PRESCALE: the two-term split without the pre-scaled low term (np 2), no rows transform; the
    # 16-channel kernel has no such variant and runs x3
    d = fake_wgrad_desc('h2', 'f32', '3x3', 2, 16, 32, 128, 64, tune=hip.TUNE_H2_NO_PRESCALE)
    k = hip.wgrad_kernel_of(d)
    assert (k.family, k.np, k.block_rows, k.layout) == ('halo16', 2, 128, 'along_c') and hip.wgrad_arith(d) == 'h2'
    assert hip.lib().scd_wgrad_rows_bn_supported(ctypes.byref(d)) == 0
    d = fake_wgrad_desc('h2', 'f32', '3x3', 2, 16, 32, 64, 16, tune=hip.TUNE_H2_NO_PRESCALE)
    assert hip.wgrad_kernel_of(d).np == 3 and hip.wgrad_arith(d) == 'x3'
    # SCD_TUNE_NO_HALO: no halo kernel at all
    assert query(hip, 'h2', 'f32', '3x3', 2, 16, 32, 128, 64, tune=hip.TUNE_NO_HALO).family == 'generic_split'


def test_h2_needs_both_bounds(hip):
    """h2 with a bound missing runs the x3 instance (2x2 waves, 64 rows) and reports x3."""
    for rb, sb_ in ((True, False), (False, True), (False, False)):
        d = fake_wgrad_desc('h2', 'f32', '3x3', 2, 16, 32, 256, 64, bound=False)
        d.rows_bound = 0x7F0000100000 if rb else None
        d.src_bound = 0x7F0000200000 if sb_ else None
        k = hip.wgrad_kernel_of(d)
        assert (k.family, k.np, k.layout, k.block_rows) == ('halo16', 3, '2x2', 64), k
        assert hip.wgrad_arith(d) == 'x3'
    assert query(hip, 'h2', 'f32', '3x3', 2, 16, 32, 64, 16, bound=False).np == 3
    assert query(hip, 'h2', 'f32', 'convT', 2, 8, 8, 128, 64, bound=False).np == 3


def test_refusals(hip):
    """What the launch refuses, the query refuses with the launch's message."""
    # rows_bn under h2 at R % 128 != 0 (the 64-row h2 block has no rows transform), under x3, on a generic shape
    for a in (('h2', 'f32', '3x3', 2, 16, 32, 192, 64), ('x3', 'f32', '3x3', 2, 16, 32, 128, 64),
              ('h2', 'f32', '3x3', 2, 16, 24, 128, 64)):
        assert hip.lib().scd_wgrad_rows_bn_supported(ctypes.byref(fake_wgrad_desc(*a))) == 0
        with pytest.raises(RuntimeError, match='scd_wgrad_rows_bn_supported'):
            query(hip, *a, form='rows_bn')
    # three rows segments
    with pytest.raises(RuntimeError, match='scd_wgrad_rows_bn_supported'):
        query(hip, 'bf16', 'bf16', '3x3', 3, 16, 32, 128, 64, form='rows_bn', rows_nseg=3)
    assert query(hip, 'bf16', 'bf16', '3x3', 4, 16, 32, 128, 64, form='rows_bn', rows_nseg=2).rows_bn
    # rows_out on the 16-channel kernel (it stores no dY)
    with pytest.raises(RuntimeError, match='rows_out'):
        query(hip, 'h2', 'f32', '3x3', 2, 16, 32, 64, 16, form='rows_bn')
    # bf16 views on a shape no bf16 kernel takes: a 3x3 the halo kernels refuse
    with pytest.raises(RuntimeError, match='bf16'):
        query(hip, 'bf16', 'bf16', '3x3', 2, 16, 24, 64, 64)
    with pytest.raises(RuntimeError, match='bf16'):
        hip.wgrad_arith(fake_wgrad_desc('bf16', 'bf16', '3x3', 2, 16, 24, 64, 64))
    # bf16 views under another arithmetic
    d = fake_wgrad_desc('bf16', 'bf16', '3x3', 2, 16, 32, 64, 64)
    d.math = hip._MATH_NAMES['x3']
    with pytest.raises(RuntimeError, match='SCD_MATH_BF16'):
        hip.wgrad_kernel_of(d)
    # the source transform and the column sums off their kernels
    with pytest.raises(RuntimeError, match='scd_wgrad_src_bn_supported'):
        query(hip, 'x3', 'f32', 'convT', 2, 8, 8, 128, 64, form='src_bn')
    with pytest.raises(RuntimeError, match='scd_wgrad_colsum_supported'):
        query(hip, 'f32', 'f32', 'convT', 2, 8, 8, 128, 64, form='colsum')
    # every view's channels are a multiple of 4 (the descriptor check), so the column sums' own c % 4 rule cannot be
    # the one that refuses: C = 8 has them, C = 6 is no valid view at all
    assert hip.wgrad_colsum_supported(fake_wgrad_desc('x3', 'f32', 'convT', 2, 8, 8, 128, 8))
    assert not hip.wgrad_colsum_supported(fake_wgrad_desc('x3', 'f32', 'convT', 2, 8, 8, 128, 6))
    with pytest.raises(RuntimeError, match='multiples of 4'):
        query(hip, 'x3', 'f32', 'convT', 2, 8, 8, 128, 6)


def test_source_segments_decide_the_ring(hip):
    """bf16 storage with a source transform: the ring for one or two coefficient segments, registers for more."""
    for nseg, fam in ((1, 'halo16_dma'), (2, 'halo16_dma'), (3, 'halo16'), (6, 'halo16')):
        k = query(hip, 'bf16', 'bf16', '3x3', 6, 16, 32, 128, 64, form='src_bn', src_nseg=nseg)
        assert (k.family, k.src_xform, k.sb) == (fam, True, True), (nseg, k)
        assert k.ring == (5 if fam == 'halo16_dma' else 0)
    # fp32 storage has no ring
    assert query(hip, 'bf16', 'f32', '3x3', 6, 16, 32, 128, 64, form='src_bn').family == 'halo16'
