"""Which kernel instance a 3x3 conv descriptor runs, pinned on the host (no GPU: scd_igemm_kernel initialises no device
and reads only the alignment of the descriptor's pointers, so the descriptors here carry fake ones).

The query goes through the launch's own decision (igemm_decide -> igemm_x3_choose -> halo16_pick / gather16_pick /
halo16_c16_pick -> halo16_instance), so what is pinned here is what scd_conv_igemm launches.  Expected values are taken
from the comments of csrc/conv_halo16.hip, not from the function under test.
"""
import ctypes

import pytest

from _conv_matrix import CASES, IDS, fake_desc


@pytest.fixture(scope='module')
def hip():
    from multimodal_siamese_cd_amd import build, hip
    build.build_lib()
    hip.load_library()
    return hip


def query(hip, *a, **k):
    keep = []
    return hip.igemm_kernel_of(fake_desc(*a, keep=keep, **k))


@pytest.mark.parametrize('case', CASES, ids=IDS)
def test_ladder_walk(hip, case):
    """Every row of the GPU matrix runs the instance it claims; the fused-record queries report that block's pixels."""
    keep = []
    d = fake_desc(case.math, case.store, case.n, case.h, case.w, case.c, case.n_out, case.form, keep=keep)
    assert hip.igemm_kernel_of(d) == case.inst
    # the queries and the launch agree: one record tile is one block's pixels
    tp = ctypes.c_int32(0)
    tiles = hip.lib().scd_igemm_stat_tiles(ctypes.byref(d), ctypes.byref(tp))
    assert tp.value == case.inst.block_pixels and tiles * tp.value == case.n * case.h * case.w


def test_matrix_is_complete():
    """Every layout row production can pick appears at the three tile widths, and every form on every row."""
    plain = {(c.inst.family, c.inst.layout, c.inst.np, c.inst.sb, c.inst.tile_width) for c in CASES if c.form == 'plain'}
    rows = [('halo16', r, 4, False) for r in (3, 4, 5)] + [('halo16', r, 1, False) for r in (0, 1)] + \
           [('halo16', r, 1, True) for r in (6, 7, 8)] + \
           [('halo16_c16', -1, 4, False), ('halo16_c16', -1, 1, False), ('halo16_c16', -1, 1, True)]
    for row in rows:
        for tw in (16, 32, 64):
            assert row + (tw,) in plain, (row, tw)
    forms = {(c.inst.layout, c.inst.np, c.inst.sb, c.form) for c in CASES if c.inst.tile_width != 16}
    for fam, r, np_, sb in rows:
        want = ['bias', 'stat', 'dst_bound', 'dst_slice', 'src_slice']
        if fam == 'halo16':
            want += ['in_bn', 'bn_bwd'] + (['bn_bwd_bound'] if np_ == 4 else [])
        for f in want:
            assert (r, np_, sb, f) in forms, (r, np_, sb, f)
    assert any(c.inst.layout == 9 for c in CASES)
    assert len({c.name for c in CASES}) == len(CASES)


@pytest.mark.parametrize('math,store,c,n_out,layout,bm,bn', [
    # h2: 1 x 4 waves from 128 outputs, 1 x 2 below, 2 x 2 waves of the same wave tile on 64-channel sources
    ('h2', 'f32', 128, 256, 3, 128, 128), ('h2', 'f32', 64, 128, 3, 128, 128), ('h2', 'f32', 128, 124, 4, 128, 64),
    ('h2', 'f32', 128, 64, 4, 128, 64), ('h2', 'f32', 64, 64, 5, 256, 64), ('h2', 'f32', 64, 96, 5, 256, 64),
    # bf16 with fp32 storage: the 2 x 2 tiles
    ('bf16', 'f32', 64, 128, 0, 128, 128), ('bf16', 'f32', 64, 64, 1, 128, 64), ('bf16', 'f32', 128, 96, 1, 128, 64),
    # bf16 storage: the 1 x N tiles at 3 blocks per SIMD
    ('bf16', 'bf16', 128, 128, 6, 128, 128), ('bf16', 'bf16', 128, 64, 7, 128, 64), ('bf16', 'bf16', 64, 64, 8, 256, 64),
    # x3 (no bound, no h2 split): the 2 x 2 tiles of every arithmetic
    ('x3', 'f32', 64, 128, 0, 128, 128), ('x3', 'f32', 64, 64, 1, 128, 64),
])
def test_automatic_layout(hip, math, store, c, n_out, layout, bm, bn):
    k = query(hip, math, store, 2, 32, 32, c, n_out)
    assert (k.family, k.layout, k.block_pixels, k.block_channels) == ('halo16', layout, bm, bn)
    assert k.np == {'h2': 4, 'bf16': 1, 'x3': 3}[math] and k.sb == (store == 'bf16') and not k.wl and not k.in_bn


def test_below_64_outputs_and_unbounded_h2_leave_the_kernel(hip):
    k = query(hip, 'x3', 'f32', 2, 32, 32, 64, 32)  # below 64 outputs: the 32x32x16 halo kernel, 256 px x 32 ch
    assert (k.family, k.layout, k.np, k.block_pixels, k.block_channels, k.tile_width) == ('halo32', -1, 3, 256, 32, 32)
    # h2 where no h2 kernel takes the conv (too few outputs, or no bound): the h2 split is ignored and the per-tap x3
    # kernel splits the fp32 weights itself
    assert query(hip, 'h2', 'f32', 2, 32, 32, 64, 32).family == 'x3'
    k = query(hip, 'h2', 'f32', 2, 32, 32, 64, 64, bound=False)
    assert (k.family, k.np, k.block_pixels, k.block_channels) == ('x3', 3, 128, 64)
    assert query(hip, 'h2', 'f32', 2, 32, 32, 64, 64, tune=hip.TUNE_H2_TILE64_128).layout == 4
    assert query(hip, 'h2', 'f32', 2, 32, 32, 64, 64, tune=hip.TUNE_H2_TILE64_2X2).layout == 1
    assert query(hip, 'h2', 'f32', 2, 32, 32, 64, 128, tune=hip.TUNE_H2_TILE_2X2).layout == 0
    assert query(hip, 'f32', 'f32', 2, 32, 32, 64, 64).family == 'f32'
    with pytest.raises(RuntimeError, match='bf16'):  # bf16 views and no bf16 kernel for the shape: the launch's error
        query(hip, 'bf16', 'bf16', 2, 32, 32, 64, 32)


@pytest.mark.parametrize('h,w,tw', [(16, 64, 16), (8, 64, 16),  # 16 first wherever 8 rows of 16 tile the map
                                    (4, 64, 64), (2, 128, 64),  # then 64 (2 rows), before 32 (4 rows)
                                    (4, 96, 32), (12, 96, 32), (6, 128, 64)])
def test_tile_width_preference(hip, h, w, tw):
    """The 128-pixel tiles try width 16, then 64, then 32 (kHalo16PrefTw, then the widest)."""
    assert query(hip, 'h2', 'f32', 2, h, w, 128, 128).tile_width == tw
    assert query(hip, 'bf16', 'bf16', 2, h, w, 128, 64).tile_width == tw


def test_tile_width_preference_c16(hip):
    """The input-layer kernel tries 16, 32, 64: on a 4 x 64 map it takes 32 where the 32-channel kernel takes 64."""
    assert query(hip, 'h2', 'f32', 2, 4, 64, 16, 64).tile_width == 32
    assert query(hip, 'h2', 'f32', 2, 8, 64, 16, 64).tile_width == 16
    assert query(hip, 'h2', 'f32', 2, 2, 64, 16, 64).tile_width == 64
    k = query(hip, 'x3', 'f32', 2, 8, 64, 16, 64)
    assert (k.family, k.np, k.block_pixels, k.block_channels) == ('halo16_c16', 3, 128, 64)


@pytest.mark.parametrize('math,store,np_', [('h2', 'f32', 4), ('bf16', 'bf16', 1)])
def test_256_pixel_tile_falls_back_to_128(hip, math, store, np_):
    hi, lo = (5, 4) if math == 'h2' else (8, 7)
    for h, w, layout, bm, tw in [(16, 16, hi, 256, 16), (8, 32, hi, 256, 32), (4, 64, hi, 256, 64),
                                 (8, 16, lo, 128, 16), (24, 48, lo, 128, 16), (2, 64, lo, 128, 64), (4, 32, lo, 128, 32)]:
        k = query(hip, math, store, 2, h, w, 64, 64)
        assert (k.layout, k.block_pixels, k.tile_width, k.np) == (layout, bm, tw, np_), (h, w, k)
    # neither tile: the map leaves the kernel (h2: x3 kernels; bf16 storage has none)
    assert query(hip, 'h2', 'f32', 2, 4, 16, 64, 64).family != 'halo16'


def test_double_buffer_lds_fit(hip):
    """Double buffering only where two halo buffers of every resident block fit 160 KB: blocks per SIMD x 2 buffers x
    planes x (rows + 2)(width + 2) halo rows x 64 B; never on 64-wide tiles of two or three planes."""
    # x3, three planes, double-buffered by default: 128 x 128 at 2 blocks, 10 x 18 rows = 138240 B fits
    assert query(hip, 'x3', 'f32', 2, 16, 32, 64, 128).db
    assert query(hip, 'x3', 'f32', 2, 12, 96, 64, 128).db           # 6 x 34 rows: 156672 B
    assert not query(hip, 'x3', 'f32', 2, 6, 128, 64, 128).db       # 64 wide
    assert not query(hip, 'x3', 'f32', 2, 16, 32, 64, 64).db        # 128 x 64 at 3 blocks: 207360 B
    # h2, two planes: single-buffered unless asked for, and then only where it fits
    assert not query(hip, 'h2', 'f32', 2, 16, 32, 128, 128).db
    on = hip.TUNE_HALO16_DB_ON
    assert query(hip, 'h2', 'f32', 2, 16, 32, 128, 128, tune=on).db       # 2 x 2 x 2 x 180 x 64 = 92160 B
    assert not query(hip, 'h2', 'f32', 2, 32, 32, 64, 64, tune=on).db     # 256 x 64: 18 x 18 rows, 165888 B > 163840
    assert not query(hip, 'h2', 'f32', 2, 24, 96, 64, 64, tune=on).db     # 256 x 64 at width 32: 10 x 34 rows, 174080 B
    assert query(hip, 'h2', 'f32', 2, 12, 96, 128, 64, tune=on).db        # 128 x 64 at width 32: 6 x 34 rows, 104448 B
    assert not query(hip, 'h2', 'f32', 2, 6, 128, 128, 128, tune=on).db   # 64 wide
    # bf16, one plane: always fits; the 1 x N tiles double-buffer from 128 channels per block
    assert query(hip, 'bf16', 'f32', 2, 6, 128, 64, 64).db
    assert query(hip, 'bf16', 'bf16', 2, 6, 128, 64, 128).db
    assert not query(hip, 'bf16', 'bf16', 2, 16, 32, 64, 64).db
    assert not query(hip, 'bf16', 'f32', 2, 16, 32, 64, 64, tune=hip.TUNE_HALO16_DB_OFF).db


def test_bf16_128x256_block_threshold(hip):
    """bf16 storage, n_out % 256 == 0: 128 x 256 blocks (row 9) from 512 of them, 128 x 128 (row 6) below."""
    k = query(hip, 'bf16', 'bf16', 2, 128, 128, 32, 512)   # 2 x 16384 / 128 x 2 = 512 blocks
    assert (k.layout, k.block_pixels, k.block_channels, k.db) == (9, 128, 256, True)
    k = query(hip, 'bf16', 'bf16', 2, 128, 112, 32, 512)  # 2 x 128 x 112 / 128 x 2 = 448
    assert (k.layout, k.block_channels) == (6, 128)
    assert query(hip, 'bf16', 'bf16', 1, 128, 128, 32, 512).layout == 6
    assert query(hip, 'bf16', 'bf16', 4, 128, 128, 32, 256).layout == 9    # 512 x 1
    assert query(hip, 'bf16', 'bf16', 4, 128, 128, 32, 384).layout == 6    # not a multiple of 256
    assert query(hip, 'bf16', 'bf16', 2, 128, 128, 32, 512, tune=hip.tune_halo16_cfg(3)).layout == 6  # forced: A/B


def test_weight_ring_refusals(hip):
    """The weight ring (A/B) runs on the h2 1 x N tiles only: not on 64-wide tiles, not on a ragged n_out, not when the
    halo is double-buffered, not under bf16."""
    ring = hip.TUNE_HALO16_WRING
    assert query(hip, 'h2', 'f32', 2, 16, 32, 128, 128, tune=ring).wl
    assert query(hip, 'h2', 'f32', 2, 12, 96, 128, 64, tune=ring).wl
    assert query(hip, 'h2', 'f32', 2, 32, 32, 64, 64, tune=ring).wl
    assert not query(hip, 'h2', 'f32', 2, 6, 128, 128, 128, tune=ring).wl     # 64 wide
    assert not query(hip, 'h2', 'f32', 2, 16, 32, 128, 136, tune=ring).wl     # 136 % 128
    assert not query(hip, 'h2', 'f32', 2, 16, 32, 128, 96, tune=ring).wl      # 96 % 64
    assert not query(hip, 'h2', 'f32', 2, 16, 32, 128, 128, tune=ring | hip.TUNE_HALO16_DB_ON).wl
    assert not query(hip, 'bf16', 'bf16', 2, 16, 32, 128, 128, tune=ring).wl
    assert not query(hip, 'h2', 'f32', 2, 16, 32, 128, 128).wl


def test_query_reports_the_launch_errors(hip):
    """A form the launch would refuse is refused by the query with the same message, and nothing is launched."""
    with pytest.raises(RuntimeError, match='input transform'):
        query(hip, 'f32', 'f32', 2, 16, 32, 64, 64, in_bn=True)
    with pytest.raises(RuntimeError, match='scd_igemm_bn_bwd_tiles'):
        query(hip, 'h2', 'f32', 2, 16, 32, 16, 64, form='bn_bwd')  # the input-layer kernel has no such epilogue
