"""The instance matrix of the 16x16x32 halo conv kernels (igemm_halo16_x3, igemm_halo16_c16): the cases
tests/test_conv_instance_matrix_gpu.py runs against fp64 and tests/test_conv_instances.py walks through the host query
(scd_igemm_kernel) on a machine without a GPU.  Test infrastructure.

Every case names the instance it is there to check.  The expected instances are written down here from the dispatcher's
comments in csrc/conv_halo16.hip (the tile-configuration list above kLayout, halo16_pick, halo16_instance), by hand, not
read back from the query:

  arithmetic / storage     n_out >= 128            64 <= n_out < 128
  h2 (fp32 storage)        row 3, 128 px x 128 ch  row 4, 128 x 64; 64-channel sources row 5, 256 x 64
  bf16, fp32 storage       row 0, 128 x 128        row 1, 128 x 64            (2 x 2 waves)
  bf16, bf16 storage       row 6, 128 x 128        row 7, 128 x 64; 64-channel sources row 8, 256 x 64
                           row 9, 128 x 256 when n_out % 256 == 0 and the grid has >= 512 such blocks

  double buffering: h2 single-buffered; bf16 on the 2 x 2 tiles double-buffered; bf16 1 x N tiles double-buffered on
  the tiles of >= 128 channels, single-buffered on the 64-channel ones.
  tile width: 16 first, then 64, 32; a 256-pixel tile that does not divide the map falls back to row 4 / 7.
  16-channel sources: igemm_halo16_c16, 128 px x 64 ch, widths tried 16, 32, 64.

Maps (n = 2 images, at least two tiles per image in each direction):
  128-pixel tiles: 16 x 32 -> width 16 (8 rows), 12 x 96 -> 32 (4 rows), 6 x 128 -> 64 (2 rows)
  256-pixel tiles: 32 x 32 -> width 16 (16 rows), 24 x 96 -> 32 (8 rows), 12 x 128 -> 64 (4 rows)
"""
from __future__ import annotations

import ctypes
from collections import namedtuple

from multimodal_siamese_cd_amd import hip

# direction: 'fwd' (mode-0 weight pack) or 'dgrad' (mode-1 pack); c = source channels of the launch, n_out its outputs
Case = namedtuple('Case', 'name math store direction n h w c n_out form inst')

MAPS = {(128, 16): (16, 32), (128, 32): (12, 96), (128, 64): (6, 128),
        (256, 16): (32, 32), (256, 32): (24, 96), (256, 64): (12, 128)}

# What each form sets in the descriptor (the coverage test keys a production launch by the same set).  'stat' and
# 'in_bn' carry the bias as the training forward does; under h2 the BatchNorm-backward data grad runs with and without
# the bound of its output, as the engine's do.
FORM_FIELDS = {
    'plain': (), 'bias': ('bias',), 'stat': ('bias', 'stat_rec'), 'in_bn': ('bias', 'stat_rec'),
    'bn_bwd': ('bn_bwd',), 'bn_bwd_bound': ('bn_bwd', 'dst_bound'), 'dst_bound': ('dst_bound',),
    'dst_slice': (), 'src_slice': (),
}
# the direction each form runs in (the launches that carry it in a training step)
FORM_DIR = {'bias': 'fwd', 'stat': 'fwd', 'in_bn': 'fwd', 'bn_bwd': 'dgrad', 'bn_bwd_bound': 'dgrad',
            'dst_bound': 'dgrad', 'dst_slice': 'dgrad', 'src_slice': 'fwd'}

# tag, arithmetic, storage, kLayout row, block pixels, block channels, double-buffered, source channels, outputs
_HALO16 = [
    ('h2_r3', 'h2', 'f32', 3, 128, 128, False, [32, 64, 96, 128], [128, 136]),
    ('h2_r4', 'h2', 'f32', 4, 128, 64, False, [32, 96, 128], [64, 96]),
    ('h2_r5', 'h2', 'f32', 5, 256, 64, False, [64], [64, 96]),
    ('bf16_r0', 'bf16', 'f32', 0, 128, 128, True, [32, 64, 96, 128], [128, 136]),
    ('bf16_r1', 'bf16', 'f32', 1, 128, 64, True, [64, 32, 128, 96], [64, 96]),
    ('sb_r6', 'bf16', 'bf16', 6, 128, 128, True, [32, 64, 96, 128], [128, 136]),
    ('sb_r7', 'bf16', 'bf16', 7, 128, 64, False, [32, 96, 128], [64, 96]),
    ('sb_r8', 'bf16', 'bf16', 8, 256, 64, False, [64], [64, 96]),
]
_C16 = [('c16_h2', 'h2', 'f32'), ('c16_bf16', 'bf16', 'f32'), ('c16_sb', 'bf16', 'bf16')]


def _inst(family, layout, bm, bn, tw, math, store, db, in_bn=False):
    return hip.IgemmKernel(family, layout, bm, bn, tw, 4 if math == 'h2' else 1, db, store == 'bf16', in_bn, False)


def _cases():
    out = []
    for tag, math, store, row, bm, bn, db, cs, nos in _HALO16:
        forms = ['bias', 'stat', 'in_bn', 'bn_bwd', 'dst_bound', 'dst_slice', 'src_slice']
        if math == 'h2':  # the engine's h2 data grads also raise their output's bound where a consumer needs one
            forms.append('bn_bwd_bound')
        for i, tw in enumerate((16, 32, 64)):  # one plain case per tile width, both directions, every chunk count
            h, w = MAPS[bm, tw]
            out.append(Case(f'{tag}-w{tw}-plain', math, store, ('fwd', 'dgrad', 'fwd')[i], 2, h, w, cs[i % len(cs)],
                            nos[i % 2], 'plain', _inst('halo16', row, bm, bn, tw, math, store, db)))
        for i, form in enumerate(forms):  # every form at a width other than 16
            tw = 32 if i % 2 == 0 else 64
            h, w = MAPS[bm, tw]
            out.append(Case(f'{tag}-w{tw}-{form}', math, store, FORM_DIR[form], 2, h, w, cs[(i + 1) % len(cs)],
                            nos[(i + 1) % 2], form,
                            _inst('halo16', row, bm, bn, tw, math, store, db, form == 'in_bn')))
    # the 256 -> 128 pixel fallback: 64-channel sources on a map 256 pixels do not tile (24 x 48: 24 % 16, 48 % 32,
    # 48 % 64 all non-zero) run rows 4 / 7 at width 16, 3 x 3 tiles per image
    out.append(Case('h2_r5to4-w16-plain', 'h2', 'f32', 'dgrad', 2, 24, 48, 64, 64, 'plain',
                    _inst('halo16', 4, 128, 64, 16, 'h2', 'f32', False)))
    out.append(Case('h2_r5to4-w16-stat', 'h2', 'f32', 'fwd', 2, 24, 48, 64, 96, 'stat',
                    _inst('halo16', 4, 128, 64, 16, 'h2', 'f32', False)))
    out.append(Case('sb_r8to7-w16-plain', 'bf16', 'bf16', 'fwd', 2, 24, 48, 64, 64, 'plain',
                    _inst('halo16', 7, 128, 64, 16, 'bf16', 'bf16', False)))
    # row 9 needs 512 blocks of 128 px x 256 ch: 2 x 128 x 128 pixels / 128 x (512 / 256) is the smallest such map, the
    # one large shape of the matrix (0.4 s of fp64 reference); in the four forms a training step runs it in
    for form in ('stat', 'in_bn', 'bn_bwd', 'plain'):
        out.append(Case(f'sb_r9-w16-{form}', 'bf16', 'bf16', FORM_DIR.get(form, 'dgrad'), 2, 128, 128, 32, 512, form,
                        _inst('halo16', 9, 128, 256, 16, 'bf16', 'bf16', True, form == 'in_bn')))
    for tag, math, store in _C16:
        nos = [64, 136, 96]
        for i, tw in enumerate((16, 32, 64)):
            h, w = MAPS[128, tw]
            out.append(Case(f'{tag}-w{tw}-plain', math, store, 'fwd', 2, h, w, 16, nos[i], 'plain',
                            _inst('halo16_c16', -1, 128, 64, tw, math, store, False)))
        for i, form in enumerate(['bias', 'stat', 'dst_bound', 'dst_slice', 'src_slice']):
            tw = 32 if i % 2 == 0 else 64
            h, w = MAPS[128, tw]
            out.append(Case(f'{tag}-w{tw}-{form}', math, store, 'fwd', 2, h, w, 16, nos[(i + 1) % 3], form,
                            _inst('halo16_c16', -1, 128, 64, tw, math, store, False)))
    return out


CASES = _cases()
IDS = [c.name for c in CASES]

SRC_SLICE_OFF, SRC_SLICE_EXTRA = 8, 16   # source at channel 8 of a buffer c + 16 wide
DST_SLICE_OFF, DST_SLICE_EXTRA = 32, 40  # destination at channel 32 of a buffer 32 + n_out + 8 wide


def instance_key(k, fields) -> tuple:
    """What the coverage test compares: the instance less its tile width and block size, and the forms set."""
    return (k.family, k.layout, k.np, k.db, k.sb, k.in_bn, k.wl, tuple(sorted(fields)))


def case_key(c: Case) -> tuple:
    return instance_key(c.inst, FORM_FIELDS[c.form])


# ------------------------------------------------------------------------------------------------
# Descriptors without a device: fake, suitably aligned, non-null pointers (the query reads their alignment only)
# ------------------------------------------------------------------------------------------------
FAKE = 0x7F0000100000  # 1 MiB aligned


def fake_desc(math: str, store: str, n: int, h: int, w: int, c: int, n_out: int, form: str = 'plain', tune: int = 0,
              bound: bool | None = None, in_bn: bool = False, keep: list | None = None) -> 'hip.IGEMM':
    """An scd_igemm_t of a 3x3 stride-1 conv as the GPU matrix builds it for `form`, on fake pointers."""
    dt, eb = (hip.DT_BF16, 2) if store == 'bf16' else (hip.DT_F32, 4)
    s_off, s_ldc = (SRC_SLICE_OFF, c + SRC_SLICE_EXTRA) if form == 'src_slice' else (0, c)
    d_off, d_ldc = (DST_SLICE_OFF, n_out + DST_SLICE_EXTRA) if form == 'dst_slice' else (0, n_out)
    src = hip.NHWC(FAKE + eb * s_off, n, h, w, c, s_ldc, dt)
    dst = hip.NHWC(2 * FAKE + eb * d_off, n, h, w, n_out, d_ldc, dt)
    nt, dy, dx = hip._taps(hip.TAPS_3X3)
    f = FORM_FIELDS[form]
    p = lambda i, on=True: (3 + i) * FAKE if on else None
    bb = None
    if 'bn_bwd' in f:
        bb = ctypes.pointer(hip.BNBWD(hip.NHWC(p(10), n, h, w, n_out, n_out, dt), 2, p(11), p(12), p(13), p(14), p(15)))
        if keep is not None:
            keep.append(bb)
    in_bn = in_bn or form == 'in_bn'
    bound = math == 'h2' if bound is None else bound
    return hip.IGEMM(src, h, w, 1, nt, dy, dx, p(0), n_out, p(1, 'bias' in f), dst, 0, p(2), p(3, 'stat_rec' in f),
                     p(4, in_bn), p(5, in_bn), 2 if in_bn else 0, bb, p(6, bound), p(7, 'dst_bound' in f),
                     hip._MATH_NAMES[math], tune, None)
