"""The six positional BatchNorm + ReLU backward exports are fillers of scd_bn_bwd_t: a malformed call is refused on the
host (no GPU touched) with the code and the scd_last_error() text that scd_bn_relu_backward_desc gives the equivalent
descriptor, and that text is the one the library gave before the entry points were folded onto the descriptor (the
literals of WANT were printed once from that library).  A reordered or dropped check changes a text here.

Two rows differ between the two calls by design, and WANT holds both texts for them: skip_mode 2 handed to
scd_bn_relu_backward_pooled, and a second skip gradient with skip_mode 1 handed to scd_bn_relu_backward_pooled2, are
refused by the positional export's own check / the pooled body, while the descriptor entry point refuses the
form / skip_mode pair itself."""
import ctypes

import pytest

# each export's positional arguments as scd_bn_bwd_t field names (the stream follows)
_HEAD = 'mean invstd gamma scale shift'
_TAIL = 'dgamma dbeta dbias_prev dy dy_bound ws ws_bytes'
EXPORTS = {
    'plain': ('scd_bn_relu_backward', f'y da nseg {_HEAD} {_TAIL}'),
    'tiles': ('scd_bn_relu_backward_tiles', f'y da nseg {_HEAD} tile_rec ntiles {_TAIL}'),
    'pooled': ('scd_bn_relu_backward_pooled', f'y gy idx gskip skip_mode nseg {_HEAD} {_TAIL}'),
    'pooled2': ('scd_bn_relu_backward_pooled2', f'y gy idx gskip skip_mode gskip2 nseg {_HEAD} {_TAIL}'),
    'head': ('scd_bn_relu_backward_head',
             f'y gout w_head n_out nseg {_HEAD} dgamma dbeta dbias_prev dy dy_bound w_grad ws ws_bytes'),
    'coef': ('scd_bn_relu_backward_coef',
             f'y da nseg {_HEAD} tile_rec ntiles coef dgamma dbeta dbias_prev da_bound dy_bound ws ws_bytes'),
}
FORMS = ('plain', 'tiles', 'pooled', 'pooled2', 'head', 'coef')  # enum scd_bn_bwd_form, in order
N, H, W, C, NSEG = 2, 4, 4, 8, 2

_POOLED_DESC = 'bn_relu_backward_desc: skip_mode 2 is the form SCD_BN_BWD_POOLED2, and only it'
WANT = {
    'plain-null_y': 'bn.y: null data',
    'plain-null_mean': 'bn_relu_backward: shape mismatch / null',
    'plain-ws_short': 'bn_relu_backward: workspace 575 < 576 bytes',
    'tiles-null_y': 'bn.y: null data',
    'tiles-null_mean': 'bn_relu_backward_tiles: shape mismatch / null',
    'tiles-ws_short': 'bn_relu_backward_tiles: workspace 575 < 576 bytes',
    'pooled-null_y': 'bn.y: null data',
    'pooled-null_mean': 'bn_relu_backward_pooled: shape mismatch / null',
    'pooled-ws_short': 'bn_relu_backward_pooled: workspace 575 < 576 bytes',
    'pooled2-null_y': 'bn.y: null data',
    'pooled2-null_mean': 'bn_relu_backward_pooled: shape mismatch / null',
    'pooled2-ws_short': 'bn_relu_backward_pooled: workspace 575 < 576 bytes',
    'head-null_y': 'bn.y: null data',
    'head-null_mean': 'bn_relu_backward_head: shape mismatch / null',
    'head-ws_short': 'bn_relu_backward_head: workspace 703 < 704 bytes',
    'coef-null_y': 'bn.y: null data',
    'coef-null_mean': 'bn_relu_backward_coef: shape mismatch / null',
    'coef-ws_short': 'bn_relu_backward_coef: workspace 575 < 576 bytes',
    'plain-da_shape': 'bn_relu_backward: shape mismatch / null',
    'tiles-dy_shape': 'bn_relu_backward_tiles: shape mismatch / null',
    'pooled-dy_shape': 'bn_relu_backward_pooled: shape mismatch / null',
    'pooled2-dy_shape': 'bn_relu_backward_pooled: shape mismatch / null',
    'head-dy_shape': 'bn_relu_backward_head: shape mismatch / null',
    'coef-da_shape': 'bn_relu_backward_coef: shape mismatch / null',
    'head-ws_short_no_wgrad': 'bn_relu_backward_head: workspace 575 < 576 bytes',
    'pooled-no_gradient': 'bn_relu_backward_pooled: neither gy nor gskip / 2^31 pixels or more',
    'pooled2-no_gradient': 'bn_relu_backward_pooled: neither gy nor gskip / 2^31 pixels or more',
    'pooled-skip_mode_2': ('bn_relu_backward_pooled: skip_mode 2 takes a second skip gradient '
                           '(scd_bn_relu_backward_pooled2)', _POOLED_DESC),
    'pooled2-gskip2_skip_mode_1': ('bn_relu_backward_pooled: skip_mode 2 needs gskip (n/2 images), gskip2 (n images) '
                                   'and nseg 2; gskip2 only with skip_mode 2', _POOLED_DESC),
    'head-n_out_5': 'bn_relu_backward_head: null gradient or weights / n_out not in [1,4] / 2^31 pixels or more',
    'tiles-ntiles_3': 'bn_relu_backward_tiles: null records / 3 tiles not divisible into 2 segments',
    'coef-ntiles_3': 'bn_relu_backward_coef: null coef / 3 tiles not divisible into 2 segments / dy_bound without '
                     'da_bound',
    'coef-dy_bound_alone': 'bn_relu_backward_coef: null coef / 0 tiles not divisible into 2 segments / dy_bound '
                           'without da_bound',
}


def _lib():
    from multimodal_siamese_cd_amd import build, hip
    build.build_lib()
    return hip, hip.load_library()


def _fields(hip, form):
    """A well-formed call of `form` as descriptor fields; every pointer is one aligned host address (the checks never
    dereference it).  Returns (fields, keep-alive)."""
    keep = ctypes.create_string_buffer(256)
    p = (ctypes.addressof(keep) + 63) & ~63

    def view(n=N, h=H, w=W):
        return hip.NHWC(p, n, h, w, C, C, hip.DT_F32)

    f = dict(y=view(), nseg=NSEG, mean=p, invstd=p, gamma=p, scale=p, shift=p, dgamma=p, dbeta=p, dbias_prev=p,
             dy=view(), dy_bound=None, ws=p, ws_bytes=hip.bn_workspace_bytes(N, H, W, C, NSEG))
    if form in ('plain', 'tiles', 'coef'):
        f['da'] = view()
    if form == 'tiles':
        f.update(tile_rec=p, ntiles=2)
    if form == 'coef':
        del f['dy']
        f.update(tile_rec=None, ntiles=0, coef=p, da_bound=None)
    if form in ('pooled', 'pooled2'):
        f.update(gy=view(h=H // 2, w=W // 2), idx=p, gskip=view(n=N // 2), skip_mode=1)
    if form == 'pooled2':
        f.update(skip_mode=2, gskip2=view())
    if form == 'head':
        f.update(gout=p, w_head=p, n_out=2, w_grad=p, ws_bytes=hip.bn_head_workspace_bytes(N, H, W, C, NSEG, 2))
    return f, keep


def _break(hip, form, how, f):
    null = hip.NHWC(None, 0, 0, 0, 0, 0, 0)
    if how == 'null_y':
        f['y'] = hip.NHWC(None, N, H, W, C, C, hip.DT_F32)
    elif how in ('da_shape', 'dy_shape'):
        f[how[:2]] = hip.NHWC(f['y'].data, N, H, W + 1, C, C, hip.DT_F32)
    elif how == 'null_mean':
        f['mean'] = None
    elif how == 'ws_short':
        f['ws_bytes'] -= 1
    elif how == 'ws_short_no_wgrad':
        f.update(w_grad=None, ws_bytes=hip.bn_workspace_bytes(N, H, W, C, NSEG) - 1)
    elif how == 'no_gradient':
        f.update(gy=null, gskip=null)
    elif how == 'skip_mode_2':
        f['skip_mode'] = 2
    elif how == 'gskip2_skip_mode_1':
        f['skip_mode'] = 1
    elif how == 'n_out_5':
        f['n_out'] = 5
    elif how == 'ntiles_3':
        f['ntiles'] = 3
    elif how == 'dy_bound_alone':
        f['dy_bound'] = f['coef']
    else:
        raise KeyError(how)


ROWS = [f'{f}-{how}' for f in FORMS for how in ('null_y', 'null_mean', 'ws_short')] + [
    'plain-da_shape', 'tiles-dy_shape', 'pooled-dy_shape', 'pooled2-dy_shape', 'head-dy_shape', 'coef-da_shape',
    'head-ws_short_no_wgrad', 'pooled-no_gradient', 'pooled2-no_gradient', 'pooled-skip_mode_2',
    'pooled2-gskip2_skip_mode_1', 'head-n_out_5', 'tiles-ntiles_3', 'coef-ntiles_3', 'coef-dy_bound_alone']


def both_calls(row):
    """((code, text) of the positional export, (code, text) of scd_bn_relu_backward_desc) for a row of the table."""
    hip, lib = _lib()
    form, how = row.split('-')
    f, keep = _fields(hip, form)
    if row == 'coef-ntiles_3':
        f['tile_rec'] = f['coef']
    _break(hip, form, how, f)
    symbol, order = EXPORTS[form]
    rc = getattr(lib, symbol)(*(f[k] for k in order.split()), None)
    positional = (rc, lib.scd_last_error().decode())
    d = hip.BNBWDDESC(form=FORMS.index(form), **f)
    rc = lib.scd_bn_relu_backward_desc(ctypes.byref(d), None)
    return positional, (rc, lib.scd_last_error().decode())


@pytest.mark.parametrize('row', ROWS)
def test_positional_export_and_descriptor_refuse_alike(row):
    positional, desc = both_calls(row)
    want = WANT[row]
    want_pos, want_desc = want if isinstance(want, tuple) else (want, want)
    assert positional[0] == desc[0] != 0
    assert positional[1] == want_pos
    assert desc[1] == want_desc


def test_table_covers_every_form():
    assert set(WANT) == set(ROWS) and {r.split('-')[0] for r in ROWS} == set(FORMS)
