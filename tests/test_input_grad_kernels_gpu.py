"""scd_input_grad on MI355X against torch.nn.grad.conv2d_input in fp64 on the CPU: max-relative < 1e-5, the project's
fp32-class kernel bar (tests/test_h2_gpu.py), for both storage types (the bf16 reference gets the same bf16-rounded
dy: the kernel widens it exactly and rounds nothing else).  The impulse test pins the tap flip, the o / j transpose and
the border bit for bit; the record tests pin which slices are written and that nothing else is."""
import pytest
import torch

pytestmark = pytest.mark.gpu

TOL = 1e-5
SENTINEL = -777.25


@pytest.fixture(scope='module')
def dev():
    from multimodal_siamese_cd_amd import hip
    hip.load_library()
    d = torch.device('cuda:0')
    hip.ensure_device(torch.empty(1, device=d))
    return d


def rel(a, b):
    a = a.detach().double().cpu()
    b = b.detach().double().cpu()
    return ((a - b).abs().max() / b.abs().max().clamp_min(1e-30)).item()


def _operands(n, c0, cin, h, w, seed, storage=torch.float32):
    """(dy NHWC in `storage` on the CPU, weight OIHW fp32, fp64 reference gx NCHW of that stored dy)."""
    g = torch.Generator().manual_seed(seed)
    dy = torch.randn(n, h, w, c0, generator=g).to(storage)
    wt = torch.randn(c0, cin, 3, 3, generator=g) / (3 * c0 ** 0.5)
    ref = torch.nn.grad.conv2d_input((n, cin, h, w), wt.double(), dy.double().permute(0, 3, 1, 2), padding=1)
    return dy, wt, ref


def _run(dev, dy, wt, records):
    from multimodal_siamese_cd_amd import hip
    dyd = dy.to(dev)
    hip.input_grad(hip.nhwc(dyd), wt.to(dev), records)
    torch.cuda.synchronize()


# C0 x cin x map: every C0 and cin of the issue's lists at least twice, every map at least twice; (37, 45) and (33, 16)
# leave partial tiles both ways and span several 8 x 32 tiles, (1, 1) and (2, 70) are thinner than the halo, C0 = 8,
# 16 are single partial chunks and 64, 128 run 2 and 4 chunks of 32 channels
CASES = [(8, 1, (16, 16)), (8, 5, (1, 1)), (16, 3, (37, 45)), (16, 16, (2, 70)), (32, 5, (33, 16)), (32, 10, (16, 16)),
         (64, 5, (37, 45)), (64, 16, (33, 16)), (64, 1, (2, 70)), (128, 10, (37, 45)), (128, 3, (1, 1)),
         (128, 16, (16, 16)), (72, 5, (33, 16))]


@pytest.mark.parametrize('storage', [torch.float32, torch.bfloat16], ids=['fp32', 'bf16'])
@pytest.mark.parametrize('c0,cin,hw', CASES)
def test_input_grad_matches_fp64(dev, c0, cin, hw, storage):
    n = 3
    dy, wt, ref = _operands(n, c0, cin, *hw, seed=c0 * 100 + cin, storage=storage)
    gx = torch.full((n, cin, *hw), SENTINEL, device=dev)
    _run(dev, dy, wt, [(gx, 0, cin, 0, 0, n)])
    e = rel(gx, ref)
    print(f'C0 {c0} cin {cin} map {hw} {storage}: max-relative {e:.2e}')
    assert e < TOL


@pytest.mark.parametrize('storage', [torch.float32, torch.bfloat16], ids=['fp32', 'bf16'])
def test_impulse_reproduces_the_weights_exactly(dev, storage):
    """dy one-hot at (y, x, o): by the formula the only outputs that read it are (y-1+ky, x-1+kx), so
    gx[:, y-1+ky, x-1+kx] == w[o, :, ky, kx] where that pixel exists, and 0 elsewhere (what conv2d_input gives too)."""
    c0, cin, h, w = 40, 5, 11, 37
    g = torch.Generator().manual_seed(3)
    wt = torch.randn(c0, cin, 3, 3, generator=g)
    spots = [(0, 0, 0), (0, w - 1, 7), (h - 1, 0, 33), (h - 1, w - 1, 39), (8, 32, 18)]  # 4 corners, 1 tile seam
    dy = torch.zeros(len(spots), h, w, c0)
    expect = torch.zeros(len(spots), cin, h, w)
    for i, (y, x, o) in enumerate(spots):
        dy[i, y, x, o] = 1.0
        for ky in range(3):
            for kx in range(3):
                yy, xx = y - 1 + ky, x - 1 + kx
                if 0 <= yy < h and 0 <= xx < w:
                    expect[i, :, yy, xx] = wt[o, :, ky, kx]
    gx = torch.full((len(spots), cin, h, w), SENTINEL, device=dev)
    _run(dev, dy.to(storage), wt, [(gx, 0, cin, 0, 0, len(spots))])
    assert torch.equal(gx.cpu(), expect)
    ref = torch.nn.grad.conv2d_input(expect.shape, wt.double(), dy.double().permute(0, 3, 1, 2), padding=1)
    assert torch.equal(expect.double(), ref)  # the expectation itself, against the reference


def test_pair_records_split_image_ranges(dev):
    """pack_pair: images [0, B) to one tensor, [B, 2B) to another, all bands."""
    b, c0, cin, hw = 2, 16, 5, (9, 35)
    dy, wt, ref = _operands(2 * b, c0, cin, *hw, seed=11)
    g1 = torch.full((b, cin, *hw), SENTINEL, device=dev)
    g2 = torch.full((b, cin, *hw), SENTINEL, device=dev)
    _run(dev, dy, wt, [(g1, 0, cin, 0, 0, b), (g2, 0, cin, 0, b, b)])
    assert rel(g1, ref[:b]) < TOL and rel(g2, ref[b:]) < TOL


def test_stream_records_write_only_their_channel_slices(dev):
    """pack_stream into 5-channel tensors: conv channels [0, 3) to x_t1.grad[:, 2:5], [3, 6) to x_t2.grad[:, 2:5];
    channels 0 and 1 of both keep the sentinel."""
    b, c0, cin, hw = 2, 24, 6, (10, 33)
    dy, wt, ref = _operands(b, c0, cin, *hw, seed=12)
    g1 = torch.full((b, 5, *hw), SENTINEL, device=dev)
    g2 = torch.full((b, 5, *hw), SENTINEL, device=dev)
    _run(dev, dy, wt, [(g1, 2, 3, 0, 0, b), (g2, 2, 3, 3, 0, b)])
    assert rel(g1[:, 2:], ref[:, :3]) < TOL and rel(g2[:, 2:], ref[:, 3:]) < TOL
    assert bool((g1[:, :2] == SENTINEL).all()) and bool((g2[:, :2] == SENTINEL).all())


def test_null_record_and_untouched_surroundings(dev):
    """One NULL record (only x_t2 requires grad); the destination is a slice of a larger sentinel-filled buffer and
    every element outside the given images and channels still holds the sentinel."""
    b, c0, cin, hw = 2, 8, 3, (5, 40)
    dy, wt, ref = _operands(2 * b, c0, cin, *hw, seed=13)
    buf = torch.full((b + 2, 4, *hw), SENTINEL, device=dev)
    g2 = buf[1:1 + b]  # contiguous images 1, 2 of 4
    _run(dev, dy, wt, [(None, 0, 0, 0, 0, 0), (g2, 1, 3, 0, b, b)])
    assert rel(g2[:, 1:], ref[b:]) < TOL
    assert bool((buf[0] == SENTINEL).all()) and bool((buf[-1] == SENTINEL).all())
    assert bool((g2[:, 0] == SENTINEL).all())


def test_dy_channel_slice_view(dev):
    """dy as a channel slice (ldc > c) of a wider NHWC buffer."""
    from multimodal_siamese_cd_amd import hip
    n, c0, cin, hw = 2, 16, 5, (7, 20)
    dy, wt, ref = _operands(n, c0, cin, *hw, seed=14)
    wide = torch.randn(n, *hw, c0 + 8, device=dev)
    wide[..., 8:] = dy.to(dev)
    gx = torch.empty((n, cin, *hw), device=dev)
    hip.input_grad(hip.nhwc(wide, 8, c0), wt.to(dev), [(gx, 0, cin, 0, 0, n)])
    assert rel(gx, ref) < TOL


def test_offsets_past_2_31_elements(dev):
    """A dy of more than 2^31 elements (bf16, 4 GiB): the last image's rows are right, so no offset wrapped.  The
    reference is formed for the bottom rows only (their dy rows and one more above)."""
    n, c0, cin, h, w = 2, 8, 2, 11600, 11600
    assert n * h * w * c0 > 2 ** 31 and h * w * c0 < 2 ** 31
    g = torch.Generator(device=dev).manual_seed(15)
    dy = torch.empty(n, h, w, c0, device=dev, dtype=torch.bfloat16)
    for i in range(n):  # filled by image: no fp32 temporary of the whole view
        dy[i] = torch.randn(h, w, c0, device=dev, generator=g).to(torch.bfloat16)
    wt = torch.randn(c0, cin, 3, 3, generator=torch.Generator().manual_seed(16)) / 8
    gx = torch.empty(n, cin, h, w, device=dev)
    from multimodal_siamese_cd_amd import hip
    hip.input_grad(hip.nhwc(dy), wt.to(dev), [(gx, 0, cin, 0, 0, n)])
    rows = 6
    tail = dy[1, h - rows - 1:].double().cpu().permute(2, 0, 1)[None]  # rows + 1 dy rows; the bottom border is real
    ref = torch.nn.grad.conv2d_input((1, cin, rows + 1, w), wt.double(), tail, padding=1)[:, :, 1:]
    assert rel(gx[1:, :, h - rows:], ref) < TOL
    top = dy[0, :rows + 1].double().cpu().permute(2, 0, 1)[None]
    ref0 = torch.nn.grad.conv2d_input((1, cin, rows + 1, w), wt.double(), top, padding=1)[:, :, :rows]
    assert rel(gx[:1, :, :rows], ref0) < TOL
