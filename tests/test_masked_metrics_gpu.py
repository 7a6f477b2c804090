"""Valid-pixel masks in the metrics on MI355X: scd_threshold_counts_masked against torch boolean arithmetic on the
CPU, MultiThresholdMetric.add_sample / add_logits with valid=, and model_evaluation on items with a `valid` key."""
import numpy as np
import pytest
import torch

from multimodal_siamese_cd_amd import hip

pytestmark = pytest.mark.gpu

THR = [0.3, 0.5, 0.7]


@pytest.fixture(scope='module')
def dev():
    hip.load_library()
    return torch.device('cuda:0')


def _inputs(shape, from_logits, seed):
    """Predictions (probabilities, or logits whose probabilities keep clear of the thresholds, so the device's and the
    CPU's sigmoid cannot decide a pixel differently), labels with about 30 % ones, a mask of about 70 % ones, and NaN
    in predictions and labels at the invalid pixels."""
    g = torch.Generator().manual_seed(seed)
    if from_logits:
        pred = torch.randn(shape, generator=g) * 2
        for t in THR:
            near = (torch.sigmoid(pred) - t).abs() < 1e-3
            pred[near] += 0.1
            assert not ((torch.sigmoid(pred) - t).abs() < 1e-4).any()
    else:
        pred = torch.rand(shape, generator=g)
        pred.view(-1)[:3] = torch.tensor(THR)  # exactly on a threshold: the rounding rule decides
    truth = (torch.rand(shape, generator=g) < 0.3).float()
    valid = torch.rand(shape, generator=g) < 0.7
    valid.view(-1)[:3] = True
    pred[~valid] = float('nan')
    truth[~valid] = float('nan')
    return pred, truth, valid


def _expected(pred, truth, valid, from_logits):
    """{#label, per threshold: #(label & positive), #positive} over valid pixels, then #valid (metrics.py:22-31)."""
    p = torch.sigmoid(pred) if from_logits else pred
    label = truth.bool() & valid
    out = [int(label.sum())]
    for t in THR:
        pos = torch.round(p - torch.tensor(t) + 0.5).bool() & valid
        out += [int((label & pos).sum()), int(pos.sum())]
    return out + [int(valid.sum())]


def _masked_counts(pred, truth, valid_u8, from_logits, dev):
    thr = torch.tensor(THR, device=dev)
    counts = torch.full((2 + 2 * len(THR),), -1, dtype=torch.int64, device=dev)
    ws = torch.empty(hip.threshold_counts_masked_workspace_bytes(pred.numel(), len(THR)), dtype=torch.uint8,
                     device=dev)
    hip.threshold_counts_masked(pred, truth, valid_u8, thr, from_logits, counts, ws)
    return counts.tolist()


@pytest.mark.parametrize('from_logits', [False, True])
@pytest.mark.parametrize('shape', [(1, 1, 11, 13), (2, 1, 37, 53)])
def test_masked_counts_against_boolean_arithmetic(dev, shape, from_logits):
    pred, truth, valid = _inputs(shape, from_logits, seed=sum(shape))
    want = _expected(pred, truth, valid, from_logits)
    assert 0 < want[-1] < pred.numel() and want[0] > 0
    pd, td, vd = pred.to(dev), truth.to(dev), valid.to(dev).view(torch.uint8)
    assert _masked_counts(pd, td, vd, from_logits, dev) == want
    # any non-zero byte counts, and a mask pointer off 4-byte alignment takes the byte loads
    buf = torch.zeros(vd.numel() + 9, dtype=torch.uint8, device=dev)
    off = buf[1:1 + vd.numel()].view(vd.shape)
    off.copy_(vd * 255)
    assert off.data_ptr() % 4 == 1
    assert _masked_counts(pd, td, off, from_logits, dev) == want
    # the metric class: TN from #valid on the device
    from multimodal_siamese_cd_amd.utils import metrics
    m = metrics.MultiThresholdMetric(THR)
    (m.add_logits if from_logits else m.add_sample)(td, pd, valid=valid)
    n_true, n_valid = want[0], want[-1]
    tp, n_pos = np.array(want[1:-1:2]), np.array(want[2:-1:2])
    assert m.TP.tolist() == tp.tolist() and m.FP.tolist() == (n_true - tp).tolist()
    assert m.FN.tolist() == (n_pos - tp).tolist() and m.TN.tolist() == (n_valid - n_true - n_pos + tp).tolist()
    assert m.TP.is_cuda and m.TN.dtype == torch.float32


@pytest.mark.parametrize('from_logits', [False, True])
def test_all_ones_mask_equals_the_unmasked_counts(dev, from_logits):
    pred, truth, _ = _inputs((2, 1, 37, 53), from_logits, seed=7)
    pred, truth = torch.nan_to_num(pred, 0.25).to(dev), torch.nan_to_num(truth, 1.0).to(dev)
    pred.view(-1)[5] = float('nan')  # NaN at a valid pixel counts as positive, as in the unmasked kernel
    thr = torch.tensor(THR, device=dev)
    plain = torch.empty(1 + 2 * len(THR), dtype=torch.int64, device=dev)
    ws = torch.empty(hip.threshold_counts_workspace_bytes(pred.numel(), len(THR)), dtype=torch.uint8, device=dev)
    hip.threshold_counts(pred, truth, thr, from_logits, plain, ws)
    ones = torch.ones(pred.shape, dtype=torch.uint8, device=dev)
    assert _masked_counts(pred, truth, ones, from_logits, dev) == plain.tolist() + [pred.numel()]


class _Items(torch.utils.data.Dataset):
    def __init__(self, with_valid):
        self.with_valid = with_valid

    def __len__(self):
        return 3

    def __getitem__(self, i):
        g = torch.Generator().manual_seed(40 + i)
        h, w = 20 + i, 24 + 3 * i
        item = {'x_t1': torch.randn((2, h, w), generator=g), 'x_t2': torch.randn((2, h, w), generator=g),
                'y_change': (torch.rand((1, h, w), generator=g) < 0.4).float()}
        if self.with_valid:
            item['valid'] = torch.rand((1, h, w), generator=g) < 0.6
        return item


class _DiffNet(torch.nn.Module):
    def forward(self, x_t1, x_t2):
        return (2 * (x_t2[:, :1] - x_t1[:, :1])).contiguous()


def test_model_evaluation_with_a_valid_key_equals_the_gathered_pixels(dev):
    from multimodal_siamese_cd_amd.utils import evaluation, metrics
    logs = []
    out = evaluation.model_evaluation(_DiffNet(), None, dev, 'validation', 1.0, 10, dataset=_Items(True),
                                      log=logs.append, thresholds=THR)
    ref = metrics.MultiThresholdMetric(THR)
    net = _DiffNet()
    for i in range(3):
        it = _Items(True)[i]
        logits = net(it['x_t1'][None].to(dev), it['x_t2'][None].to(dev))
        v = it['valid'][None].to(dev)
        ref.add_logits(it['y_change'][None].to(dev)[v].reshape(1, 1, 1, -1), logits[v].reshape(1, 1, 1, -1))
    f1 = ref.compute_f1()
    k = f1.argmax()
    assert out['validation F1'] == f1.max().item() > 0
    assert out['validation precision'] == ref.precision[k].item()
    assert out['validation recall'] == ref.recall[k].item()
    assert logs == [out]
    # and it differs from scoring every pixel: the key is not ignored
    every = evaluation.model_evaluation(_DiffNet(), None, dev, 'validation', 1.0, 10, dataset=_Items(False),
                                        log=logs.append, thresholds=THR)
    assert every['validation F1'] != out['validation F1']
