"""Frozen BatchNorm on a topology off the channel granule: the zero-padded twin (utils/networks.py) follows each
BatchNorm's own flag, and a frozen BatchNorm's statistics come back from the twin as they went in."""
import pytest
import torch

from test_frozen_bn_gpu import GRAD_TOL, _buffers, _frozen_step, _step_loss, compare_gradients, dev  # noqa: F401
from _parity import branch_matched_reference
from oracle.golden import Fixture

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize('prefixes', [None, ['inc.', 'encoder.']])
def test_frozen_step_on_the_padded_twin(dev, prefixes):  # noqa: F811
    """siamese_t12-20 (TOPOLOGY [12, 20] runs at [16, 24]) with the statistics r1/*: all BatchNorms frozen against the
    branch-matched fp64 oracle in eval mode (logits through the loss at 1e-5, every gradient at GRAD_TOL), buffers
    bit-unchanged; with only the encoder frozen, its buffers bit-unchanged and the decoder's updated once."""
    fx = Fixture('siamese_t12-20')
    net, out, loss, got, trace, before = _frozen_step(fx, dev, prefixes)
    assert net.module._twin is not None
    after = _buffers(net)
    if prefixes is None:
        P = {k: torch.from_numpy(v.copy()) for k, v in fx.params0.items()}
        B = {k: torch.from_numpy(v.copy()) for k, v in fx.prefixed('r1/').items()}
        _, lref, ref = branch_matched_reference(fx.model_type, P, fx.batch(), fx.cfg, trace, net.module,
                                                _step_loss(fx.model_type, fx.meta['alpha']), training=False, buffers=B)
        assert abs(loss.item() - lref.item()) < 1e-5
        assert set(ref) == set(got)
        assert not compare_gradients(got, ref, GRAD_TOL)
    for k, v in after.items():
        if prefixes is None or k.startswith(tuple(prefixes)):
            assert torch.equal(v, before[k]), k
        elif k.endswith('num_batches_tracked'):
            assert int(v) == int(before[k]) + 1, k
        else:
            assert not torch.equal(v, before[k]), k
