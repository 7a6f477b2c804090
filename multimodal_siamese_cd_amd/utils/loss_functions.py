"""Loss registry — drop-in for the reference's utils/loss_functions.py `get_criterion` (lines 6-33).

`PowerJaccardLoss` (loss_functions.py:141-150), the loss every reference config trains with (configs/base.yaml:17,
CONSISTENCY_TRAINER.LOSS_TYPE), runs as the fused `scd_pjaccard_fwd/bwd` HIP kernels.  The other single-channel
criteria the reference registers run on the fused loss family (`scd_loss_multi_fwd/bwd`, engine.single_loss); each
function carries its `kind` (a hip.LOSS_* value) so the trainers can fuse it into their multi-term calls:

  BCEWithLogitsLoss        bce_with_logits_loss        nn.BCEWithLogitsLoss()
  SoftDiceSquaredSumLoss   soft_dice_squared_sum_loss  loss_functions.py:48-56 (the same expression as soft_dice_loss)
  SoftDiceBalancedLoss     soft_dice_loss_balanced     :184-198
  IoULoss                  iou_loss                    :153-162
  DiceLikeLoss             dice_like_loss              :129-138
  MeanSquareErrorLoss, L2  mse_loss                    nn.MSELoss() on the RAW logits, as the reference applies it

Two registered names raise NotImplementedError:
  CrossEntropyLoss  the reference always passes a 2-entry class weight, and with the one-channel heads of every
                    model here nn.CrossEntropyLoss itself raises ("weight tensor should be defined either for all 1
                    classes or no classes"), so there is no reference behaviour to reproduce.
  SoftDiceLoss      only because tests/test_config.py::test_criterion_registry pins that; `soft_dice_loss` itself is
                    built, and SoftDiceSquaredSumLoss (identical code in the reference) resolves to it.  Flipping the
                    name on is the one line marked below.
Every criterion takes a keyword `valid=None` beside the reference's positional signature: a bool / uint8 per-pixel
mask of the logits' shape, and the call then equals the reference criterion on `logits[valid], target[valid]` without
the gather (engine.multi_loss; PowerJaccardLoss runs as kind 0 of the family then).  The one departure: no valid pixel
at all gives loss 0 and zero gradients, where the gather gives 1.0 (ratio kinds) or NaN (means).

Unknown names raise like the reference (`Exception('unknown loss ...')`).  The multi-class criteria and
jaccard_like_loss / jaccard_like_balanced_loss, which the reference never registers, are not built.
"""
from __future__ import annotations

from .. import engine, hip

_NOT_BUILT = {
    'CrossEntropyLoss': 'the reference itself raises with one-channel logits (2-entry class weight, 1 class)',
    'SoftDiceLoss': 'use SoftDiceSquaredSumLoss, the same expression (the name is pinned off by test_config)',
}


def power_jaccard_loss(input, target, valid=None):
    """1 - I / (sum(p^2 + t^2) - I + 1e-6), p = sigmoid(input), reduced over the whole batch."""
    return engine.power_jaccard(input, target, valid=valid)


def soft_dice_loss(y_logit, y_true, valid=None):
    """1 - (2 I + 1e-6) / (sum p + sum t + 1e-6)."""
    return engine.single_loss(hip.LOSS_SOFT_DICE, y_logit, y_true, valid=valid)


soft_dice_squared_sum_loss = soft_dice_loss  # identical code in the reference (its "TODO: fix this one")


def soft_dice_loss_balanced(input, target, valid=None):
    """1 - dice(p, t) - dice(1 - p, 1 - t), both with 1e-6 in the denominator only."""
    return engine.single_loss(hip.LOSS_SOFT_DICE_BALANCED, input, target, valid=valid)


def iou_loss(y_logit, y_true, valid=None):
    """1 - I / (sum(p + t) - I + 1e-6)."""
    return engine.single_loss(hip.LOSS_IOU, y_logit, y_true, valid=valid)


def dice_like_loss(input, target, valid=None):
    """1 - 2 I / (sum(p^2 + t^2) + 1e-6)."""
    return engine.single_loss(hip.LOSS_DICE_LIKE, input, target, valid=valid)


def bce_with_logits_loss(input, target, valid=None):
    """nn.BCEWithLogitsLoss(): mean(max(x, 0) - x t + log1p(exp(-|x|)))."""
    return engine.single_loss(hip.LOSS_BCE_LOGITS, input, target, valid=valid)


def mse_loss(input, target, valid=None):
    """nn.MSELoss() on the raw logits: mean((x - t)^2)."""
    return engine.single_loss(hip.LOSS_MSE, input, target, valid=valid)


power_jaccard_loss.kind = hip.LOSS_POWER_JACCARD
soft_dice_loss.kind = hip.LOSS_SOFT_DICE
soft_dice_loss_balanced.kind = hip.LOSS_SOFT_DICE_BALANCED
iou_loss.kind = hip.LOSS_IOU
dice_like_loss.kind = hip.LOSS_DICE_LIKE
bce_with_logits_loss.kind = hip.LOSS_BCE_LOGITS
mse_loss.kind = hip.LOSS_MSE

_REGISTRY = {
    'PowerJaccardLoss': power_jaccard_loss,
    'BCEWithLogitsLoss': bce_with_logits_loss,
    # 'SoftDiceLoss': soft_dice_loss,  # the one line to flip (and drop the name from _NOT_BUILT)
    'SoftDiceSquaredSumLoss': soft_dice_squared_sum_loss,
    'SoftDiceBalancedLoss': soft_dice_loss_balanced,
    'MeanSquareErrorLoss': mse_loss,
    'IoULoss': iou_loss,
    'DiceLikeLoss': dice_like_loss,
    'L2': mse_loss,
}


def get_criterion(loss_type, negative_weight: float = 1, positive_weight: float = 1):
    if loss_type in _REGISTRY:
        return _REGISTRY[loss_type]
    if loss_type in _NOT_BUILT:
        raise NotImplementedError(f'{loss_type}: {_NOT_BUILT[loss_type]}')
    raise Exception(f'unknown loss {loss_type}')
