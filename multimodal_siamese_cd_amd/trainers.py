"""Per-step loss recipes of the reference trainers, on the HIP path.

  supervised  train_supervised.py:63-79            loss = criterion(logits, y_change)
  dual task   train_supervised_dualtask.py:64-90   (L_change + (L_sem_t1 + L_sem_t2) / 2) / 2
  MMCR        train_semisupervised.py:66-121       alpha * mean(L_fusion, L_s1, L_s2) on labelled samples
                                                   + (1 - alpha) * L_cons(logits_s1, sigmoid(logits_s2)) on unlabelled
                                                   (the soft target is NOT detached, as in the reference; LOSS_TYPE
                                                   L2: MSE(sigmoid(logits_s1), sigmoid(logits_s2)), lines 101-102)

Criteria of utils/loss_functions.py carry the kind of their fused kernel, so every recipe is one fused multi-term call
(engine.multi_jaccard when every term is PowerJaccardLoss, engine.multi_loss otherwise); a foreign callable takes the
reference's boolean-mask composition.

A batch with a `valid` key (uint8 / bool (B, 1, H, W), non-zero = the pixel counts; DATALOADER.INCLUDE_MASKED) masks
every term of its recipe, the MMCR consistency term on unlabelled samples included: each term runs over the pixels
that are both in its sample subset and valid, with the semantics of `criterion(logits[v], y[v])` and no gather
(engine.multi_loss(..., valid=)).  A masked PowerJaccard recipe runs as kind 0 of the loss family, an unmasked one
keeps the dedicated kernels; a foreign callable takes the gather idiom.
"""
from __future__ import annotations

import torch

from . import engine
from .utils import loss_functions


def _fusable(*criteria) -> bool:
    """Every criterion is one of ours (utils/loss_functions.py): it carries the kind of its fused kernel."""
    return all(isinstance(getattr(c, 'kind', None), int) for c in criteria)


def _all_power_jaccard(*criteria) -> bool:
    return all(c is loss_functions.power_jaccard_loss for c in criteria)


def _gathered(criterion, valid, logits, target):
    """The gather idiom, for a foreign callable: the criterion on the valid elements (a host sync)."""
    if valid is None:
        return criterion(logits, target)
    v = valid.to(logits.device).bool()
    return criterion(logits[v], target[v])


def supervised_loss(criterion, logits, batch):
    valid = batch.get('valid')
    if valid is None:
        return criterion(logits, batch['y_change'])
    if _fusable(criterion):
        return criterion(logits, batch['y_change'], valid=valid)
    return _gathered(criterion, valid, logits, batch['y_change'])


def dualtask_loss(change_criterion, sem_criterion, outputs, batch):
    logits_change, logits_sem_t1, logits_sem_t2 = outputs
    valid = batch.get('valid')
    if _fusable(change_criterion, sem_criterion):  # one fused pass: 0.5 L_change + 0.25 L_sem_t1 + 0.25 L_sem_t2
        tensors = (logits_change, batch['y_change'], logits_sem_t1, batch['y_sem_t1'], logits_sem_t2,
                   batch['y_sem_t2'])
        if valid is None and _all_power_jaccard(change_criterion, sem_criterion):  # the shipped configs
            lab = torch.ones(logits_change.shape[0], dtype=torch.uint8, device=logits_change.device)
            spec = [(0, 1, 0.5, 0, 0), (2, 3, 0.25, 0, 0), (4, 5, 0.25, 0, 0)]
            return engine.multi_jaccard(spec, lab, *tensors)
        kc, ks = change_criterion.kind, sem_criterion.kind
        spec = [(0, 1, 0.5, 0, 0, kc, 0), (2, 3, 0.25, 0, 0, ks, 0), (4, 5, 0.25, 0, 0, ks, 0)]
        return engine.multi_loss(spec, None, *tensors, valid=valid)
    change_loss = _gathered(change_criterion, valid, logits_change, batch['y_change'])
    sem_loss = (_gathered(sem_criterion, valid, logits_sem_t1, batch['y_sem_t1'])
                + _gathered(sem_criterion, valid, logits_sem_t2, batch['y_sem_t2'])) / 2
    return (change_loss + sem_loss) / 2


def mmcr_loss(sup_criterion, cons_criterion, outputs, batch, alpha: float, cons_loss_type: str = 'PowerJaccardLoss'):
    logits_fusion, logits_s1, logits_s2 = outputs
    is_labeled = batch['is_labeled'].to(logits_fusion.device)
    y = batch['y_change']
    valid = batch.get('valid')
    l2 = cons_loss_type == 'L2'  # train_semisupervised.py:101-102: the criterion takes sigmoid(logits_s1), not logits_s1
    if _fusable(sup_criterion, cons_criterion):
        # one fused pass, subsets selected on the device: alpha/3 * (L_f + L_s1 + L_s2)[labelled]
        # + (1 - alpha) * L_cons(logits_s1 | sigmoid(logits_s1), sigmoid(logits_s2))[unlabelled]
        a = float(alpha)
        if valid is None and not l2 and _all_power_jaccard(sup_criterion, cons_criterion):  # the shipped configs
            spec = [(0, 3, a / 3, 1, 0), (1, 3, a / 3, 1, 0), (2, 3, a / 3, 1, 0), (1, 2, 1 - a, 2, 1)]
            return engine.multi_jaccard(spec, is_labeled, logits_fusion, logits_s1, logits_s2, y)
        ks, kc = sup_criterion.kind, cons_criterion.kind
        spec = [(0, 3, a / 3, 1, 0, ks, 0), (1, 3, a / 3, 1, 0, ks, 0), (2, 3, a / 3, 1, 0, ks, 0),
                (1, 2, 1 - a, 2, 1, kc, int(l2))]
        return engine.multi_loss(spec, is_labeled, logits_fusion, logits_s1, logits_s2, y, valid=valid)
    loss = None
    if valid is not None:
        valid = valid.to(logits_fusion.device)
    if bool(is_labeled.any()):
        v = None if valid is None else valid[is_labeled]
        sup = (_gathered(sup_criterion, v, logits_fusion[is_labeled], y[is_labeled])
               + _gathered(sup_criterion, v, logits_s1[is_labeled], y[is_labeled])
               + _gathered(sup_criterion, v, logits_s2[is_labeled], y[is_labeled])) / 3
        loss = alpha * sup
    if not bool(is_labeled.all()):
        nl = torch.logical_not(is_labeled)
        v = None if valid is None else valid[nl]
        first = torch.sigmoid(logits_s1[nl]) if l2 else logits_s1[nl]
        cons = (1 - alpha) * _gathered(cons_criterion, v, first, torch.sigmoid(logits_s2[nl]))
        loss = cons if loss is None else loss + cons
    return loss


def step_loss(cfg, outputs, batch, net=None):
    """Dispatch on the model family the way the reference's three trainers do.  `net`: the (wrapped) model the
    outputs come from; a model wrapped with exact_dataparallel=True forms ONE loss over the batch of all ranks
    (parallel.loss_scope), any other loss stays local."""
    from . import parallel
    with parallel.loss_scope(net):
        return _step_loss(cfg, outputs, batch)


def _step_loss(cfg, outputs, batch):
    t = cfg.MODEL.TYPE
    crit = loss_functions.get_criterion(cfg.MODEL.LOSS_TYPE)
    if t == 'dtsiameseunet':
        return dualtask_loss(crit, crit, outputs, batch)
    if t in ('whatevernet', 'whatevernet2') and isinstance(outputs, (tuple, list)):
        cons_type = cfg.CONSISTENCY_TRAINER.get('LOSS_TYPE', 'PowerJaccardLoss')
        cons = loss_functions.get_criterion(cons_type)
        return mmcr_loss(crit, cons, outputs, batch, cfg.CONSISTENCY_TRAINER.LOSS_FACTOR, cons_type)
    return supervised_loss(crit, outputs, batch)
