"""The reference's training criterion on the device, from the label mask: ``MaskBCELoss``.

Every recipe of the reference trains with ``torch.nn.BCEWithLogitsLoss`` on the class planes and on the offset planes
of the network's output and adds them as ``cls_loss + alpha * ofs_loss`` (egs/cityscape/local/train.py:183-195,
utils/train_utils.py:42-79,145-180), against float32 target planes that the dataset materialises.  Here the targets
are looked up in the int32 label mask, and the loss and its gradient come out of ONE pass per image
(``Merger.mask_bce``): the logits are read once, the gradient is written once.

``MaskDiceLoss`` and ``MaskMultiBCELoss`` are the recipes' ``--loss dice`` and ``--loss mbce`` (``SoftDiceLoss`` and
``MultiBCEWithLogitsLoss`` of utils/loss.py) on one part of the output.  Their gradient depends on totals over a whole
plane, so they take three steps: ``Merger.plane_sums``, ``Merger.plane_coeffs``, ``Merger.plane_grad``.

``MaskCELoss`` is the recipes' ``--loss ce`` (``CrossEntropyLossOneHot`` of utils/loss.py) on one part of the output:
a softmax over the part's planes per pixel, loss and gradient in ONE pass per image (``Merger.mask_ce``).

Out of scope for ``MaskCELoss``: a per-class ``weight`` (its mean divides by the sum of the targets' weights, which is
not known before the pass), a divisor of the kept pixels only (``last_sums[1]`` holds their number for a caller who
wants it), ``WeightedBCEWithLogitsLoss`` (no recipe uses it) and polygon targets.
"""
from __future__ import annotations

import torch
from torch import nn


def _batch_truth(truth, truth_classes, B, H, W):
    """The ground truth of a batch: ``truth`` a contiguous int32 [B, H, W] tensor on the GPU, ``truth_classes`` a list
    of B entries or None (no image has instances).  Returns the list."""
    if not (truth.is_cuda and truth.dtype == torch.int32 and truth.is_contiguous()
            and tuple(truth.shape) == (B, H, W)):
        raise ValueError("truth: a contiguous int32 [B, H, W] tensor on the GPU")
    if truth_classes is None:
        truth_classes = [None] * B
    if len(truth_classes) != B:
        raise ValueError("truth_classes: one int32 tensor (or None) per image")
    return truth_classes


class _MaskBCE(torch.autograd.Function):
    @staticmethod
    def forward(ctx, prediction, module, truth, truth_classes, want_grad):
        loss, sums, grad = module._run(prediction.detach(), truth, truth_classes, want_grad)
        module.last_sums = sums
        ctx.grad = grad
        return loss

    @staticmethod
    def backward(ctx, grad_output):
        grad, ctx.grad = ctx.grad, None
        if grad is None:
            raise RuntimeError("MaskBCELoss: backward was already run, or forward ran without a gradient")
        return grad.mul_(grad_output), None, None, None, None      # (no test for 1.0: that would synchronise)


class MaskBCELoss(nn.Module):
    """``cls_loss + alpha * ofs_loss`` of the reference with mean reduction, from the label mask.

    ``merger``: a :class:`mergenet_amd.segmenter.Merger` on the prediction's GPU (any capacity: the pass takes any
    image size); ``num_classes`` C and ``offsets`` (O pairs ``(di, dj)``) split the prediction's channels: the first
    C are the class logits, the next O the offset logits.  C or O may be 0 (offset-only or class-only training).

    ``forward(prediction [B, C+O, H, W], truth [B, H, W] int32, truth_classes)``: ``prediction`` contiguous float32,
    float16 or bfloat16 LOGITS on the GPU; ``truth`` the label masks (0 = no instance); ``truth_classes`` a list of
    B int32 device tensors -- entry g-1 the class of label g of that image -- or None entries for images without
    instances (None for the whole list: no image has any).  Returns the loss as a float32 device scalar

        sums[0] / (B*C*H*W) + alpha * sum(sums[1:1+O]) / (B*O*H*W)

    where ``sums`` are the totals of ``Merger.mask_bce`` over the batch: with no ignore class exactly
    ``BCEWithLogitsLoss()(prediction[:, :C], class_targets) + alpha * BCEWithLogitsLoss()(prediction[:, C:],
    offset_targets)``.  A pixel whose truth class lies outside 0..C-1 is an ignore class: it contributes 0 to the class
    loss and gets no class gradient, but it still COUNTS in the divisor B*C*H*W; the number of kept pixels is in
    ``last_sums[1 + O]`` for a caller who wants another normalisation.

    One kernel pass per image, all added into one ``sums`` buffer; nothing is synchronised with the host and no plane
    is copied (``prediction[b, :C]`` and ``prediction[b, C:]`` are contiguous blocks).  When ``prediction`` requires a
    gradient (and gradients are enabled) the same pass writes it, already scaled by the mean's divisors, into one
    buffer of the prediction's shape and dtype; ``backward`` multiplies that buffer by the incoming gradient in place
    and returns it, so a forward result can be back-propagated once.  Otherwise (``torch.no_grad()``, validation) no
    gradient buffer is allocated and the loss is the same bits.

    ``last_sums``: the float64 [2+O] totals of the last forward on the device -- ``last_sums[1:1+O] / (B*H*W)`` are
    the per-offset losses the reference logs.

    float16: a gradient scaled by 1 / (B*C*H*W) underflows binary16 at any real image size, and nothing here
    rescales it behind the caller's back.  Train in bfloat16 or float32, or call ``Merger.mask_bce`` with
    ``scale_class`` / ``scale_same`` of a loss scaler's choosing."""

    def __init__(self, merger, num_classes: int, offsets, alpha: float = 1.0):
        super().__init__()
        self.merger = merger
        self.num_classes = int(num_classes)
        self.offsets = [(int(di), int(dj)) for di, dj in offsets]
        self.alpha = float(alpha)
        if self.num_classes < 0 or self.num_classes + len(self.offsets) == 0:
            raise ValueError("MaskBCELoss needs class planes or offset planes")
        self.last_sums = None

    def _run(self, prediction, truth, truth_classes, want_grad: bool):
        C, O = self.num_classes, len(self.offsets)
        if not (prediction.is_cuda and prediction.dim() == 4 and prediction.is_contiguous()):
            raise ValueError("prediction: a contiguous [B, C+O, H, W] tensor on the GPU")
        B, K, H, W = prediction.shape
        if K != C + O:
            raise ValueError("prediction has %d channels, the criterion %d classes and %d offsets" % (K, C, O))
        truth_classes = _batch_truth(truth, truth_classes, B, H, W)
        scale_class = 1.0 / (B * C * H * W) if C else 0.0
        scale_same = self.alpha / (B * O * H * W) if O else 0.0
        grad = torch.empty_like(prediction) if want_grad else None
        sums = None
        for b in range(B):
            out = None
            if want_grad:
                out = (grad[b, :C] if C else None, grad[b, C:] if O else None)
            res = self.merger.mask_bce(prediction[b, :C] if C else None, prediction[b, C:] if O else None,
                                       self.offsets, truth[b], truth_classes[b], scale_class, scale_same,
                                       grad=want_grad, into=sums, out=out)
            sums = res["sums"]
        loss = sums[0] * scale_class + sums[1:1 + O].sum() * scale_same
        return loss.to(torch.float32), sums, grad

    def forward(self, prediction, truth, truth_classes=None):
        want_grad = prediction.requires_grad and torch.is_grad_enabled()     # (grad mode is off inside the Function)
        return _MaskBCE.apply(prediction, self, truth, truth_classes, want_grad)


# ---- the criteria whose gradient needs totals over a plane: soft Dice and weighted multi-BCE ----------------------

class _PlaneLoss(torch.autograd.Function):
    @staticmethod
    def forward(ctx, prediction, module, truth, truth_classes):
        pred = prediction.detach()
        loss, sums, coeffs = module._sums_and_coeffs(pred, truth, truth_classes)
        module.last_sums = sums
        ctx.save_for_backward(prediction)
        ctx.module, ctx.truth, ctx.truth_classes, ctx.coeffs = module, truth, truth_classes, coeffs
        return loss

    @staticmethod
    def backward(ctx, grad_output):
        (prediction,) = ctx.saved_tensors
        factor = grad_output.detach().to(torch.float32).contiguous()      # (a device scalar: the kernel reads it)
        grad = ctx.module._gradient(prediction.detach(), ctx.truth, ctx.truth_classes, ctx.coeffs, factor)
        return grad, None, None, None


class _MaskPlaneLoss(nn.Module):
    """What :class:`MaskDiceLoss` and :class:`MaskMultiBCELoss` share: one part of the output, three steps.  A subclass
    supplies ``_sums_and_coeffs`` and says how the gradient pass takes its coefficients:"""

    complement = False            # with q = sigmoid(-x), z = !y, as the sums were taken (MaskDiceLoss(mode='0'))
    coeffs_per_image = False      # as [B, 4, P], one set per image, not one [4, P] for the batch

    def __init__(self, merger, part, offsets=None):
        super().__init__()
        if part not in ("class", "offset"):
            raise ValueError("part: 'class' or 'offset'")
        self.merger = merger
        self.part = part
        self.offsets = None if offsets is None else [(int(di), int(dj)) for di, dj in offsets]
        if part == "offset" and not self.offsets:
            raise ValueError("the offset part needs its offsets")
        self.last_sums = None

    def _check(self, prediction, truth, truth_classes):
        if not (prediction.is_cuda and prediction.dim() == 4 and prediction.shape[0] > 0
                and all(prediction[b].is_contiguous() for b in range(prediction.shape[0]))):
            raise ValueError("prediction: a [B, P, H, W] tensor on the GPU whose images are contiguous [P, H, W] blocks")
        B, P, H, W = prediction.shape
        if self.part == "offset" and P != len(self.offsets):
            raise ValueError("prediction has %d planes, the criterion %d offsets" % (P, len(self.offsets)))
        return B, P, H, W, _batch_truth(truth, truth_classes, B, H, W)

    def _gradient(self, prediction, truth, truth_classes, coeffs, factor):
        B, P, H, W, tcs = self._check(prediction, truth, truth_classes)
        grad = torch.empty((B, P, H, W), dtype=prediction.dtype, device=prediction.device)
        for b in range(B):
            self.merger.plane_grad(prediction[b], self.part, self.offsets, truth[b], tcs[b],
                                   coeffs[b] if self.coeffs_per_image else coeffs, factor=factor,
                                   complement=self.complement, out=grad[b])
        return grad

    def forward(self, prediction, truth, truth_classes=None):
        return _PlaneLoss.apply(prediction, self, truth, truth_classes)


class MaskDiceLoss(_MaskPlaneLoss):
    """``SoftDiceLoss(mode, smooth)`` of the reference (utils/loss.py:38-58; ``--loss dice`` of the Cityscapes recipe
    is mode ``'0'`` on the offset planes, egs/cityscape/local/train.py:193-204) on ONE part of the network's output,
    from the label mask: no target plane is materialised.

    ``merger``: a :class:`mergenet_amd.segmenter.Merger` on the prediction's GPU; ``part``: ``'class'`` or
    ``'offset'`` (then ``offsets``, one pair per plane); ``mode='0'`` takes ``1 - p`` and ``1 - t`` (``1 - p`` as
    ``sigmoid(-x)``: nothing cancels where the zeros are rare); ``smooth`` > 0.

    ``forward(prediction [B, P, H, W], truth [B, H, W] int32, truth_classes=None)``: ``prediction`` float32, float16
    or bfloat16 LOGITS, possibly a channel slice of the network's output -- every ``prediction[b]`` must be a
    contiguous [P, H, W] block; ``truth``, ``truth_classes`` as for :class:`MaskBCELoss`.  Returns, as a float32 device
    scalar, the sum over the planes of ``1 - (2*sum(p*t) + smooth) / (sum(p) + sum(t) + smooth)`` with the sums over
    the WHOLE batch (``labels.dice_loss`` is the numpy statement).  A pixel whose truth class lies outside 0..P-1
    (class part) is left out of every sum and gets gradient 0.

    Forward: B passes for the sums, added into one buffer (``last_sums``, float64 [5*P + 1]), and one small launch
    for the loss and the planes' coefficients; no gradient buffer exists and nothing is synchronised.  Backward: B
    gradient passes into a fresh tensor of the prediction's dtype; the incoming gradient is read by the kernel as a
    device scalar.  The prediction is saved, so a result may be back-propagated more than once.  Under
    ``torch.no_grad()``, or when the prediction requires no gradient, only the forward's launches run."""

    def __init__(self, merger, part, offsets=None, mode: str = "1", smooth: float = 1.0):
        super().__init__(merger, part, offsets)
        if mode not in ("0", "1"):
            raise ValueError("mode: '0' or '1'")
        if not (smooth > 0 and smooth < float("inf")):
            raise ValueError("smooth must be finite and > 0")
        self.mode, self.smooth, self.complement = mode, float(smooth), mode == "0"

    def _sums_and_coeffs(self, prediction, truth, truth_classes):
        B, P, H, W, tcs = self._check(prediction, truth, truth_classes)
        comp = self.complement
        sums = None
        for b in range(B):
            sums = self.merger.plane_sums(prediction[b], self.part, self.offsets, truth[b], tcs[b], complement=comp,
                                          terms=False, into=sums)
        res = self.merger.plane_coeffs("dice", sums, pixels=H * W, smooth=self.smooth, scale=1.0, complement=comp)
        return res["loss"].to(torch.float32), sums, res["coeffs"]


class MaskMultiBCELoss(_MaskPlaneLoss):
    """``MultiBCEWithLogitsLoss`` of the reference (utils/loss.py:63-76, ``--loss mbce``) on ONE part of the network's
    output, from the label mask.  Per image and plane ``S = sum sigmoid(x)``, ``w = (H*W - S + 1) / (S + 1)``; an
    element's weight is w where its target is 1, else 1; the loss is the mean over all B*P*H*W elements of weight
    times BCE term (``labels.multi_bce_loss`` is the numpy statement).  The weight is a function of the prediction
    and the gradient is that of the loss as stated, the weight's own derivative INCLUDED -- what the reference's torch
    computed; a current torch refuses to differentiate ``binary_cross_entropy_with_logits`` with respect to its
    weight.

    Arguments and ``forward`` as for :class:`MaskDiceLoss`.  A pixel whose truth class lies outside 0..P-1 (class
    part) is left out of S, contributes 0 and gets gradient 0; it still COUNTS in H*W and in the divisor.
    Forward: per image one pass for the sums (``last_sums``, float64 [B, 5*P + 1]) and one small launch for its
    coefficients, the loss added up on the device.  Backward: B gradient passes, the incoming gradient read by the
    kernel.  The prediction is saved, so a result may be back-propagated more than once.

    float16: a gradient scaled by 1 / (B*P*H*W) underflows binary16 at any real image size, and nothing here
    rescales it behind the caller's back.  Train in bfloat16 or float32, or scale the loss before ``backward`` (the
    factor reaches the kernel before the rounding to float16)."""

    coeffs_per_image = True

    def _sums_and_coeffs(self, prediction, truth, truth_classes):
        B, P, H, W, tcs = self._check(prediction, truth, truth_classes)
        dev = prediction.device
        sums = torch.empty((B, 5 * P + 1), dtype=torch.float64, device=dev)
        coeffs = torch.empty((B, 4, P), dtype=torch.float32, device=dev)
        loss = None
        for b in range(B):
            self.merger.plane_sums(prediction[b], self.part, self.offsets, truth[b], tcs[b], terms=True, out=sums[b])
            loss = self.merger.plane_coeffs("mbce", sums[b], pixels=H * W, scale=1.0 / (B * P * H * W), into=loss,
                                            out=coeffs[b])["loss"]
        return loss.to(torch.float32), sums, coeffs


# ---- cross-entropy over the planes of one part --------------------------------------------------------------------

class _MaskCE(torch.autograd.Function):
    @staticmethod
    def forward(ctx, prediction, module, truth, truth_classes, want_grad):
        loss, sums, grad = module._run(prediction.detach(), truth, truth_classes, want_grad)
        module.last_sums = sums
        ctx.grad = grad
        return loss

    @staticmethod
    def backward(ctx, grad_output):
        grad, ctx.grad = ctx.grad, None
        if grad is None:
            raise RuntimeError("MaskCELoss: backward was already run, or forward ran without a gradient")
        return grad.mul_(grad_output), None, None, None, None      # (no test for 1.0: that would synchronise)


class MaskCELoss(_MaskPlaneLoss):
    """``CrossEntropyLossOneHot()`` of the reference (utils/loss.py:24-35: ``F.cross_entropy(input,
    target.max(1)[1])`` with mean reduction; ``--loss ce`` of egs/coco/local/train.py:145-154 on the class planes and of
    egs/cityscape/local/train.py:193-204 on the offset planes) on ONE part of the network's output, from the label
    mask: neither the one-hot target planes nor their argmax are materialised.

    ``merger``, ``part``, ``offsets`` and the arguments of ``forward(prediction [B, P, H, W], truth [B, H, W] int32,
    truth_classes=None)`` as for :class:`MaskDiceLoss`: every ``prediction[b]`` a contiguous [P, H, W] block of
    float32, float16 or bfloat16 LOGITS.  The target plane of a pixel is its truth class (class part) or the first
    offset plane whose target is 1, plane 0 if none is (offset part): what ``max(1)[1]`` elects.  Returns the loss as a
    float32 device scalar

        sums[0] / (B*H*W)

    where ``sums`` are the totals of ``Merger.mask_ce`` over the batch (``labels.mask_ce`` is the numpy statement):
    with no ignore class exactly ``CrossEntropyLossOneHot()(prediction, targets)``.  A pixel whose truth class lies
    outside 0..P-1 (class part) is an ignore class: it contributes 0 and gets gradient 0, but it still COUNTS in the
    divisor B*H*W -- the reference has no ignore class and would elect class 0 there; ``last_sums[1]`` holds the
    number of kept pixels for a caller who wants another normalisation.

    One kernel pass per image, all added into one ``sums`` buffer (``last_sums``, float64 [2]); nothing is
    synchronised with the host and no plane is copied.  When ``prediction`` requires a gradient (and gradients are
    enabled) the same pass writes it, already scaled by 1 / (B*H*W), into one buffer of the prediction's shape and
    dtype; ``backward`` multiplies that buffer by the incoming gradient in place and returns it, so a forward result
    can be back-propagated once.  Otherwise (``torch.no_grad()``, validation) no gradient buffer is allocated and the
    loss is the same bits.

    float16: a gradient scaled by 1 / (B*H*W) underflows binary16 at any real image size, and nothing here rescales
    it behind the caller's back.  Train in bfloat16 or float32, or call ``Merger.mask_ce`` with a ``scale`` of a loss
    scaler's choosing.

    Not offered: a per-class ``weight``, a divisor of the kept pixels only (see the module's documentation)."""

    def _run(self, prediction, truth, truth_classes, want_grad: bool):
        B, P, H, W, tcs = self._check(prediction, truth, truth_classes)
        scale = 1.0 / (B * H * W)
        grad = torch.empty((B, P, H, W), dtype=prediction.dtype, device=prediction.device) if want_grad else None
        sums = None
        for b in range(B):
            sums = self.merger.mask_ce(prediction[b], self.part, self.offsets, truth[b], tcs[b], scale,
                                       grad=want_grad, into=sums, out=grad[b] if want_grad else None)["sums"]
        return (sums[0] * scale).to(torch.float32), sums, grad

    def forward(self, prediction, truth, truth_classes=None):
        want_grad = prediction.requires_grad and torch.is_grad_enabled()     # (grad mode is off inside the Function)
        return _MaskCE.apply(prediction, self, truth, truth_classes, want_grad)
