"""The reference's training criterion on the device, from the label mask: ``MaskBCELoss``.

Every recipe of the reference trains with ``torch.nn.BCEWithLogitsLoss`` on the class planes and on the offset planes
of the network's output and adds them as ``cls_loss + alpha * ofs_loss`` (egs/cityscape/local/train.py:183-195,
utils/train_utils.py:42-79,145-180), against float32 target planes that the dataset materialises.  Here the targets
are looked up in the int32 label mask, and the loss and its gradient come out of ONE pass per image
(``Merger.mask_bce``): the logits are read once, the gradient is written once.
"""
from __future__ import annotations

import torch
from torch import nn


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
        if not (truth.is_cuda and truth.dtype == torch.int32 and truth.is_contiguous()
                and tuple(truth.shape) == (B, H, W)):
            raise ValueError("truth: a contiguous int32 [B, H, W] tensor on the GPU")
        if truth_classes is None:
            truth_classes = [None] * B
        if len(truth_classes) != B:
            raise ValueError("truth_classes: one int32 tensor (or None) per image")
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
