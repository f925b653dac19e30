"""Inputs built from a label map, for the tests of the sweep's lean form (test_lean_groups.py, test_gpu_lean_sweep.py)."""
import numpy as np


def pos_bits_of(lab, offs):
    """uint32 [H, W]: bit k of pixel p is set iff p + offset k is inside the image and carries p's label -- the positive
    masks the sweep leaves on maps_from_labels(lab, ...)."""
    H, W = lab.shape
    bits = np.zeros((H, W), np.uint32)
    for k, (di, dj) in enumerate(offs):
        r0, r1 = max(0, -di), min(H, H - di)
        c0, c1 = max(0, -dj), min(W, W - dj)
        if r0 >= r1 or c0 >= c1:
            continue
        same = lab[r0:r1, c0:c1] == lab[r0 + di:r1 + di, c0 + dj:c1 + dj]
        bits[r0:r1, c0:c1] |= same.astype(np.uint32) << np.uint32(k)
    return bits


def maps_from_labels(lab, class_of_label, C, offs):
    """(class_probs float32 [C, H, W], sameness_probs float32 [O, H, W]): sameness 0.95 inside a label, 0.05 across,
    1.0 where the edge leaves the image (as synth writes it); class maps peaked (0.9) on the label's class."""
    H, W = lab.shape
    cls = np.vectorize(lambda l: class_of_label[int(l)])(lab)
    cp = np.full((C, H, W), 0.1 / max(C - 1, 1), np.float32)
    for c in range(C):
        cp[c][cls == c] = 0.9
    sp = np.ones((len(offs), H, W), np.float32)
    for k, (di, dj) in enumerate(offs):
        r0, r1 = max(0, -di), min(H, H - di)
        c0, c1 = max(0, -dj), min(W, W - dj)
        if r0 >= r1 or c0 >= c1:
            continue
        same = lab[r0:r1, c0:c1] == lab[r0 + di:r1 + di, c0 + dj:c1 + dj]
        sp[k, r0:r1, c0:c1] = np.where(same, np.float32(0.95), np.float32(0.05))
    return cp, sp


def stripes(H, W, width):
    """Vertical stripes `width` columns wide, alternating labels 0 and 1..: with width < 63 every run of 63 links along
    a row is broken, so no 64-pixel group can be uniform."""
    lab = np.zeros((H, W), np.int32)
    for s, c0 in enumerate(range(0, W, width)):
        lab[:, c0:c0 + width] = 0 if s % 2 == 0 else (s + 1) // 2
    return lab
