"""Who owns a context's memory (mergenet_amd/csrc/mn_memory.h), on the GPU: one Merger of 32 x 64 pixels, 3 classes and
4 offsets goes through every path that allocates -- create, a default segment, the general rounds (the record lists
swapped for the full-size ones), the exact engine, the reference-order loop, the host-pointer entry point (staging),
and the four buffers allocated where an entry point first needs them -- then a two-image ExactBatch (the batch
arrays).  ``workspace_bytes()`` after each step is held to what the library reported BEFORE its allocations moved
into the registry, and the device memory that is still missing once every context is closed to what it left missing
then.  Run as a program this file prints the figures (profiles/context_memory_bytes.log keeps the two raw runs).

Where the paths are reached at this shape: 2048 pixels x 4 offsets are fewer records than exact_limit, so the DEFAULT
segment already runs the exact engine (x_ensure) and, its maps having tied pops, the redo in the reference's order
(r_ensure): the two blocks are the 3662080 bytes of that step.  The explicit exact and reference-order steps then run
x_ensure / r_ensure on a workspace that fits and add nothing; "rounds" adds the fast-path group (the full-size record
lists are as large as the small ones here).  The contexts of the batch allocate both workspaces afresh.
"""
import ctypes
import gc

import numpy as np
import pytest

from mergenet_amd import segmenter as seg
from mergenet_amd import synth

pytestmark = pytest.mark.gpu

H, W, C, O = 32, 64, 3, 4

# What the build of the parent commit (hand-kept `bytes` counter, destroy lists) printed for this walk:
# profiles/context_memory_bytes.log, first run.  Not taken from the build under test.
PARENT_STEPS = [
    ('create', 1544960),
    ('default', 5207040),
    ('rounds', 5313792),
    ('exact', 5313792),
    ('exact, reference order', 5313792),
    ('host staging', 5395712),
    ('match_instances', 5481728),
    ('DatasetEval.add', 7087360),
    ('map_scores', 7873792),
    ('mask_bce', 7873792),
    ('plane_sums', 13083904),
    ('batch image 0', 5207040),
    ('batch image 1', 5207040),
]
PARENT_RETAINED = 287309824         # bytes of device memory missing after the last close, same run


def walk():
    """[(step, workspace bytes)] of the walk and the device memory it did not give back."""
    import torch
    offs = synth.generate_offsets(8, O)
    s = synth.synth_v1(H, W, C, offs, 1001, num_instances=3)
    cp, sp = torch.from_numpy(s.class_probs).cuda(), torch.from_numpy(s.sameness_probs).cuda()
    truth = torch.from_numpy(np.ascontiguousarray(s.instances, np.int32)).cuda()
    truth_classes = torch.tensor(s.instance_class[1:], dtype=torch.int32).cuda()
    G = int(truth_classes.numel())
    seg.Merger(H, W, C, O).close()             # (the runtime's own one-time allocations are not the library's)
    torch.cuda.synchronize()
    torch.cuda.empty_cache()
    free_before = torch.cuda.mem_get_info()[0]

    steps, keep = [], []
    m = seg.Merger(H, W, C, O)

    def step(name, result=None):
        keep.append(result)
        steps.append((name, m.workspace_bytes()))

    step("create")
    mask, table, _, stats = m.segment(cp, sp, offs, seg.default_options(clip_inputs=1))
    step("default")
    step("rounds", m.segment(cp, sp, offs, seg.default_options(clip_inputs=1, mode=seg.MN_MODE_ROUNDS)))
    step("exact", m.segment(cp, sp, offs, seg.default_options(clip_inputs=1, mode=seg.MN_MODE_EXACT)))
    step("exact, reference order", m.segment(cp, sp, offs, seg.default_options(
        clip_inputs=1, mode=seg.MN_MODE_EXACT, tie_order=seg.MN_TIES_REFERENCE)))
    # mn_segment_host on the Merger's own context (HostContext, which binds it, owns a context of its own)
    f32p, i32p = ctypes.POINTER(ctypes.c_float), ctypes.POINTER(ctypes.c_int)
    off = np.ascontiguousarray(np.asarray(offs, np.int32).reshape(-1, 2))
    h_mask, h_table, h_stats = np.zeros((H, W), np.int32), np.zeros(H * W, np.int32), seg.MnStats()
    rc = m.lib.mn_segment_host(m.handle, s.class_probs.ctypes.data_as(f32p), C, s.sameness_probs.ctypes.data_as(f32p), O,
                               W, H, C, off.ctypes.data_as(i32p), h_mask.ctypes.data_as(i32p),
                               h_table.ctypes.data_as(i32p), None, ctypes.byref(seg.default_options()),
                               ctypes.byref(h_stats))
    assert rc == 0, rc
    step("host staging")
    K = int(stats["num_instances"])
    overlaps = m.overlap_table(mask, truth, K, G)
    step("match_instances", m.match_instances(overlaps, table, truth_classes))
    ev = m.dataset_eval(num_classes=C)
    ev.add(overlaps, table, truth_classes)
    step("DatasetEval.add", ev)
    step("map_scores", m.map_scores(cp, sp, offs, truth, truth_classes))
    step("mask_bce", m.mask_bce(cp, sp, offs, truth, truth_classes))
    step("plane_sums", m.plane_sums(cp, "class", None, truth, truth_classes))
    torch.cuda.synchronize()
    m.close()

    batch = seg.ExactBatch(H, W, C, O, 2)
    keep.append(batch.segment([cp, cp], [sp, sp], offs, seg.default_options(clip_inputs=1, mode=seg.MN_MODE_EXACT)))
    steps += [("batch image %d" % i, b.workspace_bytes()) for i, b in enumerate(batch.mergers)]
    torch.cuda.synchronize()
    batch.close()

    del keep, ev, overlaps, mask, table        # (the inputs were there at the first reading and stay for the second)
    gc.collect()
    torch.cuda.synchronize()
    torch.cuda.empty_cache()
    return steps, free_before - torch.cuda.mem_get_info()[0]


@pytest.fixture(scope="module")
def walked():
    return walk()


def test_workspace_bytes_are_the_parents_after_every_step(walked):
    steps, _ = walked
    print("steps:", steps)
    assert steps == PARENT_STEPS


def test_closed_contexts_give_back_what_the_parents_did(walked):
    _, retained = walked
    print("retained:", retained, "parent:", PARENT_RETAINED)
    assert retained <= PARENT_RETAINED


if __name__ == "__main__":
    got_steps, got_retained = walk()
    print("library:", seg.LIB_PATH)
    for name, nbytes in got_steps:
        print("    (%r, %d)," % (name, nbytes))
    print("retained after the last close: %d bytes" % got_retained)
