#!/usr/bin/env python
"""Generate tests/golden/lowp_*.npz: the reference's result on 16-bit probability maps.

Needs the reference's own merger compiled into oracle/_ref/ (oracle/Makefile; a GPU box never runs this):

    python tests/golden/make_golden_lowp.py

Each of the twelve maps (tests/lowp_util.specs) is quantised to float16 or bfloat16, widened back to float32
(exact) and handed to the reference through the binding's preprocessing, clip included.  A fixture holds DATA
only: the recipe, a sha256 of the 16-bit input bytes, the reference's mask and class list.
"""
import json
import os
import sys
import time

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import lowp_util  # noqa: E402
from oracle import checker as ck  # noqa: E402


def main():
    ck.build()
    if not ck.have_reference():
        raise SystemExit("oracle/_ref/libcsegment_ref.so missing: the reference tree is not present")
    for spec in lowp_util.specs():
        q = lowp_util.quantized_inputs(spec)
        t = time.time()
        ref = ck.run_reference(q["class_probs"], q["sameness_probs"], spec["C"], q["offsets"], *spec["opts"])
        dt = time.time() - t
        np.savez_compressed(os.path.join(HERE, spec["name"] + ".npz"), spec=json.dumps(spec),
                            sha256=lowp_util.digest(q["class_bits"], q["same_bits"]),
                            mask=ref.mask.astype(np.int32),
                            object_class=np.asarray(ref.object_class, np.int32), ref_seconds=dt)
        sp = q["sameness_probs"]
        print("%-28s K=%-3d %.2fs  sameness == 1.0: %.1f %%  == 0.0: %d" %
              (spec["name"], len(ref.object_class), dt, 100.0 * float((sp == 1.0).mean()), int((sp == 0.0).sum())),
              flush=True)


if __name__ == "__main__":
    main()
