#!/usr/bin/env python3
"""Generator of tests/golden/loss_tail_pins.json: SHA-256 digests of the output bytes of every kernel family of csrc/loss_tail.hip
(both forms of the fused tail, forward and backward, the conversion kernels and the class counters), each beside the digest of its
input bytes.  The cases and the digest function are the test's own (tests/test_gpu_multiclass.py loss_tail_pin_digests), so the
file and the test cannot drift apart.

The file pins BITS across a change of the kernels that must not move them: it is made from a tree whose csrc/ is that of the
commit given on the command line, before the kernels are touched, and only ever regenerated from such a tree.

usage: python tests/golden/make_loss_tail_pins.py COMMIT   (needs the MI355X and the built library; COMMIT: `git rev-parse HEAD`
                                                            of the tree the library was built from)
"""
import json
import os
import sys

import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def main():
    commit = sys.argv[1]
    assert torch.cuda.is_available(), "make_loss_tail_pins.py records what the MI355X computes; there is nothing to record without one"
    import mi355seg
    from test_gpu_multiclass import loss_tail_pin_digests
    mi355seg.lib()
    out = {"_what": "SHA-256 of input and output bytes per case (see make_loss_tail_pins.py)", "commit": commit,
           "device": torch.cuda.get_device_name(0), "loss_tail": loss_tail_pin_digests(mi355seg.functional)}
    with open(os.path.join(HERE, "loss_tail_pins.json"), "w") as fh:
        json.dump(out, fh, indent=1)
        fh.write("\n")
    print(f"{len(out['loss_tail'])} loss_tail cases on {out['device']}")


if __name__ == "__main__":
    main()
