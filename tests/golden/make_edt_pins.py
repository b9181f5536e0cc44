#!/usr/bin/env python3
"""Generator of tests/golden/edt_pins.json: SHA-256 digests of the output bytes of the two distance-transform families,
``functional.edt3d`` (csrc/surface.hip, fp64 squared distances) and ``functional.signed_distance_map`` (csrc/boundary.hip, fp32),
on inputs the GPU tests already build, each beside the digest of its input bytes.  The cases and the digest functions are the
tests' own (tests/test_gpu_hd95.py edt_pin_digests, tests/test_gpu_boundary.py sdm_pin_digests), so the file and the tests cannot
drift apart.

The file pins BITS across a change of the kernels that must not move them: it is made from a tree whose csrc/ is that of the
commit given on the command line, before the kernels are touched, and only ever regenerated from such a tree.

usage: python tests/golden/make_edt_pins.py COMMIT        (needs the MI355X and the built library; COMMIT: `git rev-parse HEAD`
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
    assert torch.cuda.is_available(), "make_edt_pins.py records what the MI355X computes; there is nothing to record without one"
    import mi355seg
    from test_gpu_boundary import sdm_pin_digests
    from test_gpu_hd95 import edt_pin_digests
    mi355seg.lib()
    out = {"_what": "SHA-256 of input and output bytes per case (see make_edt_pins.py)", "commit": commit,
           "device": torch.cuda.get_device_name(0), "edt3d": edt_pin_digests(mi355seg.functional),
           "signed_distance_map": sdm_pin_digests(mi355seg.functional)}
    with open(os.path.join(HERE, "edt_pins.json"), "w") as fh:
        json.dump(out, fh, indent=1)
        fh.write("\n")
    print(f"{len(out['edt3d'])} edt3d cases, {len(out['signed_distance_map'])} signed_distance_map cases on {out['device']}")


if __name__ == "__main__":
    main()
