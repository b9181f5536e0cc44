#!/usr/bin/env python3
"""Table of the library's pure host queries about Conv3d -- workspace sizes and "is there such a form" answers -- over a grid of
geometries and every dispatch setting, reduced to one line: the number of answers and the sha256 of all of them in order.  Two
builds that print the same line size every workspace alike and answer every support question alike: the way to show that a change
to the dispatchers in csrc/conv_generic.hip / csrc/conv_bf16_api.hip left the allocation sizes, which are behaviour, alone.

usage: conv_query_table.py            (MI355SEG_LIB_PATH selects another build of the library, as everywhere)

No GPU is needed: nothing here launches a kernel or touches device memory."""
import hashlib
import itertools
import os
import struct
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]
import mi355seg  # noqa: E402

GEOM_QUERIES = ("mi355seg_conv3d_ws_bytes", "mi355seg_conv3d_ws_bytes_bf16", "mi355seg_conv3d_amax_use_f32", "mi355seg_stem_wgrad_bnbwd_supported_f32")
PITCH_QUERIES = ("mi355seg_conv3d_fused_supported_f32", "mi355seg_conv3d_fused_supported_bf16")
ACTS = range(5)                 # mi355seg_conv3d_pro_supported_f32 takes the activation code
MATHS = ((0, 16), (2, 16), (2, 32), (3, 16))        # (MI355SEG_MATH_* code, bf16x6 MFMA shape): fp32, bf16x6 / 16, bf16x6 / 32, f16x3
CHANNELS = (1, 2, 4, 8, 16, 24, 32, 64, 128, 256, 512)
EXTENTS = ((8, 8, 8), (16, 16, 16), (32, 32, 32), (128, 128, 128), (9, 11, 34))
KSP = ((1, 1, 0), (3, 1, 1), (5, 1, 2), (3, 2, 1), (2, 2, 0), (4, 4, 0), (16, 16, 0))


def geometries():
    import test_gpu_bf16
    import test_gpu_conv_paths
    out = [c[0] for c in test_gpu_conv_paths.CONV_CASES] + [c[0] for c in test_gpu_conv_paths.YAMAX_CASES]
    out += list(test_gpu_bf16.CONV_CASES) + list(test_gpu_bf16.B16S_CASES) + [c[0] for c in test_gpu_bf16.DEMOTION_CASES]
    for n, (d, h, w), cin, cout, (k, s, p) in itertools.product((1, 2), EXTENTS, CHANNELS, CHANNELS, KSP):
        if min(d, h, w) + 2 * p >= k:
            out.append((n, d, h, w, cin, cout, k, s, p))
    return list(dict.fromkeys(out))


def main():
    L = mi355seg.lib()
    math0, shape0, tiles0, wide0 = (L.query(f"mi355seg_get_{n}") for n in ("conv_math", "x3_shape", "b16_tiles", "wgrad_wide"))
    geoms = geometries()
    h, count = hashlib.sha256(), 0
    try:
        for (math, shape), tiles, wide in itertools.product(MATHS, range(3), range(3)):
            L.call("mi355seg_set_conv_math", math)
            L.call("mi355seg_set_x3_shape", shape)
            L.call("mi355seg_set_b16_tiles", tiles)
            L.call("mi355seg_set_wgrad_wide", wide)
            for g in geoms:
                cin, cout = g[4], g[5]
                row = [L.query(q, *g) for q in GEOM_QUERIES]
                row += [L.query(q, *g, cin + e, cout + e) for q in PITCH_QUERIES for e in (0, 4)]
                row += [L.query("mi355seg_conv3d_pro_supported_f32", *g, a) for a in ACTS]
                h.update(struct.pack(f"<13q{len(row)}Q", math, shape, tiles, wide, *g, *row))
                count += len(row)
    finally:
        L.call("mi355seg_set_conv_math", math0)
        L.call("mi355seg_set_x3_shape", shape0)
        L.call("mi355seg_set_b16_tiles", tiles0)
        L.call("mi355seg_set_wgrad_wide", wide0)
    print(f"{count} answers over {len(geoms)} geometries x {len(MATHS) * 9} settings  sha256 {h.hexdigest()}")


if __name__ == "__main__":
    main()
