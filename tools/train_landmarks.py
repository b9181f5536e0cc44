#!/usr/bin/env python3
"""Train the Nyul landmarks of ``config.intensity=histogram`` / ``histogram_znorm`` from a directory of ``.npy`` volumes
(mi355seg.data.train_landmarks: per volume the percentiles 1, 10, 20, ..., 90, 99 of the masked voxels on the device, rescaled to
0 .. 100, averaged in fp64) and write them as 11 float64 values for ``config.intensity_landmarks``.

usage: train_landmarks.py DIR OUT.npy [--mask none|mean|NUMBER] [--device cuda:0]"""
import argparse
import glob
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np  # noqa: E402
from mi355seg.data import train_landmarks  # noqa: E402


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("dir")
    ap.add_argument("out")
    ap.add_argument("--mask", default="none", help="none, mean or a number T (voxels with x > T), as config.intensity_mask")
    ap.add_argument("--device", default="cuda:0")
    a = ap.parse_args(argv)
    files = sorted(glob.glob(os.path.join(a.dir, "*.npy")))
    if not files:
        raise FileNotFoundError(f"no .npy volumes under {a.dir}")
    mask = a.mask if a.mask in ("none", "mean") else float(a.mask)
    landmarks = train_landmarks(files, mask, a.device)
    np.save(a.out, landmarks)
    print(f"{len(files)} volumes, mask {mask}: landmarks {np.array2string(landmarks, precision=4)} -> {a.out}")
    return landmarks


if __name__ == "__main__":
    main()
