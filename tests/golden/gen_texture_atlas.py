#!/usr/bin/env python3
"""The reference's texture atlas as plain data for the GPU box: gridworld/texture.png (128 x 128 RGBA, the file its
pyglet Renderer binds, gridworld/render.py:56-73) decoded with PIL to uint8 [128, 128, 4], row 0 = the top image row.
Writes tests/golden/texture_atlas.npz (key `atlas`).  Build container only (needs the reference tree)."""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import ref_harness as H  # noqa: E402


def main():
    from PIL import Image
    png = os.path.join(H.REFERENCE_ROOT, 'gridworld', 'texture.png')
    with Image.open(png) as im:
        atlas = np.asarray(im.convert('RGBA'), dtype=np.uint8)
    assert atlas.shape == (128, 128, 4), atlas.shape
    path = os.path.join(HERE, 'texture_atlas.npz')
    np.savez_compressed(path, atlas=atlas)
    print('texture_atlas: %s from %s -> %d B' % (atlas.shape, png, os.path.getsize(path)))


if __name__ == '__main__':
    main()
