"""CPU model of the renderer's planes (include/igw_render.h: igw_render_aux; DESIGN.md section 8, "Planes"), derived
from a pov_model.render() result and the pose -- not from the kernel's cell walk:

  depth    the model's t (inf for sky)
  surface  block: the hit point e + t d, stepped half a cell against the face's outward normal, rounded to the cell:
           face * 1089 + (y+1)*121 + (x+5)*11 + (z+5); ground: the quad floor(g + 0.5) that contains the point:
           6 * 1089 + (qx+18)*37 + (qz+18); sky: -1
  label    block: the grid's id at that cell, clamped to 1..6; ground: 7 WHITE (|qx|, |qz| <= 5) / 8 GREY; sky: 0

and the bound on the f32 depth ("Planes": depth error), with its constants.
"""
import numpy as np

import pov_model as M

CELLS, GROUND_SPAN = 1089, 37
# outward normal of each face, in the order of pov_model.FACE_NAMES (top, bottom, left, right, front, back)
NORMALS = np.array([(0, 1, 0), (0, -1, 0), (-1, 0, 0), (1, 0, 0), (0, 0, 1), (0, 0, -1)], np.float64)
AXIS = np.array([1, 1, 0, 0, 2, 2])          # the axis of that normal; the ground's is 1
SKY = (np.inf, 0, -1)
U32 = 2.0 ** -24                             # unit roundoff of binary32


def planes(res, pose, grid):
    """(depth f64 [H,W], label int [H,W], surface int [H,W]) of a pov_model.render() result for pose / grid."""
    face, t = res['face'], res['t']
    H, W = face.shape
    e = np.asarray(pose[:3], np.float64)
    d = M.rays(float(pose[3]), float(pose[4]), W, H)
    g = np.asarray(grid).reshape(9, 11, 11).astype(int)
    depth = np.where(face >= 0, t, np.inf)
    label = np.zeros((H, W), int)
    surface = np.full((H, W), -1, int)
    with np.errstate(all='ignore'):
        hit = e + np.where(np.isfinite(depth), depth, 0.0)[..., None] * d
    blk = (face >= 0) & (face < M.GROUND)
    if blk.any():
        n = NORMALS[face[blk]]
        c = np.rint(hit[blk] - 0.5 * n).astype(int)          # the centre of the block behind the face
        x, y, z = c[:, 0] + 5, c[:, 1] + 1, c[:, 2] + 5
        assert (x >= 0).all() and (x <= 10).all() and (y >= 0).all() and (y <= 8).all() and (z >= 0).all() \
            and (z <= 10).all()
        label[blk] = np.clip(g[y, x, z], 1, 6)
        surface[blk] = face[blk] * CELLS + y * 121 + x * 11 + z
    gnd = face == M.GROUND
    if gnd.any():
        qx = np.floor(hit[gnd][:, 0] + 0.5).astype(int)
        qz = np.floor(hit[gnd][:, 2] + 0.5).astype(int)
        label[gnd] = np.where((np.abs(qx) <= 5) & (np.abs(qz) <= 5), 7, 8)
        surface[gnd] = 6 * CELLS + (qx + 18) * GROUND_SPAN + (qz + 18)
    return depth, label, surface


def normal_component(res, pose):
    """|d_n| [H,W]: the ray's component along the normal of the face hit (the ground's is y); nan for sky."""
    face = res['face']
    H, W = face.shape
    d = M.rays(float(pose[3]), float(pose[4]), W, H)
    ax = np.where(face >= M.GROUND, 1, AXIS[np.clip(face, 0, 5)])
    dn = np.abs(np.take_along_axis(d, ax[..., None], -1)[..., 0])
    return np.where(face >= 0, dn, np.nan)


def depth_constants(W, H):
    """(c1, c2) of |dt| <= 2^-24 (c1 t + c2 (1 + t) / |d_n|), from the kernel's operations (DESIGN.md section 8,
    "Planes"): t = ((plane - origin) - p) * (1 / d_n) in f32, one rounding per operation.
      c1 = 3: the subtraction of the eye fraction, the reciprocal and the multiply round once each, relative to t.
      c2 = 6 (2 + W/H) + 1: d_n = (f_n + a r_n) + b u_n with f, r, u rounded from f64 (1 each), a and b products of
      an exact integer and the rounded 1/H, rounded (2 each), two products and two sums (1 each): at most
      2|f_n| + 5|a r_n| + 4|b u_n| + |d_n| <= 6 (|f_n| + |a r_n| + |b u_n|) <= 6 (2 + W/H) units, times t / |d_n|;
      the eye fraction p in [0, 1) is rounded once (1 unit, over |d_n|); the last unit covers the terms of second
      order and the model's own f64 rounding."""
    return 3.0, 6.0 * (2.0 + W / H) + 1.0


def depth_bound(t, dn, W, H):
    c1, c2 = depth_constants(W, H)
    return U32 * (c1 * t + c2 * (1.0 + t) / dn)


# ---- the scenes the GPU tests compare against this model (tests/test_gpu_render_aux.py) ----------------------------
def structure():
    """Every colour on a 3 x 3 base with a tower, an arch and loose blocks: all six faces of every colour can be seen
    from the poses of scenes()."""
    g = np.zeros((9, 11, 11), np.int8)
    g[0, 4:7, 4:7] = 3
    g[1:6, 5, 5] = [1, 2, 4, 5, 6]
    g[2, 2, 2:5] = 2
    g[0:2, 2, 2] = 5
    g[0:2, 2, 4] = 6
    for c in range(1, 7):
        g[c, 8, 1 + c] = c
        g[0, 1 + c, 9] = 7 - c
    return g


def scenes():
    """[(pose, grid)]: eyes inside and outside the build zone, above, level and below, off the lattice (a ray from a
    lattice point through a symmetric pixel meets cell edges exactly, which is the boundary band by definition)."""
    rng = np.random.RandomState(23)
    house = structure()
    dense = (rng.rand(9, 11, 11) < 0.12) * rng.randint(1, 7, (9, 11, 11))
    dense[:, 4:7, 4:7] = 0
    dense = dense.astype(np.int8)
    empty = np.zeros((9, 11, 11), np.int8)
    out = []
    for k in range(6):                       # a ring of outside eyes looking at the structure
        a = np.radians(17 + 60 * k)
        eye = np.array([11.3 * np.cos(a) + 0.0137, 3.2 + 0.7 * k, 11.3 * np.sin(a) - 0.0113])
        v = np.array([0.0, 1.5, 0.0]) - eye
        v /= np.linalg.norm(v)
        out.append(((*eye, np.degrees(np.arctan2(v[0], -v[2])), np.degrees(np.arcsin(v[1]))), house))
    out += [((0.2137, 9.3071, -0.3113, 20.0, -88.0), house),          # straight down on it
            ((3.3137, -1.2929, 3.4887, -40.0, 35.0), house),           # from the floor, looking up: bottom faces
            ((-3.4863, 0.4071, -3.2113, 130.0, 5.0), house),
            ((0.3137, 0.2071, 0.4887, 75.0, -20.0), dense),
            ((-0.4863, 2.6071, 0.2887, -110.0, 10.0), dense),
            ((0.1137, 5.9071, -0.2113, 200.0, -55.0), dense),
            ((14.0137, 6.0071, -13.9887, -45.0, -20.0), dense),        # from beyond the zone, the far edge in frame
            ((3.0137, 2.0071, -4.0113, 45.0, -20.0), empty),
            ((17.5137, 0.5071, 17.4887, 135.0, -10.0), empty),         # at the ground's corner, looking off it
            ((0.0137, -3.0071, 0.0113, 10.0, 60.0), house)]            # below the ground: no ground, blocks from below
    return out
