"""CPU model of the first-person frame contract ("First-person frames"), in float64.

A deliberately different algorithm from the HIP kernel's cell walk: brute force over every quad of the scene.  Each
face of each present block is a quad given by its four corners in the vertex order of the reference's cube_vertices
and the texture corners (0,0) (1,0) (1,1) (0,1) of tex_coord; its front side follows from the winding (GL's
counter-clockwise front faces).  Per pixel ray: plane hit, inside-rectangle test, back-face test, 0.1 <= t <= 30,
nearest wins, then u / v from the quad's own edge vectors and the texel.  The ground is the 37 x 37 top-only quads at
y = -1.5; one plane hit locates the quad that contains the point (they tile the plane), which is that brute force
with the rectangle test done by rounding.

Besides the frame it returns per-pixel MARGINS: how far the answer is from changing -- distance (in texels) to the
nearest texel boundary of the hit, and (in world units) to the edge of any quad that could win, to the second-nearest
hit and to the near / far limits.  A pixel whose margins are >= TEXEL_BAND / WORLD_BAND is "clean": an f32 renderer
must reproduce it exactly.
"""
import numpy as np

CLEAR = np.array([128, 176, 255, 255], np.uint8)
NEAR, FAR = 0.1, 30.0
TEXEL_BAND, WORLD_BAND = 1e-3, 1e-4

# face name -> (corner offsets v0..v3 in units of the half size, sub-tile (column, row) in eighths of the atlas)
FACES = {
    'top': ([(-1, 1, -1), (-1, 1, 1), (1, 1, 1), (1, 1, -1)], (0, 1)),
    'bottom': ([(-1, -1, -1), (1, -1, -1), (1, -1, 1), (-1, -1, 1)], (1, 0)),
    'left': ([(-1, -1, -1), (-1, -1, 1), (-1, 1, 1), (-1, 1, -1)], (0, 0)),
    'right': ([(1, -1, 1), (1, -1, -1), (1, 1, -1), (1, 1, 1)], (0, 0)),
    'front': ([(-1, -1, 1), (1, -1, 1), (1, 1, 1), (-1, 1, 1)], (1, 1)),
    'back': ([(1, -1, -1), (-1, -1, -1), (-1, 1, -1), (1, 1, -1)], (1, 1)),
}
FACE_NAMES = list(FACES)
GROUND = len(FACE_NAMES)          # face code of the ground; -1 = sky
# atlas tile (column, row from the bottom) of each texture id (WHITE -1, GREY 0, BLUE 1 .. YELLOW 6)
TILES = {-1: (0, 0), 0: (1, 0), 1: (2, 0), 2: (3, 0), 3: (0, 1), 4: (1, 1), 5: (2, 1), 6: (3, 1)}


def basis(yaw, pitch):
    """forward, right, up of the camera for yaw / pitch in degrees (get_sight_vector is forward)."""
    y, p = np.radians(yaw), np.radians(pitch)
    f = np.array([np.sin(y) * np.cos(p), np.sin(p), -np.cos(y) * np.cos(p)])
    r = np.array([np.cos(y), 0.0, np.sin(y)])
    u = np.array([-np.sin(y) * np.sin(p), np.cos(p), np.cos(y) * np.sin(p)])
    return f, r, u


def rays(yaw, pitch, W, H):
    """[H, W, 3] ray directions whose parameter is the eye-space depth; row 0 is the top image row."""
    f, r, u = basis(yaw, pitch)
    a = ((2 * np.arange(W) + 1) / W - 1) * (W / H)
    b = 1 - (2 * np.arange(H) + 1) / H
    return f + a[None, :, None] * r + b[:, None, None] * u


def block_quads(grid):
    """Every face of every present block: corner v0 [Q,3], edges e1 = v1 - v0, e2 = v3 - v0, the texel origin of
    its sub-tile (column, row from the bottom, in units of the sub-tile) and its face code."""
    g = np.asarray(grid).reshape(9, 11, 11)
    cy, cx, cz = np.nonzero(g)
    v0s, e1s, e2s, tile, code = [], [], [], [], []
    for k, (name, (corners, (su, sv))) in enumerate(FACES.items()):
        c = 0.5 * np.array(corners, np.float64)
        centre = np.stack([cx - 5.0, cy - 1.0, cz - 5.0], 1)
        v0s.append(centre + c[0])
        e1s.append(np.broadcast_to(c[1] - c[0], centre.shape))
        e2s.append(np.broadcast_to(c[3] - c[0], centre.shape))
        ids = g[cy, cx, cz].astype(int)
        tx = np.array([TILES[i][0] for i in ids]).reshape(-1)
        ty = np.array([TILES[i][1] for i in ids]).reshape(-1)
        tile.append(np.stack([2 * tx + su, 2 * ty + sv], 1))
        code.append(np.full(len(ids), k))
    return (np.concatenate(v0s), np.concatenate(e1s), np.concatenate(e2s), np.concatenate(tile),
            np.concatenate(code))


def render(pose, grid, atlas, W, H, channels=3):
    """pose (x, y, z, yaw, pitch) float64, grid [9,11,11] ids, atlas uint8 [S,S,4] (row 0 = top).  Returns dict:
    image uint8 [H,W,channels], face [H,W] (-1 sky, 0..5 FACE_NAMES, 6 ground), t [H,W], texel (col, row-from-bottom)
    [H,W,2], margin_texel and margin_world [H,W] (inf where nothing bounds them)."""
    with np.errstate(all='ignore'):   # rays parallel to a plane: inf / nan, masked below
        return _render(pose, grid, atlas, W, H, channels)


def _render(pose, grid, atlas, W, H, channels):
    x, y, z, yaw, pitch = [float(v) for v in pose]
    e = np.array([x, y, z])
    S = atlas.shape[0]
    sub = S // 8
    d = rays(yaw, pitch, W, H).reshape(-1, 3)
    P = d.shape[0]
    best_t = np.full(P, np.inf)
    face = np.full(P, -1)
    texel = np.zeros((P, 2), int)
    m_tex = np.full(P, np.inf)
    cand_edge, cand_t = [], []          # per candidate quad group: edge distance / t arrays [P, q]
    uv_best = np.zeros((P, 2))
    tsz = np.zeros(P, int)
    torg = np.zeros((P, 2), int)

    v0, e1, e2, tile, code = block_quads(grid)
    if len(v0):
        n = np.cross(e1, e2)                                           # outward normal by the winding
        front = ((e - v0) * n).sum(1) > 0                              # back-face culling
        v0, e1, e2, tile, code, n = v0[front], e1[front], e2[front], tile[front], code[front], n[front]
    if len(v0):
        dn = d @ n.T                                                   # [P, Q]
        t = ((v0 - e) * n).sum(1)[None, :] / dn
        t = np.where(dn < 0, t, np.inf)                                # the ray must travel into the front side
        p = e[None, None, :] + t[..., None] * d[:, None, :]            # [P, Q, 3]
        rel = p - v0[None]
        u = np.where(np.isfinite(t), (rel * e1[None]).sum(2), -1.0)    # edges are unit vectors
        v = np.where(np.isfinite(t), (rel * e2[None]).sum(2), -1.0)
        edge = np.minimum(np.minimum(u, 1 - u), np.minimum(v, 1 - v))  # >= 0 inside the rectangle
        inside = edge >= 0
        valid = inside & (t >= NEAR) & (t <= FAR)
        tv = np.where(valid, t, np.inf)
        k = np.argmin(tv, 1)
        hit = np.isfinite(tv[np.arange(P), k])
        best_t = np.where(hit, tv[np.arange(P), k], np.inf)
        face = np.where(hit, code[k], -1)
        uv_best = np.stack([u[np.arange(P), k], v[np.arange(P), k]], 1)
        torg = tile[k] * sub
        tsz[:] = sub
        cand_edge.append(np.where(np.isfinite(t), edge, np.inf))
        cand_t.append(np.where(inside, t, np.inf))

    # the ground: top faces of the quads centred on x, z in [-18, 18], y = -1.5 (front side up)
    if y > -1.5:
        tg = np.where(d[:, 1] < 0, (-1.5 - y) / d[:, 1], np.inf)
        gx, gz = x + tg * d[:, 0], z + tg * d[:, 2]
        qx, qz = np.floor(gx + 0.5), np.floor(gz + 0.5)               # the quad containing the point
        ginside = np.isfinite(tg) & (np.abs(qx) <= 18) & (np.abs(qz) <= 18)
        # top face corners: v0 = (qx-.5, qz-.5), e1 = +z, e2 = +x -> u = z - (qz - .5), v = x - (qx - .5)
        gu, gv = gz - (qz - 0.5), gx - (qx - 0.5)
        gedge = np.where(np.isfinite(tg), np.minimum(np.minimum(gu, 1 - gu), np.minimum(gv, 1 - gv)), np.inf)
        # outside the 37 x 37 quads: the distance to the outer edge
        out = np.maximum(np.abs(gx), np.abs(gz)) - 18.5
        gedge = np.where(ginside, gedge, np.where(np.isfinite(tg), np.abs(out), np.inf))
        gvalid = ginside & (tg >= NEAR) & (tg <= FAR) & (tg < best_t)
        white = (np.abs(qx) <= 5) & (np.abs(qz) <= 5)
        best_t = np.where(gvalid, tg, best_t)
        face = np.where(gvalid, GROUND, face)
        uv_best = np.where(gvalid[:, None], np.stack([gu, gv], 1), uv_best)
        torg = np.where(gvalid[:, None], np.stack([np.where(white, 0, 2 * sub), np.zeros(P, int)], 1), torg)
        tsz = np.where(gvalid, 2 * sub, tsz)
        cand_edge.append(gedge[:, None])
        cand_t.append(np.where(ginside, tg, np.inf)[:, None])

    hit = face >= 0
    # texel: GL_NEAREST on the quad's tile
    fu, fv = uv_best[:, 0] * tsz, uv_best[:, 1] * tsz
    col = torg[:, 0] + np.clip(np.floor(fu), 0, np.maximum(tsz - 1, 0)).astype(int)
    rowb = torg[:, 1] + np.clip(np.floor(fv), 0, np.maximum(tsz - 1, 0)).astype(int)
    texel = np.stack([col, rowb], 1)
    dist = lambda a: np.abs(a - np.round(a))  # noqa: E731
    m_tex = np.where(hit, np.minimum(dist(fu), dist(fv)), np.inf)

    # world margin: any quad that could win (hit point on / near its rectangle with t up to the winner's), the
    # second-nearest hit, and the near / far limits of every rectangle hit
    m_world = np.full(P, np.inf)
    lim = np.where(hit, best_t, FAR) + 1e-3
    for ed, ct in zip(cand_edge, cand_t):
        m_world = np.minimum(m_world, np.where(np.isfinite(ct) & (ct <= lim[:, None]), np.abs(ct - NEAR), np.inf).min(1))
        m_world = np.minimum(m_world, np.where(np.isfinite(ct), np.abs(ct - FAR), np.inf).min(1))
        other = np.where(np.isfinite(ct) & (ct >= NEAR) & (ct <= FAR) & (np.abs(ct - best_t[:, None]) > 0),
                         np.abs(ct - best_t[:, None]), np.inf)
        m_world = np.minimum(m_world, other.min(1))
    # rectangle edges: every quad whose plane is hit in [NEAR - band, winner's t (or FAR) + band]
    if len(v0):
        ed = cand_edge[0]
        tq = np.where(dn < 0, t, np.inf)
        near_enough = (tq >= NEAR - 1e-3) & (tq <= lim[:, None])
        m_world = np.minimum(m_world, np.where(near_enough, np.abs(ed), np.inf).min(1))
    if y > -1.5:
        ged = cand_edge[-1][:, 0]
        near_enough = (tg >= NEAR - 1e-3) & (tg <= lim)
        m_world = np.minimum(m_world, np.where(near_enough, np.abs(ged), np.inf))

    img = np.empty((P, 4), np.uint8)
    img[:] = CLEAR
    img[hit] = atlas[S - 1 - rowb[hit], col[hit]]
    return {'image': img.reshape(H, W, 4)[..., :channels], 'face': face.reshape(H, W), 't': best_t.reshape(H, W),
            'texel': texel.reshape(H, W, 2), 'margin_texel': m_tex.reshape(H, W), 'margin_world': m_world.reshape(H, W)}


def clean(res):
    """Pixels an f32 renderer must reproduce exactly."""
    return (res['margin_texel'] >= TEXEL_BAND) & (res['margin_world'] >= WORLD_BAND)


def compare(frame, res):
    """(mismatches among clean pixels, mismatches in the boundary band, pixels compared)."""
    frame = np.asarray(frame)
    bad = (frame != res['image']).any(-1)
    c = clean(res)
    return int((bad & c).sum()), int((bad & ~c).sum()), int(bad.size)


def pose_of_agent(agent_rows):
    """[n, 64] uint8 agent records (include/igw.h) -> [n, 5] float64 x, y, z, yaw, pitch."""
    f = np.ascontiguousarray(agent_rows)[:, :40].view(np.float64)
    return f[:, :5]


def coded_atlas(side=128):
    """An atlas whose texel (col, row-from-bottom) has RGB = (col, row-from-bottom, 255 - col ^ row): a frame decodes
    to the texel each pixel sampled, so a wrong face, sub-tile or orientation shows as a wrong coordinate."""
    col = np.arange(side)[None, :].repeat(side, 0)
    rowb = (side - 1 - np.arange(side))[:, None].repeat(side, 1)
    a = np.empty((side, side, 4), np.uint8)
    a[..., 0], a[..., 1] = col, rowb
    a[..., 2] = 255 - (col ^ rowb)
    a[..., 3] = 255
    return a


def decode(frame):
    """(col, row-from-bottom) per pixel of a frame rendered with coded_atlas; (-1, -1) for the clear colour."""
    f = np.asarray(frame).astype(int)
    sky = (f[..., :3] == CLEAR[:3]).all(-1) & ((255 - (f[..., 0] ^ f[..., 1])) != f[..., 2])
    out = np.stack([f[..., 0], f[..., 1]], -1)
    out[sky] = -1
    return out


def shade(res, atlas, channels=3):
    """The frame of a render() result with another atlas of the same side (the geometry does not depend on it)."""
    S = atlas.shape[0]
    col, rowb = res['texel'][..., 0], res['texel'][..., 1]
    img = np.empty(res['face'].shape + (4,), np.uint8)
    img[:] = CLEAR
    hit = res['face'] >= 0
    img[hit] = atlas[S - 1 - rowb[hit], col[hit]]
    return dict(res, image=img[..., :channels])
