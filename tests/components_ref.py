"""The numpy / scipy reference of the connected components of a resident batch (include/vent_hip.h,
"the connected components of a device-resident batch"): scipy.ndimage.label under the four
neighbourhoods (4 and 8 slice by slice), the sizes by np.bincount, the roots -- the smallest linear
index of each component -- by np.minimum.at, the size classes, the summary and the rank rule of the
filter; and the seeded inputs the host and GPU tests share.  Integers throughout."""
import functools

import numpy as np
from scipy import ndimage as ndi

CONNS = (4, 8, 6, 26)
# (2, 2, 1) is the smallest volume a batch takes; (41, 37, 9) partial tiles; (64, 64, 24) whole tiles;
# (130, 70, 3) several tiles both ways with a remainder; (8, 8, 70) three tiles along Z, the last partial;
# (300, 280, 2) many thin tiles
SHAPES = [(2, 2, 1), (5, 3, 1), (41, 37, 9), (64, 64, 24), (130, 70, 3), (8, 8, 70), (300, 280, 2)]
EDGE_SETS = [(), (2,), (2, 5, 10, 100, 1000)]
TILE = (16, 16, 24)          # the kernels' tile: the tests assert that components span more than one
N_STUDIES = 8
EMPTY, FULL, CHECKER, RAND40, RAND60, SERPENTINE, BRIDGE, DIAGONAL = range(N_STUDIES)


def structure(conn):
    """The 3 x 3 x 3 structuring element of scipy.ndimage.label for 6 and 26, 3 x 3 for 4 and 8."""
    return ndi.generate_binary_structure(3 if conn in (6, 26) else 2, 1 if conn in (4, 6) else 3 if conn == 26 else 2)


def label_volume(S, conn):
    """(labels int64 [R][C][Z] with 0 off S and 1..n on it, n): scipy's labels; 4 and 8 slice by slice."""
    S = np.asarray(S) != 0
    if conn in (6, 26):
        lab, n = ndi.label(S, structure(conn))
        return lab.astype(np.int64), int(n)
    lab = np.zeros(S.shape, np.int64)
    n = 0
    for z in range(S.shape[2]):
        l, k = ndi.label(S[:, :, z], structure(conn))
        lab[:, :, z] = np.where(l > 0, l + n, 0)
        n += int(k)
    return lab, n


def components(a, conn):
    """(root int32 [R][C][Z], size uint32 [R][C][Z], roots int64 [n], sizes int64 [n]) of one volume:
    the per-voxel maps and the components in the order of their roots."""
    lab, n = label_volume(a, conn)
    flat = lab.ravel()
    sizes = np.bincount(flat, minlength=n + 1)
    roots = np.full(n + 1, flat.size, np.int64)
    np.minimum.at(roots, flat, np.arange(flat.size, dtype=np.int64))
    roots[0], sizes[0] = -1, 0
    root = roots[lab].astype(np.int32)
    size = sizes[lab].astype(np.uint32)
    order = np.argsort(roots[1:])
    return root, size, roots[1:][order], sizes[1:][order].astype(np.int64)


def summary(roots, sizes, edges):
    """(counts int64 [len(edges) + 1][2], stats int64 [4]) from the components of one study."""
    e = np.asarray(edges, dtype=np.int64)
    cls = np.searchsorted(e, sizes, side='right')
    counts = np.zeros((len(e) + 1, 2), np.int64)
    counts[:, 0] = np.bincount(cls, minlength=len(e) + 1)
    counts[:, 1] = np.bincount(cls, weights=sizes, minlength=len(e) + 1).astype(np.int64)
    if len(sizes) == 0:
        return counts, np.array([0, 0, 0, -1], np.int64)
    big = int(np.flatnonzero(sizes == sizes.max())[0])           # roots ascend: the first is the smaller root
    return counts, np.array([sizes.sum(), len(sizes), sizes[big], roots[big]], np.int64)


def reference(vols, conn, edges):
    """dict(root int32 [B][R][C][Z], size uint32, counts int64 [B][classes][2], stats int64 [B][4])."""
    out = [components(a, conn) for a in vols]
    cs = [summary(o[2], o[3], edges) for o in out]
    return dict(root=np.stack([o[0] for o in out]), size=np.stack([o[1] for o in out]),
                counts=np.stack([c[0] for c in cs]), stats=np.stack([c[1] for c in cs]))


def ranks(roots, sizes):
    """int64 [n]: the number of components with a greater key (size, -root)."""
    order = np.lexsort((roots, -sizes))                           # size descending, then root ascending
    r = np.empty(len(sizes), np.int64)
    r[order] = np.arange(len(sizes))
    return r


def filter_volume(a, conn, min_size, keep_largest):
    """(out, components kept, voxels kept): ``a`` with the voxels of every component below min_size, or
    of rank >= keep_largest > 0, cleared; a kept voxel keeps its value."""
    a = np.asarray(a)
    root, size, roots, sizes = components(a, conn)
    keep = sizes >= min_size
    if keep_largest > 0:
        keep &= ranks(roots, sizes) < keep_largest
    stays = np.isin(root, roots[keep]) & (root >= 0)
    return np.where(stays, a, 0).astype(a.dtype), int(keep.sum()), int(sizes[keep].sum())


def filter_reference(vols, conn, min_size, keep_largest):
    """(out [B][R][C][Z], kept int64 [B][2]); min_size and keep_largest scalars or one value per study."""
    n = len(vols)
    ms = np.broadcast_to(np.asarray(min_size), (n,))
    kl = np.broadcast_to(np.asarray(keep_largest), (n,))
    res = [filter_volume(vols[q], conn, int(ms[q]), int(kl[q])) for q in range(n)]
    return np.stack([r[0] for r in res]), np.array([[r[1], r[2]] for r in res], np.int64)


def bfs_components(a, conn):
    """(root int32, size uint32) by a plain breadth-first search over the definition's offsets: what the
    host test holds scipy's labels against, on small volumes."""
    S = np.asarray(a) != 0
    R, C, Z = S.shape
    offs = [(dr, dc, dz) for dr in (-1, 0, 1) for dc in (-1, 0, 1) for dz in (-1, 0, 1)
            if (dr, dc, dz) != (0, 0, 0) and (dz == 0 or conn in (6, 26))
            and (conn in (8, 26) or abs(dr) + abs(dc) + abs(dz) == 1)]
    root = np.full(S.shape, -1, np.int32)
    size = np.zeros(S.shape, np.uint32)
    for start in np.argwhere(S):                                 # in index order: the start is the root
        if root[tuple(start)] >= 0:
            continue
        r0 = int((start[0] * C + start[1]) * Z + start[2])
        todo, members = [tuple(start)], [tuple(start)]
        root[tuple(start)] = r0
        while todo:
            r, c, z = todo.pop()
            for dr, dc, dz in offs:
                p = (r + dr, c + dc, z + dz)
                if 0 <= p[0] < R and 0 <= p[1] < C and 0 <= p[2] < Z and S[p] and root[p] < 0:
                    root[p] = r0
                    todo.append(p)
                    members.append(p)
        size[tuple(np.array(members).T)] = len(members)
    return root, size


def serpentine(shape):
    """bool [R][C][Z], the same on every slice: the even rows whole, joined at alternating ends on the
    odd rows -- one one-pixel corridor through every tile of the plane, the chain that needs the most
    merge steps."""
    R, C, Z = shape
    s = np.zeros((R, C), bool)
    s[0::2] = True
    for i, r in enumerate(range(1, R - 1, 2)):
        s[r, C - 1 if i % 2 == 0 else 0] = True
    return np.repeat(s[:, :, None], Z, axis=2)


@functools.lru_cache(maxsize=None)
def batch_inputs(shape):
    """uint8 [8][R][C][Z], read-only: empty; all ones; the in-plane checkerboard; seeded fills of
    density 0.4 and 0.6 (ragged clusters around the 4-connected percolation point) in values 1 / 2 /
    255; the serpentine; BRIDGE, rows 0 and R - 1 of slice 0 whole and column 0 of slice 1 whole -- two
    parts that join only through another slice; DIAGONAL, one-voxel lines that hold together by
    diagonal steps only: r = c in slice 0 and r = C - 1 - c in the last slice, both over tile corners,
    and (i, i, 20 + i), over the corner of two tiles along Z; and a lone voxel at (0, C / 2, Z / 2)."""
    R, C, Z = shape
    rng = np.random.default_rng(4391 + int(np.prod(shape)))
    a = np.zeros((N_STUDIES,) + tuple(shape), np.uint8)
    a[FULL] = 1
    rr, cc = np.mgrid[0:R, 0:C]
    a[CHECKER] = (((rr + cc) % 2) == 0)[:, :, None]
    vals = np.array([1, 2, 255], np.uint8)
    for q, p in ((RAND40, 0.4), (RAND60, 0.6)):
        a[q] = (rng.random(shape) < p) * vals[rng.integers(0, 3, shape)]
    a[SERPENTINE] = serpentine(shape) * 3
    a[BRIDGE, 0, :, 0] = 1
    a[BRIDGE, R - 1, :, 0] = 2
    if Z > 1:
        a[BRIDGE, :, 0, 1] = 255
    k = np.arange(min(R, C))
    a[DIAGONAL, k, k, 0] = 1
    a[DIAGONAL, k, C - 1 - k, Z - 1] = 7
    i = np.arange(max(0, min(R, C, Z - 20)))
    a[DIAGONAL, i, i, 20 + i] = 9
    a[DIAGONAL, 0, C // 2, Z // 2] = 5
    a.setflags(write=False)
    return a


@functools.lru_cache(maxsize=None)
def batch_reference(shape, conn, edges=()):
    out = reference(batch_inputs(shape), conn, edges)
    for v in out.values():
        v.setflags(write=False)
    return out


def tiles_spanned(root, q_root):
    """The number of kernel tiles the component of linear root q_root touches (one study's root map)."""
    p = np.argwhere(root == q_root)
    return len({(r // TILE[0], c // TILE[1], z // TILE[2]) for r, c, z in p})
