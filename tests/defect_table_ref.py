"""The numpy reference of the defect table of a resident batch (include/vent_hip.h, "the defect table of
a device-resident batch") on top of components_ref: the rows from its components and ranks, the sums by
np.add.at on int64, the faces by comparing the root map with its six shifts, the signal rule in float32
step by step.  Integers throughout."""
import numpy as np

import components_ref as K

COLS = 18
MAX_ROWS = 1024
F32 = np.float32
FX = F32(16777216.0)                     # 2^24: the fixed-point scale
(ROOT, SIZE, SUM_R, SUM_C, SUM_Z, MIN_R, MAX_R, MIN_C, MAX_C, MIN_Z, MAX_Z, FACES_R, FACES_C, FACES_Z, N_SIG, SUM_FX,
 MIN_FX, MAX_FX) = range(COLS)


def exposed_faces(root):
    """int64 [3][R][C][Z]: per axis, how many of a voxel's two faces normal to it are exposed -- the
    neighbour position lies outside the volume, or the neighbour's root differs from the voxel's."""
    out = np.zeros((3,) + root.shape, np.int64)
    for ax in range(3):
        n = root.shape[ax]
        for step in (-1, 1):
            nb = np.full(root.shape, -2, np.int64)               # -2: outside the volume, no voxel's root
            src = [slice(None)] * 3
            dst = [slice(None)] * 3
            src[ax] = slice(1, n) if step == 1 else slice(0, n - 1)
            dst[ax] = slice(0, n - 1) if step == 1 else slice(1, n)
            nb[tuple(dst)] = root[tuple(src)]
            out[ax] += nb != root
    return out


def signal_fx(x, d):
    """(counted bool, fx int64) of every voxel: nv = float32(x / d); counted when 0 <= nv < 64, and then
    fx = int64(float32(nv * 2^24))."""
    with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
        nv = (np.asarray(x, dtype=F32) / F32(d)).astype(F32)
        ok = (nv >= F32(0)) & (nv < F32(64))
        fx = np.where(ok, (np.where(ok, nv, F32(0)) * FX).astype(F32), F32(0)).astype(np.int64)
    return ok, fx


def full_table(root, roots, sizes, x=None, d=None):
    """int64 [n][18]: the row of every component of one study, in the order of the ranks, from its root
    map (components_ref) and its components in the order of their roots; x, d: the N4 volume and the
    divisor, or None for VH_DT_NO_SIGNAL.  A component's row does not depend on min_size or max_rows:
    they choose a prefix of this table (cut)."""
    n = len(roots)
    rows = np.zeros((n, COLS), np.int64)
    if n == 0:
        return rows
    rank = K.ranks(roots, sizes)
    rows[rank, ROOT] = roots
    rows[rank, SIZE] = sizes
    row_of = np.full(root.size, -1, np.int64)
    row_of[roots] = rank
    on = np.flatnonzero(root.ravel() >= 0)
    j = row_of[root.ravel()[on]]
    r, c, z = np.unravel_index(on, root.shape)
    big = np.iinfo(np.int64).max
    for s, lo, hi, v in ((SUM_R, MIN_R, MAX_R, r), (SUM_C, MIN_C, MAX_C, c), (SUM_Z, MIN_Z, MAX_Z, z)):
        v = v.astype(np.int64)
        np.add.at(rows[:, s], j, v)
        rows[:, lo] = big
        np.minimum.at(rows[:, lo], j, v)
        np.maximum.at(rows[:, hi], j, v)
    faces = exposed_faces(root)
    for ax, col in enumerate((FACES_R, FACES_C, FACES_Z)):
        np.add.at(rows[:, col], j, faces[ax].ravel()[on])
    if x is not None:
        ok, fx = signal_fx(np.asarray(x).ravel()[on], d)
        jo, fo = j[ok], fx[ok]
        np.add.at(rows[:, N_SIG], jo, 1)
        np.add.at(rows[:, SUM_FX], jo, fo)
        m = np.full(n, big, np.int64)
        np.minimum.at(m, jo, fo)
        rows[:, MIN_FX] = np.where(rows[:, N_SIG] > 0, m, 0)
        np.maximum.at(rows[:, MAX_FX], jo, fo)
    return rows


def cut(full, min_size, max_rows):
    """(rows int64 [max_rows][18], stats int64 [4]) from full_table's rows: the qualifying components
    are a prefix of the rank order, the rows its first max_rows; an unused row is -1 and zeros."""
    rows = np.zeros((max_rows, COLS), np.int64)
    rows[:, ROOT] = -1
    qual = full[:, SIZE] >= min_size
    n_qual = int(qual.sum())
    assert qual[:n_qual].all()                                   # a prefix: the ranks descend in size
    n_rows = min(n_qual, max_rows)
    rows[:n_rows] = full[:n_rows]
    return rows, np.array([n_rows, n_qual, full[:n_rows, SIZE].sum(), full[:n_qual, SIZE].sum()], np.int64)


def table(root, roots, sizes, min_size, max_rows, x=None, d=None):
    """(rows, stats) of one study: cut(full_table(...))."""
    return cut(full_table(root, roots, sizes, x, d), min_size, max_rows)


def batch_tables(vols, conn, x=None, d=None):
    """[full_table] of byte volumes; x [B][R][C][Z] and d [B], or None."""
    out = []
    for q in range(len(vols)):
        root, _, roots, sizes = K.components(vols[q], conn)
        out.append(full_table(root, roots, sizes, None if x is None else x[q], None if x is None else d[q]))
    return out


def cut_batch(fulls, min_size, max_rows):
    """dict(rows int64 [B][max_rows][18], stats int64 [B][4], truncated bool [B]) from batch_tables';
    min_size a scalar or one value per study."""
    ms = np.broadcast_to(np.asarray(min_size), (len(fulls),))
    out = [cut(f, int(m), max_rows) for f, m in zip(fulls, ms)]
    stats = np.stack([o[1] for o in out])
    return dict(rows=np.stack([o[0] for o in out]), stats=stats, truncated=stats[:, 0] < stats[:, 1])


def reference(vols, conn, min_size, max_rows, x=None, d=None):
    """cut_batch(batch_tables(...)): the table of a batch of byte volumes."""
    return cut_batch(batch_tables(vols, conn, x, d), min_size, max_rows)


def brute_force(root, size, min_size, max_rows):
    """The same table by a plain loop over the voxels of components_ref.bfs_components' maps (root,
    size): what the host test holds the vectorised reference against, on small volumes."""
    R, C, Z = root.shape
    comps = sorted({(int(size[p]), int(root[p])) for p in zip(*np.nonzero(root >= 0))}, key=lambda t: (-t[0], t[1]))
    qual = [t for t in comps if t[0] >= min_size]
    rows = np.zeros((max_rows, COLS), np.int64)
    rows[:, ROOT] = -1
    kept = qual[:max_rows]
    stats = np.array([len(kept), len(qual), sum(t[0] for t in kept), sum(t[0] for t in qual)], np.int64)
    row_of = {t[1]: j for j, t in enumerate(kept)}
    for j, t in enumerate(kept):
        rows[j, ROOT], rows[j, SIZE] = t[1], t[0]
        rows[j, [MIN_R, MIN_C, MIN_Z]] = max(R, C, Z)
    for r in range(R):
        for c in range(C):
            for z in range(Z):
                j = row_of.get(int(root[r, c, z]), -1) if root[r, c, z] >= 0 else -1
                if j < 0:
                    continue
                me = root[r, c, z]
                row = rows[j]
                row[SUM_R] += r; row[SUM_C] += c; row[SUM_Z] += z
                row[MIN_R] = min(row[MIN_R], r); row[MAX_R] = max(row[MAX_R], r)
                row[MIN_C] = min(row[MIN_C], c); row[MAX_C] = max(row[MAX_C], c)
                row[MIN_Z] = min(row[MIN_Z], z); row[MAX_Z] = max(row[MAX_Z], z)
                for col, (dr, dc, dz) in ((FACES_R, (1, 0, 0)), (FACES_C, (0, 1, 0)), (FACES_Z, (0, 0, 1))):
                    for s in (-1, 1):
                        p = (r + s * dr, c + s * dc, z + s * dz)
                        inside = 0 <= p[0] < R and 0 <= p[1] < C and 0 <= p[2] < Z
                        row[col] += (not inside) or root[p] != me
    return rows, stats
