"""Numpy restatement of the surface-nets rules (include/radnerf.h,
rn_surface_count), vectorised and fp32 throughout, a mesh checker, and the
analytic lattices the mesh tests share.

A lattice is sigma (nz + 1, ny + 1, nx + 1) fp32, x fastest; lo and step are
3 fp32 each.  surface_nets(sigma, iso, lo, step) -> vertices (V, 3) f32, faces
(F, 3) i32, normals (V, 3) f32.
"""
import numpy as np

F32 = np.float32


def box_step(lo, hi, res):
    """lo, step as the product forms them: step = (hi - lo) / n in fp32"""
    lo, hi = np.asarray(lo, F32).reshape(3), np.asarray(hi, F32).reshape(3)
    return lo, ((hi - lo) / np.asarray(res, F32)).astype(F32)


def lattice_points(lo, step, res):
    """world x, y, z of every lattice point, (nz + 1, ny + 1, nx + 1) each:
    lo + float32(i) * step"""
    ax = [(lo[d] + np.arange(res[d] + 1, dtype=F32) * step[d]).astype(F32) for d in range(3)]
    z, y, x = np.meshgrid(ax[2], ax[1], ax[0], indexing="ij")
    return x, y, z


def surface_nets(sigma, iso, lo, step):
    sigma = np.ascontiguousarray(sigma, F32)
    iso = F32(iso)
    lo, step = np.asarray(lo, F32), np.asarray(step, F32)
    pz, py, px = sigma.shape
    nz, ny, nx = pz - 1, py - 1, px - 1
    with np.errstate(all="ignore"):
        inside = sigma >= iso                                   # NaN: outside
        # ---- cells: corner q at offset (q & 1, q >> 1 & 1, q >> 2 & 1)
        off = [(q & 1, q >> 1 & 1, q >> 2 & 1) for q in range(8)]
        cin = np.stack([inside[dz:dz + nz, dy:dy + ny, dx:dx + nx] for dx, dy, dz in off], -1)
        active = cin.any(-1) & ~cin.all(-1)                    # (nz, ny, nx): ascending c
        ids = (np.cumsum(active.ravel()) - 1).reshape(active.shape)
        ids = np.where(active, ids, -1)
        k, j, i = np.nonzero(active)
        V = len(i)
        S = np.stack([sigma[k + dz, j + dy, i + dx] for dx, dy, dz in off], -1)      # (V, 8)
        tot = np.zeros((V, 3), F32)
        cnt = np.zeros(V, F32)
        g = np.zeros((V, 3), F32)
        for a in range(3):
            r0, r1 = [d for d in range(3) if d != a]           # lower, higher remaining axis
            for e in range(4):
                q0 = ((e & 1) << r0) | ((e >> 1) << r1)
                q1 = q0 | (1 << a)
                s0, s1 = S[:, q0], S[:, q1]
                g[:, a] = g[:, a] + (s1 - s0)
                cross = (s0 >= iso) != (s1 >= iso)
                t = (iso - s0) / (s1 - s0)
                t = np.fmin(np.fmax(t, F32(0)), F32(1))         # NaN -> 0
                pt = np.zeros((V, 3), F32)
                pt[:, a] = t
                pt[:, r0] = F32(e & 1)
                pt[:, r1] = F32(e >> 1)
                tot = np.where(cross[:, None], tot + pt, tot)
                cnt = np.where(cross, cnt + F32(1), cnt)
        cell = np.stack([i, j, k], 1).astype(F32)
        pos = cell + tot / cnt[:, None]
        vertices = (lo[None, :] + pos * step[None, :]).astype(F32)
        nrm = np.sqrt((g[:, 0] * g[:, 0] + g[:, 1] * g[:, 1]) + g[:, 2] * g[:, 2])
        ok = np.isfinite(g).all(1) & (nrm > 0)
        normals = np.where(ok[:, None], -g / nrm[:, None], F32(0)).astype(F32)
        # ---- faces: edge from point P along a, ordered by 3 p + a
        n = (nx, ny, nz)
        P = np.stack(np.meshgrid(np.arange(px), np.arange(py), np.arange(pz), indexing="ij"), -1)
        P = P.transpose(2, 1, 0, 3)                            # [pk, pj, pi] -> (pi, pj, pk)
        emit = np.zeros((pz, py, px, 3), bool)
        for a in range(3):
            b, c = (a + 1) % 3, (a + 2) % 3
            nxt = np.roll(inside, -1, axis=2 - a)              # inside[P + e_a] where P_a < n_a
            emit[..., a] = ((inside != nxt) & (P[..., a] <= n[a] - 1)
                            & (P[..., b] >= 1) & (P[..., b] <= n[b] - 1)
                            & (P[..., c] >= 1) & (P[..., c] <= n[c] - 1))
        keys = np.nonzero(emit.ravel())[0]                     # ascending 3 p + a
        p, a = keys // 3, keys % 3
        Pq = P.reshape(-1, 3)[p]
        b, c = (a + 1) % 3, (a + 2) % 3
        rows = np.arange(len(keys))
        corner = []
        for ob, oc in ((-1, -1), (0, -1), (0, 0), (-1, 0)):
            C = Pq.copy()
            C[rows, b] += ob
            C[rows, c] += oc
            corner.append(ids[C[:, 2], C[:, 1], C[:, 0]])
        v0, v1, v2, v3 = corner
        pin = inside.ravel()[p]
        q1, q3 = np.where(pin, v1, v3), np.where(pin, v3, v1)
        faces = np.stack([v0, q1, v2, v0, v2, q3], 1).reshape(-1, 3).astype(np.int32)
    return vertices, faces, normals


def check_mesh(vertices, faces):
    """-> dict(edges_once, closed, euler, volume): every directed edge occurs
    once; closed: every directed edge's reverse occurs too; V - E + F over the
    referenced vertices; the signed volume (positive: outward faces)."""
    f = np.asarray(faces, np.int64)
    if len(f) == 0:
        return dict(edges_once=True, closed=True, euler=0, volume=0.0)
    d = np.concatenate([f[:, [0, 1]], f[:, [1, 2]], f[:, [2, 0]]])
    m = int(f.max()) + 1
    key, rev = d[:, 0] * m + d[:, 1], d[:, 1] * m + d[:, 0]
    once = len(np.unique(key)) == len(key)
    closed = bool(np.isin(rev, key).all())
    und = np.unique(np.minimum(d[:, 0], d[:, 1]) * m + np.maximum(d[:, 0], d[:, 1]))
    v = np.asarray(vertices, np.float64)
    vol = float(np.einsum("ij,ij->i", v[f[:, 0]], np.cross(v[f[:, 1]], v[f[:, 2]])).sum() / 6.0)
    return dict(edges_once=bool(once), closed=closed,
                euler=int(len(np.unique(f)) - len(und) + len(f)), volume=vol)


# ---- the analytic lattices: each builder -> sigma, lo, step, hi ------------------------
UNIT = ((-1.0, -1.0, -1.0), (1.0, 1.0, 1.0))
SPHERE_C, SPHERE_R = (0.07, -0.11, 0.05), 0.6
SPHERE_ISO = float(F32(20.0) * np.exp(F32(-3.0)))


def sphere(n):
    """s = 20 exp(-3 (r / R)^2) round SPHERE_C on [-1, 1]^3, n^3 cells; the
    level SPHERE_ISO is the sphere of radius R"""
    lo, step = box_step(*UNIT, (n,) * 3)
    x, y, z = lattice_points(lo, step, (n,) * 3)
    r2 = (x - F32(SPHERE_C[0])) ** 2 + (y - F32(SPHERE_C[1])) ** 2 + (z - F32(SPHERE_C[2])) ** 2
    s = F32(20.0) * np.exp(F32(-3.0) * r2 / F32(SPHERE_R * SPHERE_R))
    return s.astype(F32), lo, step, np.asarray(UNIT[1], F32)


def torus(n=24, R=0.55, r=0.22):
    """s = 1 - d / r, d the distance to the circle of radius R in z = 0; level 0"""
    lo, step = box_step(*UNIT, (n,) * 3)
    x, y, z = lattice_points(lo, step, (n,) * 3)
    d = np.sqrt((np.sqrt(x * x + y * y) - F32(R)) ** 2 + z * z)
    return (F32(1.0) - d / F32(r)).astype(F32), lo, step, np.asarray(UNIT[1], F32)


def one_point():
    """a single inside point in the middle of a 5^3-point lattice; level 0.5"""
    s = np.zeros((5, 5, 5), F32)
    s[2, 2, 2] = 1.0
    lo, step = box_step(*UNIT, (4,) * 3)
    return s, lo, step, np.asarray(UNIT[1], F32)


def empty():
    lo, step = box_step(*UNIT, (4, 3, 2))
    return np.zeros((3, 4, 5), F32), lo, step, np.asarray(UNIT[1], F32)


def half_space(n=8):
    """s = 0.3 - x - 0.5 y: a sheet that leaves the box; level 0"""
    lo, step = box_step(*UNIT, (n,) * 3)
    x, y, z = lattice_points(lo, step, (n,) * 3)
    return (F32(0.3) - x - F32(0.5) * y).astype(F32), lo, step, np.asarray(UNIT[1], F32)


NOISE_ISO = 0.25


def noise():
    """12 x 9 x 5 cells of uniform noise with NaN, +inf, -inf and values equal
    to the level planted in it; level NOISE_ISO"""
    res = (12, 9, 5)
    rng = np.random.default_rng(11)
    s = rng.uniform(-1.0, 1.0, (res[2] + 1, res[1] + 1, res[0] + 1)).astype(F32)
    flat = s.reshape(-1)
    where = rng.permutation(flat.size)
    for q, val in enumerate((np.nan, np.inf, -np.inf, NOISE_ISO)):
        flat[where[12 * q:12 * q + 12]] = val
    hi = (1.0, 0.5, 0.75)
    lo, step = box_step((-0.5, -0.25, 0.0), hi, res)
    return s, lo, step, np.asarray(hi, F32)


def smooth(res=(64, 60, 40)):
    """a smooth field with several sheets on a non-cubic lattice; level 0"""
    hi = (1.0, 0.9, 0.6)
    lo, step = box_step((-1.0, -0.9, -0.6), hi, res)
    x, y, z = lattice_points(lo, step, res)
    s = (np.sin(F32(4.0) * x) * np.cos(F32(3.0) * y) + np.sin(F32(5.0) * z + x)
         - F32(0.3) * y).astype(F32)
    return s, lo, step, np.asarray(hi, F32)
