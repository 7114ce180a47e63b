"""Shared pieces of tests/test_nw_affine.py and tests/test_nw_affine_gpu.py:
placements of a shared mesh under general affine maps (Scene.transform,
rt_nw_transform), the ctypes view of their checker (tests/native/
nw_affine_ref.cpp, built into the package's lib/), the composition of a
placement's chain restated in float64, and the merged brute force — the
checker's winner over the affine placements against the oracle's over the
rest of the scene, by (t, insertion index).

A chain lists a placement's nodes from the world down to the shared handle:
("translate", off), ("rotate_y", degrees), ("transform", 3 x 4 matrix),
("move", off0, off1, time0, time1)."""
import ctypes as C
import math
import os

import numpy as np

import a_dive_into_ray_tracing_amd.nextweek as nw
import nw_instance_util as U
import nw_mesh_util as M
import nw_motion_util as V
import nw_smooth_util as SU
import oracle_py as O

F32 = np.float32
REF_PATH = os.path.join(M.REPO, "a_dive_into_ray_tracing_amd", "lib", "libnw_affine_ref.so")
_fp = C.POINTER(C.c_float)
_ip = C.POINTER(C.c_int32)
_ref = None


def ref():
    global _ref
    if _ref is None:
        L = C.CDLL(REF_PATH)
        L.nwa_closest.argtypes = [_fp, C.c_int32, _fp, C.c_int32, _fp, C.c_int32, _ip, _fp, _ip, _ip]
        L.nwa_records.argtypes = [_fp, C.c_int32, _fp, C.c_int32, _fp, C.c_int32, _fp, C.c_int32, _ip, _fp, C.c_int32, _fp,
                                  C.c_int32, _ip, _ip, _fp, _fp, _ip, _ip]
        _ref = L
    return _ref


# ---- composition, as include/rtmi_nw.h rt_nw_transform states it -------------------
def _ry(deg):
    th = deg * math.pi / 180.0
    c, s = math.cos(th), math.sin(th)
    return [c, 0.0, s, 0.0, 1.0, 0.0, -s, 0.0, c]


def _mv(A, v):
    return [A[3 * i] * v[0] + A[3 * i + 1] * v[1] + A[3 * i + 2] * v[2] for i in range(3)]


def _mm(A, B):
    return [A[3 * i] * B[j] + A[3 * i + 1] * B[3 + j] + A[3 * i + 2] * B[6 + j] for i in range(3) for j in range(3)]


def compose(chain):
    """(A, b, b1 or None, (time0, time1), affine) of a chain, world down, in
    double: translate b += A off; rotate_y A = A Ry; transform b += A m_b, A = A
    m_A; a move is a translate with two offsets, carried side by side.  Until
    the first transform node, A is Ry of the summed angles (the classical
    placement's form)."""
    theta, A, affine = 0.0, None, False
    b, b1, times = [0.0, 0.0, 0.0], None, (0.0, 1.0)

    def cur():
        return A if affine else _ry(theta)

    for node in chain:
        kind = node[0]
        if kind == "rotate_y":
            if affine:
                A = _mm(A, _ry(float(node[1])))
            else:
                theta = theta + float(node[1])
        elif kind == "translate":
            d = _mv(cur(), [float(x) for x in node[1]])
            b = [b[a] + d[a] for a in range(3)]
            if b1 is not None:
                b1 = [b1[a] + d[a] for a in range(3)]
        elif kind == "move":
            assert b1 is None
            d0, d1 = _mv(cur(), [float(x) for x in node[1]]), _mv(cur(), [float(x) for x in node[2]])
            b, b1 = [b[a] + d0[a] for a in range(3)], [b[a] + d1[a] for a in range(3)]
            times = (float(node[3]), float(node[4]))
        else:
            assert kind == "transform"
            m = np.asarray(node[1], np.float64).reshape(3, 4)
            if not affine:
                A, affine = _ry(theta), True
            d = _mv(A, [float(x) for x in m[:, 3]])
            b = [b[a] + d[a] for a in range(3)]
            if b1 is not None:
                b1 = [b1[a] + d[a] for a in range(3)]
            A = _mm(A, [float(x) for x in m[:, :3].reshape(9)])
    return (np.array(cur()).reshape(3, 3), np.array(b), None if b1 is None else np.array(b1), times, affine)


def inverse(A):
    """A^-1 as the library forms it: the adjugate over the determinant, in double (9 values, row-major)."""
    a = [float(x) for x in np.asarray(A).reshape(9)]
    adj = [a[4] * a[8] - a[5] * a[7], a[2] * a[7] - a[1] * a[8], a[1] * a[5] - a[2] * a[4],
           a[5] * a[6] - a[3] * a[8], a[0] * a[8] - a[2] * a[6], a[2] * a[3] - a[0] * a[5],
           a[3] * a[7] - a[4] * a[6], a[1] * a[6] - a[0] * a[7], a[0] * a[4] - a[1] * a[3]]
    det = a[0] * adj[0] + a[1] * adj[3] + a[2] * adj[6]
    return np.array([x / det for x in adj])


def build(s, h, chain):
    """The chain's nodes over handle h."""
    for node in reversed(chain):
        if node[0] == "translate":
            h = s.translate(h, node[1])
        elif node[0] == "rotate_y":
            h = s.rotate_y(h, node[1])
        elif node[0] == "move":
            h = s.move(h, node[1], node[2], node[3], node[4])
        else:
            h = s.transform(h, node[1])
    return h


def frozen(chain, T):
    """The chain with its move replaced by what stands for it at the instant T:
    the composed ends rounded to float, off(T) of them, and a translate at the
    top of the chain that brings the composed translation to exactly that."""
    if not any(n[0] == "move" for n in chain):
        return chain
    A, b, b1, (t0, t1), _ = compose(chain)
    off = V.off_at(b.astype(F32), b1.astype(F32), t0, t1, T)
    still = [n for n in chain if n[0] != "move"]
    _, bs, _, _, _ = compose(still)
    return [("translate", [float(off[a]) - float(bs[a]) for a in range(3)])] + still


def shear(k=0.5, scale=(1.0, 1.0, 1.0), translate=(0, 0, 0)):
    """x += k y after the scales."""
    A = np.array([[1.0, k, 0.0], [0.0, 1.0, 0.0], [0.0, 0.0, 1.0]]) @ np.diag(np.asarray(scale, np.float64))
    return np.concatenate([A, np.asarray(translate, np.float64).reshape(3, 1)], axis=1)


# ---- a scene of placements of one mesh ----------------------------------------------
class Placed:
    """A scene whose first objects are placements of one shared mesh (each n_tri
    flattened triangles, in the order of `chains`), then other objects."""

    def __init__(self, scene, chains, local, n_tri):
        self.scene, self.chains, self.local, self.n_tri = scene, chains, local, n_tri
        self.comp = [compose(c) for c in chains]
        self.affine = [p for p, c in enumerate(self.comp) if c[4]]
        self.first = [p * n_tri for p in range(len(chains))]
        assert scene.affine_stats() == (len(self.affine), len(chains) - len(self.affine))

    def table(self):
        """The checker's 24-word rows of the affine placements."""
        rows = np.zeros((len(self.affine), 24), F32)
        ints = rows.view(np.int32)
        for r, p in enumerate(self.affine):
            A, b, b1, (t0, t1), _ = self.comp[p]
            rows[r, :9] = inverse(A).astype(F32)
            rows[r, 9:12] = b.astype(F32)
            rows[r, 12:15] = (b if b1 is None else b1).astype(F32)
            rows[r, 15], rows[r, 16] = F32(t0), F32(t1)
            ints[r, 17:21] = [0 if b1 is None else 1, self.first[p], 0, self.n_tri]
        return rows

    def keep(self):
        """The flattened indices outside the affine placements."""
        k = np.ones(self.scene.flat()["n_obj"], bool)
        for p in self.affine:
            k[self.first[p]:self.first[p] + self.n_tri] = False
        return np.nonzero(k)[0]

    def reduced(self, T):
        """(flat view at T without the affine placements' rows, its attribute view, the kept indices)."""
        keep = self.keep()
        fl, fa = self.scene.flat(time=T), self.scene.flat_attr()
        fl = dict(fl, obj=np.ascontiguousarray(fl["obj"].reshape(-1, 16)[keep]).reshape(-1), n_obj=len(keep))
        fa = dict(fa, attr_of_obj=np.ascontiguousarray(fa["attr_of_obj"][keep])) if fa["attr"].size else None
        return fl, fa, keep


def local_arrays(mesh_builder):
    """The mesh added unplaced to a scene of its own: SU.scene_arrays of it (local triangles, materials, attributes)."""
    s = nw.Scene()
    s.add(mesh_builder(s))
    return SU.scene_arrays(s)


def placed(mesh_builder, chains, n_tri):
    """One mesh (mesh_builder(scene) -> handle), shared, placed by every chain; nothing else."""
    s = nw.Scene()
    h = s.shared(mesh_builder(s))
    for c in chains:
        s.add(build(s, h, c))
    s.set_background(0.7, 0.8, 1.0)
    return Placed(s, chains, local_arrays(mesh_builder), n_tri)


def world_triangles(pl, p, T=0.0):
    """Placement p's triangles in float64 world space, n x 3 x 3: A v + b(T) of the local float vertices."""
    A, b, b1, (t0, t1), _ = pl.comp[p]
    if b1 is not None:
        b = V.off_at(b.astype(F32), b1.astype(F32), t0, t1, T).astype(np.float64)
    return pl.local["obj"][:pl.n_tri, :9].astype(np.float64).reshape(-1, 3, 3) @ A.T + b


def watertight_rays(m, verts, faces, seed=7):
    """M.watertight_rays from the image of M.INSIDE under the 3 x 4 map m: 150 000
    normal directions, every world vertex minus the origin as float32 computes
    it, that vector times 3, a random point on every world edge minus the
    origin, the six axis directions (float32 rows o.xyz d.xyz time)."""
    g = np.random.default_rng(seed)
    A, b = np.asarray(m)[:, :3], np.asarray(m)[:, 3]
    o = (A @ np.array(M.INSIDE) + b).astype(F32)
    vf = (np.asarray(verts, np.float64) @ A.T + b).astype(F32)
    to_v = vf - o
    e = np.array(sorted({(min(x, y), max(x, y)) for a_, b_, c_ in faces for x, y in ((a_, b_), (b_, c_), (c_, a_))}))
    s = g.random(len(e)).astype(F32)[:, None]
    on_edge = (vf[e[:, 0]] + s * (vf[e[:, 1]] - vf[e[:, 0]])).astype(F32) - o
    axes = np.array([[1, 0, 0], [-1, 0, 0], [0, 1, 0], [0, -1, 0], [0, 0, 1], [0, 0, -1]], F32)
    d = np.concatenate([g.normal(size=(150_000, 3)).astype(F32), to_v, (to_v * F32(3)).astype(F32), on_edge, axes])
    return np.concatenate([np.broadcast_to(o, d.shape), d, np.zeros((len(d), 1), F32)], axis=1).astype(F32)


def affine_closest(pl, rays):
    """The checker's closest hit over the affine placements: (insertion index or -1, t, row of table(), triangle)."""
    a, tab, r = pl.local, pl.table(), SU.rays8(rays)
    n = len(r)
    idx, t, pp, jj = np.zeros(n, np.int32), np.zeros(n, F32), np.zeros(n, np.int32), np.zeros(n, np.int32)
    rc = ref().nwa_closest(a["obj"].ctypes.data_as(_fp), len(a["obj"]), tab.ctypes.data_as(_fp), len(tab), r.ctypes.data_as(_fp), n,
                           idx.ctypes.data_as(_ip), t.ctypes.data_as(_fp), pp.ctypes.data_as(_ip), jj.ctypes.data_as(_ip))
    assert rc == 0, rc
    return idx, t, pp, jj


def affine_records(pl, rays, place, tri, t):
    """The checker's records of the rays with place >= 0: (rows p n u v, material, side code)."""
    a, tab, r = pl.local, pl.table(), SU.rays8(rays)
    n = len(r)
    rec, mat, side = np.zeros((n, 8), F32), np.zeros(n, np.int32), np.zeros(n, np.int32)
    place, tri, t = np.ascontiguousarray(place, np.int32), np.ascontiguousarray(tri, np.int32), np.ascontiguousarray(t, F32)
    rc = ref().nwa_records(a["obj"].ctypes.data_as(_fp), len(a["obj"]), a["mat"].ctypes.data_as(_fp), len(a["mat"]),
                           a["tex"].ctypes.data_as(_fp), len(a["tex"]), a["attr"].ctypes.data_as(_fp), len(a["attr"]),
                           a["attr_of_obj"].ctypes.data_as(_ip), tab.ctypes.data_as(_fp), len(tab), r.ctypes.data_as(_fp), n,
                           place.ctypes.data_as(_ip), tri.ctypes.data_as(_ip), t.ctypes.data_as(_fp), rec.ctypes.data_as(_fp),
                           mat.ctypes.data_as(_ip), side.ctypes.data_as(_ip))
    assert rc == 0, rc
    return rec, mat, side


def merged(pl, rays, records=False):
    """The whole scene's brute-force closest hit per ray (rows o.xyz d.xyz time):
    the checker over the affine placements merged with the oracle over the rest
    at each ray's time, by (t, insertion index).  (index, t, face), with records
    also (rows p n u v, material, side code; side -1 where the oracle won)."""
    rays = np.ascontiguousarray(rays, F32)
    n = len(rays)
    ai, at, ap, aj = affine_closest(pl, rays)
    idx, t, face = np.full(n, -1, np.int32), np.full(n, np.inf, F32), np.full(n, -1, np.int32)
    rec, mat, side = np.zeros((n, 8), F32), np.zeros(n, np.int32), np.full(n, -1, np.int32)
    for T in np.unique(rays[:, 6]):
        sel = np.nonzero(rays[:, 6] == T)[0]
        fl, fa, keep = pl.reduced(float(T))
        if records:
            oi, ot, orec, omat = O.nw_records(fl, rays[sel], flat_attr=fa)
            of = np.full(len(sel), -1, np.int32)
            rec[sel], mat[sel] = orec, omat
        else:
            oi, ot, of = O.nw_hits(fl, rays[sel], flat_attr=fa)
        hit = oi >= 0
        idx[sel] = np.where(hit, keep[np.maximum(oi, 0)], -1)
        t[sel] = np.where(hit, ot, np.inf)
        face[sel] = of
    wins = (ai >= 0) & ((idx < 0) | (at < t) | ((at == t) & (ai < idx)))
    idx[wins], t[wins], face[wins] = ai[wins], at[wins], -1
    if not records:
        return idx, np.where(idx >= 0, t, F32(np.inf)).astype(F32), face, wins
    arec, amat, aside = affine_records(pl, rays, np.where(wins, ap, -1), aj, at)
    rec[wins], mat[wins], side[wins] = arec[wins], amat[wins], aside[wins]
    return idx, t, rec, mat, side, wins


# ---- scene A --------------------------------------------------------------------------
A_TRIS = 320
A_BOX = ((-1.2, -3.4, 1.6), (0.6, -2.5, 3.0))
A_MOVE = ((-0.8, 1.6, -3.0), (0.0, 2.2, -3.3), 0.25, 0.75)
A_CLASSIC_MOVE = ((-2.9, 0.3, 0.8), (-1.7, 0.9, 0.2), 0.0, 1.0)
A_CHAINS = [
    [("translate", (0.4, 0.2, 3.2)), ("rotate_y", 30.0)],
    [("transform", nw.affine(scale=1.5, axis=(1, 1, 0), angle=40.0, translate=(-2.6, 0.5, -0.6)))],
    [("rotate_y", 20.0), ("transform", nw.affine(scale=1.4, translate=(2.8, -1.0, 0.6))), ("transform", shear(0.5, (2.0, 0.5, 1.0)))],
    [("move", *A_MOVE), ("transform", nw.affine(scale=(1.7, 1.2, 1.5), axis=(0, 1, 1), angle=25.0))],
    [("move", *A_CLASSIC_MOVE), ("rotate_y", 75.0)],
]


def a_mesh(s, subdiv=2, smooth=True):
    v, f = M.icosphere(subdiv)
    mat = s.lambertian(s.image(SU.TEXTURE))
    if not smooth:  # (flat shaded: the uvs and the texture alone)
        return s.mesh(v, f, uvs=SU.affine_uvs(v), mat=mat)
    return s.mesh(v, f, normals=SU.sphere_normals(v), uvs=SU.affine_uvs(v), smooth=True, mat=mat)


def scene_a(T=None, chains=A_CHAINS, subdiv=2, extras=True, smooth=True):
    """The issue's scene A: icosphere(2) with the sphere's normals, uvs and an
    image texture, shared and placed five times — classical; a rotation about
    (1, 1, 0) with scale 1.5; scales (2, 0.5, 1) with a shear (under a uniform
    1.4, so that it wins its share of the rays) under a rotate_y node; a moving affine placement on the division path; a classical moving
    placement — plus U.SPHERES and a box.  T: the moves frozen at that instant."""
    s = nw.Scene()
    h = s.shared(a_mesh(s, subdiv, smooth))
    chains = [c if T is None else frozen(c, T) for c in chains]
    for c in chains:
        s.add(build(s, h, c))
    if extras:
        grey = s.lambertian(s.solid(0.6, 0.5, 0.4))
        sm = [grey, s.metal(s.solid(0.7, 0.6, 0.5), 0.0), s.dielectric(1.5), s.lambertian(s.solid(0.9, 0.2, 0.2))]
        for (c, r), m in zip(U.SPHERES, sm):
            s.add(s.sphere(c, r, m))
        s.add(s.box(*A_BOX, s.metal(s.solid(0.8, 0.7, 0.3), 0.1)))
    s.set_background(0.7, 0.8, 1.0)
    return Placed(s, chains, local_arrays(lambda q: a_mesh(q, subdiv, smooth)), 20 * 4 ** subdiv)


def a_rays(pl, n, seed, grazing=0):
    """SU.hit_rays over scene A at mid-exposure (signed zeros, axis-aligned
    directions), the last `grazing` of them grazing rays of the mesh taken
    through the affine placements in turn; times cycle through V.RAY_TIMES."""
    rays = SU.hit_rays(pl.scene.flat(time=0.5), n - grazing, seed)
    times = np.array(V.RAY_TIMES, F32)
    if grazing:
        v, f = M.icosphere(2)
        loc = SU.grazing_rays(v, f, grazing, seed)
        out = np.array(loc, F32)
        for r, p in enumerate(pl.affine):
            A, b, b1, (t0, t1), _ = pl.comp[p]
            sel = np.arange(grazing) % len(pl.affine) == r
            tm = times[(np.arange(grazing) + n - grazing) % len(times)][sel]
            off = np.array([b if b1 is None else V.off_at(b.astype(F32), b1.astype(F32), t0, t1, T).astype(np.float64) for T in tm])
            out[sel, :3] = (loc[sel, :3].astype(np.float64) @ A.T + off).astype(F32)
            out[sel, 3:6] = (loc[sel, 3:6].astype(np.float64) @ A.T).astype(F32)
        rays = np.concatenate([rays, out])
    rays[:, 6] = times[np.arange(len(rays)) % len(times)]
    return np.ascontiguousarray(rays, F32)


def bits(x):
    return np.ascontiguousarray(x, F32).view(np.int32)
