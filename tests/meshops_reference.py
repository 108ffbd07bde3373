"""The mesh clean-up of csrc/meshops.hip restated in numpy (fp64), the rule of include/gsr.h spelled out: a row of faces is a FACE iff its three
indices are in [0, Nv) and pairwise different; any other row is not there.  Host union-find for the labels, bincount for the face counts, mask plus
cumsum for the compaction, and the two fp64 sums of the normals and the smoothing in ascending face order (np.add.at applies its updates one after the
other in index order, and the corners are listed face by face).  Plus the meshes the tests share and the distances they compare with.

Bars.  The normals and the smoothed positions are the SAME fp64 operations in the same order in the kernels (built with -ffp-contract=off, operands
converted to fp64 first) and here, rounded once to fp32: the expectation is 0 ulp.  HOST_MAX_ULP is what the host build of the kernels shows over every
case of tests/test_meshops_cpu.py (measured: 0 everywhere).  On the device the only operations whose result the flags do not pin to one correctly
rounded value are the math library's fp64 divide and square root; a last-bit difference there moves the final fp32 rounding by at most one ulp:
DEVICE_MAX_ULP = HOST_MAX_ULP + 1, derived, not measured."""
import numpy as np

HOST_MAX_ULP = 0                       # measured on the host build (tests/test_meshops_cpu.py prints the figure): same operations, same order
DEVICE_MAX_ULP = HOST_MAX_ULP + 1      # + one fp32 ulp for the device's fp64 divide / square root (see above)


# ---- the rule -----------------------------------------------------------------------------------------------------------------------------------
def is_face(nv, faces):
    f = np.asarray(faces, dtype=np.int64).reshape(-1, 3)
    inside = ((f >= 0) & (f < nv)).all(axis=1)
    return inside & (f[:, 0] != f[:, 1]) & (f[:, 1] != f[:, 2]) & (f[:, 0] != f[:, 2])


def components(nv, faces):
    """-> (vertex_label [nv] int32: the smallest vertex of the component, face_count [nv] int32: faces per label).  Host union-find."""
    f = np.asarray(faces, dtype=np.int64).reshape(-1, 3)
    f = f[is_face(nv, f)]
    parent = list(range(nv))

    def find(x):
        root = x
        while parent[root] != root:
            root = parent[root]
        while parent[x] != root:
            parent[x], x = root, parent[x]
        return root

    for a, b, c in f.tolist():
        for u, v in ((a, b), (b, c)):
            ru, rv = find(u), find(v)
            if ru != rv:
                parent[max(ru, rv)] = min(ru, rv)
    label = np.array([find(v) for v in range(nv)], dtype=np.int32).reshape(nv)
    count = np.bincount(label[f[:, 0]], minlength=nv).astype(np.int32) if len(f) else np.zeros(nv, np.int32)
    return label, count


def compact(vertices, colors, faces, keep):
    """faces[keep & is_face] with the cumsum remapping -> (vertices', colors' or None, faces')."""
    v = np.asarray(vertices, dtype=np.float32).reshape(-1, 3)
    f = np.asarray(faces, dtype=np.int32).reshape(-1, 3)
    nv = len(v)
    k = is_face(nv, f) & (np.ones(len(f), bool) if keep is None else (np.asarray(keep).reshape(-1) != 0))
    used = np.zeros(nv, dtype=bool)
    used[f[k].reshape(-1)] = True
    new = np.cumsum(used) - 1
    return v[used], (None if colors is None else np.asarray(colors, np.float32).reshape(-1, 3)[used]), new[f[k]].astype(np.int32).reshape(-1, 3)


def filter_keep(nv, faces, min_faces=0, keep_largest=None):
    """2DGS's rule -> the keep mask [Nf]: threshold = max(min_faces, the keep_largest-th largest component face count), ties kept."""
    f = np.asarray(faces, dtype=np.int64).reshape(-1, 3)
    label, count = components(nv, f)
    threshold = int(min_faces)
    if keep_largest is not None:
        sizes = np.sort(count)[::-1]
        threshold = max(threshold, int(sizes[min(keep_largest, nv) - 1])) if nv else threshold
    ok = is_face(nv, f)
    keep = np.zeros(len(f), dtype=bool)
    keep[ok] = count[label[f[ok, 0]]] >= threshold
    return keep


def vertex_normals(vertices, faces):
    """Area-weighted, fp64 sums in ascending face order, one rounding -> [Nv,3] float32."""
    p = np.asarray(vertices, dtype=np.float32).reshape(-1, 3).astype(np.float64)
    nv = len(p)
    f = np.asarray(faces, dtype=np.int64).reshape(-1, 3)
    f = f[is_face(nv, f)]
    with np.errstate(all="ignore"):
        a, b, c = p[f[:, 0]], p[f[:, 1]], p[f[:, 2]]
        u, w = b - a, c - a
        cross = np.stack([u[:, 1] * w[:, 2] - u[:, 2] * w[:, 1], u[:, 2] * w[:, 0] - u[:, 0] * w[:, 2], u[:, 0] * w[:, 1] - u[:, 1] * w[:, 0]], axis=1)
        n = np.zeros((nv, 3), dtype=np.float64)
        np.add.at(n, f.reshape(-1), np.repeat(cross, 3, axis=0))      # corner by corner, face by face: every vertex sums in ascending face order
        length = np.sqrt((n[:, 0] * n[:, 0] + n[:, 1] * n[:, 1]) + n[:, 2] * n[:, 2])
        zero = (n[:, 0] == 0) & (n[:, 1] == 0) & (n[:, 2] == 0)
        out = n / length[:, None]
    out[zero] = 0.0
    return out.astype(np.float32)


def smooth_step(p32, f, weight):
    p = p32.astype(np.float64)
    nv = len(p)
    with np.errstate(all="ignore"):
        s = np.zeros((nv, 3), dtype=np.float64)
        idx = f.reshape(-1)                                                              # corner 3 f + k belongs to vertex f[k]
        pj = p[np.stack([f[:, 1], f[:, 2], f[:, 0]], axis=1).reshape(-1)]                # the corner after it in the face's cyclic order
        pk = p[np.stack([f[:, 2], f[:, 0], f[:, 1]], axis=1).reshape(-1)]                # and the one after that
        np.add.at(s, idx, pj + pk)
        count = np.bincount(idx, minlength=nv)
        m = s / (2.0 * count.astype(np.float64))[:, None]
        out = (p + np.float64(np.float32(weight)) * (m - p)).astype(np.float32)
    out[count == 0] = p32[count == 0]
    return out


def smooth(vertices, faces, iterations, lam, mu):
    """Taubin: `iterations` times a step with lam then one with mu, fp64 inside a step, fp32 between steps -> [Nv,3] float32."""
    p = np.array(vertices, dtype=np.float32).reshape(-1, 3)
    f = np.asarray(faces, dtype=np.int64).reshape(-1, 3)
    f = f[is_face(len(p), f)]
    for _ in range(iterations):
        p = smooth_step(p, f, lam)
        p = smooth_step(p, f, mu)
    return p


# ---- distances ----------------------------------------------------------------------------------------------------------------------------------
def ulp_distance(a, b):
    """Per component, in fp32 units in the last place; two NaNs are 0 apart, a NaN and a number 2^32."""
    a, b = np.asarray(a, np.float32), np.asarray(b, np.float32)
    def ordered(x):
        i = x.view(np.int32).astype(np.int64)
        return np.where(i < 0, -(i & 0x7FFFFFFF), i)
    d = np.abs(ordered(a) - ordered(b))
    na, nb = np.isnan(a), np.isnan(b)
    return np.where(na & nb, 0, np.where(na | nb, 1 << 32, d))


def edge_distance(nv, faces, sources, limit):
    """Edges from the nearest of `sources` along faces, capped at limit + 1 -> [nv] int."""
    f = np.asarray(faces, dtype=np.int64).reshape(-1, 3)
    f = f[is_face(nv, f)]
    dist = np.full(nv, limit + 1, dtype=np.int64)
    dist[list(sources)] = 0
    for step in range(1, limit + 1):
        near = (dist[f] < step).any(axis=1)
        reach = np.unique(f[near].reshape(-1))
        reach = reach[dist[reach] > step]
        dist[reach] = step
    return dist


def same_bits(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes()


# ---- meshes -------------------------------------------------------------------------------------------------------------------------------------
def tetrahedron():
    """The regular tetrahedron on alternate corners of the cube, faces counter-clockwise seen from outside."""
    v = np.array([[1, 1, 1], [1, -1, -1], [-1, 1, -1], [-1, -1, 1]], dtype=np.float32)
    f = np.array([[0, 1, 2], [0, 3, 1], [0, 2, 3], [1, 3, 2]], dtype=np.int32)
    return v, f


def two_tetrahedra_sharing_a_vertex():
    """The tetrahedron and its mirror image through its vertex 0: 7 vertices, 8 faces, one shared vertex and no shared edge."""
    v, f = tetrahedron()
    mirrored = (2 * v[0] - v).astype(np.float32)
    second = np.where(f == 0, 0, f + 3)[:, ::-1]      # (the point reflection turns the winding around)
    return np.concatenate([v, mirrored[1:]]), np.concatenate([f, second]).astype(np.int32)


def strip(n_faces, order, seed=5):
    """A triangle strip of n_faces faces over n_faces + 2 vertices whose ids are `order` ('reverse' or 'random') along the strip."""
    n = n_faces + 2
    along = np.arange(n)
    ids = along[::-1].copy() if order == "reverse" else np.random.default_rng(seed).permutation(n)
    rng = np.random.default_rng(seed + 1)
    pos = np.stack([along // 2, along % 2, rng.random(n) * 0.3], axis=1).astype(np.float32)
    vertices = np.empty((n, 3), dtype=np.float32)
    vertices[ids] = pos
    i = np.arange(n_faces)
    f = np.where((i % 2 == 0)[:, None], np.stack([i, i + 1, i + 2], axis=1), np.stack([i + 1, i, i + 2], axis=1))
    return vertices, ids[f].astype(np.int32)


def sphere(levels=3, radius=1.0, centre=(0.0, 0.0, 0.0)):
    """An octahedron subdivided `levels` times and pushed onto the sphere: 8 * 4^levels faces, closed, outward."""
    verts = [(1, 0, 0), (-1, 0, 0), (0, 1, 0), (0, -1, 0), (0, 0, 1), (0, 0, -1)]
    faces = [(0, 2, 4), (2, 1, 4), (1, 3, 4), (3, 0, 4), (2, 0, 5), (1, 2, 5), (3, 1, 5), (0, 3, 5)]
    for _ in range(levels):
        mid, out = {}, []

        def midpoint(a, b):
            key = (min(a, b), max(a, b))
            if key not in mid:
                m = np.add(verts[a], verts[b], dtype=np.float64)
                verts.append(tuple(m / np.linalg.norm(m)))
                mid[key] = len(verts) - 1
            return mid[key]

        for a, b, c in faces:
            ab, bc, ca = midpoint(a, b), midpoint(b, c), midpoint(c, a)
            out += [(a, ab, ca), (ab, b, bc), (ca, bc, c), (ab, bc, ca)]
        faces = out
    v = (np.array(verts, dtype=np.float64) * radius + np.array(centre, dtype=np.float64)).astype(np.float32)
    return v, np.array(faces, dtype=np.int32)


def bipyramid(n, radius, centre):
    """A closed blob of 2 n faces: a ring of n vertices and two apexes."""
    t = np.arange(n) * (2 * np.pi / n)
    ring = np.stack([np.cos(t), np.sin(t), np.zeros(n)], axis=1)
    v = (np.concatenate([ring, [[0, 0, 1.0], [0, 0, -1.0]]]) * radius + np.array(centre)).astype(np.float32)
    i, j = np.arange(n), (np.arange(n) + 1) % n
    f = np.concatenate([np.stack([np.full(n, n), i, j], axis=1), np.stack([np.full(n, n + 1), j, i], axis=1)])
    return v, f.astype(np.int32)


def join(parts):
    vs, fs, base = [], [], 0
    for v, f in parts:
        vs.append(v)
        fs.append(f + base)
        base += len(v)
    return np.concatenate(vs).astype(np.float32), np.concatenate(fs).astype(np.int32)


BLOB_FACES = (4, 20, 60)


def composed(seed=11, levels=3, second_60=False):
    """One large sphere, three blobs of 4 / 20 / 60 faces, 7 vertices no face uses, the three kinds of rows that are no faces interleaved, vertex ids
    permuted and faces shuffled -> (vertices, colors, faces).  second_60: one more blob of 60 faces (a tie for filter_components)."""
    rng = np.random.default_rng(seed)
    tet_v, tet_f = tetrahedron()
    parts = [sphere(levels), ((tet_v * 0.05 + np.array([1.5, 0, 0])).astype(np.float32), tet_f), bipyramid(10, 0.08, (0, 1.6, 0)),
             bipyramid(30, 0.1, (0, 0, -1.7))] + ([bipyramid(30, 0.1, (1.2, 1.2, 1.2))] if second_60 else [])
    v, f = join(parts)
    v = np.concatenate([v, rng.random((7, 3)).astype(np.float32) * 3])
    nv = len(v)
    perm = rng.permutation(nv)
    vertices = np.empty_like(v)
    vertices[perm] = v
    f = perm[f].astype(np.int32)
    bad = np.array([[-1, 0, 1], [0, 1, nv], [2, 2, 3]] * 5, dtype=np.int32)
    f = np.concatenate([f, bad])
    f = f[rng.permutation(len(f))]
    return vertices, rng.random((nv, 3)).astype(np.float32), np.ascontiguousarray(f)


def blob_field(n, blobs=24, seed=2):
    """An analytic signed distance field on an n^3 grid (voxel (ix,iy,iz) at (ix,iy,iz) / n, stored [nz,ny,nx]): a sphere of radius 0.2 in the middle
    and `blobs` small spheres around it, in units of the truncation (clamped to [-1, 1]) -> float32 [n,n,n]."""
    rng = np.random.default_rng(seed)
    z, y, x = np.meshgrid(*([np.arange(n) / n] * 3), indexing="ij")
    d = np.sqrt((x - 0.5) ** 2 + (y - 0.5) ** 2 + (z - 0.5) ** 2) - 0.2
    for _ in range(blobs):
        while True:
            c = 0.1 + 0.8 * rng.random(3)
            if np.linalg.norm(c - 0.5) > 0.3:
                break
        d = np.minimum(d, np.sqrt((x - c[0]) ** 2 + (y - c[1]) ** 2 + (z - c[2]) ** 2) - (1.2 + rng.random()) / n)
    return np.clip(d * n / 3.0, -1.0, 1.0).astype(np.float32)
