"""Reference of TSDF fusion and marching tetrahedra (csrc/tsdf.hip, gsr_scene/mesh.py): the integrate rule of include/gsr.h in fp64 numpy, a
marching-tetrahedra reference that returns vertex KEYS (owner voxel index * 7 + direction), faces as key triples and positions, the scenes every
mesh test uses, and the bars.

THE FRAGILE SET of the integrate.  A voxel is fragile when, for some view, a decision of the rule lies within a margin of its threshold, so that
an fp32 evaluation may legitimately decide the other way.  With u = 2^-24 (fp32 unit roundoff) and, per view, S_j = sum_i |p_i R_ij| + |T_j| (the
magnitudes that enter camera coordinate j):
  * cam_j in fp32 is an fmaf chain (3 roundings, each <= u S_j) over a position whose three coordinates carry one rounding each (<= u S_j in
    all): |cam_j - fp64| <= 4 u S_j.  Margin of `z > near`: MARGIN_ULPS u S_z with MARGIN_ULPS = 16, four times that.
  * pix_x = fx x / z + W / 2: the product, the quotient and the sum round once each (<= 3 u (|fx x / z| + W / 2)), the errors of x and z enter
    as fx (4 u S_x + |x / z| 4 u S_z) / z.  Margin of the floor AND of the bounds 0 and W (which are integers: "px within the margin of an
    integer" covers the two floors and the four bounds at once): MARGIN_ULPS u (fx (S_x + |x / z| S_z) / z + |fx x / z| + W / 2); likewise in y.
  * sdf = d - z >= -sdf_trunc: d is an fp32 datum, the subtraction rounds once: margin MARGIN_ULPS u (S_z + d).
Fragile voxels are left out of value comparisons; a test case may hold at most 5 % of them (asserted).

THE BAR of tsdf off the fragile set, absolute, in units of  eps32 max(1, max_v max(S_z, d) / sdf_trunc),  eps32 = 2^-23:  an observation
t = min(1, (d - z) / trunc) is off by at most (4 u S_z + u |d - z|) / trunc + u <= 3 units; the sum of n <= V of them in view order adds at
most (n - 1) u n, which the final division by (weight + n) >= n turns into (V - 1) / 2 units at most; the product tsdf * weight, the sum and
the division add 1.5.  DERIVED_UNITS(V) = 4.5 + (V - 1) / 2.  The host build shows MEASURED["tsdf_units"] at most (tests/test_mesh_cpu.py
prints and checks it); the device takes the same correctly rounded operations, and is given 4 x that, never above the derived bar.
rgb: colours in [0,1] are data; only the sums and the final update round: (V - 1) / 2 + 1.5 units of eps32 max|colour|; measured likewise.
weight must be EQUAL.

THE EXTRACTION takes an fp32 volume as given: its decisions (observed, inside, valid) are comparisons of stored floats, so vertex keys and faces
must be EQUAL (faces up to rotation).  A position is p0 + t voxel e with t = s0 / (s0 - s1) in [0,1]: the difference, the quotient, the product
and the sum round once each, p0 = fmaf(voxel, i, origin) once: |error| <= u (3 voxel + 2 |p|) per coordinate; POSITION_ULPS = 4 of
eps32 (voxel + |p|_max) is the bar."""
import math

import numpy as np

from mip_reference import camera_record

U32 = 2.0 ** -24
EPS32 = 2.0 ** -23
MARGIN_ULPS = 16.0
FRAGILE_CAP = 0.05
POSITION_ULPS = 4.0

MEASURED = {
    "tsdf_units": 1.09,     # largest |tsdf - reference| of the host build in the units above, over the sweeps of tests/test_mesh_cpu.py (derived: 4.5 at V 1)
    "rgb_units": 0.86,       # ... of rgb in units of eps32 max|colour| (derived: 1.5 at V 1, 9.5 at V 17)
}


def derived_units(V):
    return 4.5 + (V - 1) / 2.0


def rgb_derived_units(V):
    return 1.5 + (V - 1) / 2.0


def bars(V):
    return {"tsdf_units": min(4.0 * MEASURED["tsdf_units"], derived_units(V)), "rgb_units": min(4.0 * MEASURED["rgb_units"], rgb_derived_units(V))}


DIRS = np.array([[1, 0, 0], [0, 1, 0], [0, 0, 1], [1, 1, 0], [1, 0, 1], [0, 1, 1], [1, 1, 1]], dtype=np.int64)
PERMS = [(0, 1, 2), (0, 2, 1), (1, 0, 2), (1, 2, 0), (2, 0, 1), (2, 1, 0)]      # lexicographic


# ---- the integrate rule -----------------------------------------------------------------------------------------------------------------------
def voxel_positions(dims, origin, voxel):
    nx, ny, nz = dims
    iz, iy, ix = np.meshgrid(np.arange(nz), np.arange(ny), np.arange(nx), indexing="ij")
    idx = np.stack([ix, iy, iz], axis=-1).reshape(-1, 3).astype(np.float64)
    return np.asarray(origin, dtype=np.float64)[None, :] + float(voxel) * idx


def integrate(dims, origin, voxel, trunc, near, cams, depth, color=None, state=None):
    """The rule of include/gsr.h in fp64.  cams [V,16], depth [V,H,W], color [V,3,H,W] or None; state = (tsdf, weight, rgb) flat fp64 arrays or None (a
    fresh volume).  -> dict(tsdf, weight, rgb, fragile [N] bool, unit [N]: eps32 max(1, max_v max(S_z, d) / trunc))."""
    N = dims[0] * dims[1] * dims[2]
    p = voxel_positions(dims, origin, voxel)
    cams = np.asarray(cams, dtype=np.float64)
    depth = np.asarray(depth, dtype=np.float64)
    V, H, W = depth.shape
    voxel, trunc, near = float(voxel), float(trunc), float(near)
    if state is None:
        tsdf, weight, rgb = np.ones(N), np.zeros(N), np.zeros((3, N))
    else:
        tsdf, weight, rgb = (np.array(a, dtype=np.float64) for a in state)
    s, n, c = np.zeros(N), np.zeros(N), np.zeros((3, N))
    fragile = np.zeros(N, dtype=bool)
    scale = np.zeros(N)
    for v in range(V):
        rec = cams[v]
        if not np.isfinite(rec).all():
            continue
        R, T, fx, fy = rec[:9].reshape(3, 3), rec[9:12], rec[12], rec[13]
        cam = p @ R + T[None, :]
        S = np.abs(p) @ np.abs(R) + np.abs(T)[None, :]
        x, y, z = cam[:, 0], cam[:, 1], cam[:, 2]
        front = z > near
        fragile |= np.abs(z - near) <= MARGIN_ULPS * U32 * S[:, 2]
        zz = np.where(front, z, 1.0)
        pu, pv = fx * x / zz + W / 2.0, fy * y / zz + H / 2.0
        mu = MARGIN_ULPS * U32 * (abs(fx) * (S[:, 0] + np.abs(x / zz) * S[:, 2]) / zz + np.abs(fx * x / zz) + W / 2.0)
        mv = MARGIN_ULPS * U32 * (abs(fy) * (S[:, 1] + np.abs(y / zz) * S[:, 2]) / zz + np.abs(fy * y / zz) + H / 2.0)
        near_image = front & (pu > -1) & (pu < W + 1) & (pv > -1) & (pv < H + 1)
        fragile |= near_image & ((np.abs(pu - np.round(pu)) <= mu) | (np.abs(pv - np.round(pv)) <= mv))
        ix, iy = np.floor(pu), np.floor(pv)
        on = front & (ix >= 0) & (ix < W) & (iy >= 0) & (iy < H)
        ixc, iyc = np.where(on, ix, 0).astype(np.int64), np.where(on, iy, 0).astype(np.int64)
        d = depth[v, iyc, ixc]
        ok = on & np.isfinite(d) & (d > 0)
        dd = np.where(ok, d, 0.0)
        sdf = dd - z
        fragile |= ok & (np.abs(sdf + trunc) <= MARGIN_ULPS * U32 * (S[:, 2] + dd))
        take = ok & (sdf >= -trunc)
        s += np.where(take, np.minimum(1.0, sdf / trunc), 0.0)
        n += take
        if color is not None:
            c += np.where(take[None, :], np.asarray(color[v], dtype=np.float64)[:, iyc, ixc], 0.0)
        scale = np.maximum(scale, np.where(ok, np.maximum(S[:, 2], dd), 0.0))
    hit = n > 0
    den = np.where(hit, weight + n, 1.0)
    out_t = np.where(hit, (tsdf * weight + s) / den, tsdf)
    out_c = np.where(hit[None, :], (rgb * weight[None, :] + c) / den[None, :], rgb)
    return {"tsdf": out_t, "weight": weight + n, "rgb": out_c, "fragile": fragile, "unit": EPS32 * np.maximum(1.0, scale / trunc)}


def check_integrate(who, got_tsdf, got_weight, got_rgb, ref, V, color_max=1.0, calls=1, bar=None):
    """Asserts the comparison of the module docstring; -> the largest errors in units {tsdf_units, rgb_units}.  `bar`: {name: units}, default the
    derived ones; `calls`: sequential calls fold their errors (the bar scales)."""
    keep = ~ref["fragile"]
    share = 1.0 - keep.mean()
    assert share <= FRAGILE_CAP, f"{who}: {share:.3%} of the voxels are fragile"
    gw = np.asarray(got_weight, dtype=np.float64).reshape(-1)
    assert np.array_equal(gw[keep], ref["weight"][keep]), f"{who}: weight differs on {int((gw[keep] != ref['weight'][keep]).sum())} voxels off the fragile set"
    bar = bar or {"tsdf_units": derived_units(V), "rgb_units": rgb_derived_units(V)}
    gt = np.asarray(got_tsdf, dtype=np.float64).reshape(-1)
    assert np.isfinite(gt).all()
    fig = {"tsdf_units": float((np.abs(gt - ref["tsdf"]) / ref["unit"])[keep].max(initial=0.0))}
    if got_rgb is not None:
        gc = np.asarray(got_rgb, dtype=np.float64).reshape(3, -1)
        fig["rgb_units"] = float((np.abs(gc - ref["rgb"])[:, keep] / (EPS32 * color_max)).max(initial=0.0))
    print(f"[mesh] {who}: fragile {share:.3%}, " + ", ".join(f"{k} {v:.3f} (bar {calls * bar[k]:.3f})" for k, v in fig.items()), flush=True)
    for k, v in fig.items():
        assert v <= calls * bar[k], (who, k, v, calls * bar[k])
    return fig


# ---- scenes of the integrate ------------------------------------------------------------------------------------------------------------------
SPHERE_RADIUS = 0.37
VOXEL = 0.05
TRUNC = 4 * VOXEL
NEAR = 0.05


def volume_origin(dims):
    """The volume centred on the sphere, off the lattice by a fraction of a voxel (no camera looks exactly at a voxel)."""
    return (np.array([0.013, -0.007, 0.021]) - 0.5 * VOXEL * (np.array(dims) - 1)).astype(np.float32)


def look_at_cameras(V, H, W):
    """[V,16] fp32: cameras on a spiral of radius 2 around the origin looking at it; with V >= 2 the second one sits INSIDE the volume (voxels behind
    it and in front of its near plane)."""
    focal = 1.1 * W
    rows = []
    for v in range(V):
        t = (v + 0.5) / V
        phi, ct = 2.399963 * v + 0.3, 0.9 - 1.6 * t
        st = math.sqrt(1.0 - ct * ct)
        radius = 0.45 if (v == 1 and V >= 2) else 2.0      # (outside the sphere: it sees the near side like everybody else)
        rows.append(camera_record((radius * st * math.cos(phi), radius * st * math.sin(phi), radius * ct), 0.37 * v, focal, float(W), float(H)))
    return np.stack(rows).astype(np.float32)


def sphere_depth(cams, H, W, radius=SPHERE_RADIUS, bad_pixels=True):
    """[V,H,W] fp32 view-space z of the sphere at the origin seen through the pixel centres, 0 on the background; `bad_pixels`: a NaN, an inf and a
    negative pixel per view where the image has room."""
    cams = np.asarray(cams, dtype=np.float64)
    out = np.zeros((cams.shape[0], H, W), dtype=np.float32)
    ys, xs = np.meshgrid(np.arange(H) + 0.5, np.arange(W) + 0.5, indexing="ij")
    for v, rec in enumerate(cams):
        R, T, fx, fy = rec[:9].reshape(3, 3), rec[9:12], rec[12], rec[13]
        dirs = np.stack([(xs - W / 2.0) / fx, (ys - H / 2.0) / fy, np.ones_like(xs)], axis=-1) @ R.T      # cam = x R + T  =>  x = (cam - T) R^T
        o = -T @ R.T
        a, b, c = (dirs * dirs).sum(-1), 2.0 * (dirs @ o), float(o @ o) - radius * radius
        disc = b * b - 4 * a * c
        root = np.sqrt(np.maximum(disc, 0.0))
        near_t, far_t = (-b - root) / (2 * a), (-b + root) / (2 * a)
        t = np.where(near_t > 0, near_t, far_t)      # (from inside the sphere: the far intersection)
        out[v] = np.where((disc > 0) & (t > 0), t, 0.0)
        if bad_pixels and H * W >= 12:
            flat = out[v].reshape(-1)
            flat[(7 * v + 3) % (H * W)] = np.nan
            flat[(11 * v + 5) % (H * W)] = np.inf
            flat[(13 * v + 8) % (H * W)] = -1.0
    return out


def view_colors(V, H, W, seed=0):
    return np.random.default_rng(1000 + seed).random((V, 3, H, W), dtype=np.float32)


_cases = {}


def integrate_case(dims, V, H, W, color):
    """-> (origin fp32 [3], cams, depth, color or None, reference): computed once, shared, never written."""
    key = (tuple(dims), V, H, W, bool(color))
    if key not in _cases:
        origin = volume_origin(dims)
        cams = look_at_cameras(V, H, W)
        depth = sphere_depth(cams, H, W)
        col = view_colors(V, H, W, V) if color else None
        ref = integrate(dims, origin, np.float32(VOXEL), np.float32(TRUNC), np.float32(NEAR), cams, depth, col)
        for a in (origin, cams, depth) + ((col,) if color else ()) + tuple(ref.values()):
            a.setflags(write=False)
        _cases[key] = (origin, cams, depth, col, ref)
    return _cases[key]


# ---- marching tetrahedra ------------------------------------------------------------------------------------------------------------------------
def _tet_corners(perm):
    v0 = np.zeros(3, dtype=np.int64)
    v1 = v0.copy(); v1[perm[0]] = 1
    v2 = v1.copy(); v2[perm[1]] = 1
    return [v0, v1, v2, np.ones(3, dtype=np.int64)]


def _case_faces(corners, inside):
    """The faces of one tetrahedron case as lists of (lo corner, hi corner) edges.  The winding is found HERE from the case alone, with exact
    arithmetic on fictitious edge midpoints: of the two candidate windings the one whose normal points from the inside corners to the outside
    ones.  (The kernel derives the same thing from permutation parities; the two derivations share nothing.)"""
    ins = [k for k in range(4) if inside[k]]
    outs = [k for k in range(4) if not inside[k]]
    if len(ins) in (0, 4):
        return []
    mid = lambda e: (corners[e[0]] + corners[e[1]]) * 0.5
    edge = lambda p, q: (min(p, q), max(p, q))
    toward = np.mean([corners[k] for k in outs], axis=0) - np.mean([corners[k] for k in ins], axis=0)
    if len(ins) == 2:
        (a, b), (c, d) = ins, outs
        loop = [edge(a, c), edge(a, d), edge(b, d), edge(b, c)]
    else:
        a = ins[0] if len(ins) == 1 else outs[0]
        b, c, d = [k for k in range(4) if k != a]
        loop = [edge(a, b), edge(a, c), edge(a, d)]
    normal = np.cross(mid(loop[1]) - mid(loop[0]), mid(loop[2]) - mid(loop[0]))
    assert abs(float(normal @ toward)) > 1e-9
    if normal @ toward < 0:
        loop = [loop[0]] + loop[:0:-1]
    return [loop[:3]] if len(loop) == 3 else [loop[:3], [loop[0], loop[2], loop[3]]]


_CASES = None


def _case_table():
    """[tetrahedron][inside mask] -> faces as triples of (owner corner offset [3], direction 0..6)."""
    global _CASES
    if _CASES is None:
        _CASES = []
        for perm in PERMS:
            corners = _tet_corners(perm)
            row = []
            for m in range(16):
                faces = []
                for face in _case_faces(corners, [(m >> k) & 1 for k in range(4)]):
                    tri = []
                    for lo, hi in face:
                        delta = corners[hi] - corners[lo]
                        tri.append((corners[lo], int(np.flatnonzero((DIRS == delta).all(axis=1))[0])))
                    faces.append(tri)
                row.append(faces)
            _CASES.append((corners, row))
    return _CASES


def marching_tetrahedra(tsdf, weight, dims, origin, voxel, min_weight=1.0):
    """tsdf, weight: fp32 arrays [nz,ny,nx].  -> (keys [Nv] sorted int64, faces [Nf,3] int64 of keys in (cell, tetrahedron, face) order,
    positions [Nv,3] fp64, ratio [Nv] fp64)."""
    nx, ny, nz = dims
    s = np.asarray(tsdf, dtype=np.float32).reshape(nz, ny, nx)
    w = np.asarray(weight, dtype=np.float32).reshape(nz, ny, nx)
    observed = (w >= np.float32(min_weight)) & np.isfinite(s)
    inside = s < 0
    if min(dims) < 2:
        return np.zeros(0, dtype=np.int64), np.zeros((0, 3), dtype=np.int64), np.zeros((0, 3)), np.zeros(0)
    valid = np.ones((nz - 1, ny - 1, nx - 1), dtype=bool)
    for dz in (0, 1):
        for dy in (0, 1):
            for dx in (0, 1):
                valid &= observed[dz:nz - 1 + dz, dy:ny - 1 + dy, dx:nx - 1 + dx]
    # the vertices: ends differ and a valid cell contains the edge (cells c with c <= p and p + dir <= c + 1)
    keys = []
    index = np.arange(nx * ny * nz).reshape(nz, ny, nx)
    for d, (dx, dy, dz) in enumerate(DIRS):
        differ = np.zeros((nz, ny, nx), dtype=bool)
        differ[:nz - dz, :ny - dy, :nx - dx] = inside[:nz - dz, :ny - dy, :nx - dx] != inside[dz:, dy:, dx:]
        held = np.zeros((nz, ny, nx), dtype=bool)
        for oz in range(0, 2 - dz):
            for oy in range(0, 2 - dy):
                for ox in range(0, 2 - dx):      # the cell at p - o
                    held[oz:nz - 1 + oz, oy:ny - 1 + oy, ox:nx - 1 + ox] |= valid
        keys.append(index[differ & held] * 7 + d)
    keys = np.sort(np.concatenate(keys))
    # the faces
    table = _case_table()
    faces = []
    mixed = valid.copy()
    for cz, cy, cx in np.argwhere(mixed):
        corner_in = inside[cz:cz + 2, cy:cy + 2, cx:cx + 2]
        if corner_in.all() or not corner_in.any():
            continue
        for corners, row in table:
            m = sum(int(corner_in[c[2], c[1], c[0]]) << k for k, c in enumerate(corners))
            for tri in row[m]:
                faces.append([int(index[cz + lo[2], cy + lo[1], cx + lo[0]]) * 7 + d for lo, d in tri])
    faces = np.array(faces, dtype=np.int64).reshape(-1, 3)
    owner, d = keys // 7, keys % 7
    p0 = np.stack([owner % nx, (owner // nx) % ny, owner // (nx * ny)], axis=1)
    flat = s.reshape(-1).astype(np.float64)
    far = owner + DIRS[d, 0] + DIRS[d, 1] * nx + DIRS[d, 2] * nx * ny
    ratio = flat[owner] / (flat[owner] - flat[far])
    positions = np.asarray(origin, dtype=np.float64)[None, :] + float(voxel) * (p0 + ratio[:, None] * DIRS[d])
    return keys, faces, positions, ratio


def canonical_rotation(faces):
    """Every face rotated so that its smallest entry comes first (equality up to rotation becomes equality)."""
    faces = np.asarray(faces, dtype=np.int64).reshape(-1, 3)
    k = np.argmin(faces, axis=1)
    rows = np.arange(len(faces))
    return np.stack([faces[rows, k], faces[rows, (k + 1) % 3], faces[rows, (k + 2) % 3]], axis=1)


def check_mesh(who, vertices, faces, colors, tsdf, weight, rgb, dims, origin, voxel, min_weight=1.0):
    """The kernel's mesh (index form) against the reference extraction of the same volume: key set and order, faces up to rotation, positions
    and colours within the bar.  -> (keys, faces as keys)."""
    keys, ref_faces, positions, ratio = marching_tetrahedra(tsdf, weight, dims, origin, voxel, min_weight)
    vertices = np.asarray(vertices).reshape(-1, 3)
    faces = np.asarray(faces).reshape(-1, 3)
    assert len(vertices) == len(keys), f"{who}: {len(vertices)} vertices, the reference has {len(keys)}"
    assert len(faces) == len(ref_faces), f"{who}: {len(faces)} faces, the reference has {len(ref_faces)}"
    if len(faces):
        assert faces.min() >= 0 and faces.max() < len(keys)
        got = keys[faces.astype(np.int64)]      # (vertices are in key order: index -> key)
        assert np.array_equal(canonical_rotation(got), canonical_rotation(ref_faces)), f"{who}: the face list differs from the reference"
    if len(keys):
        bar = POSITION_ULPS * EPS32 * (float(voxel) + float(np.abs(positions).max()))
        err = float(np.abs(vertices.astype(np.float64) - positions).max())
        print(f"[mesh] {who}: {len(keys)} vertices, {len(faces)} faces, position error {err:.3e} (bar {bar:.3e})", flush=True)
        assert err <= bar, (who, err, bar)
        if colors is not None:
            nx, ny, nz = dims
            c = np.asarray(rgb, dtype=np.float64).reshape(3, -1)
            owner, d = keys // 7, keys % 7
            far = owner + DIRS[d, 0] + DIRS[d, 1] * nx + DIRS[d, 2] * nx * ny
            want = (c[:, owner] + ratio[None, :] * (c[:, far] - c[:, owner])).T
            # a + t (b - a) with t within 2 u: three roundings of values <= max|c| and t's error times |b - a|
            cbar = 6.0 * EPS32 * max(float(np.abs(c).max()), 1e-30)
            assert float(np.abs(np.asarray(colors, dtype=np.float64).reshape(-1, 3) - want).max()) <= cbar
    return keys, (keys[faces.astype(np.int64)] if len(faces) else ref_faces)


# ---- invariants of an indexed mesh ------------------------------------------------------------------------------------------------------------------
def mesh_invariants(vertices, faces):
    """-> dict(unused vertices, most uses of a directed edge, histogram of faces per undirected edge, euler, signed volume)."""
    v = np.asarray(vertices, dtype=np.float64).reshape(-1, 3)
    f = np.asarray(faces, dtype=np.int64).reshape(-1, 3)
    used = np.zeros(len(v), dtype=bool)
    used[f.reshape(-1)] = True
    a, b = np.concatenate([f[:, 0], f[:, 1], f[:, 2]]), np.concatenate([f[:, 1], f[:, 2], f[:, 0]])
    n = max(len(v), 1)
    _, directed = np.unique(a * n + b, return_counts=True)
    _, undirected = np.unique(np.minimum(a, b) * n + np.maximum(a, b), return_counts=True)
    volume = float(np.einsum("ij,ij->i", v[f[:, 0]], np.cross(v[f[:, 1]], v[f[:, 2]])).sum() / 6.0) if len(f) else 0.0
    return {"unused": int((~used).sum()), "directed_max": int(directed.max(initial=0)), "per_edge": sorted(set(undirected.tolist())),
            "euler": len(v) - len(undirected) + len(f), "volume": volume}


# ---- volumes of the extraction -------------------------------------------------------------------------------------------------------------------
def analytic_volume(kind, n=20):
    """An analytic signed distance on n^3 voxels (voxel 1, origin 0), clipped to [-1,1]; -> (tsdf fp32 [n,n,n], analytic enclosed volume)."""
    z, y, x = np.meshgrid(*(np.arange(n, dtype=np.float64),) * 3, indexing="ij")
    c = (n - 1) / 2.0 + np.array([0.13, -0.21, 0.07])
    x, y, z = x - c[0], y - c[1], z - c[2]
    if kind == "sphere":
        r = 6.3
        sd, vol = np.sqrt(x * x + y * y + z * z) - r, 4.0 / 3.0 * math.pi * r ** 3
    else:
        R, r = 5.6, 2.02
        sd, vol = np.sqrt((np.sqrt(x * x + y * y) - R) ** 2 + z * z) - r, 2.0 * math.pi ** 2 * R * r * r
    return np.clip(sd, -1.0, 1.0).astype(np.float32), vol


def noise_volume(n=10, seed=5, unobserved=0.0):
    """Noise in [-1,1] with 10 % exact zeros and a positive border; -> (tsdf fp32 [n,n,n], weight fp32 [n,n,n]: 0 on `unobserved` of the voxels)."""
    rng = np.random.default_rng(seed)
    s = rng.uniform(-1.0, 1.0, (n, n, n)).astype(np.float32)
    s[rng.random((n, n, n)) < 0.10] = 0.0
    s[0], s[-1], s[:, 0], s[:, -1], s[:, :, 0], s[:, :, -1] = 1.0, 1.0, 1.0, 1.0, 1.0, 1.0
    w = np.ones((n, n, n), dtype=np.float32)
    w[rng.random((n, n, n)) < unobserved] = 0.0
    return s, w
