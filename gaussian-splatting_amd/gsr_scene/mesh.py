"""TSDF fusion of rendered depth maps and mesh extraction next to the operator: the step 2DGS, Gaussian Opacity Fields, RaDe-GS and PGSR end with.
Depth maps rendered from the trained Gaussians (the per-pixel probe's median or expected depth) are fused into a dense truncated signed
distance volume; marching tetrahedra turns the volume into an indexed triangle mesh.

    TSDFVolume(origin, voxel_size, dims=(nx, ny, nz), sdf_trunc, device, color=False, near=0.05)
        .integrate(depth [V,H,W] or [H,W], cameras, color=None)           Curless-Levoy update, weight 1 per observation, all views in one kernel
        .extract(min_weight=1.0) -> Mesh(vertices, faces, colors)          marching tetrahedra: indexed, watertight where the volume is observed
    depth_from_probe(probe, alpha=None, kind="median" | "expected")       view-space z of a PixelProbe, 0 where there is none
    save_mesh_ply(path, mesh) / load_mesh_ply(path)                       binary little-endian PLY, round trip bit-exact
    components(mesh) -> Components(vertex_label, face_count)              connected components over vertices
    compact(mesh, keep_face) -> Mesh                                      faces[keep], unreferenced vertices dropped, indices remapped
    filter_components(mesh, min_faces=0, keep_largest=None) -> Mesh       2DGS's post_process_mesh(cluster_to_keep): floaters go
    vertex_normals(mesh) -> [Nv,3]                                        area-weighted, pointing to positive tsdf
    smooth(mesh, iterations=10, lam=0.5, mu=-0.53) -> Mesh                Taubin smoothing: the voxel staircase goes, the volume stays

Both hot pieces are native (csrc/tsdf.hip): gsr_tsdf_integrate walks all V views inside ONE kernel, so the volume is read and
written once per call; gsr_mesh_count / gsr_mesh_emit are count -> scan -> emit with one host read of the two counts in between.  include/gsr.h
states the semantics and the numerics contract; INTEGRATION.md 3n the recipe.  There is no CPU fallback.

    vol = gsr_scene.mesh.TSDFVolume(origin=(-2, -2, -2), voxel_size=4 / 512, dims=(512, 512, 512), sdf_trunc=4 * 4 / 512, device="cuda")
    for cams in batches_of_training_cameras:                              # camera objects or the packed records of gsr_scene.mip.pack_cameras
        depth = torch.stack([gsr_scene.mesh.depth_from_probe(rasterizer_of(c).probe(...)[0]) for c in cams])
        vol.integrate(depth, cams)
    gsr_scene.mesh.save_mesh_ply("mesh.ply", vol.extract())

The clean-up after the extraction is native too (csrc/meshops.hip):

    m = gsr_scene.mesh.filter_components(vol.extract(), keep_largest=1)   # or min_faces=50
    m = gsr_scene.mesh.smooth(m, iterations=10)
    normals = gsr_scene.mesh.vertex_normals(m)

A row of `faces` whose indices are not three different numbers in [0, Nv) is not a face: it joins nothing, counts nowhere and survives no compaction.
Components are connected through shared VERTICES (two closed surfaces touching in one vertex are one component; Open3D's
cluster_connected_triangles joins across shared edges and reports two).

The PLY container is written here with numpy: a mesh needs the list property `vertex_indices`, which the in-tree plyfile stand-in refuses."""
from __future__ import annotations

from typing import NamedTuple, Optional

import numpy as np
import torch

from . import mip as _mip


class Mesh(NamedTuple):
    """vertices [Nv,3] float32, faces [Nf,3] int32 (counter-clockwise seen from outside: normals point to positive tsdf), colors [Nv,3] float32 or
    None.  Vertices are ordered by (owner voxel, edge direction), faces by (cell, tetrahedron, face)."""
    vertices: torch.Tensor
    faces: torch.Tensor
    colors: Optional[torch.Tensor]


def _pkg():
    import diff_gaussian_rasterization as pkg
    return pkg


def depth_from_probe(probe, alpha: Optional[torch.Tensor] = None, kind: str = "median") -> torch.Tensor:
    """[H,W] view-space z for TSDFVolume.integrate from a PixelProbe: `median` is its median_depth (0 where no contributor reaches the threshold,
    which integrate treats as an invalid pixel); `expected` is expected_depth / alpha with the rendered alpha image [H,W] or [1,H,W], 0 where alpha
    is 0."""
    pkg = _pkg()
    if kind == "median":
        return probe.median_depth
    if kind != "expected":
        raise pkg.GsrError(f"depth_from_probe: kind must be 'median' or 'expected', got {kind!r}")
    if alpha is None:
        raise pkg.GsrError("depth_from_probe: kind 'expected' needs the rendered alpha image (expected_depth is not normalised)")
    a = alpha.reshape(probe.expected_depth.shape).to(probe.expected_depth.dtype)
    return torch.where(a > 0, probe.expected_depth / a.clamp_min(1e-30), torch.zeros_like(a))


class TSDFVolume:
    """A dense truncated signed distance volume of dims = (nx, ny, nz) voxels on `device`; voxel (ix,iy,iz) sits at origin + voxel_size (ix,iy,iz).
    State: `tsdf` [nz,ny,nx] (running mean in [-1,1], 1 when fresh), `weight` [nz,ny,nx] (observations), `rgb` [3,nz,ny,nx] with color=True."""

    def __init__(self, origin, voxel_size: float, dims, sdf_trunc: float, device, color: bool = False, near: float = 0.05):
        pkg = _pkg()
        try:
            self.origin = tuple(float(v) for v in origin)
            self.dims = tuple(int(v) for v in dims)
        except (TypeError, ValueError):
            raise pkg.GsrError(f"TSDFVolume: origin must be three numbers and dims three integers, got {origin!r}, {dims!r}")
        if len(self.origin) != 3 or len(self.dims) != 3 or min(self.dims) < 0:
            raise pkg.GsrError(f"TSDFVolume: origin must be three numbers and dims three integers >= 0, got {origin!r}, {dims!r}")
        nx, ny, nz = self.dims
        if nx * ny * nz >= 2 ** 31:
            raise pkg.GsrError(f"TSDFVolume: {nx} x {ny} x {nz} voxels are 2^31 or more")
        self.voxel_size, self.sdf_trunc, self.near = float(voxel_size), float(sdf_trunc), float(near)
        if not (self.voxel_size > 0 and self.sdf_trunc > 0 and self.near >= 0):
            raise pkg.GsrError(f"TSDFVolume: need voxel_size > 0, sdf_trunc > 0, near >= 0, got {voxel_size}, {sdf_trunc}, {near}")
        self.tsdf = torch.ones((nz, ny, nx), dtype=torch.float32, device=torch.device(device))
        self.device = self.tsdf.device      # ("cuda" has become "cuda:0": what the tensors handed to integrate carry)
        self.weight = torch.zeros((nz, ny, nx), dtype=torch.float32, device=self.device)
        self.rgb = torch.zeros((3, nz, ny, nx), dtype=torch.float32, device=self.device) if color else None
        self._sizes_checked = set()         # packed device records whose W, H have been read back once (see _check_sizes)
        pkg._require_cuda(self.tsdf, "TSDFVolume")

    def _check_sizes(self, what: str, cameras, H: int, W: int) -> None:
        """Every record's width and height must be the depth stack's.  Camera objects and host tensors are checked on the host; packed records on
        the device are read back ONCE per tensor (storage, offset, shape, version), so a loop over batches synchronises at most once per batch
        and not at all on a second pass."""
        pkg = _pkg()
        if torch.is_tensor(cameras):
            if cameras.dim() != 2 or cameras.shape[1] != _mip.RECORD:
                return      # (pack_cameras names the shape)
            key = None
            if cameras.device.type != "cpu":
                key = (cameras.untyped_storage().data_ptr(), cameras.storage_offset(), tuple(cameras.shape), tuple(cameras.stride()), cameras._version, H, W)
                if key in self._sizes_checked:
                    return
            sizes = [(float(w), float(h)) for w, h in cameras[:, 14:16].detach().cpu().tolist()]
        else:
            key, cameras = None, list(cameras)
            sizes = [(float(getattr(c, "image_width", W)), float(getattr(c, "image_height", H))) for c in cameras]      # (pack_cameras names a missing one)
        for i, (w, h) in enumerate(sizes):
            if w != W or h != H:
                raise pkg.GsrError(f"{what}: camera {i} is {w:g} x {h:g} (W x H), the depth maps are {W} x {H}")
        if key is not None:
            if len(self._sizes_checked) >= 4096:
                self._sizes_checked.clear()
            self._sizes_checked.add(key)

    @torch.no_grad()
    def integrate(self, depth: torch.Tensor, cameras, color: Optional[torch.Tensor] = None) -> "TSDFVolume":
        """Folds V views into the volume: depth [V,H,W] (or [H,W] with one camera) is view-space z, non-positive / NaN / inf where a pixel has none;
        cameras are camera objects or packed [V,16] records (gsr_scene.mip.pack_cameras) whose width and height are the stack's; color [V,3,H,W]
        (or [3,H,W]) goes with a volume made with color=True.  One kernel for all views.  No host synchronisation with camera objects or host records; packed records on the device are
        read back once per tensor for the size check (_check_sizes)."""
        pkg = _pkg()
        what = "TSDFVolume.integrate"
        if not torch.is_tensor(depth) or depth.dtype != torch.float32 or depth.dim() not in (2, 3):
            raise pkg.GsrError(f"{what}: depth must be a float32 tensor of shape [V,H,W] or [H,W], got "
                               f"{tuple(depth.shape) if torch.is_tensor(depth) else type(depth).__name__} {getattr(depth, 'dtype', '')}")
        pkg._require_cuda(depth, "depth")
        if depth.device != self.device:
            raise pkg.GsrError(f"{what}: depth on {depth.device}, the volume on {self.device}")
        if depth.dim() == 2:
            depth = depth[None]
            color = color[None] if torch.is_tensor(color) and color.dim() == 3 else color
        V, H, W = (int(v) for v in depth.shape)
        if V == 0:
            return self
        if H < 1 or W < 1:
            raise pkg.GsrError(f"{what}: the depth maps must be at least 1 x 1, got {H} x {W}")
        if not torch.is_tensor(cameras):
            cameras = list(cameras)
        cams = _mip.pack_cameras(cameras, self.device)
        if int(cams.shape[0]) != V:
            raise pkg.GsrError(f"{what}: {int(cams.shape[0])} cameras for {V} depth maps")
        self._check_sizes(what, cameras, H, W)      # (the kernel addresses with the call's H and W whatever a record says: this is a courtesy)
        if (color is None) != (self.rgb is None):
            raise pkg.GsrError(f"{what}: color goes with a volume made with color=True (color {'given' if color is not None else 'missing'})")
        if color is not None:
            if not torch.is_tensor(color) or color.dtype != torch.float32 or tuple(color.shape) != (V, 3, H, W):
                raise pkg.GsrError(f"{what}: color must be a float32 tensor of shape {(V, 3, H, W)}, got "
                                   f"{tuple(color.shape) if torch.is_tensor(color) else type(color).__name__} {getattr(color, 'dtype', '')}")
            pkg._require_cuda(color, "color")
            color = color.contiguous()
        depth = depth.contiguous()
        nx, ny, nz = self.dims
        lib = pkg._lib.load()
        with torch.cuda.device(self.device):
            pkg._lib.check(lib.gsr_tsdf_integrate(nx, ny, nz, *self.origin, self.voxel_size, self.sdf_trunc, self.near, V, pkg._ptr(cams), H, W,
                                                  pkg._ptr(depth), pkg._ptr(color), pkg._ptr(self.tsdf), pkg._ptr(self.weight), pkg._ptr(self.rgb),
                                                  pkg._stream_ptr(self.device)), f"gsr_tsdf_integrate ({nx} x {ny} x {nz}, V {V}, {W} x {H})")
        return self

    @torch.no_grad()
    def extract(self, min_weight: float = 1.0) -> Mesh:
        """Marching tetrahedra over the cells whose eight corners have weight >= min_weight: an indexed mesh, every directed edge used at most once,
        closed wherever the surface stays inside observed cells.  One host read (the two counts) between the count and the emit."""
        pkg = _pkg()
        nx, ny, nz = self.dims
        lib = pkg._lib.load()
        nbytes = int(lib.gsr_mesh_scratch_bytes(nx, ny, nz))
        if nbytes == 0 and nx * ny * nz > 0:
            raise pkg.GsrError(f"TSDFVolume.extract: {nx} x {ny} x {nz} voxels are more than the extraction takes (178956970)")
        scratch = torch.empty(nbytes + 128, dtype=torch.uint8, device=self.device)
        scratch = scratch[(-scratch.data_ptr()) % 128:]
        counts = torch.empty(2, dtype=torch.int32, device=self.device)
        with torch.cuda.device(self.device):
            stream = pkg._stream_ptr(self.device)
            pkg._lib.check(lib.gsr_mesh_count(nx, ny, nz, pkg._ptr(self.tsdf), pkg._ptr(self.weight), float(min_weight), pkg._ptr(scratch),
                                              pkg._ptr(counts), stream), f"gsr_mesh_count ({nx} x {ny} x {nz})")
            nv, nf = (int(v) for v in counts.tolist())      # the one synchronisation
            vertices = torch.empty((nv, 3), dtype=torch.float32, device=self.device)
            faces = torch.empty((nf, 3), dtype=torch.int32, device=self.device)
            colors = torch.empty((nv, 3), dtype=torch.float32, device=self.device) if self.rgb is not None else None
            pkg._lib.check(lib.gsr_mesh_emit(nx, ny, nz, *self.origin, self.voxel_size, pkg._ptr(self.tsdf), pkg._ptr(self.rgb), pkg._ptr(scratch),
                                             nv, nf, pkg._ptr(vertices), pkg._ptr(colors), pkg._ptr(faces), stream),
                           f"gsr_mesh_emit ({nx} x {ny} x {nz}, {nv} vertices, {nf} faces)")
        return Mesh(vertices, faces, colors)


# ---- PLY ----------------------------------------------------------------------------------------------------------------------------------
def _to_u8(colors: np.ndarray) -> np.ndarray:
    return np.clip(np.rint(np.nan_to_num(colors.astype(np.float64)) * 255.0), 0, 255).astype(np.uint8)


def save_mesh_ply(path: str, mesh: Mesh) -> None:
    """Binary little-endian PLY: `vertex` with x y z float (and red green blue uchar when the mesh has colours: round(255 c), clamped), `face` with
    `property list uchar int vertex_indices`.  Positions and indices round-trip bit-exactly through load_mesh_ply."""
    v = mesh.vertices.detach().cpu().numpy().astype("<f4").reshape(-1, 3)
    f = mesh.faces.detach().cpu().numpy().astype("<i4").reshape(-1, 3)
    has_color = mesh.colors is not None
    vt = np.dtype([("x", "<f4"), ("y", "<f4"), ("z", "<f4")] + ([("red", "u1"), ("green", "u1"), ("blue", "u1")] if has_color else []))
    vrec = np.empty(len(v), dtype=vt)
    vrec["x"], vrec["y"], vrec["z"] = v[:, 0], v[:, 1], v[:, 2]
    if has_color:
        c = _to_u8(mesh.colors.detach().cpu().numpy().reshape(-1, 3))
        vrec["red"], vrec["green"], vrec["blue"] = c[:, 0], c[:, 1], c[:, 2]
    frec = np.empty(len(f), dtype=np.dtype([("n", "u1"), ("i", "<i4", (3,))]))
    frec["n"], frec["i"] = 3, f
    header = ["ply", "format binary_little_endian 1.0", f"element vertex {len(v)}", "property float x", "property float y", "property float z"]
    if has_color:
        header += ["property uchar red", "property uchar green", "property uchar blue"]
    header += [f"element face {len(f)}", "property list uchar int vertex_indices", "end_header"]
    with open(path, "wb") as out:
        out.write(("\n".join(header) + "\n").encode("ascii"))
        out.write(vrec.tobytes())
        out.write(frec.tobytes())


def load_mesh_ply(path: str) -> Mesh:
    """What save_mesh_ply wrote (that layout only: triangles, float positions, optional uchar colours) -> Mesh on the CPU, colours as c / 255."""
    pkg = _pkg()
    with open(path, "rb") as f:
        data = f.read()
    end = data.find(b"end_header\n")
    if not data.startswith(b"ply\n") or end < 0:
        raise pkg.GsrError(f"load_mesh_ply: {path} is not a PLY file")
    lines = data[:end].decode("ascii").split("\n")
    body = end + len(b"end_header\n")
    if "format binary_little_endian 1.0" not in lines:
        raise pkg.GsrError(f"load_mesh_ply: {path} is not binary little-endian")
    elements, current = {}, None
    for line in lines:
        word = line.split()
        if word[:1] == ["element"]:
            current = word[1]
            elements[current] = (int(word[2]), [])
        elif word[:1] == ["property"] and current is not None:
            elements[current][1].append(" ".join(word[1:]))
    xyz, rgb = ["float x", "float y", "float z"], ["uchar red", "uchar green", "uchar blue"]
    if list(elements) != ["vertex", "face"] or elements["vertex"][1] not in (xyz, xyz + rgb) or elements["face"][1] != ["list uchar int vertex_indices"]:
        raise pkg.GsrError(f"load_mesh_ply: {path} does not have the layout of save_mesh_ply (vertex x y z [red green blue], face vertex_indices)")
    nv, nf = elements["vertex"][0], elements["face"][0]
    has_color = len(elements["vertex"][1]) == 6
    vt = np.dtype([("p", "<f4", (3,))] + ([("c", "u1", (3,))] if has_color else []))
    ft = np.dtype([("n", "u1"), ("i", "<i4", (3,))])
    if len(data) != body + nv * vt.itemsize + nf * ft.itemsize:
        raise pkg.GsrError(f"load_mesh_ply: {path} holds {len(data) - body} bytes of data, its header asks for {nv * vt.itemsize + nf * ft.itemsize}")
    vrec = np.frombuffer(data, dtype=vt, count=nv, offset=body)
    frec = np.frombuffer(data, dtype=ft, count=nf, offset=body + nv * vt.itemsize)
    if nf and not (frec["n"] == 3).all():
        raise pkg.GsrError(f"load_mesh_ply: {path} has faces that are not triangles")
    colors = torch.from_numpy(vrec["c"].astype(np.float32) / np.float32(255.0)) if has_color else None
    return Mesh(torch.from_numpy(vrec["p"].astype(np.float32)), torch.from_numpy(frec["i"].astype(np.int32)), colors)


# ---- clean-up of an extracted mesh (csrc/meshops.hip) ---------------------------------------------------------------------------------------
class Components(NamedTuple):
    """vertex_label [Nv] int32: the smallest vertex index of the vertex's component (a vertex no face uses is its own component); face_count [Nv]
    int32: the faces of the component whose label is the index, 0 at every index that is no label."""
    vertex_label: torch.Tensor
    face_count: torch.Tensor


def _describe(t) -> str:
    return f"{tuple(t.shape)} {t.dtype}" if torch.is_tensor(t) else type(t).__name__


def _checked_mesh(what: str, mesh):
    """-> (vertices, faces, colors) contiguous, after the shape / dtype / device checks every clean-up call shares."""
    pkg = _pkg()
    try:
        v, f, c = mesh.vertices, mesh.faces, mesh.colors
    except AttributeError:
        raise pkg.GsrError(f"{what}: expected a Mesh(vertices, faces, colors), got {type(mesh).__name__}")
    if not torch.is_tensor(v) or v.dtype != torch.float32 or v.dim() != 2 or v.shape[1] != 3:
        raise pkg.GsrError(f"{what}: vertices must be a float32 tensor of shape [Nv,3], got {_describe(v)}")
    if not torch.is_tensor(f) or f.dtype != torch.int32 or f.dim() != 2 or f.shape[1] != 3:
        raise pkg.GsrError(f"{what}: faces must be an int32 tensor of shape [Nf,3], got {_describe(f)}")
    if c is not None and (not torch.is_tensor(c) or c.dtype != torch.float32 or tuple(c.shape) != tuple(v.shape)):
        raise pkg.GsrError(f"{what}: colors must be None or a float32 tensor of shape {tuple(v.shape)}, got {_describe(c)}")
    pkg._require_cuda(v, "vertices")
    for name, t in (("faces", f), ("colors", c)):
        if t is not None and t.device != v.device:
            raise pkg.GsrError(f"{what}: {name} on {t.device}, vertices on {v.device}")
    if 3 * int(f.shape[0]) >= 2 ** 31:
        raise pkg.GsrError(f"{what}: {int(f.shape[0])} faces have 2^31 or more corners")
    return v.contiguous(), f.contiguous(), (c.contiguous() if c is not None else None)


def _meshops_scratch(lib, nv: int, nf: int, device) -> torch.Tensor:
    nbytes = int(lib.gsr_meshops_scratch_bytes(nv, nf))
    scratch = torch.empty(nbytes + 128, dtype=torch.uint8, device=device)
    return scratch[(-scratch.data_ptr()) % 128:]


@torch.no_grad()
def components(mesh) -> Components:
    """Connected components over vertices (two vertices are connected when a face holds both).  The call synchronises the mesh's stream: the
    host reads one word per round of the labelling."""
    pkg = _pkg()
    v, f, _ = _checked_mesh("components", mesh)
    nv, nf = int(v.shape[0]), int(f.shape[0])
    lib = pkg._lib.load()
    label = torch.empty(nv, dtype=torch.int32, device=v.device)
    count = torch.empty(nv, dtype=torch.int32, device=v.device)
    scratch = _meshops_scratch(lib, nv, nf, v.device)
    with torch.cuda.device(v.device):
        pkg._lib.check(lib.gsr_mesh_components(nv, nf, pkg._ptr(f), pkg._ptr(label), pkg._ptr(count), pkg._ptr(scratch), pkg._stream_ptr(v.device)),
                       f"gsr_mesh_components ({nv} vertices, {nf} faces)")
    return Components(label, count)


def _compact(what: str, v, f, c, keep) -> Mesh:
    pkg = _pkg()
    nv, nf = int(v.shape[0]), int(f.shape[0])
    lib = pkg._lib.load()
    scratch = _meshops_scratch(lib, nv, nf, v.device)
    counts = torch.empty(2, dtype=torch.int32, device=v.device)
    with torch.cuda.device(v.device):
        stream = pkg._stream_ptr(v.device)
        pkg._lib.check(lib.gsr_mesh_compact_count(nv, nf, pkg._ptr(f), pkg._ptr(keep), pkg._ptr(scratch), pkg._ptr(counts), stream),
                       f"gsr_mesh_compact_count ({nv} vertices, {nf} faces)")
        nv2, nf2 = (int(x) for x in counts.tolist())      # the one synchronisation
        vertices = torch.empty((nv2, 3), dtype=torch.float32, device=v.device)
        faces = torch.empty((nf2, 3), dtype=torch.int32, device=v.device)
        colors = torch.empty((nv2, 3), dtype=torch.float32, device=v.device) if c is not None else None
        pkg._lib.check(lib.gsr_mesh_compact_emit(nv, nf, pkg._ptr(v), pkg._ptr(c), pkg._ptr(f), pkg._ptr(keep), pkg._ptr(scratch), nv2, nf2,
                                                 pkg._ptr(vertices), pkg._ptr(colors), pkg._ptr(faces), stream),
                       f"gsr_mesh_compact_emit ({nv} -> {nv2} vertices, {nf} -> {nf2} faces)")
    return Mesh(vertices, faces, colors)


@torch.no_grad()
def compact(mesh, keep_face) -> Mesh:
    """The faces with keep_face[f] set (a [Nf] bool or uint8 tensor; None keeps every face), the vertices they use, indices remapped; both keep
    their relative order.  Rows that are no faces never survive.  One host read (the two counts)."""
    pkg = _pkg()
    v, f, c = _checked_mesh("compact", mesh)
    keep = keep_face
    if keep is not None:
        if not torch.is_tensor(keep) or keep.dtype not in (torch.bool, torch.uint8) or tuple(keep.shape) != (int(f.shape[0]),):
            raise pkg.GsrError(f"compact: keep_face must be a bool or uint8 tensor of shape ({int(f.shape[0])},), got {_describe(keep)}")
        if keep.device != v.device:
            raise pkg.GsrError(f"compact: keep_face on {keep.device}, vertices on {v.device}")
        keep = keep.contiguous().view(torch.uint8) if keep.dtype == torch.bool else keep.contiguous()
    return _compact("compact", v, f, c, keep)


@torch.no_grad()
def filter_components(mesh, min_faces: int = 0, keep_largest: Optional[int] = None) -> Mesh:
    """2DGS's post_process_mesh rule: keeps the faces of every component with at least max(min_faces, the keep_largest-th largest component's
    face count) faces -- ties at the threshold are all kept -- and the vertices they use.  The threshold and the mask are a few torch
    operations on the device; labelling and compaction are native."""
    pkg = _pkg()
    if keep_largest is not None and int(keep_largest) < 1:
        raise pkg.GsrError(f"filter_components: keep_largest must be None or >= 1, got {keep_largest}")
    v, f, c = _checked_mesh("filter_components", mesh)
    nv, nf = int(v.shape[0]), int(f.shape[0])
    if nv == 0 or nf == 0:
        return _compact("filter_components", v, f, c, None)
    label, count = components(Mesh(v, f, None))
    threshold = torch.full((), int(min_faces), dtype=torch.int32, device=v.device)
    if keep_largest is not None:      # (indices that are no label hold 0: more components asked for than there are keeps every face)
        threshold = torch.maximum(threshold, torch.topk(count, min(int(keep_largest), nv)).values[-1])
    first = f[:, 0].long()
    safe = torch.where((first >= 0) & (first < nv), first, torch.zeros_like(first))      # (a row that is no face is dropped by the compaction)
    keep = (count[label[safe].long()] >= threshold).view(torch.uint8)
    return _compact("filter_components", v, f, c, keep)


@torch.no_grad()
def vertex_normals(mesh) -> torch.Tensor:
    """[Nv,3] float32 unit normals, area-weighted (the sum of the incident faces' cross products, in fp64), pointing to positive tsdf for a mesh
    of TSDFVolume.extract; (0,0,0) at a vertex without a face or with a zero sum."""
    pkg = _pkg()
    v, f, _ = _checked_mesh("vertex_normals", mesh)
    nv, nf = int(v.shape[0]), int(f.shape[0])
    lib = pkg._lib.load()
    out = torch.empty((nv, 3), dtype=torch.float32, device=v.device)
    scratch = _meshops_scratch(lib, nv, nf, v.device)
    with torch.cuda.device(v.device):
        pkg._lib.check(lib.gsr_mesh_vertex_normals(nv, nf, pkg._ptr(v), pkg._ptr(f), pkg._ptr(out), pkg._ptr(scratch), pkg._stream_ptr(v.device)),
                       f"gsr_mesh_vertex_normals ({nv} vertices, {nf} faces)")
    return out


@torch.no_grad()
def smooth(mesh, iterations: int = 10, lam: float = 0.5, mu: float = -0.53) -> Mesh:
    """Taubin smoothing: `iterations` times a step towards the neighbours' mean with weight lam, then one with weight mu (negative: it undoes the
    shrinkage).  A neighbour weighs by the faces on the edge to it (include/gsr.h).  Faces and colours are carried over, the input is not written."""
    pkg = _pkg()
    v, f, c = _checked_mesh("smooth", mesh)
    if int(iterations) < 0:
        raise pkg.GsrError(f"smooth: iterations must be >= 0, got {iterations}")
    nv, nf = int(v.shape[0]), int(f.shape[0])
    lib = pkg._lib.load()
    out = torch.empty((nv, 3), dtype=torch.float32, device=v.device)
    scratch = _meshops_scratch(lib, nv, nf, v.device)
    with torch.cuda.device(v.device):
        pkg._lib.check(lib.gsr_mesh_smooth(nv, nf, pkg._ptr(v), pkg._ptr(f), int(iterations), float(lam), float(mu), pkg._ptr(out), pkg._ptr(scratch),
                                           pkg._stream_ptr(v.device)), f"gsr_mesh_smooth ({nv} vertices, {nf} faces, {iterations} iterations)")
    return Mesh(out, f, c)
