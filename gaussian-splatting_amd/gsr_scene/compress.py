"""Vector-quantised compression of a trained scene ("Compressed 3D Gaussian Splatting", Niedermayr et al., CVPR 2024; Compact3D; LightGaussian;
gsplat's PngCompression): k-means codebooks over the per-Gaussian parameters -- the 45 floats of `features_rest` first of all -- and 16-bit
indices in place of the rows.

    kmeans(rows[P,D], K, weights=None, iters=10, init=None, generator=None) -> (codebook[K,D], idx[P] int32, inertia[iters] float64)
    compress(model, clusters={"features_rest": 4096, "scaling": 4096, "rotation": 4096}, weights=None, iters=10, generator=None) -> dict
    decompress(c) -> dict in the layout of gsr_scene.load_gaussians_ply
    save_compressed(path, c) / load_compressed(path)                       one .npz, indices as uint16, bit-exact both ways

Both steps of a Lloyd iteration are native (csrc/vq.hip): the assignment runs on the fp32 matrix pipe and never writes a
P x K distance block (gsr_vq_assign), the update is a stable sort and fixed-order fp64 segment sums without floating-point atomics
(gsr_vq_update), so two runs give the same bits.  include/gsr.h states the numerics and the containment contract; INTEGRATION.md 3m the recipe.
There is no CPU fallback.

`weights` ([P], >= 0) is the hook for sensitivity-weighted clustering (a caller accumulates |d image / d parameter| per view); computing
sensitivities, bit-depth quantisation of the codebooks and entropy coding are not part of this module."""
from __future__ import annotations

from typing import Dict, Optional, Tuple

import numpy as np
import torch

DEFAULT_CLUSTERS = {"features_rest": 4096, "scaling": 4096, "rotation": 4096}
MAX_D, MAX_K = 64, 65536


def _pkg():
    import diff_gaussian_rasterization as pkg
    return pkg


class _Lloyd:
    """The two C entry points over one scratch buffer for a fixed (P, D, K)."""

    def __init__(self, P: int, D: int, K: int, device):
        self.pkg = _pkg()
        self.lib = self.pkg._lib.load()
        self.P, self.D, self.K, self.device = P, D, K, device
        nbytes = int(self.lib.gsr_vq_scratch_bytes(P, D, K))
        if nbytes == 0:
            raise ValueError(f"kmeans: need 1 <= D <= {MAX_D} and 1 <= K <= {MAX_K}, got D = {D}, K = {K}")
        self.scratch = torch.empty(nbytes, dtype=torch.uint8, device=device)

    def assign(self, rows, codebook):
        pkg = self.pkg
        idx = torch.empty(self.P, dtype=torch.int32, device=self.device)
        dist2 = torch.empty(self.P, dtype=torch.float32, device=self.device)
        with torch.cuda.device(self.device):
            pkg._lib.check(self.lib.gsr_vq_assign(self.P, self.D, self.K, pkg._ptr(rows), pkg._ptr(codebook), pkg._ptr(idx), pkg._ptr(dist2),
                                                  pkg._ptr(self.scratch), pkg._stream_ptr(self.device)), f"gsr_vq_assign (P {self.P}, D {self.D}, K {self.K})")
        return idx, dist2

    def update(self, rows, weights, idx, codebook):
        """In place on `codebook` (a cluster without weight keeps its row); -> mass [K]."""
        pkg = self.pkg
        mass = torch.empty(self.K, dtype=torch.float32, device=self.device)
        with torch.cuda.device(self.device):
            pkg._lib.check(self.lib.gsr_vq_update(self.P, self.D, self.K, pkg._ptr(rows), pkg._ptr(weights), pkg._ptr(idx), pkg._ptr(codebook),
                                                  pkg._ptr(mass), pkg._ptr(self.scratch), pkg._stream_ptr(self.device)),
                           f"gsr_vq_update (P {self.P}, D {self.D}, K {self.K})")
        return mass


@torch.no_grad()
def kmeans(rows: torch.Tensor, K: int, *, weights: Optional[torch.Tensor] = None, iters: int = 10, init: Optional[torch.Tensor] = None,
           generator: Optional[torch.Generator] = None) -> Tuple[torch.Tensor, torch.Tensor, torch.Tensor]:
    """Lloyd's algorithm over rows [P,D] float32 (1 <= D <= 64) with K <= 65536 centroids -> (codebook [K,D] float32, idx [P] int32,
    inertia [iters] float64).  idx is the assignment of the last iteration, codebook the weighted means of its clusters (idx is -1 for a row
    with a non-finite component, which belongs to no cluster), inertia[i] = sum w dist2 of iteration i's assignment in fp64.

    The rows are centred on their weighted mean, computed in fp64, before clustering: the assignment is translation-invariant and the
    centring removes the cancellation of its score form |c|^2 - 2 x.c.  The mean is added back to the codebook; the means of the LAST update
    are taken over the rows as given, in fp64, so a cluster of one row returns that row bit for bit.
    init: a [K,D] tensor, or K distinct rows drawn with torch.randperm(P, generator=generator).  K > P raises ValueError.
    weights: [P] float32; a negative or non-finite weight counts as 0.
    After every update but the last, the clusters that ended without weight (mass == 0) are re-seeded with the rows of largest w dist2, as far
    as there are rows with w dist2 > 0 (a row on its centroid, without weight or with a non-finite component never seeds).  This costs ONE
    host read per iteration (the number of clusters to seed); everything else stays on the stream."""
    pkg = _pkg()
    if not torch.is_tensor(rows) or rows.dim() != 2 or rows.dtype != torch.float32:
        raise pkg.GsrError(f"kmeans: rows must be a float32 tensor of shape [P,D], got "
                           f"{tuple(rows.shape) if torch.is_tensor(rows) else type(rows).__name__} {getattr(rows, 'dtype', '')}")
    pkg._require_cuda(rows, "rows")
    P, D, K, iters = int(rows.shape[0]), int(rows.shape[1]), int(K), int(iters)
    if K > P:
        raise ValueError(f"kmeans: K = {K} centroids for P = {P} rows")
    if iters < 1:
        raise ValueError(f"kmeans: iters must be at least 1, got {iters}")
    dev = rows.device
    rows = rows.detach().contiguous()
    w = None
    if weights is not None:
        if not torch.is_tensor(weights) or tuple(weights.shape) != (P,) or weights.dtype != torch.float32 or weights.device != dev:
            raise pkg.GsrError(f"kmeans: weights must be a float32 tensor of shape ({P},) on {dev}")
        w = weights.detach().contiguous()
    lloyd = _Lloyd(P, D, K, dev)      # (refuses D, K outside the limits)

    rows64 = rows.double()
    if w is None:
        w64 = torch.ones(P, dtype=torch.float64, device=dev)
    else:
        w64 = torch.where(torch.isfinite(w) & (w > 0), w, torch.zeros_like(w)).double()
    good = torch.isfinite(rows).all(dim=1)
    wm = w64 * good
    total = wm.sum()
    mean = (torch.where(good[:, None], rows64, torch.zeros_like(rows64)) * wm[:, None]).sum(dim=0) / torch.where(total > 0, total, torch.ones_like(total))
    x = (rows64 - mean).float().contiguous()

    if init is None:
        gdev = generator.device if generator is not None else torch.device("cpu")
        pick = torch.randperm(P, generator=generator, device=gdev)[:K].to(dev)
        cb = x[pick].clone()
    else:
        if not torch.is_tensor(init) or tuple(init.shape) != (K, D) or init.dtype != torch.float32 or init.device != dev:
            raise pkg.GsrError(f"kmeans: init must be a float32 tensor of shape ({K}, {D}) on {dev}")
        cb = (init.detach().double() - mean).float().contiguous()

    inertia = torch.zeros(iters, dtype=torch.float64, device=dev)
    idx = None
    for it in range(iters):
        idx, dist2 = lloyd.assign(x, cb)
        score = w64 * dist2.double()
        inertia[it] = score.sum()
        if it == iters - 1:
            break
        mass = lloyd.update(x, w, idx, cb)
        empty = mass == 0
        n_seed = int(torch.minimum(empty.sum(), (score > 0).sum()))      # the one host read of the iteration
        if n_seed:      # only rows that are off their centroid (score > 0: finite, with weight) can seed; what is left of the empty clusters stays
            cb[torch.nonzero(empty)[:n_seed, 0]] = x[torch.topk(score, n_seed).indices]
    out = (cb.double() + mean).float().contiguous()      # what a cluster without weight keeps
    lloyd.update(rows, w, idx, out)
    return out, idx, inertia


def _canonical_rotation(q: torch.Tensor) -> torch.Tensor:
    """Unit quaternions with w >= 0: q and -q are one rotation, and k-means must not average the two signs."""
    q = q / q.norm(dim=1, keepdim=True).clamp_min(1e-30)
    return torch.where(q[:, :1] < 0, -q, q)


@torch.no_grad()
def compress(model: Dict[str, torch.Tensor], clusters: Optional[Dict[str, int]] = None, *, weights: Optional[torch.Tensor] = None, iters: int = 10,
             generator: Optional[torch.Generator] = None) -> dict:
    """model: the dict of gsr_scene.load_gaussians_ply (tensors on the GPU).  Every key of `clusters` (default: features_rest, scaling and
    rotation with 4096 entries each) is flattened to [P, D], clustered with kmeans and replaced by {"codebook": [K,D] float32 on the model's device,
    "idx": [P] uint16 ON THE HOST (what save_compressed writes; decompress moves it to the codebook), "shape": the tensor's shape}; a clustered key
    must be float32; `rotation` is normalised and sign-canonicalised (w >= 0) first.  Every other key passes through untouched.
    A model with non-finite values raises ValueError."""
    clusters = dict(DEFAULT_CLUSTERS if clusters is None else clusters)
    for key in clusters:
        if key not in model:
            raise KeyError(f"compress: the model has no '{key}'")
    for key, t in model.items():
        if torch.is_tensor(t) and t.is_floating_point() and not bool(torch.isfinite(t).all()):
            raise ValueError(f"compress: '{key}' holds non-finite values")
    out = {}
    for key, t in model.items():
        if key not in clusters:
            out[key] = t
            continue
        if not torch.is_tensor(t) or t.dtype != torch.float32:
            raise TypeError(f"compress: '{key}' must be a float32 tensor (decompress returns float32), got {getattr(t, 'dtype', type(t).__name__)}")
        P = int(t.shape[0])
        rows = t.detach().reshape(P, -1).contiguous()
        if key == "rotation":
            rows = _canonical_rotation(rows).contiguous()
        codebook, idx, _ = kmeans(rows, int(clusters[key]), weights=weights, iters=iters, generator=generator)
        out[key] = {"codebook": codebook, "idx": torch.from_numpy(idx.cpu().numpy().astype(np.uint16)), "shape": tuple(int(s) for s in t.shape)}
    return out


def _is_entry(v) -> bool:
    return isinstance(v, dict) and {"codebook", "idx", "shape"} <= set(v)


def decompress(c: dict) -> Dict[str, torch.Tensor]:
    """The model in the layout of load_gaussians_ply: a clustered key is codebook[idx] in its original shape, on the codebook's device."""
    out = {}
    for key, v in c.items():
        if _is_entry(v):
            index = torch.from_numpy(v["idx"].cpu().numpy().astype(np.int64)).to(v["codebook"].device)
            out[key] = v["codebook"][index].reshape(v["shape"])
        else:
            out[key] = v
    return out


def save_compressed(path: str, c: dict) -> None:
    """One .npz at `path`: per clustered key `<key>.codebook` (float32), `<key>.idx` (uint16) and `<key>.shape`, every other key as it is."""
    arrays = {}
    for key, v in c.items():
        if _is_entry(v):
            arrays[key + ".codebook"] = v["codebook"].detach().cpu().numpy()
            arrays[key + ".idx"] = v["idx"].cpu().numpy().astype(np.uint16)
            arrays[key + ".shape"] = np.asarray(v["shape"], dtype=np.int64)
        else:
            arrays[key] = v.detach().cpu().numpy()
    with open(path, "wb") as f:
        np.savez(f, **arrays)


def load_compressed(path: str, device="cpu") -> dict:
    """Inverse of save_compressed, bit for bit."""
    out = {}
    with np.load(path) as z:
        names = list(z.files)
        for name in names:
            if name.endswith(".codebook"):
                key = name[:-len(".codebook")]
                out[key] = {"codebook": torch.from_numpy(z[name]).to(device), "idx": torch.from_numpy(z[key + ".idx"]),
                            "shape": tuple(int(s) for s in z[key + ".shape"])}
            elif not (name.endswith(".idx") or name.endswith(".shape")):
                out[name] = torch.from_numpy(z[name]).to(device)
    return out
