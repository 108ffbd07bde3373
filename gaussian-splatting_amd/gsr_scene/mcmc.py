"""3DGS-MCMC density control next to the operator (Kheradmand et al. 2024, "3D Gaussian Splatting as Markov Chain Monte Carlo";
gsplat's `MCMCStrategy`): the scheme that replaces clone / split / prune (gsr_scene/densify.py) by

    a fixed cap on the number of Gaussians                                  add_new(optimizer, cap_max)
    relocation of dead Gaussians onto live ones, image unchanged            relocate(optimizer, dead_mask)
    covariance-shaped noise on the means after every optimizer step         inject_noise(optimizer, noise_scale)

Two pieces are native (csrc/mcmc.hip): the noise is one streaming HIP pass over the raw parameters (gsr_mcmc_inject_noise;
upstream: ~20 small torch kernels and [P,3,3] temporaries per iteration), the opacity / scale correction of a relocated Gaussian is a closed
form in fp64 (gsr_mcmc_relocation; upstream: a double loop of up to 1 326 fp32 powf calls per Gaussian that returns inf for small
opacities).  Everything else is index bookkeeping on the optimizer, with the conventions of densify.py: one tensor per param group, groups
named xyz / f_dc / f_rest / opacity / scaling / rotation, state keys exp_avg / exp_avg_sq -- torch.optim.Adam, gsr_optim.FusedAdam and
diff_gaussian_rasterization.SparseGaussianAdam.  Activations are the reference's: opacity = sigmoid(raw), scale = exp(raw)."""
from __future__ import annotations

from typing import Dict, Optional, Tuple

import torch
import torch.nn as nn

from .densify import GROUPS, _groups, _repack

MAX_RATIO = 51            # upstream's binomial table has 51 rows: a Gaussian sampled more often is corrected as if 51 times
_EPS32 = float(torch.finfo(torch.float32).eps)


def _relocation_closed_form(opacities: torch.Tensor, scales: torch.Tensor, ratios: torch.Tensor) -> Tuple[torch.Tensor, torch.Tensor]:
    """The arithmetic of gsr_mcmc_relocation as a torch fp64 expression (CPU tensors; tests/mcmc_reference.py holds it to upstream's
    double loop): o' = -expm1(log1p(-o) / N), D = sum_k (-1)^k C(N, k+1) o'^(k+1) / sqrt(k+1), scale o / D."""
    o32 = opacities.reshape(-1)
    o = o32.double()
    N = ratios.reshape(-1).clamp(1, MAX_RATIO).double()
    valid = (o32 > 0) & (o32 < 1)
    os_ = torch.where(valid, o, torch.full_like(o, 0.5))
    o1 = -torch.expm1(torch.log1p(-os_) / N)
    D, c, p = torch.zeros_like(o), torch.ones_like(o), torch.ones_like(o)
    for k in range(int(N.max()) if N.numel() else 0):
        c = c * (N - k).clamp(min=0) / (k + 1)      # C(N, k+1), 0 once k >= N
        p = p * o1
        D = D + (-1.0) ** k * c * p / (k + 1) ** 0.5
    f = torch.where(valid, os_ / D, torch.ones_like(o))
    new_o = torch.where(valid, o1.to(torch.float32), o32)
    new_s = torch.where(valid[:, None], (scales.double() * f[:, None]).to(torch.float32), scales)
    return new_o.reshape(opacities.shape), new_s


def _relocation_native(opacities: torch.Tensor, scales: torch.Tensor, ratios: torch.Tensor) -> Tuple[torch.Tensor, torch.Tensor]:
    import diff_gaussian_rasterization as pkg
    lib = pkg._lib.load()
    pkg._require_cuda(opacities, "opacities")
    o = opacities.detach().reshape(-1).contiguous().float()
    s = scales.detach().contiguous().float()
    r = ratios.reshape(-1).to(torch.int32).contiguous()
    n = int(o.numel())
    assert s.shape == (n, 3) and r.numel() == n, "opacities [n] or [n,1], scales [n,3], ratios [n]"
    new_o, new_s = torch.empty_like(o), torch.empty_like(s)
    with torch.cuda.device(o.device):
        pkg._lib.check(lib.gsr_mcmc_relocation(n, pkg._ptr(o), pkg._ptr(s), pkg._ptr(r), pkg._ptr(new_o), pkg._ptr(new_s),
                                               pkg._stream_ptr(o.device)), "gsr_mcmc_relocation")
    return new_o.reshape(opacities.shape), new_s


def compute_relocation(opacities: torch.Tensor, scales: torch.Tensor, ratios: torch.Tensor) -> Tuple[torch.Tensor, torch.Tensor]:
    """gsplat's `compute_relocation` (without its binomial table): ACTIVATED opacities [n] or [n,1], scales [n,3] and the number of copies
    each Gaussian is replaced by, ratios [n] (clamped to 1..51) -> (new_opacities, new_scales).  fp64 inside, HIP for device tensors;
    o == 0 gives opacity 0 and the scale unchanged, o outside [0, 1) or not finite hands both back as they came."""
    if opacities.is_cuda:
        return _relocation_native(opacities, scales, ratios)
    return _relocation_closed_form(opacities.detach().float(), scales.detach().float(), ratios)


def _raw(optimizer) -> Dict[str, torch.Tensor]:
    return {name: g["params"][0] for name, g in _groups(optimizer).items()}


@torch.no_grad()
def inject_noise(optimizer, noise_scale: float, *, noise: Optional[torch.Tensor] = None, generator: Optional[torch.Generator] = None,
                 k: float = 100.0, x0: float = 0.995) -> None:
    """xyz += Sigma xi * sigmoid(k ((1 - opacity) - x0)) * noise_scale, in place on the optimizer's `xyz` tensor, as ONE HIP pass over the raw
    xyz / scaling / rotation / opacity groups (Sigma = R diag(exp(scaling))^2 R^T is never formed).  `noise_scale` is upstream's
    noise_lr * xyz_lr; xi is `noise` ([P,3], standard normal) or drawn here with torch.randn(generator=generator), so that a seed
    reproduces a run.  A Gaussian with a NaN / inf scale, a zero quaternion or a NaN opacity keeps its mean until it is relocated."""
    import diff_gaussian_rasterization as pkg
    p = _raw(optimizer)
    xyz, scaling, rotation, opacity = (p[n].detach() for n in ("xyz", "scaling", "rotation", "opacity"))
    P = int(xyz.shape[0])
    if P == 0:
        return
    pkg._require_cuda(xyz, "xyz")
    if noise is None:
        noise = torch.randn(P, 3, device=xyz.device, dtype=torch.float32, generator=generator)
    for name, t, shape in (("xyz", xyz, (P, 3)), ("scaling", scaling, (P, 3)), ("rotation", rotation, (P, 4)), ("opacity", opacity, (P, 1)),
                           ("noise", noise, (P, 3))):
        if tuple(t.shape) != shape or t.dtype != torch.float32 or not t.is_contiguous() or t.device != xyz.device:
            raise pkg.GsrError(f"inject_noise: {name} must be a contiguous float32 tensor of shape {shape} on {xyz.device}, got "
                               f"{tuple(t.shape)} {t.dtype} on {t.device}")
    lib = pkg._lib.load()
    with torch.cuda.device(xyz.device):
        pkg._lib.check(lib.gsr_mcmc_inject_noise(P, pkg._ptr(xyz), pkg._ptr(scaling), pkg._ptr(rotation), pkg._ptr(opacity), pkg._ptr(noise), 0,
                                                 float(noise_scale), float(k), float(x0), pkg._stream_ptr(xyz.device)), "gsr_mcmc_inject_noise")


def _sample(probs: torch.Tensor, n: int, generator: Optional[torch.Generator]) -> torch.Tensor:
    """n draws with replacement, probability proportional to probs (torch.multinomial takes at most 2^24 categories: beyond that, the
    inverse of the cumulative sum)."""
    if probs.numel() <= 1 << 24:
        return torch.multinomial(probs, n, replacement=True, generator=generator)
    cdf = torch.cumsum(probs.double(), 0)
    u = torch.rand(n, device=probs.device, dtype=torch.float64, generator=generator) * cdf[-1]
    return torch.searchsorted(cdf, u).clamp(max=probs.numel() - 1)


def _corrected(p: Dict[str, torch.Tensor], sampled: torch.Tensor, min_opacity: float) -> Tuple[torch.Tensor, torch.Tensor]:
    """Raw opacity [n,1] and scaling [n,3] of the rows `sampled` once each of them stands for bincount + 1 copies of itself."""
    opacity = torch.sigmoid(p["opacity"].detach()[sampled])
    scale = torch.exp(p["scaling"].detach()[sampled])
    ratios = torch.bincount(sampled, minlength=int(p["xyz"].shape[0]))[sampled] + 1
    new_o, new_s = compute_relocation(opacity, scale, ratios)
    new_o = new_o.clamp(min=min_opacity, max=1.0 - _EPS32)
    return torch.logit(new_o), torch.log(new_s)


def _zero_moments(optimizer, rows: torch.Tensor) -> None:
    for g in _groups(optimizer).values():
        state = optimizer.state.get(g["params"][0], None)
        if state is not None:
            for key in ("exp_avg", "exp_avg_sq"):
                if key in state:
                    state[key][rows] = 0


@torch.no_grad()
def relocate(optimizer, dead_mask: torch.Tensor, *, min_opacity: float = 0.005, sampled: Optional[torch.Tensor] = None,
             generator: Optional[torch.Generator] = None) -> int:
    """gsplat's `relocate` / 3dgs-mcmc's `relocate_gs`: every dead Gaussian (dead_mask [P] or [P,1], bool) becomes a copy of a live one
    drawn with probability proportional to its opacity (with replacement; `sampled`: the live rows to use instead, sampled[i] for the i-th dead row in index order), and
    the live one's opacity and scale are corrected for the copies it now shares its place with.  The Adam moments of the sampled rows are
    zeroed.  In place: the parameters and the optimizer state keep their identity.  Returns the number of relocated Gaussians; 0, and
    nothing is touched, when no Gaussian is dead or none is alive to sample from."""
    p = _raw(optimizer)
    dead_mask = dead_mask.reshape(-1).bool()
    dead = torch.nonzero(dead_mask).squeeze(-1)
    alive = torch.nonzero(~dead_mask).squeeze(-1)
    n = int(dead.numel())
    if n == 0 or alive.numel() == 0:
        return 0
    if sampled is None:
        probs = torch.sigmoid(p["opacity"].detach()[alive]).reshape(-1)
        sampled = alive[_sample(probs, n, generator)]
    sampled = sampled.reshape(-1).to(dead.device, torch.int64)
    assert sampled.numel() == n, "one sampled row per dead row"
    assert not bool(dead_mask[sampled].any()), "sampled rows must be alive"
    raw_o, raw_s = _corrected(p, sampled, min_opacity)
    p["opacity"].detach()[sampled] = raw_o.reshape(-1, 1)
    p["scaling"].detach()[sampled] = raw_s
    for name in GROUPS:
        t = p[name].detach()
        t[dead] = t[sampled]
    _zero_moments(optimizer, sampled)
    return n


@torch.no_grad()
def add_new(optimizer, cap_max: int, *, growth: float = 1.05, min_opacity: float = 0.005, sampled: Optional[torch.Tensor] = None,
            generator: Optional[torch.Generator] = None) -> Dict[str, nn.Parameter]:
    """gsplat's `sample_add` / 3dgs-mcmc's `add_new_gs`: grow to min(cap_max, int(growth P)) Gaussians.  The new ones are copies of rows
    drawn over ALL Gaussians with probability proportional to opacity (`sampled`: the rows to use instead), with the same correction as
    `relocate`; the moments of the sampled rows and of the copies are zero.  Returns the optimizer's parameters by group name -- new
    nn.Parameter objects when Gaussians were added (one repack, as densify.py), the ones it holds when P has reached cap_max already."""
    p = _raw(optimizer)
    P = int(p["xyz"].shape[0])
    n = max(0, min(int(cap_max), int(growth * P)) - P)
    if sampled is not None:
        sampled = sampled.reshape(-1).to(p["xyz"].device, torch.int64)[:n]
        n = int(sampled.numel())
    if n == 0 or P == 0:
        return dict(p)
    if sampled is None:
        sampled = _sample(torch.sigmoid(p["opacity"].detach()).reshape(-1), n, generator)
    raw_o, raw_s = _corrected(p, sampled, min_opacity)
    p["opacity"].detach()[sampled] = raw_o.reshape(-1, 1)
    p["scaling"].detach()[sampled] = raw_s
    _zero_moments(optimizer, sampled)
    src = torch.cat([torch.arange(P, device=sampled.device), sampled])
    return _repack(optimizer, src, P, {})


def attach(gaussians, cap_max: int, *, min_opacity: float = 0.005, growth: float = 1.05, generator: Optional[torch.Generator] = None):
    """Binds MCMC density control to an instance of the reference's `scene.gaussian_model.GaussianModel` (duck-typed: `optimizer` with the
    six named groups and the `_xyz` ... `_rotation` attributes), with the method names of the 3dgs-mcmc code base:

        gaussians.training_setup(opt)
        gsr_scene.mcmc.attach(gaussians, cap_max=1_000_000)
        ...                                                                    # every densification_interval iterations:
        gaussians.relocate_gs(dead_mask=(gaussians.get_opacity <= 0.005).squeeze(-1))
        gaussians.add_new_gs(cap_max=1_000_000)
        ...                                                                    # after every optimizer.step():
        gaussians.inject_noise(xyz_lr, noise_lr=5e5)

    gsr_scene.densify.attach is independent of this one.  Returns the instance."""
    import types

    def _install(self, params):
        self._xyz, self._features_dc, self._features_rest = params["xyz"], params["f_dc"], params["f_rest"]
        self._opacity, self._scaling, self._rotation = params["opacity"], params["scaling"], params["rotation"]

    def relocate_gs(self, dead_mask=None):
        if dead_mask is None:
            dead_mask = (torch.sigmoid(self._opacity.detach()) <= min_opacity).squeeze(-1)
        return relocate(self.optimizer, dead_mask, min_opacity=min_opacity, generator=generator)

    def add_new_gs(self, cap_max=cap_max):
        before = int(self._xyz.shape[0])
        _install(self, add_new(self.optimizer, cap_max, growth=growth, min_opacity=min_opacity, generator=generator))
        return int(self._xyz.shape[0]) - before

    def inject_noise_(self, xyz_lr, noise_lr=5e5):
        inject_noise(self.optimizer, noise_lr * xyz_lr, generator=generator)

    gaussians.relocate_gs = types.MethodType(relocate_gs, gaussians)
    gaussians.add_new_gs = types.MethodType(add_new_gs, gaussians)
    gaussians.inject_noise = types.MethodType(inject_noise_, gaussians)
    return gaussians
