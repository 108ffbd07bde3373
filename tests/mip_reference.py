"""Reference of the 3D smoothing filter of Mip-Splatting (csrc/mip.hip, gsr_scene/mip.py): upstream's two functions restated in fp64 torch,
operation for operation, the scene generator every mip test uses, and the bars.

compute_3d_filter is GaussianModel.compute_3D_filter of the Mip-Splatting code base: the loop over cameras with `xyz @ R + T`, the depth test
z > 0.2, the clamp of z to 0.001 before the division, the screen enlarged by 15 % on every side, `distance[valid] = min(distance[valid], z[valid])`,
the fill of the unseen with the maximum over the seen, `distance / focal_length * 0.2 ** 0.5`.  The library's two documented departures
(include/gsr.h) are stated here too: nothing seen at all leaves 100000 (upstream raises), and a mean that is not finite is unseen.
filtered_activations is get_scaling_with_3D_filter / get_opacity_with_3D_filter: det1 = prod s^2, det2 = prod (s^2 + f^2),
opacity sigmoid(raw) sqrt(det1 / det2), scales sqrt(s^2 + f^2); in fp64 the two determinants stay in range for every input of the tests.

THE FRAGILE SET.  A Gaussian is fragile when, for some camera, its fp64 z lies within 1e-5 of 0.2, or it passes the depth test and its fp64
projection lies within 1e-5 W (1e-5 H) pixels of a bound of the enlarged screen: an fp32 evaluation may legitimately decide the other way
there.  Fragile Gaussians are left out of value comparisons; a test scene may hold at most 1 % of them (asserted before any kernel runs).

BARS.  Each is 4 x the largest error of the HOST build of the kernel source (tests/test_mip_cpu.py prints them) against this file over all cases
of the CPU test, and never above the cap that follows from the number formats:
  sweep        in units of 2^-24 S_i / focal sqrt(0.2), S_i = max_c (sum_j |m_j R_j2| + |T_2|): a three-term fp32 dot product is within 3 units of
               the fp64 value, the division and the product add one each; cap 8 units.  (A Gaussian nobody sees holds the largest seen
               distance: its unit is taken with the largest S of the scene.)
  activations  forward: relative, element by element (every step is a product, a quotient or a sum of positive terms); gradients: relative to
               the column maximum, cap 1e-5, the project's gradient bar."""
import math

import numpy as np
import torch

NEAR_Z = 0.2
FAR = 100000.0
SQRT_FIFTH = 0.2 ** 0.5
FRAGILE = 1e-5
FRAGILE_CAP = 0.01
SWEEP_CAP_UNITS = 8.0
GRAD_CAP = 1e-5

MEASURED = {
    "sweep_units": 2.75,          # |filter_3D - reference| in the units above (4 x is above the cap: the bar is the cap)
    "scales": 1.24e-7,            # forward, relative per element; at P 1027
    "opacity": 3.43e-7,           # at P 1027
    "draw_scales": 5.87e-8,       # relative to the column maximum; at P 64
    "draw_opacity": 1.39e-7,      # at P 3
}
BARS = {
    "sweep_units": min(4.0 * MEASURED["sweep_units"], SWEEP_CAP_UNITS),
    "scales": 4.0 * MEASURED["scales"],
    "opacity": 4.0 * MEASURED["opacity"],
    "draw_scales": min(4.0 * MEASURED["draw_scales"], GRAD_CAP),
    "draw_opacity": min(4.0 * MEASURED["draw_opacity"], GRAD_CAP),
}


# ---- upstream's two functions ---------------------------------------------------------------------------------------------------------------
def compute_3d_filter(means, cameras):
    """means [P,3], cameras [C,16] (the record of include/gsr.h) -> filter_3D [P] fp64, seen [P] bool."""
    xyz = means.double()
    cams = cameras.double()
    P = xyz.shape[0]
    finite = torch.isfinite(xyz).all(dim=1)
    xyz = torch.where(finite[:, None], xyz, torch.zeros_like(xyz))
    distance = torch.ones(P, dtype=torch.float64) * FAR
    valid_points = torch.zeros(P, dtype=torch.bool)
    focal_length = 0.0
    for cam in cams:
        R, T = cam[:9].reshape(3, 3), cam[9:12]
        focal_x, focal_y, width, height = (float(v) for v in cam[12:16])
        xyz_cam = xyz @ R + T[None, :]
        valid_depth = xyz_cam[:, 2] > NEAR_Z
        x, y, z = xyz_cam[:, 0], xyz_cam[:, 1], xyz_cam[:, 2]
        z = torch.clamp(z, min=0.001)
        x = x / z * focal_x + width / 2.0
        y = y / z * focal_y + height / 2.0
        in_screen = torch.logical_and(torch.logical_and(x >= -0.15 * width, x <= width * 1.15),
                                      torch.logical_and(y >= -0.15 * height, y <= 1.15 * height))
        valid = torch.logical_and(torch.logical_and(valid_depth, in_screen), finite)      # (departure 2: a non-finite mean is unseen)
        distance[valid] = torch.min(distance[valid], xyz_cam[:, 2][valid])
        valid_points = torch.logical_or(valid_points, valid)
        if focal_length < focal_x:
            focal_length = focal_x
    if bool(valid_points.any()):                                                          # (departure 1: upstream raises on the empty max)
        distance[~valid_points] = distance[valid_points].max()
    return distance / focal_length * SQRT_FIFTH, valid_points


def filtered_activations(raw_scales, raw_opacity, filter_3D):
    """raw_scales [P,3], raw_opacity [P,1], filter_3D [P,1] -> scales' [P,3], opacity' [P,1]; fp64, differentiable."""
    scales = torch.exp(raw_scales.double())
    f = filter_3D.double()
    scales_square = torch.square(scales)
    det1 = scales_square.prod(dim=1)
    scales_after_square = scales_square + torch.square(f)
    det2 = scales_after_square.prod(dim=1)
    coef = torch.sqrt(det1 / det2)
    return torch.sqrt(scales_after_square), torch.sigmoid(raw_opacity.double()) * coef[..., None]


def filtered_activations_fp32(raw_scales, raw_opacity, filter_3D):
    """The same chain in the tensors' own precision and on their device: what a training loop runs without the kernel."""
    scales = torch.exp(raw_scales)
    scales_square = torch.square(scales)
    det1 = scales_square.prod(dim=1)
    scales_after_square = scales_square + torch.square(filter_3D)
    det2 = scales_after_square.prod(dim=1)
    coef = torch.sqrt(det1 / det2)
    return torch.sqrt(scales_after_square), torch.sigmoid(raw_opacity) * coef[..., None]


# ---- the scene ------------------------------------------------------------------------------------------------------------------------------
def camera_record(position, roll, focal_x, width, height):
    """One [16] fp64 record: a camera at `position` looking at the origin, rolled about its axis."""
    p = np.asarray(position, dtype=np.float64)
    fwd = -p / np.linalg.norm(p)
    helper = np.array([0.0, 0.0, 1.0]) if abs(fwd[2]) < 0.9 else np.array([1.0, 0.0, 0.0])
    right = np.cross(helper, fwd)
    right /= np.linalg.norm(right)
    up = np.cross(fwd, right)
    c, s = math.cos(roll), math.sin(roll)
    right, up = c * right + s * up, -s * right + c * up
    w2c = np.stack([right, up, fwd])              # cam = w2c (x - p)
    R = w2c.T                                     # cam = x R + T
    T = -w2c @ p
    return np.concatenate([R.reshape(-1), T, [focal_x, 1.01 * focal_x, width, height]])


def make_scene(P, C, seed=None):
    """-> means [P,3] fp32, cameras [C,16] fp32 (torch, CPU): points uniform in [-3,3]^3, cameras on a sphere of radius 4 looking at the origin
    with a random roll, alternating 256 x 192 and 320 x 240, focal_x in {300, 320, 340}, focal_y = 1.01 focal_x.  seed = P + C."""
    rng = np.random.default_rng(P + C if seed is None else seed)
    means = rng.uniform(-3.0, 3.0, size=(P, 3))
    cams = []
    for c in range(C):
        d = rng.normal(size=3)
        d /= np.linalg.norm(d)
        w, h = ((256, 192), (320, 240))[c & 1]
        cams.append(camera_record(4.0 * d, rng.uniform(0.0, 2.0 * math.pi), (300.0, 320.0, 340.0)[int(rng.integers(3))], w, h))
    return torch.from_numpy(means.astype(np.float32)), torch.from_numpy(np.stack(cams).astype(np.float32))


def fragile_set(means, cameras):
    """[P] bool: the Gaussians an fp32 evaluation may legitimately decide differently (see the module docstring)."""
    xyz, cams = means.double(), cameras.double()
    fragile = torch.zeros(xyz.shape[0], dtype=torch.bool)
    for cam in cams:
        R, T = cam[:9].reshape(3, 3), cam[9:12]
        fx, fy, w, h = (float(v) for v in cam[12:16])
        xyz_cam = xyz @ R + T[None, :]
        z = xyz_cam[:, 2]
        fragile |= (z - NEAR_Z).abs() <= FRAGILE
        zc = torch.clamp(z, min=0.001)
        x = xyz_cam[:, 0] / zc * fx + w / 2.0
        y = xyz_cam[:, 1] / zc * fy + h / 2.0
        near_x = ((x + 0.15 * w).abs() <= FRAGILE * w) | ((x - 1.15 * w).abs() <= FRAGILE * w)
        near_y = ((y + 0.15 * h).abs() <= FRAGILE * h) | ((y - 1.15 * h).abs() <= FRAGILE * h)
        fragile |= (z > NEAR_Z) & (near_x | near_y)
    return fragile


def sweep_units(means, cameras, seen):
    """[P] fp64: the error unit of every Gaussian's filter_3D, 2^-24 S_i / focal sqrt(0.2).  (In a scene where nothing is seen every distance is
    the constant 100000, which no dot product produced: S is 100000 there, and the division and the product are all that rounds.)"""
    xyz, cams = means.double(), cameras.double()
    xyz = torch.where(torch.isfinite(xyz), xyz, torch.zeros_like(xyz))
    S = (xyz.abs()[:, None, :] * cams[None, :, 2:9:3].abs()).sum(dim=2) + cams[None, :, 11].abs()      # [P,C]; R_j2 = record[3 j + 2]
    S = S.max(dim=1).values
    S = torch.where(seen, S, S.max().expand_as(S)) if bool(seen.any()) else torch.full_like(S, FAR)
    return 2.0 ** -24 * S / float(cams[:, 12].max()) * SQRT_FIFTH


_SCENES = {}


def scene_reference(P, C):
    """-> means, cameras, filter_3D fp64 [P], seen [P], compared [P] (not fragile), units [P]; computed once per (P, C), the fragile share
    asserted."""
    if (P, C) not in _SCENES:
        means, cams = make_scene(P, C)
        want, seen = compute_3d_filter(means, cams)
        fragile = fragile_set(means, cams)
        assert int(fragile.sum()) <= FRAGILE_CAP * P, (P, C, int(fragile.sum()))
        _SCENES[P, C] = (means, cams, want, seen, ~fragile, sweep_units(means, cams, seen))
    return _SCENES[P, C]


def check_sweep(what, got, got_seen, P, C):
    """got [P] fp32, got_seen [P] uint8 / bool (or None) against scene_reference(P, C) off the fragile set -> the error in units."""
    _, _, want, seen, compared, units = scene_reference(P, C)
    if got_seen is not None:
        assert torch.equal(got_seen.bool()[compared], seen[compared]), f"{what}: seen differs off the fragile set"
    err = float(((got.double() - want).abs() / units)[compared].max())
    print(f"[mip] sweep {what}: P {P} C {C}, seen {float(seen.double().mean()):.2f}, fragile {int((~compared).sum())}, error {err:.2f} units "
          f"(bar {BARS['sweep_units']:.2f}, cap {SWEEP_CAP_UNITS:g})", flush=True)
    assert err <= BARS["sweep_units"], (what, P, C, err)
    return err


# ---- activation cases -----------------------------------------------------------------------------------------------------------------------
def activation_case(P, seed):
    """raw scales in [-16, 2] (upstream's fp32 det1 underflows on some rows), raw opacity in [-8, 8], f = 0 on every fourth row and log-uniform
    in [1e-4, 1] elsewhere, and the two incoming gradients -> raw_scales [P,3], raw_opacity [P,1], filter_3D [P,1], g_s [P,3], g_o [P,1]."""
    g = torch.Generator().manual_seed(seed)
    rs = torch.rand(P, 3, generator=g) * 18.0 - 16.0
    ro = torch.rand(P, 1, generator=g) * 16.0 - 8.0
    f = torch.exp(torch.rand(P, 1, generator=g) * math.log(1e4) + math.log(1e-4))
    f[::4] = 0.0
    if P >= 3:      # two rows whose fp32 prod s^2 is below the smallest normal number for certain, one of them with f = 0 (upstream: 0 / 0)
        rs[1] = torch.tensor([-16.0, -15.5, -15.0])
        rs[2] = torch.tensor([-15.0, -16.0, -14.5])
        f[2] = 0.0
    gs = torch.randn(P, 3, generator=g)
    go = torch.randn(P, 1, generator=g)
    return rs.contiguous(), ro.contiguous(), f.contiguous(), gs.contiguous(), go.contiguous()


_ACT = {}


def activation_reference(P, seed):
    """-> scales' [P,3], opacity' [P,1], dL/draw_scales [P,3], dL/draw_opacity [P,1] in fp64 (autograd of upstream's expression) for
    activation_case(P, seed) with both incoming gradients."""
    if (P, seed) not in _ACT:
        rs, ro, f, gs, go = activation_case(P, seed)
        a, b = rs.double().requires_grad_(True), ro.double().requires_grad_(True)
        s, o = filtered_activations(a, b, f)
        ((s * gs.double()).sum() + (o * go.double()).sum()).backward()
        _ACT[P, seed] = (s.detach(), o.detach(), a.grad, b.grad)
    return _ACT[P, seed]


def rel_elem(got, want):
    """max over the elements of |got - want| / |want| (absolute where the reference is zero)."""
    w = want.abs()
    return float(((got.double() - want).abs() / torch.where(w > 0, w, torch.ones_like(w))).max())


def rel_max(got, want):
    """max |got - want| / max |want|."""
    scale = float(want.abs().max())
    return float((got.double() - want).abs().max()) / (scale if scale > 0 else 1.0)


def check_activations(what, got, P, seed):
    """got = (scales', opacity', dL/draw_scales, dL/draw_opacity) of the kernels on activation_case(P, seed)."""
    want = activation_reference(P, seed)
    figures = {"scales": rel_elem(got[0], want[0]), "opacity": rel_elem(got[1].reshape(-1, 1), want[1]),
               "draw_scales": rel_max(got[2], want[2]), "draw_opacity": rel_max(got[3].reshape(-1, 1), want[3])}
    print(f"[mip] activations {what}: P {P}, " + ", ".join(f"{k} {e:.2e} (bar {BARS[k]:.1e})" for k, e in figures.items()), flush=True)
    for k, e in figures.items():
        assert e <= BARS[k], (what, k, e, BARS[k])
    return figures
