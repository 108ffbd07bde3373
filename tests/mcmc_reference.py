"""The yardstick of the 3DGS-MCMC tests (tests/test_mcmc_cpu.py, tests/test_gpu_mcmc.py): upstream's arithmetic restated in numpy / torch.

Relocation (gsplat's `compute_relocation`, 3dgs-mcmc's utils/reloc_utils.py):
  relocation_double_loop   upstream AS WRITTEN -- a 51 x 51 binomial table, new_o = 1 - (1 - o)^(1/N), the double sum over i and k -- in fp64
  relocation_closed_form   what the library computes: new_o = -expm1(log1p(-o) / N), one sum with C(N, k+1), in fp64
The two agree to 1e-12 or better on the grid o in {0.005 .. 1 - 1e-6} x N in {1 .. 51}; at o = 1e-6 they differ by up to 1.9e-9, which is the
double loop's own `1 - pow` cancellation (pow rounds (1 - o)^(1/N) to 1 ulp of 1, that is 1e-16 absolute, of a new_o of 2e-8).

Relocation kernel: its outputs are fp32 roundings of an fp64 evaluation.  Measured against fp32(relocation_closed_form) over the grid, some 450
random rows with ratios 1..60 and the edge rows: 0 ulp on the host build and on the MI355X (the fp64 expm1 / log1p / sqrt of either side
differ in the last fp64 digits only, which moves an fp32 rounding once in ~10^7 values); the bar is RELOC_ULPS = 2.

Noise (MCMCStrategy.step_post_backward -> inject_noise_to_position):
  noise_delta(dtype)       upstream's expression -- L = R diag(s), Sigma = L L^T, bmm(Sigma, xi) * gate * noise_scale -- in fp64 or fp32
The bar of the noise kernel is component-wise  NOISE_C * eps_fp32 * max(s)^2 * |xi| * g * noise_scale  (+ one fp32 denormal step, 2^-149:
g goes down to e^-99, and no fp32 result is finer than that).  NOISE_C is TWICE what upstream's expression in fp32 shows against fp64 in that
unit on the inputs of the tests (noise_case at P = 1 .. 1027, measure_fp32_restatement): 27.9 measured -- the gate multiplies the rounding of
1 - o and of its own argument by k = 100, so half an ulp there is up to 25 eps of g -- so NOISE_C = 56.  (The 2 098 179 rows of the GPU test's
grid-stride case show 86; that case is held to the smaller constant too.)  The kernel evaluates the gate in fp64 and shows 8.5 of that unit
from raw parameters and 17.2 from activated ones (an opacity rounded to fp32 before the gate sees it: up to 25 by the same argument) on the
host build, 8.5 / 17.2 on the MI355X.  Test infrastructure."""
import math

import numpy as np
import torch

EPS32 = float(np.finfo(np.float32).eps)
DENORM32 = 2.0 ** -149
MAX_RATIO = 51
RELOC_ULPS = 2
NOISE_C_MEASURED = 28.0     # fp32 restatement against fp64, max over the test inputs, in eps max(s)^2 |xi| g noise_scale
NOISE_C = 2.0 * NOISE_C_MEASURED
GATE_K, GATE_X0 = 100.0, 0.995
RELOC_GRID_O = (0.005, 0.01, 0.1, 0.5, 0.9, 0.99, 0.999, 1.0 - 1e-6)
RELOC_GRID_N = (1, 2, 3, 5, 10, 25, 51)


# ---- relocation -----------------------------------------------------------------------------------------------------------------------
def binomial_table(n_max=MAX_RATIO):
    """binoms[n, k] = C(n, k) for k <= n, as upstream builds it (math.comb)."""
    b = np.zeros((n_max, n_max), dtype=np.float64)
    for n in range(n_max):
        for k in range(n + 1):
            b[n, k] = math.comb(n, k)
    return b


def relocation_double_loop(o, N):
    """Upstream's kernel for one Gaussian, in fp64: (new_opacity, scale factor) with new_scale = scale * factor."""
    binoms = binomial_table()
    N = min(max(int(N), 1), MAX_RATIO)
    o = np.float64(o)
    new_o = np.float64(1.0) - np.power(np.float64(1.0) - o, np.float64(1.0) / N)
    denom = np.float64(0.0)
    for i in range(1, N + 1):
        for k in range(i):
            denom += binoms[i - 1, k] * (-1.0) ** k / np.sqrt(np.float64(k + 1)) * np.power(new_o, np.float64(k + 1))
    return float(new_o), float(o / denom)


def relocation_closed_form(o, N):
    """The collapsed form for one Gaussian, in fp64 (hockey stick: sum_{i=k+1}^{N} C(i-1, k) = C(N, k+1))."""
    N = min(max(int(N), 1), MAX_RATIO)
    o = np.float64(o)
    new_o = -np.expm1(np.log1p(-o) / N)
    D = np.float64(0.0)
    for k in range(N):
        D += (-1.0) ** k * math.comb(N, k + 1) * new_o ** (k + 1) / np.sqrt(np.float64(k + 1))
    return float(new_o), float(o / D)


def relocation_expected(opacities, scales, ratios):
    """fp32 arrays [n], [n,3], int ratios [n] -> what gsr_mcmc_relocation must return (fp32 roundings of the fp64 closed form; o == 0: opacity
    0, scale unchanged; o outside [0, 1) or not finite: the inputs)."""
    opacities, scales = np.asarray(opacities, np.float32), np.asarray(scales, np.float32)
    new_o, new_s = opacities.copy(), scales.copy()
    for i, (o, N) in enumerate(zip(opacities.tolist(), np.asarray(ratios).tolist())):
        if 0.0 < o < 1.0:
            a, f = relocation_closed_form(o, N)
            new_o[i] = np.float32(a)
            new_s[i] = (scales[i].astype(np.float64) * f).astype(np.float32)
    return new_o, new_s


def ulps32(a, b):
    """Distance in fp32 steps between two finite float32 arrays (as ordered integers)."""
    def key(x):
        i = np.ascontiguousarray(x, np.float32).view(np.int32).astype(np.int64)
        return np.where(i < 0, -(i & 0x7FFFFFFF), i)
    return np.abs(key(a) - key(b))


def relocation_inputs(n, seed):
    """n rows: the grid first (as far as it fits), then random opacities in (0, 1) on a logit scale with ratios 1..60 (the clamp at 51 is hit),
    the last rows -- from n >= 8 on -- the edges o = 0, 1, NaN, -0.25, 1.5, +inf."""
    g = np.random.default_rng(seed)
    o = (1.0 / (1.0 + np.exp(-g.uniform(-8, 8, n)))).astype(np.float32)
    r = g.integers(1, 61, n).astype(np.int32)
    grid = [(a, b) for a in RELOC_GRID_O + (1e-6,) for b in RELOC_GRID_N]
    for i, (a, b) in enumerate(grid[:max(0, n - 8)]):
        o[i], r[i] = a, b
    if n >= 8:
        o[-6:] = [0.0, 1.0, np.nan, -0.25, 1.5, np.inf]
        r[-8], r[-7] = 60, 0      # (ratio above the table and below 1 on ordinary opacities)
    s = np.exp(g.uniform(np.log(1e-4), np.log(10.0), (n, 3))).astype(np.float32)
    return o, s, r


def check_relocation(got_o, got_s, want_o, want_s, o, s):
    ok = (o > 0) & (o < 1)
    uo, us = ulps32(got_o[ok], want_o[ok]), ulps32(got_s[ok], want_s[ok])
    print(f"[mcmc] relocation: {int(ok.sum())} rows, opacity {int(uo.max(initial=0))} ulp, scale {int(us.max(initial=0))} ulp", flush=True)
    assert int(uo.max(initial=0)) <= RELOC_ULPS and int(us.max(initial=0)) <= RELOC_ULPS
    # the edges: o == 0 -> 0 and the scale as it was; o outside [0, 1) or not finite -> both as they came (bit for bit)
    assert np.array_equal(got_o[~ok].view(np.int32), o[~ok].view(np.int32)) and np.array_equal(got_s[~ok].view(np.int32), s[~ok].view(np.int32))


# ---- noise ----------------------------------------------------------------------------------------------------------------------------
def quaternion_to_rotation(q):
    """[N,4] (w,x,y,z), normalised here -> [N,3,3]; utils/general_utils.py build_rotation, in q's dtype."""
    q = q / torch.sqrt((q * q).sum(dim=1, keepdim=True))
    r, x, y, z = q[:, 0], q[:, 1], q[:, 2], q[:, 3]
    return torch.stack([1 - 2 * (y * y + z * z), 2 * (x * y - r * z), 2 * (x * z + r * y),
                        2 * (x * y + r * z), 1 - 2 * (x * x + z * z), 2 * (y * z - r * x),
                        2 * (x * z - r * y), 2 * (y * z + r * x), 1 - 2 * (x * x + y * y)], dim=1).view(-1, 3, 3)


def noise_gate(opacity_raw, dtype=torch.float64, k=GATE_K, x0=GATE_X0):
    o = torch.sigmoid(opacity_raw.to(dtype)).reshape(-1)
    return 1.0 / (1.0 + torch.exp(-k * ((1 - o) - x0)))


def noise_delta(scaling_raw, rotation, opacity_raw, xi, noise_scale, dtype=torch.float64, k=GATE_K, x0=GATE_X0):
    """Upstream's displacement from RAW parameters, every operation in `dtype`: [P,3]."""
    s = torch.exp(scaling_raw.to(dtype))
    R = quaternion_to_rotation(rotation.to(dtype))
    L = R * s[:, None, :]                          # R diag(s)
    cov = torch.bmm(L, L.transpose(1, 2))
    g = noise_gate(opacity_raw, dtype, k, x0)
    return torch.bmm(cov, xi.to(dtype)[:, :, None]).squeeze(-1) * g[:, None] * noise_scale


def noise_unit(scaling_raw, opacity_raw, xi, noise_scale, k=GATE_K, x0=GATE_X0):
    """eps_fp32 max(s)^2 |xi| g noise_scale per Gaussian, fp64 [P,1]: the unit the noise bar is counted in."""
    s = torch.exp(scaling_raw.double()).amax(dim=1)
    return (EPS32 * s * s * xi.double().norm(dim=1) * noise_gate(opacity_raw, torch.float64, k, x0) * noise_scale)[:, None]


def noise_bar(scaling_raw, opacity_raw, xi, noise_scale, c=NOISE_C):
    return c * noise_unit(scaling_raw, opacity_raw, xi, noise_scale) + DENORM32


def noise_case(P, seed):
    """Raw parameters of P Gaussians: scales 1e-4 .. 10 (log-uniform), unnormalised quaternions (norm 0.1 .. 10), opacities drawn from 0.001
    (gate ~ 0.6), 0.005 (gate 0.5), 0.5 (gate ~ e^-49.5) and a logit-uniform rest, standard-normal xi, a random xyz.  fp32 tensors."""
    g = torch.Generator().manual_seed(seed)
    scaling = (torch.rand(P, 3, generator=g, dtype=torch.float64) * (math.log(10.0) - math.log(1e-4)) + math.log(1e-4)).float()
    q = torch.randn(P, 4, generator=g, dtype=torch.float64)
    rotation = (q / q.norm(dim=1, keepdim=True) * torch.exp(torch.rand(P, 1, generator=g, dtype=torch.float64) * 4.6 - 2.3)).float()
    o = torch.sigmoid(torch.rand(P, generator=g, dtype=torch.float64) * 12 - 7)
    pick = torch.randint(0, 4, (P,), generator=g)
    for j, v in enumerate((0.001, 0.005, 0.5)):
        o[pick == j] = v
    if P >= 3:
        o[:3] = torch.tensor([0.001, 0.005, 0.5], dtype=torch.float64)
    opacity = torch.logit(o).float().reshape(P, 1)
    xi = torch.randn(P, 3, generator=g)
    xyz = torch.randn(P, 3, generator=g) * 3
    return dict(xyz=xyz, scaling=scaling, rotation=rotation, opacity=opacity, xi=xi)


def measure_fp32_restatement(case, noise_scale):
    """max over components of |upstream in fp32 - upstream in fp64| (less one denormal step) in units of noise_unit, over the Gaussians whose
    gate fp32 can hold as a normal number (g >= 2^-126, opacity below ~0.87: beyond, exp overflows in fp32 and upstream's gate is exactly 0,
    an error of 100 % of nothing that says nothing about the arithmetic)."""
    d64 = noise_delta(case["scaling"], case["rotation"], case["opacity"], case["xi"], noise_scale, torch.float64)
    d32 = noise_delta(case["scaling"], case["rotation"], case["opacity"], case["xi"], noise_scale, torch.float32)
    unit = noise_unit(case["scaling"], case["opacity"], case["xi"], noise_scale)
    rows = noise_gate(case["opacity"]) >= 2.0 ** -126
    return float((((d32.double() - d64).abs() - DENORM32).clamp(min=0) / unit)[rows].max())


# poisoned inputs of the noise pass: name -> (field, component or None = the whole row, value)
POISON = {"scale_nan": ("scaling", 1, math.nan), "scale_inf": ("scaling", 2, math.inf), "quat_zero": ("rotation", None, 0.0),
          "opacity_nan": ("opacity", 0, math.nan), "xi_inf": ("xi", 1, math.inf), "xi_nan": ("xi", 0, math.nan)}
