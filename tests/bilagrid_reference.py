"""The bilateral-grid slice and the total variation of a set of grids, restated in torch on the CPU (fp64 unless a dtype is given): explicit
corner arithmetic, gradients by autograd.  include/gsr.h states the semantics; tests/test_bilagrid_cpu.py holds this file to
F.grid_sample(align_corners=True, padding_mode="border") and the kernels of csrc/bilagrid.hip to this file.

    fx = (x + 0.5) / W (Gw - 1), fy = (y + 0.5) / H (Gh - 1), fz = clamp((0.299 r + 0.587 g + 0.114 b) (L - 1), 0, L - 1)
    i0 = min(floor(f), n - 2), t = f - i0;  A(p) = the trilinear blend of the 8 corners;  out_i = sum_{j<3} A_ij rgb_j + A_i3

torch.clamp passes the gradient where min <= x <= max, both ends included, and nothing outside: with i0 capped at n - 2 that is the stated
convention -- the slope of cell i0 while the unclamped fz lies in [0, L - 1] (at fz == L - 1 exactly: the last cell's), 0 outside.

Bars (the issue's): 1e-5 of the largest reference value per tensor for outputs and gradients; a pixel whose fp64 fz lies within 1e-4 of an
integer in [0, L - 1] is excused from the IMAGE gradient only (the gradient jumps there), at most 0.5 % of an image."""
import torch

LUMA = (0.299, 0.587, 0.114)
BAR = 1e-5
EXCUSE_DIST = 1e-4
EXCUSE_MAX = 0.005


def identity_grids(N, L, Gh, Gw, dtype=torch.float32):
    eye = torch.tensor([1.0, 0, 0, 0, 0, 1.0, 0, 0, 0, 0, 1.0, 0], dtype=dtype)
    return eye.view(1, 12, 1, 1, 1).repeat(N, 1, L, Gh, Gw).contiguous()


def _cell(f, n):
    i0 = f.detach().floor().clamp(min=0, max=n - 2).long()
    return i0, f - i0


def guidance(image):
    return LUMA[0] * image[0] + LUMA[1] * image[1] + LUMA[2] * image[2]


def slice_image(grid, image):
    """grid [12,L,Gh,Gw], image [3,H,W] (one dtype) -> out [3,H,W]; differentiable in both."""
    _, L, Gh, Gw = grid.shape
    _, H, W = image.shape
    dt = image.dtype
    fx = (torch.arange(W, dtype=dt) + 0.5) / W * (Gw - 1)
    fy = (torch.arange(H, dtype=dt) + 0.5) / H * (Gh - 1)
    fz = (guidance(image) * (L - 1)).clamp(0, L - 1)
    x0, tx = _cell(fx, Gw)
    y0, ty = _cell(fy, Gh)
    z0, tz = _cell(fz, L)
    x0, tx, y0, ty = x0[None, :], tx[None, :], y0[:, None], ty[:, None]
    A = 0
    for dz in (0, 1):
        wz = tz if dz else 1 - tz
        for dy in (0, 1):
            wy = ty if dy else 1 - ty
            for dx in (0, 1):
                wx = tx if dx else 1 - tx
                A = A + (wz * wy * wx)[None] * grid[:, z0 + dz, y0 + dy, x0 + dx]
    ones = torch.ones_like(image[0])
    v = (image[0], image[1], image[2], ones)
    return torch.stack([sum(A[4 * i + j] * v[j] for j in range(4)) for i in range(3)])


def slice_grid_sample(grid, image):
    """The same through torch's 5-D grid_sample."""
    import torch.nn.functional as F
    _, L, Gh, Gw = grid.shape
    _, H, W = image.shape
    dt = image.dtype
    u = ((torch.arange(W, dtype=dt) + 0.5) / W)[None, :].expand(H, W)
    v = ((torch.arange(H, dtype=dt) + 0.5) / H)[:, None].expand(H, W)
    coords = torch.stack([u * 2 - 1, v * 2 - 1, guidance(image) * 2 - 1], dim=-1)[None, None]      # (x, y, z) in [-1, 1]
    A = F.grid_sample(grid[None], coords, mode="bilinear", padding_mode="border", align_corners=True)[0, :, 0]      # [12,H,W]
    ones = torch.ones_like(image[0])
    vv = (image[0], image[1], image[2], ones)
    return torch.stack([sum(A[4 * i + j] * vv[j] for j in range(4)) for i in range(3)])


def slice_with_grads(grid, image, dL_dout, fn=slice_image):
    """-> out, dL/dgrid, dL/dimage (detached, the dtype of the inputs)."""
    g = grid.detach().clone().requires_grad_(True)
    im = image.detach().clone().requires_grad_(True)
    out = fn(g, im)
    out.backward(dL_dout)
    return out.detach(), g.grad, im.grad


def total_variation(X):
    """X [N,12,L,Gh,Gw] -> 0-dim; the literal restatement: mean squared forward difference per axis, summed, over N."""
    N = X.shape[0]
    dl = X[:, :, 1:] - X[:, :, :-1]
    dh = X[:, :, :, 1:] - X[:, :, :, :-1]
    dw = X[:, :, :, :, 1:] - X[:, :, :, :, :-1]
    return ((dl ** 2).sum() / (dl.numel() // N) + (dh ** 2).sum() / (dh.numel() // N) + (dw ** 2).sum() / (dw.numel() // N)) / N


def excused(image64, L):
    """[H,W] bool: pixels whose fp64 fz lies within EXCUSE_DIST of an integer in [0, L - 1] -- their image gradient is not compared."""
    fz = guidance(image64.double()) * (L - 1)
    near = (fz - fz.round()).abs() <= EXCUSE_DIST
    return near & (fz.round() >= 0) & (fz.round() <= L - 1)


def make_case(H, W, L, Gh, Gw, seed, kind="uniform"):
    """grid [12,L,Gh,Gw], image [3,H,W], dL_dout [3,H,W], all fp32.  uniform: pixels in [-0.2, 1.2], the guidance clamps on both sides."""
    g = torch.Generator().manual_seed(seed)
    grid = identity_grids(1, L, Gh, Gw)[0] + 0.5 * torch.randn(12, L, Gh, Gw, generator=g)
    if kind == "uniform":
        image = torch.rand(3, H, W, generator=g) * 1.4 - 0.2
    else:
        image = torch.full((3, H, W), 1.0 if kind == "white" else 0.0)
    dL_dout = torch.randn(3, H, W, generator=g)
    return grid.contiguous(), image.contiguous(), dL_dout.contiguous()


def check_against_reference(got_out, got_dgrid, got_dimage, grid, image, dL_dout, what, allow_excuses=True):
    """The three tensors of a kernel run against this file in fp64, at the issue's bars; prints every figure before it asserts."""
    L = grid.shape[1]
    out, dgrid, dimage = slice_with_grads(grid.double(), image.double(), dL_dout.double())
    e_out = float((got_out.double() - out).abs().max() / out.abs().max())
    e_grid = float((got_dgrid.double() - dgrid).abs().max() / dgrid.abs().max())
    skip = excused(image, L) if allow_excuses else torch.zeros(image.shape[1:], dtype=torch.bool)
    frac = float(skip.float().mean())
    line = f"[bilagrid] {what}: out {e_out:.2e}, dgrid {e_grid:.2e}"
    e_img = None
    if got_dimage is not None:
        err = (got_dimage.double() - dimage).abs().amax(0)
        e_img = float(err[~skip].max() / dimage.abs().max()) if bool((~skip).any()) else 0.0
        line += f", dimage {e_img:.2e} ({frac * 100:.3f} % of the pixels excused)"
    print(line + f" (bar {BAR:g})", flush=True)
    assert frac <= EXCUSE_MAX, (what, frac)
    assert e_out <= BAR, (what, "out", e_out)
    assert e_grid <= BAR, (what, "dgrid", e_grid)
    assert e_img is None or e_img <= BAR, (what, "dimage", e_img)


# ---- the end-to-end check: 50 Adam steps on one identity grid towards a smooth per-pixel affine of the image, with the TV term ------------------
E2E_H, E2E_W, E2E_L, E2E_GH, E2E_GW = 48, 64, 8, 16, 16
E2E_STEPS, E2E_LR, E2E_TV_WEIGHT = 50, 2e-3, 10.0
# |loss after step 50 in fp32 torch - in fp64 torch| / the fp64 value, this file's loop on the CPU (tests/test_bilagrid_cpu.py re-measures it); the
# kernels' loop may differ from the fp64 loop by ten times that
E2E_FP32_MEASURED = 2.25e-7      # fp64 loop: 2.791573e-03 -> 6.548962e-04; fp32 loop: -> 6.548961e-04
E2E_BAR = 10.0 * E2E_FP32_MEASURED


def e2e_case(dtype=torch.float32):
    """image [3,H,W] in [0, 1] and target = gain(x, y) image + offset(x, y), gain and offset smooth in the pixel position and per channel."""
    image = torch.rand(3, E2E_H, E2E_W, generator=torch.Generator().manual_seed(5)).double()
    yy = ((torch.arange(E2E_H, dtype=torch.float64) + 0.5) / E2E_H)[None, :, None]
    xx = ((torch.arange(E2E_W, dtype=torch.float64) + 0.5) / E2E_W)[None, None, :]
    c = torch.arange(3, dtype=torch.float64)[:, None, None]
    gain = 0.75 + 0.35 * xx + 0.1 * c * yy
    offset = 0.06 * torch.sin(3.0 * xx + c) - 0.04 * yy
    return image.to(dtype), (gain * image + offset).to(dtype)


def e2e_loop(grids, image, target, slice_fn, tv_fn, optimizer):
    """E2E_STEPS steps on loss = mean((slice(grids, image) - target)^2) + E2E_TV_WEIGHT tv(grids) -> (loss before the first step, loss after the
    last).  grids: a leaf [1,12,L,Gh,Gw] the optimizer holds; slice_fn(grids, image) -> [3,H,W]; tv_fn(grids) -> 0-dim."""
    def loss_fn():
        return ((slice_fn(grids, image) - target) ** 2).mean() + E2E_TV_WEIGHT * tv_fn(grids)
    first = None
    for _ in range(E2E_STEPS):
        optimizer.zero_grad()
        loss = loss_fn()
        first = float(loss.detach()) if first is None else first
        loss.backward()
        optimizer.step()
    with torch.no_grad():
        return first, float(loss_fn())


def e2e_reference(dtype):
    """The loop through this file and torch.optim.Adam on the CPU in `dtype`."""
    image, target = e2e_case(dtype)
    grids = identity_grids(1, E2E_L, E2E_GH, E2E_GW, dtype).requires_grad_(True)
    opt = torch.optim.Adam([grids], lr=E2E_LR)
    return e2e_loop(grids, image, target, lambda G, im: slice_image(G[0], im), total_variation, opt)
