"""Reference for the distortion loss on a rendered frame (include/gsr.h gsr_distortion / gsr_distortion_backward), built on the oracle without touching
it, and the bars the test files hold the product to (tests/test_distortion_cpu.py on the SIMT build, tests/test_gpu_distortion.py on the MI355X).

Reference: from `aux` of O.rasterize(..., want_fragile=True, return_aux=True), per tile of the band, the record of the shared walk
(tests/blend_reference.py), contrib = keep & ~dead, w = alpha_eff * Texcl under contrib, t = aux["depths"] (depth_mode 0) or its reciprocal (1),
sigma = +1 / -1, c = t of the tile's list position 0 and t' = t - c.  By the closed forms of the header, along the list (dim 1):
    A_< = cumsum(w) - w, B_< = cumsum(w t') - w t', A_> = A_tot - cumsum(w), B_> = B_tot - cumsum(w t')
    D = 2 sigma sum w (t' A_< - B_<)                  saved = (A_tot, B_tot)
    u = 2 sigma [t' (A_< - A_>) - B_< + B_>]          v = 2 sigma w (A_< - A_>)          s = g u under contrib
    dL/dalpha = Texcl s - (sum_{j>i} w_j s_j) / (1 - alpha_eff),   m = a_raw dL/dalpha     (tests/feature_geometry_reference.py's lines, with this s)
records [P,7]: words 0..5 of feature_geometry_reference and word 9 = (sum_p g v) * (1 for depth_mode 1, -z^2 for depth_mode 0).
Pixels of aux["fragile"] get dL = 0 in the tests' inputs (mask_fragile) and are not compared in the maps; input condition: fragile share < 1 %.

autograd_oracle / check_reference hold the reference itself to the oracle's autograd before it judges anything: D is formed there by the PAIRWISE sum
sum_ij w_i w_j (t_i - t_j) sgn_ij with sgn = +-sigma by list order from weights recomputed differentiably with the expressions of O._blend_tile, and
asserted equal to the |t_i - t_j| form (the order assumption).  Words 0, 1 (scaled by 0.5 W, 0.5 H) against means2D.grad, word 5 against the opacity
gradient, and -word9 / z^2 against the gradient of a detached copy of the depths that only t reads (the depth path of means3D.grad), each within
REF_BAR = 2e-5 of max |grad| (feature_geometry_reference's: the fp32 rounding of the frame's values inside `aux`).

Bars on the product: the project's 1e-5 of the reference's maximum, per word and per map -- or 2 x d32 where that is larger, d32 being the distance of
reference(..., dtype=float32), the same formulas in torch fp32, from the fp64 reference on the same frame and inputs (never the kernel's output); the
factor 2 is for the kernel's different summation order.  Both distances are printed with helpers.parity_report under distortion_*.
Test infrastructure."""
import torch

from helpers import O, parity_report
from blend_reference import TILE, mask_fragile, tiles  # noqa: F401  (mask_fragile: the tests reach it through this module)

BAR = 1e-5
REF_BAR = 2e-5
WORDS = ("px", "py", "A", "B", "C", "opacity", "invdepth")


def _suffix(x):
    """sum_{j>i} x_j along dim 1."""
    return torch.flip(torch.cumsum(torch.flip(x, dims=[1]), dim=1), dims=[1]) - x


def reference(aux, s, G, depth_mode, dtype=torch.float64):
    """G = dL/dD [H,W] (mask its fragile pixels first) -> dict(distortion [H,W], saved [2,H,W], records [P,7] (words 0..5 and 9) in `dtype`,
    pairs = contributing (pixel, Gaussian) pairs, multi = pixels with at least two contributors, count [H,W] contributors per pixel, pixels [P]
    contributing pixels per Gaussian)."""
    W, H = int(s.image_width), int(s.image_height)
    P = aux["means2D"].shape[0]
    G = G.detach().reshape(H, W).to(dtype)
    op_all = aux["opacity"].detach().to(dtype).reshape(-1)
    z_all = aux["depths"].detach().to(dtype)
    t_all = 1.0 / z_all if depth_mode else z_all
    sig2 = -2.0 if depth_mode else 2.0
    D = torch.zeros(H, W, dtype=dtype)
    saved = torch.zeros(2, H, W, dtype=dtype)
    count = torch.zeros(H, W, dtype=torch.int64)
    rec = torch.zeros(P, 7, dtype=dtype)
    pixels = torch.zeros(P, dtype=torch.int64)      # contributing pixels per Gaussian
    pairs = 0
    for t in tiles(aux, s, dtype):
        yy0, yy1, x0, x1 = t.window
        hh, ww = yy1 - yy0, x1 - x0
        ids, dx, dy, A, B, Cc, Texcl = t.ids, t.dx, t.dy, t.A, t.B, t.Cc, t.Texcl
        contrib = t.keep & ~t.dead
        zero = torch.zeros_like(t.alpha)
        tp = (t_all[ids] - t_all[ids[0]])[None, :]
        w = torch.where(contrib, t.alpha_eff * Texcl, zero)
        wt = w * tp
        cw, cwt = torch.cumsum(w, dim=1), torch.cumsum(wt, dim=1)
        Atot, Btot = cw[:, -1:], cwt[:, -1:]
        Apre, Bpre, Asuf, Bsuf = cw - w, cwt - wt, Atot - cw, Btot - cwt
        put = lambda dst, v: dst[yy0:yy1, x0:x1].copy_(v.reshape(hh, ww))      # noqa: E731
        put(D, sig2 * (w * (tp * Apre - Bpre)).sum(1))
        put(saved[0], Atot[:, 0])
        put(saved[1], Btot[:, 0])
        put(count, contrib.sum(1))
        g = G[yy0:yy1, x0:x1].reshape(-1, 1)
        u = sig2 * (tp * (Apre - Asuf) - Bpre + Bsuf)
        v = sig2 * w * (Apre - Asuf)
        s_i = torch.where(contrib, g * u, zero)
        sw = s_i * w
        dL_dalpha = torch.where(contrib, Texcl * s_i - _suffix(sw) / (1.0 - t.alpha_eff), zero)
        m = torch.where(contrib, t.a_raw * dL_dalpha, zero)
        Gs = torch.where(contrib, t.a_raw / op_all[ids][None, :] * dL_dalpha, zero)
        rec.index_add_(0, ids, torch.stack([(m * (-A * dx - B * dy)).sum(0), (m * (-Cc * dy - B * dx)).sum(0), -0.5 * (m * dx * dx).sum(0),
                                            -(m * dx * dy).sum(0), -0.5 * (m * dy * dy).sum(0), Gs.sum(0), (g * v).sum(0)], dim=1))
        pixels.index_add_(0, ids, contrib.sum(0))
        pairs += int(contrib.sum())
    if not depth_mode:
        rec[:, 6] = rec[:, 6] * (-z_all * z_all)
    return dict(distortion=D, saved=saved, records=rec, pairs=pairs, multi=int((count >= 2).sum()), count=count, pixels=pixels)


def autograd_oracle(cam, leaves, form, G, depth_mode, aa=False):
    """The oracle's autograd on fp64 copies of the leaves `leaves` (tests/test_composite_cpu.make_leaves), loss = sum D G with D the PAIRWISE sum ->
    dict of the leaves' gradients, `means2D` (in the units of means2D.grad), `depth` (the gradient of the depths through t alone, [P]) and
    `distortion` (D [H,W], detached).  Asserts that the signed-by-list-order form equals the |t_i - t_j| form."""
    import test_composite_cpu as T
    s0 = O.settings_from_camera(cam, torch.zeros(3), 3, 1.0, aa)
    keys = ("means", "opac", "cov") if form == "precomp" else ("means", "opac", "scales", "rot")
    lv = {k: leaves[k].detach().double().requires_grad_(True) for k in keys}
    P = lv["means"].shape[0]
    m2 = torch.zeros(P, 3, dtype=torch.float64, requires_grad=True)
    kw = {k: v for k, v in T.call_kwargs({**lv, "colors": None, "shs": None}, form, oracle=True).items() if k not in ("shs", "colors_precomp", "means2D")}
    aux = O.rasterize(s=s0, means2D=m2, colors_precomp=torch.zeros(P, 3, dtype=torch.float64), return_aux=True, **kw)[3]
    W, H = int(s0.image_width), int(s0.image_height)
    G = G.detach().double().reshape(H, W)
    gx, _ = aux["grid"]
    y0, y1 = aux["band"]
    tz = aux["depths"].detach().clone().requires_grad_(True)      # only t reads it: its gradient is the depth path
    t_all = 1.0 / tz if depth_mode else tz
    sigma = -1.0 if depth_mode else 1.0
    D = torch.zeros(H, W, dtype=torch.float64)
    D_abs = torch.zeros(H, W, dtype=torch.float64)
    loss = torch.zeros((), dtype=torch.float64)
    for tile in range(y0 * gx, y1 * gx):
        tyi, txi = divmod(int(tile), gx)
        x0, yy0 = txi * TILE, tyi * TILE
        x1, yy1 = min(x0 + TILE, W), min(yy0 + TILE, H)
        a, b = int(aux["ranges"][tile, 0]), int(aux["ranges"][tile, 1])
        if b <= a:
            continue
        ids = aux["point_list"][a:b].long()
        ys, xs = torch.meshgrid(torch.arange(yy0, yy1), torch.arange(x0, x1), indexing="ij")
        px, py = xs.reshape(-1).double(), ys.reshape(-1).double()
        n, N = px.shape[0], ids.shape[0]
        xy, conic, opac = aux["means2D"][ids], aux["conic"][ids], aux["opacity"][ids]
        # ---- O._blend_tile's expressions ----
        dx = xy[None, :, 0] - px[:, None]
        dy = xy[None, :, 1] - py[:, None]
        A, B, Cc = conic[None, :, 0], conic[None, :, 1], conic[None, :, 2]
        power = -0.5 * (A * dx * dx + Cc * dy * dy) - B * dx * dy
        a_raw = opac[None, :] * torch.exp(power)
        alpha = O._st_min(a_raw, O.ALPHA_MAX)
        with torch.no_grad():
            keep = (power <= 0) & (alpha >= O.ALPHA_MIN)
        alpha_eff = torch.where(keep, alpha, torch.zeros_like(alpha))
        Tincl = torch.cumprod(1.0 - alpha_eff, dim=1)
        Texcl = torch.cat([torch.ones(n, 1, dtype=torch.float64), Tincl[:, :-1]], dim=1)
        with torch.no_grad():
            term = keep & (Tincl < O.T_EPS)
            dead = torch.cumsum(term.to(torch.int32), dim=1) > 0
            contrib = keep & ~dead
        w = torch.where(contrib, alpha_eff * Texcl, torch.zeros_like(alpha_eff))
        # ---- the pairwise sum: M_ij = (t_i - t_j) sgn_ij, sgn = sigma where i lies behind j in the list, -sigma in front ----
        t = t_all[ids]
        diff = t[:, None] - t[None, :]
        pos = torch.arange(N)
        sgn = sigma * torch.sign((pos[:, None] - pos[None, :]).double())
        d_tile = ((w @ (diff * sgn)) * w).sum(1)
        with torch.no_grad():
            D_abs[yy0:yy1, x0:x1] = ((w @ diff.abs()) * w).sum(1).reshape(yy1 - yy0, x1 - x0)
            D[yy0:yy1, x0:x1] = d_tile.reshape(yy1 - yy0, x1 - x0)
        loss = loss + (d_tile * G[yy0:yy1, x0:x1].reshape(-1)).sum()
    assert float(D.max()) > 0.0
    assert float((D - D_abs).abs().max()) <= 1e-12 * float(D_abs.max()), "t is not monotone along a list"
    loss.backward(retain_graph=True)
    depth_path = tz.grad.clone()
    aux["depths"].backward(depth_path)      # ... and chains on to the leaves
    out = {k: v.grad for k, v in lv.items()}
    out.update(means2D=m2.grad, depth=depth_path, distortion=D)
    return out


def check_reference(key, ref, oracle, aux, s):
    """The reference's map (outside the fragile pixels), its words 0, 1 (scaled to the units of means2D.grad), 5 and the depth path -word9 / z^2 against the oracle's autograd."""
    W, H = int(s.image_width), int(s.image_height)
    rec = ref["records"]
    z = aux["depths"].detach().double()
    want2, wanto, wantd = oracle["means2D"].double(), oracle["opac"].double().reshape(-1), oracle["depth"].double()
    got2 = rec[:, :2] * torch.tensor([0.5 * W, 0.5 * H], dtype=rec.dtype)
    got_o = rec[:, 5]      # (frames without antialiasing: word 5 is dL/d(opacity * aa factor))
    got_d = -rec[:, 6] / (z * z)
    d2 = float((got2 - want2[:, :2]).abs().max()) / float(want2[:, :2].abs().max())
    do = float((got_o - wanto).abs().max()) / float(wanto.abs().max())
    dd = float((got_d - wantd).abs().max()) / float(wantd.abs().max())
    dm = float((ref["distortion"] - oracle["distortion"])[~aux["fragile"]].abs().max()) / float(oracle["distortion"].abs().max())      # (the fp64 frame may flip a mask on a fragile pixel)
    frag = float(aux["fragile"].float().mean())
    parity_report(key, map_vs_pairwise=dm, means2D_vs_autograd=d2, opacity_vs_autograd=do, depth_vs_autograd=dd, fragile_share=frag, pairs=ref["pairs"])
    assert frag < 0.01, frag
    assert dm < REF_BAR and d2 < REF_BAR and do < REF_BAR and dd < REF_BAR, (dm, d2, do, dd)
    return d2, do, dd


def check_map(key, got, got_saved, ref, ref32, aux):
    """The bars of the module docstring on D [H,W] and saved [2,H,W] against reference() outputs `ref` (fp64) and `ref32` (fp32)."""
    ok = ~aux["fragile"]
    frag = float(aux["fragile"].float().mean())
    assert got.dtype == torch.float32 and got_saved.dtype == torch.float32
    nums, bars = {}, {}
    planes = (("distortion", got, ref["distortion"], ref32["distortion"]), ("saved_w", got_saved[0], ref["saved"][0], ref32["saved"][0]),
              ("saved_wt", got_saved[1], ref["saved"][1], ref32["saved"][1]))
    for name, g, want, w32 in planes:
        g = g.detach().cpu().double()
        assert tuple(g.shape) == tuple(want.shape)
        scale = float(want.abs().max())
        assert scale > 0.0
        nums[f"{name}_rel_max"] = float((g - want)[ok].abs().max()) / scale
        nums[f"{name}_d32"] = float((w32.double() - want)[ok].abs().max()) / scale
        bars[name] = max(BAR, 2.0 * nums[f"{name}_d32"])
    nums.update(fragile_share=frag, multi=ref["multi"])
    parity_report(key, **nums)
    assert frag < 0.01, frag
    few = ok & (ref["count"] < 2)
    assert float(got.detach().cpu()[few].abs().sum()) == 0.0      # fewer than two contributors: D = 0 exactly
    none = ref["count"] == 0
    assert float(got_saved.detach().cpu()[:, none & ok].abs().sum()) == 0.0
    for name in bars:
        assert nums[f"{name}_rel_max"] <= bars[name], (name, nums)
    return nums


def check_records(key, got, ref, ref32, aux):
    """The bars of the module docstring on the [P,12] records `got` against reference() outputs `ref` (fp64) and `ref32` (fp32)."""
    frag = float(aux["fragile"].float().mean())
    g = got.detach().cpu().double()
    want = ref["records"]
    assert got.dtype == torch.float32 and tuple(g.shape) == (want.shape[0], 12)
    scale = want.abs().amax(dim=0)
    assert bool((scale > 0).all()) and ref["pairs"] > 0
    seven = torch.cat([g[:, :6], g[:, 9:10]], dim=1)
    rel = (seven - want).abs().amax(dim=0) / scale
    d32 = (ref32["records"].double() - want).abs().amax(dim=0) / scale
    nums = {f"{n}_rel_max": float(rel[k]) for k, n in enumerate(WORDS)}
    nums.update({f"{n}_d32": float(d32[k]) for k, n in enumerate(WORDS)})
    nums.update(fragile_share=frag, pairs=ref["pairs"])
    parity_report(key, **nums)
    assert frag < 0.01, frag
    assert float(g[:, [6, 7, 8, 10, 11]].abs().max()) == 0.0
    assert bool((ref["pixels"] == 0).any()) and float(g[ref["pixels"] == 0].abs().sum()) == 0.0      # rows without a contributing pixel
    for k, n in enumerate(WORDS):
        assert float(rel[k]) <= max(BAR, 2.0 * float(d32[k])), (n, nums)
    return nums
