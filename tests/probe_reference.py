"""Reference for the per-pixel probe (include/gsr.h gsr_pixel_probe), built on the oracle without touching it, and the bars both test files hold the
product to (tests/test_probe_cpu.py on the SIMT build, tests/test_gpu_probe.py on the MI355X).

Reference: from `aux` of O.rasterize(..., want_fragile=True, return_aux=True), per tile of the band, the record of the shared walk
(tests/blend_reference.py: power / alpha / keep / Tincl / Texcl / dead), evaluated in fp64; contrib = keep & ~dead, w = alpha * Texcl, T' = Tincl,
z = aux["depths"], g = aux["point_list"].  Per pixel: count = #contrib, expected_depth = sum w z, median = the first contributor with T' < threshold,
top = the contributor with the largest w.  Pixels without a contributor, and pixels outside the band, hold the defaults (0, 0, -1, -1, 0, 0).

Near flags, per pixel -- where a discrete output may legitimately differ between fp32 and fp64:
  near_median  some contributor has T' within 1e-4 relative of the threshold;
  near_top     the two largest weights of the pixel's contributors differ by less than 1e-5;
  near_count   blend_reference.near_threshold: an evaluated pair has alpha within 1e-4 relative of 1/255 or T' within 1e-4 relative of 1e-4.  An entry that
               flips there also scales every later T of the pixel by (1 - alpha), so it explains a median or top mismatch of that pixel as well.

Bars (each measured distance is printed with helpers.parity_report under probe_*), on pixels outside aux["fragile"]:
  count, median_id, top_id  equal.  A mismatch is acceptable only on a pixel flagged near (count: near_count; median_id: near_median or near_count;
                            top_id: near_top or near_count): unexplained mismatches are 0, explained ones at most 1 per 1000 pixels with a contributor;
  expected_depth            within 1e-5 of max |reference|: the project's image bar for sum w c with c <= 1, scaled by the largest value of the quantity;
  top_weight                within 1e-5 absolute: weight_max's bar;
  median_depth              where median_id agrees, within 1e-6 relative of aux["depths"][median_id]: a copy of one fp32 per-Gaussian value;
  inputs                    fragile plus near pixels < 1 % of the frame (a condition on the scene, checked on the reference alone).
Test infrastructure."""
import torch

from helpers import parity_report
from blend_reference import near_threshold, tiles


def reference(aux, s, threshold=0.5, dtype=torch.float64):
    """-> dict of [H,W] tensors: expected_depth, top_weight (`dtype`), median_id, top_id, count (int64), near_median, near_top, near_count, terminated
    (bool), and `longest` (the longest list)."""
    W, H = int(s.image_width), int(s.image_height)
    z_all = aux["depths"].detach().to(dtype)
    e_depth, top_w = torch.zeros(H, W, dtype=dtype), torch.zeros(H, W, dtype=dtype)
    med_id, top_id = torch.full((H, W), -1, dtype=torch.int64), torch.full((H, W), -1, dtype=torch.int64)
    count = torch.zeros(H, W, dtype=torch.int64)
    near_m, near_t, near_c, terminated = (torch.zeros(H, W, dtype=torch.bool) for _ in range(4))
    longest = 0
    for t in tiles(aux, s, dtype):
        yy0, yy1, x0, x1 = t.window
        ids, n, hh, ww = t.ids, t.n, yy1 - yy0, x1 - x0
        longest = max(longest, ids.shape[0])
        z = z_all[ids]
        contrib = t.keep & ~t.dead
        w = torch.where(contrib, t.alpha_eff * t.Texcl, torch.zeros_like(t.alpha))
        has = contrib.any(1)
        put = lambda dst, v: dst[yy0:yy1, x0:x1].copy_(v.reshape(hh, ww))      # noqa: E731
        put(count, contrib.sum(1))
        put(e_depth, (w * z[None, :]).sum(1))
        below = contrib & (t.Tincl < threshold)
        first = below.to(torch.int8).argmax(1)      # (the first maximum: the first True)
        put(med_id, torch.where(below.any(1), ids[first], torch.full_like(first, -1)))
        ranked = torch.where(contrib, w, torch.full_like(w, -1.0))
        k = min(2, ranked.shape[1])
        best = torch.topk(ranked, k, dim=1)
        put(top_w, torch.where(has, best.values[:, 0], torch.zeros(n, dtype=dtype)))
        put(top_id, torch.where(has, ids[best.indices[:, 0]], torch.full_like(first, -1)))
        if k == 2:
            put(near_t, (best.values[:, 1] > 0) & (best.values[:, 0] - best.values[:, 1] < 1e-5))
        put(near_m, (contrib & ((t.Tincl - threshold).abs() < 1e-4 * threshold)).any(1))
        put(near_c, near_threshold(t).any(1))
        put(terminated, t.dead[:, -1])
    return dict(expected_depth=e_depth, top_weight=top_w, median_id=med_id, top_id=top_id, count=count, near_median=near_m, near_top=near_t,
                near_count=near_c, terminated=terminated, longest=longest)


def input_condition(ref, aux):
    """Share of the frame that is fragile or near (the bars' input condition: < 1 %)."""
    return float((aux["fragile"] | ref["near_median"] | ref["near_top"] | ref["near_count"]).float().mean())


def check(key, got, ref, aux):
    """The bars of the module docstring on a PixelProbe `got` against reference() output `ref`; returns the measured numbers."""
    ok = ~aux["fragile"]
    g = [t.detach().cpu() for t in got]
    g_ed, g_md, g_mi, g_ti, g_tw, g_n = g[0].double(), g[1].double(), g[2].long(), g[3].long(), g[4].double(), g[5].long()
    has = ok & (ref["count"] > 0)
    n_has = int(has.sum())
    scale = float(ref["expected_depth"].abs().max())
    d_depth = float((g_ed - ref["expected_depth"])[ok].abs().max()) / scale
    d_top = float((g_tw - ref["top_weight"])[ok].abs().max())
    bad_n = ok & (g_n != ref["count"])
    bad_m = ok & (g_mi != ref["median_id"])
    bad_t = ok & (g_ti != ref["top_id"])
    un_n = int((bad_n & ~ref["near_count"]).sum())
    un_m = int((bad_m & ~(ref["near_median"] | ref["near_count"])).sum())
    un_t = int((bad_t & ~(ref["near_top"] | ref["near_count"])).sum())
    same = ok & (g_mi == ref["median_id"]) & (g_mi >= 0)
    z = aux["depths"].detach().double()[g_mi.clamp(min=0)]
    d_med = float(((g_md - z).abs() / z.abs())[same].max()) if bool(same.any()) else 0.0
    nums = dict(expected_depth_rel_max=d_depth, top_weight_abs_max=d_top, median_depth_rel_max=d_med,
                count_mismatch=int(bad_n.sum()), median_id_mismatch=int(bad_m.sum()), top_id_mismatch=int(bad_t.sum()),
                count_unexplained=un_n, median_id_unexplained=un_m, top_id_unexplained=un_t, with_contributor=n_has, with_median=int(same.sum()),
                fragile_share=float(aux["fragile"].float().mean()), near_median_share=float(ref["near_median"].float().mean()),
                near_top_share=float(ref["near_top"].float().mean()), near_count_share=float(ref["near_count"].float().mean()),
                fragile_or_near_share=input_condition(ref, aux), terminated_share=float(ref["terminated"].float().mean()), longest_list=ref["longest"])
    parity_report(key, **nums)
    assert nums["fragile_or_near_share"] < 0.01, nums
    assert [t.dtype for t in got] == [torch.float32, torch.float32, torch.int32, torch.int32, torch.float32, torch.int32]
    assert n_has > 0 and scale > 0.0 and int(same.sum()) > 0
    assert d_depth < 1e-5, nums
    assert d_top < 1e-5, nums
    assert d_med <= 1e-6, nums
    assert un_n == 0 and un_m == 0 and un_t == 0, nums
    assert max(int(bad_n.sum()), int(bad_m.sum()), int(bad_t.sum())) * 1000 <= n_has, nums
    # defaults and consistency, on every pixel
    none = g_n == 0
    assert bool((g_mi[none] == -1).all()) and bool((g_ti[none] == -1).all())
    assert float(g_ed[none].abs().max() if none.any() else 0.0) == 0.0 and float(g_tw[none].abs().max() if none.any() else 0.0) == 0.0
    assert bool(((g_ti >= 0) == (g_n > 0)).all()) and bool((g_n[g_mi >= 0] > 0).all())
    assert float(g_md[g_mi < 0].abs().max() if (g_mi < 0).any() else 0.0) == 0.0
    return nums


# ---- hand-computable frames (no oracle): identity camera at the origin looking down +z, 64 x 48, antialiasing off ----
HAND_W, HAND_H, HAND_PX, HAND_PY = 64, 48, 32, 24


def _on_ray(cam, z):
    """The point at depth z that projects onto the centre of pixel (HAND_PX, HAND_PY): pix = ((ndc + 1) W - 1) / 2."""
    nx, ny = (2 * HAND_PX + 1) / HAND_W - 1.0, (2 * HAND_PY + 1) / HAND_H - 1.0
    return [nx * cam.tanfovx * z, ny * cam.tanfovy * z, z]


def hand_frame(which):
    """-> (camera, dict(means, opac, scales, rot)).  "isolated": index 0 lies behind the camera (culled), index 1 is one opaque Gaussian (opacity 0.95,
    sigma 2.8 px) at depth 4 over pixel (32, 24).  "layers": two concentric Gaussians of sigma 5.5 px over that pixel, index 0 the BACK one (depth 6, opacity
    0.9), index 1 the FRONT one (depth 4, opacity 0.3) -- the ids are not the list positions."""
    from helpers import make_camera
    cam = make_camera(HAND_W, HAND_H)
    if which == "isolated":
        means, opac, scales = [[0.0, 0.0, -5.0], _on_ray(cam, 4.0)], [[0.9], [0.95]], [[0.2] * 3, [0.2] * 3]
    else:
        means, opac, scales = [_on_ray(cam, 6.0), _on_ray(cam, 4.0)], [[0.9], [0.3]], [[0.6] * 3, [0.4] * 3]
    f = lambda v: torch.tensor(v, dtype=torch.float32)      # noqa: E731
    return cam, dict(means=f(means), opac=f(opac), scales=f(scales), rot=f([[1.0, 0.0, 0.0, 0.0]] * 2))


def check_isolated(probe):
    """probe(threshold) -> (PixelProbe, radii) of hand_frame("isolated").  Within 2 px of the centre alpha >= 0.95 exp(-0.5 (2 / 2.8)^2) = 0.73, so T' < 0.5:
    top and median are the Gaussian; beyond 3.31 sigma = 9.4 px alpha < 1/255, so from 12 px on nothing contributes."""
    got, radii = probe(0.5)
    g = [t.detach().cpu() for t in got]
    ys, xs = torch.meshgrid(torch.arange(HAND_H), torch.arange(HAND_W), indexing="ij")
    d = ((xs - HAND_PX) ** 2 + (ys - HAND_PY) ** 2).double().sqrt()
    core, far = d <= 2.0, d >= 12.0
    assert radii.tolist()[0] == 0 and radii.tolist()[1] > 0
    assert bool((g[2][core] == 1).all()) and bool((g[3][core] == 1).all()) and bool((g[5][core] == 1).all())
    assert float((g[1][core] - 4.0).abs().max()) <= 4e-6
    assert float((g[0][core] - g[4][core] * 4.0).abs().max()) <= 4e-5 and float(g[4][core].min()) >= 0.72
    assert abs(float(g[4][HAND_PY, HAND_PX]) - 0.95) <= 1e-5
    for t, v in zip(g, (0.0, 0.0, -1, -1, 0.0, 0)):
        assert bool((t[far] == v).all())
    assert bool(((g[3] == 1) | (g[3] == -1)).all()) and bool(((g[2] == 1) | (g[2] == -1)).all())


def check_layers(probe):
    """probe(threshold) -> (PixelProbe, radii) of hand_frame("layers").  At the centre pixel both Gaussians have G = 1: the front one (index 1) blends with
    w = 0.3 and leaves T' = 0.7, the back one (index 0) with w = 0.7 * 0.9 = 0.63 and T' = 0.07."""
    (a, _), (b, _) = probe(0.5), probe(0.8)
    at = lambda t: t.detach().cpu()[HAND_PY, HAND_PX].item()      # noqa: E731
    assert at(a.count) == 2 and at(b.count) == 2
    assert at(a.median_id) == 0 and at(a.top_id) == 0 and at(b.median_id) == 1 and at(b.top_id) == 0
    assert abs(at(a.median_depth) - 6.0) <= 6e-6 and abs(at(b.median_depth) - 4.0) <= 4e-6
    assert abs(at(a.top_weight) - 0.63) <= 1e-5
    want = 0.3 * 4.0 + 0.7 * 0.9 * 6.0
    assert abs(at(a.expected_depth) - want) <= 1e-5 * 6.0 and at(a.expected_depth) == at(b.expected_depth)
