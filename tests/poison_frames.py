"""Frames with non-finite and out-of-range Gaussian parameters, shared by the CPU-shim tests (tests/test_poison_cpu.py) and the GPU tests
(tests/test_gpu_poison.py), and the contract both hold the library to.  A VICTIM is a Gaussian with a poisoned parameter.

  G  geometry poison (NaN / +-inf in a mean, a scale, a quaternion or a precomputed covariance; a scale of 1e15 or 1e19): the victim is culled
     -- radii = 0, tiles_touched = 0, in no list -- and the frame equals the HIDDEN frame (the victim's parameters clean, its mean behind the
     camera) bit for bit in every forward output and every gradient row; the victim's own gradient rows are exactly 0.
  F  odd but finite (negative / zero scale, zero quaternion, opacity 0, < 0, 2, 1/255 and its neighbours, view depth 0.2 and its neighbours):
     ordinary input -- the oracle's bars, bit-exact integers.
  H  huge finite (scale 1e4, 3e5 on every axis): integers against the oracle, finite image and gradients.
  O  NaN / +inf opacity: listed with the reference rectangle, alpha = fminf(0.99, opacity G) = 0.99 wherever the exponent is <= 0; the oracle's
     bars off the fragile pixels; the victim's own gradient rows are the only non-finite ones.
  C  NaN / +-inf colour (one SH coefficient, or colors_precomp): fmaxf(x + 0.5, 0) shows an SH colour that evaluates to NaN or -inf as 0 (a -inf
     coefficient times a negative basis value is +inf; colors_precomp is not clamped, as in the reference).  A colour that is shown non-finite is
     contained to the TILES of the victim's rectangle (oracle's non-finite pixels <= kernel's <= those tiles), its non-finite gradient rows to the
     Gaussians listed there; every other row is the clean frame's to summation order.  Pixels outside the victim's reference-rectangle tiles are
     the clean frame's bits.

The frame: make_camera(128, 96) (identity rotation: view depth = z exactly), make_scene(600, seed 4, s_med 0.05) -- 583 visible, lists up to
37 deep, 0.008 % of the pixels fragile.  `guard_fragile_share` keeps a changed seed from quietly emptying the parity checks.  Test infrastructure."""
import copy
import functools
import math
from dataclasses import dataclass
from typing import NamedTuple, Optional

import numpy as np
import torch

from helpers import O, make_camera, make_scene, oracle_settings

W, H, P = 128, 96, 600
BG = (0.1, 0.2, 0.3)
N_VICTIMS = 6                    # every single-kind frame poisons the same six Gaussians (one per component of the widest row, cov3D)
FRAGILE_SHARE_MAX = 0.01
NAN, INF = math.nan, math.inf
_f = np.float32
T255 = _f(1.0) / _f(255.0)
NEAR = _f(0.2)


class Kind(NamedTuple):
    name: str
    group: str            # G, F, H, O or C
    field: str            # means3D, scales, rotations, cov3D_precomp, opacities, shs, colors_precomp, or "depth" (the mean, moved along its ray)
    comps: object         # flat component indices within the victim's row, victim i takes comps[i % len]; "all" = every component
    value: object         # the value written; "neg" = minus the magnitude of what is there


def _three(prefix, group, field, comps):
    return [Kind(f"{prefix}_nan", group, field, comps, NAN), Kind(f"{prefix}_pinf", group, field, comps, INF), Kind(f"{prefix}_ninf", group, field, comps, -INF)]


KINDS = (
    _three("mean", "G", "means3D", (0, 1, 2)) + _three("scale", "G", "scales", (0, 1, 2)) + _three("quat", "G", "rotations", (0, 1, 2, 3))
    + _three("cov", "G", "cov3D_precomp", (0, 1, 2, 3, 4, 5))
    + [Kind("scale_1e15", "G", "scales", (0, 1, 2), 1e15),          # covariance finite, determinant overflows
       Kind("scale_1e19", "G", "scales", (0, 1, 2), 1e19),          # covariance overflows
       Kind("scale_negative", "F", "scales", (0, 1, 2), "neg"), Kind("scale_zero", "F", "scales", "all", 0.0), Kind("quat_zero", "F", "rotations", "all", 0.0),
       Kind("opacity_zero", "F", "opacities", (0,), 0.0), Kind("opacity_negative", "F", "opacities", (0,), -0.3), Kind("opacity_two", "F", "opacities", (0,), 2.0),
       Kind("opacity_1_255", "F", "opacities", (0,), float(T255)), Kind("opacity_1_255_above", "F", "opacities", (0,), float(np.nextafter(T255, _f(1)))),
       Kind("opacity_1_255_below", "F", "opacities", (0,), float(np.nextafter(T255, _f(0)))),
       Kind("depth_near", "F", "depth", None, float(NEAR)), Kind("depth_near_above", "F", "depth", None, float(np.nextafter(NEAR, _f(1)))),
       Kind("depth_near_below", "F", "depth", None, float(np.nextafter(NEAR, _f(0)))),
       Kind("scale_1e4", "H", "scales", "all", 1e4), Kind("scale_3e5", "H", "scales", "all", 3e5),
       Kind("opacity_nan", "O", "opacities", (0,), NAN), Kind("opacity_pinf", "O", "opacities", (0,), INF)]
    + _three("sh", "C", "shs", (1, 3 * 5 + 2, 3 * 15 + 0)) + _three("color", "C", "colors_precomp", (0, 1, 2)))
KIND = {k.name: k for k in KINDS}


def names(*groups, form=None):
    return [k.name for k in KINDS if k.group in groups and (form is None or form_of(k) == form)]


def form_of(kind):
    """The call form a kind needs: "sh" (shs + scales + rotations), "cov" (shs + cov3D_precomp) or "colors" (colors_precomp + scales + rotations)."""
    return {"cov3D_precomp": "cov", "colors_precomp": "colors"}.get(kind.field, "sh")


@dataclass
class Frame:
    sc: object                                # gsr_synth.Scene
    colors: Optional[torch.Tensor] = None     # colors_precomp (form "colors"), else SH
    cov: Optional[torch.Tensor] = None        # cov3D_precomp (form "cov"), else scales + rotations

    def field(self, name):
        return {"colors_precomp": self.colors, "cov3D_precomp": self.cov}[name] if name in ("colors_precomp", "cov3D_precomp") else getattr(self.sc, name)

    def clone(self):
        sc = copy.copy(self.sc)
        for k in ("means3D", "scales", "rotations", "opacities", "shs"):
            setattr(sc, k, getattr(self.sc, k).clone())
        return Frame(sc, None if self.colors is None else self.colors.clone(), None if self.cov is None else self.cov.clone())

    def oracle_kwargs(self, leaves=None):
        """Keyword arguments of O.rasterize / O.preprocess besides means3D and opacities (leaves: the differentiable stand-ins by field name)."""
        t = (lambda k: leaves[k]) if leaves is not None else self.field
        kw = dict(colors_precomp=t("colors_precomp")) if self.colors is not None else dict(shs=t("shs"))
        kw.update(dict(cov3D_precomp=t("cov3D_precomp")) if self.cov is not None else dict(scales=t("scales"), rotations=t("rotations")))
        return kw

    def fields(self):
        return ["means3D", "opacities"] + list(self.oracle_kwargs())


def camera():
    return make_camera(W, H)


def settings(antialiasing=False):
    return oracle_settings(camera(), bg=torch.tensor(BG), sh_degree=3, antialiasing=antialiasing)


@functools.lru_cache(maxsize=None)
def _clean(form):
    sc = make_scene(P, camera(), seed=4, s_med=0.05)
    colors = torch.rand(P, 3, generator=torch.Generator().manual_seed(2)) if form == "colors" else None
    cov = O.compute_cov3d(sc.scales, sc.rotations, 1.0, torch.float32) if form == "cov" else None
    return Frame(sc, colors, cov)


def clean(form="sh"):
    """The unpoisoned frame of a call form (a fresh copy: the caller may write into it)."""
    return _clean(form).clone()


@functools.lru_cache(maxsize=None)
def _candidates():
    """Victims are taken from the Gaussians that matter: visible with radius > 3 in the clean frame, centre on the screen, nearest first."""
    f = _clean("sh")
    with torch.no_grad():
        pre = O.preprocess(f.sc.means3D, f.sc.opacities, settings(), snug=True, **f.oracle_kwargs())
    xy = pre["means2D"]
    ok = pre["visible"] & (pre["radii"] > 3) & (xy[:, 0] > 0) & (xy[:, 0] < W) & (xy[:, 1] > 0) & (xy[:, 1] < H) & (f.sc.opacities[:, 0] > 0.3)
    idx = torch.nonzero(ok)[:, 0]
    assert int(pre["visible"].sum()) > 500 and len(idx) >= 120, (int(pre["visible"].sum()), len(idx))
    return idx[torch.argsort(pre["depths"][idx])]


def victim_set(n=N_VICTIMS):
    """n victims spread over the nearer half of the candidates (nothing in front of most of them: what they give reaches the image)."""
    cand = _candidates()
    assert 2 * n <= len(cand)
    pick = torch.linspace(0, len(cand) // 2 - 1, n).round().long()
    return cand[pick].tolist()


def poison(frame, kind, victims):
    """Write `kind` into the rows `victims` of `frame`, in place."""
    for i, v in enumerate(victims):
        if kind.field == "depth":      # along the victim's own ray: the screen position stays, the view depth becomes exactly the value
            m = frame.sc.means3D[v].double()
            frame.sc.means3D[v] = torch.stack([m[0] * kind.value / m[2], m[1] * kind.value / m[2], torch.tensor(kind.value, dtype=torch.float64)]).float()
            continue
        row = frame.field(kind.field)[v].view(-1)
        for c in (range(row.numel()) if kind.comps == "all" else [kind.comps[i % len(kind.comps)]]):
            row[c] = -abs(float(row[c])) if kind.value == "neg" else kind.value


def hide(frame, victims):
    """Move the rows `victims` behind the camera (identity rotation at the origin: z < 0), everything else as it is."""
    frame.sc.means3D[victims] = torch.tensor([0.0, 0.0, -5.0])


class Built(NamedTuple):
    kind: object
    victims: list
    poisoned: Frame
    hidden: Frame
    clean: Frame


def build(kind, victims=None):
    """-> the poisoned frame, the hidden frame (victims clean but behind the camera) and the clean frame of one kind."""
    kind = KIND[kind] if isinstance(kind, str) else kind
    victims = victim_set() if victims is None else list(victims)
    form = form_of(kind)
    p, h = clean(form), clean(form)
    poison(p, kind, victims)
    hide(h, victims)
    return Built(kind, victims, p, h, clean(form))


PLACEMENTS = {      # structural placements of culled victims (G kinds)
    "first_last_63_64": ("scale_pinf", [0, 63, 64, P - 1]),
    "workgroup_256_511": ("mean_nan", list(range(256, 512))),      # a whole 256-thread projection workgroup without a listed Gaussian
    "every_gaussian": ("quat_nan", list(range(P))),                # P > 0 with R == 0
}


def build_placement(name):
    kind, victims = PLACEMENTS[name]
    return build(kind, victims)


def build_mixed():
    """One victim of every G, F, O and C kind that the SH + scales + rotations call form can carry, at once -> (frame, {kind name: victim})."""
    kinds = [k for k in KINDS if k.group in "GFOC" and form_of(k) == "sh"]
    victims = victim_set(len(kinds))
    f = clean("sh")
    for k, v in zip(kinds, victims):
        poison(f, k, [v])      # (one victim: the first of the kind's components)
    return f, {k.name: v for k, v in zip(kinds, victims)}


# ---- the oracle's side ----------------------------------------------------------------------------------------------------------------
def loss_weights(seed=0):
    g = torch.Generator().manual_seed(seed)
    return torch.randn(3, H, W, generator=g), torch.randn(1, H, W, generator=g) * 0.3


GRAD_KEYS = {"means3D": "means3D", "opacities": "opacities", "shs": "shs", "colors_precomp": "colors", "scales": "scales", "rotations": "rotations",
             "cov3D_precomp": "cov", "means2D": "means2D"}      # field name -> the name of its gradient array in both test files


def run_oracle(frame, s=None, grad=False):
    """-> (color, radii, invdepth, aux[, grads]) of the oracle with the fragile mask; grads of sum(color wc) + sum(invdepth wd) by gradient name."""
    s = settings() if s is None else s
    if not grad:
        with torch.no_grad():
            return O.rasterize(frame.sc.means3D, None, frame.sc.opacities, s, want_fragile=True, return_aux=True, **frame.oracle_kwargs())
    L = {k: frame.field(k).detach().clone().requires_grad_(True) for k in frame.fields()}
    L["means2D"] = torch.zeros(frame.sc.P, 3, requires_grad=True)
    col, radii, invd, aux = O.rasterize(L["means3D"], L["means2D"], L["opacities"], s, want_fragile=True, return_aux=True, **frame.oracle_kwargs(L))
    wc, wd = loss_weights()
    ((col * wc).sum() + (invd * wd).sum()).backward()
    grads = {GRAD_KEYS[k]: (torch.zeros_like(v) if v.grad is None else v.grad).detach() for k, v in L.items()}
    return col.detach(), radii, invd.detach(), {k: (v.detach() if torch.is_tensor(v) else v) for k, v in aux.items()}, grads


def guard_fragile_share(aux):
    """A frame goes through image parity only while the oracle calls at most 1 % of its pixels fragile: a condition, not a measurement."""
    share = float(aux["fragile"].float().mean())
    assert share <= FRAGILE_SHARE_MAX, f"{share:.4f} of the pixels are fragile: the parity check of this frame would test too little"
    return share


def reference_rect(frame, s=None):
    """[P, 4] (minx, miny, maxx, maxy) of the reference's tile square per Gaussian."""
    with torch.no_grad():
        return O.preprocess(frame.sc.means3D, frame.sc.opacities, settings() if s is None else s, snug=False, **frame.oracle_kwargs())["rect"]


def tile_pixels(rects):
    """bool[H, W]: the pixels of the tiles of the given rectangles [n, 4]."""
    m = torch.zeros(H, W, dtype=torch.bool)
    for x0, y0, x1, y1 in rects.tolist():
        m[y0 * 16:y1 * 16, x0 * 16:x1 * 16] = True
    return m


def listed_in(rects, out):
    """The Gaussians listed in the tiles of the given rectangles (sorted unique indices), from a forward's point list and tile ranges."""
    gx = (W + 15) // 16
    pl, rng = out["point_list"].cpu().long(), out["ranges"].cpu().long()
    got = [torch.zeros(0, dtype=torch.long)]
    for x0, y0, x1, y1 in rects.tolist():
        for ty in range(y0, y1):
            for tx in range(x0, x1):
                a, b = rng[ty * gx + tx].tolist()
                got.append(pl[a:b])
    return torch.unique(torch.cat(got))


# ---- the contract, on the outputs of either runner ---------------------------------------------------------------------------------------
# `out`: color [3,H,W], invdepth [1,H,W], radii [P], tiles_touched [P], point_list [R], ranges [T,2], R (+ final_T, n_contrib of a tracking
# forward); `grads`: {name: array [P, ...]} of the loss of `loss_weights`.  Tensors or numpy arrays, on any device.
FORWARD_KEYS = ("color", "invdepth", "radii", "tiles_touched", "point_list", "ranges", "final_T", "n_contrib")


def _t(a):
    return (a if torch.is_tensor(a) else torch.from_numpy(np.asarray(a))).detach().cpu()


def same_bits(a, b):
    """Equal as bit patterns, NaN included (-0 and +0 differ: no computation here is expected to change either)."""
    a, b = _t(a).contiguous(), _t(b).contiguous()
    if a.shape != b.shape or a.dtype != b.dtype:
        return False
    return torch.equal(a.view(torch.int32), b.view(torch.int32)) if a.dtype == torch.float32 else torch.equal(a, b)


def check_structure(out, n_gaussians=P):
    """What must hold for every frame whatever it contains: R is the sum of tiles_touched, the lists name Gaussians, the ranges lie in [0, R]."""
    R = int(out["R"])
    assert int(_t(out["tiles_touched"]).long().sum()) == R, (int(_t(out["tiles_touched"]).long().sum()), R)
    pl, rng = _t(out["point_list"]).long(), _t(out["ranges"]).long()
    assert pl.numel() == R and (R == 0 or (int(pl.min()) >= 0 and int(pl.max()) < n_gaussians))
    assert int(rng.min()) >= 0 and int(rng.max()) <= R and bool((rng[:, 0] <= rng[:, 1]).all())
    assert int((rng[:, 1] - rng[:, 0]).sum()) == R


def check_culled(out, victims):
    v = torch.tensor(victims, dtype=torch.long)
    assert int(_t(out["radii"])[v].abs().max()) == 0, "a victim has a radius"
    assert int(_t(out["tiles_touched"])[v].abs().max()) == 0, "a victim touches tiles"
    assert not bool(torch.isin(_t(out["point_list"]).long(), v).any()), "a victim is listed"


def check_equals_hidden(out, grads, out_h, grads_h, victims):
    """G: the poisoned frame is the hidden frame bit for bit, and the victims' gradient rows are exactly 0."""
    check_culled(out, victims)
    check_culled(out_h, victims)
    assert int(out["R"]) == int(out_h["R"])
    for k in FORWARD_KEYS:
        if k in out and k in out_h:
            assert same_bits(out[k], out_h[k]), f"{k} differs from the hidden frame"
    if grads is None:
        return
    v = torch.tensor(victims, dtype=torch.long)
    for k in grads:
        a = _t(grads[k])
        assert same_bits(a, grads_h[k]), f"dL/d{k} differs from the hidden frame"
        assert bool(torch.isfinite(a).all()), f"dL/d{k} is not finite"
        assert bool((a[v] == 0).all()), f"dL/d{k}: a victim's row is not zero"


def rows_mask(rows, n=P):
    m = torch.zeros(n, dtype=torch.bool)
    m[torch.as_tensor(rows, dtype=torch.long)] = True
    return m


def check_grads_against_oracle(grads, grads_o, skip_rows=(), what=""):
    """The suite's bars against the oracle's autograd: max 1e-4 and 99.9th percentile 1e-5 of max |grad|, over the rows not in skip_rows."""
    keep = ~rows_mask(skip_rows)
    for k, b in grads_o.items():
        a, b = _t(grads[k]).double()[keep], _t(b).double()[keep]
        assert bool(torch.isfinite(a).all()) and bool(torch.isfinite(b).all()), f"{what} dL/d{k}: a row besides the victims' is not finite"
        scale = float(b.abs().max())
        if scale == 0.0:
            assert float(a.abs().max()) == 0.0, f"{what} dL/d{k}"
            continue
        d = (a - b).abs() / scale
        mx, q = float(d.max()), float(torch.quantile(d.flatten()[:4_000_000], 0.999))
        print(f"[poison] {what} dL/d{k}: max {mx:.2e}, p99.9 {q:.2e} of max |grad|", flush=True)
        assert mx < 1e-4 and q < 1e-5, f"{what} dL/d{k}: max {mx:.3e}, p99.9 {q:.3e}"


def check_non_finite_rows_within(grads, rows, what=""):
    """The non-finite gradient rows are among `rows`; -> how many rows are non-finite in any array."""
    allowed, bad = rows_mask(rows), torch.zeros(P, dtype=torch.bool)
    for k, a in grads.items():
        bad |= ~torch.isfinite(_t(a).reshape(P, -1)).all(dim=1)
    assert not bool((bad & ~allowed).any()), f"{what}: non-finite gradient rows {torch.nonzero(bad & ~allowed)[:, 0].tolist()[:10]} outside the allowed set"
    return int(bad.sum())


def check_reassociation(grads, grads_ref, skip_rows=(), what=""):
    """The bar of test_split_sh_equals_fused_form -- rtol 1e-4, atol 1e-6 max |grad| -- on the rows not in skip_rows, which must be finite."""
    keep = ~rows_mask(skip_rows)
    for k, b in grads_ref.items():
        a, b = _t(grads[k])[keep], _t(b)[keep]
        assert bool(torch.isfinite(a).all()), f"{what} dL/d{k}: a non-finite row outside the allowed set"
        assert torch.allclose(a, b, rtol=1e-4, atol=1e-6 * float(b.abs().max())), f"{what} dL/d{k}: {float((a - b).abs().max()):.3e} of {float(b.abs().max()):.3e}"


def check_same_outside(out, out_clean, pixels, what=""):
    """O, C: the pixels outside the victims' reference-rectangle tiles are the clean frame's bits."""
    outside = ~pixels
    assert int(outside.sum()) > 0
    for k in ("color", "invdepth"):
        a, b = _t(out[k]), _t(out_clean[k])
        assert same_bits(a[:, outside], b[:, outside]), f"{what}: {k} changed outside the victims' tiles"


def check_image_with_non_finite(s, col, radii, invd, aux, out, tiles, what=""):
    """tests/test_gpu_parity.py check_forward for a frame whose image may hold non-finite pixels (an infinite colour): bit-exact integers; off the
    fragile pixels the oracle's non-finite pixels are among the kernel's, the kernel's among `tiles` (bool[H, W], the victims' binned tiles), and
    where the kernel's pixel is finite it meets the oracle's at 1e-5.  -> (non-finite pixels of the oracle, of the kernel)."""
    assert torch.equal(_t(out["radii"]).int(), radii.int()) and torch.equal(_t(out["tiles_touched"]).long(), aux["tiles_touched"])
    assert int(out["R"]) == int(aux["R"]) and torch.equal(_t(out["point_list"]).long(), aux["point_list"]) and torch.equal(_t(out["ranges"]).long(), aux["ranges"])
    ok = ~aux["fragile"]
    g_col, g_inv = _t(out["color"]), _t(out["invdepth"])
    bad_o, bad_k = ~torch.isfinite(col).all(dim=0), ~torch.isfinite(g_col).all(dim=0)
    assert not bool((bad_o & ~bad_k & ok).any()), f"{what}: the oracle has a non-finite pixel where the kernel's is finite"
    assert not bool((bad_k & ~tiles).any()), f"{what}: a non-finite pixel outside the tiles of the victims' rectangles"
    fin = ok & ~bad_k
    err = (g_col - col).abs().amax(dim=0)[fin]
    assert float(err.max()) <= 1e-5, f"{what}: image error {float(err.max()):.3e}"
    assert bool(torch.isfinite(g_inv).all()) and float((g_inv - invd).abs()[0][ok].max()) <= 1e-5 * max(1.0, float(invd.abs().max()))
    if "n_contrib" in out:
        assert torch.equal(_t(out["n_contrib"]).long()[ok], aux["n_contrib"][ok])
        assert float((_t(out["final_T"]) - aux["final_T"]).abs()[ok].max()) <= 5e-6
    return int(bad_o.sum()), int(bad_k.sum())


def reference_tiles_of(frame, victims):
    return tile_pixels(reference_rect(frame)[victims])


def check_colour_frame(kind, b, out, grads, out_clean, grads_clean, col, radii, invd, aux):
    """The C contract on the outputs of either call form."""
    s, f, v = settings(), b.poisoned, b.victims
    binned = aux["rect"][v]
    tiles = tile_pixels(binned)
    n_o, n_k = check_image_with_non_finite(s, col, radii, invd, aux, out, tiles, kind)
    check_same_outside(out, out_clean, reference_tiles_of(f, v), kind)
    listed = listed_in(binned, out)
    assert len(listed) < P // 2
    if not bool(torch.isfinite(aux["rgb"][v]).all()):      # a colour that is shown non-finite: contained to the victims' tiles and to the Gaussians listed there
        assert 0 < n_o <= n_k, (n_o, n_k)
        n_rows = check_non_finite_rows_within(grads, listed, kind)
        assert n_rows > 0
        print(f"[poison] {kind}: non-finite pixels oracle {n_o} / kernel {n_k} / in the victims' tiles {int(tiles.sum())}; non-finite rows {n_rows} of {len(listed)} listed", flush=True)
    else:      # shown as 0: a finite image that differs from the clean one; only the victims' own rows may be non-finite
        assert n_o == 0 and n_k == 0
        assert float((_t(out["color"]) - _t(out_clean["color"])).abs().max()) > 1e-3, "the victims do not show"
        n_rows = check_non_finite_rows_within(grads, v, kind)
        print(f"[poison] {kind}: {n_rows} non-finite gradient rows, all the victims' own", flush=True)
    check_reassociation(grads, grads_clean, skip_rows=listed, what=kind)
    return bool(torch.isfinite(aux["rgb"][v]).all())
