"""Non-finite and out-of-range Gaussian parameters, end to end, on the CPU: the frames and the contract of tests/poison_frames.py against
(1) the per-Gaussian math of csrc/gsr_math.h compiled for the host (tests/host_math_harness.cpp, as tests/test_host_math.py), bit for bit
    against the oracle's preprocess -- every kind, antialiasing off and on, snug and reference rectangles, a band of tile rows;
(2) the whole library behind its C ABI (tests/_build/libgsr_simt.so, forward / backward of tests/test_simt_abi_cpu.py; gsr_mark_visible);
(3) the shipped package on that library for the split-SH call form and the alpha image.
Every buffer the library is handed ends in guard bytes that are checked after each call (test_simt_abi_cpu.guards_intact), and every frame's
lists are checked for range (poison_frames.check_structure): an overrun shows here, in the test process.  This file is the gate of
tests/test_gpu_poison.py: a frame runs on the GPU only after it has passed here.  Test infrastructure: the product has no CPU path."""
import ctypes as C
import shutil

import numpy as np
import pytest
import torch

from helpers import O, fptr, host_cam, host_math_lib, np32
import poison_frames as PF
import test_gpu_parity as G
from test_simt_abi_cpu import backward, forward, guarded, guards_intact, lib, ptr  # noqa: F401  (lib: fixture)
from test_simt_package_cpu import package_on_the_cpu, simt_lib  # noqa: F401  (simt_lib: fixture)

pytestmark = pytest.mark.skipif(shutil.which("g++") is None, reason="g++ not available")


# ---- 1. the per-Gaussian math ----------------------------------------------------------------------------------------------------------
def host_preprocess(s, frame, snug, tile_rows):
    hl = host_math_lib()
    Pn, M = frame.sc.P, frame.sc.shs.shape[1]
    hc = host_cam(s, M, *tile_rows)
    out_f, out_i, out_cov = np.zeros((Pn, 12), np.float32), np.zeros((Pn, 8), np.int32), np.zeros((Pn, 6), np.float32)
    hl.host_set_snug(1 if snug else 0)
    try:
        hl.host_preprocess(C.byref(hc), Pn, fptr(np32(frame.sc.means3D)), fptr(np32(frame.sc.scales)) if frame.cov is None else None,
                           fptr(np32(frame.sc.rotations)) if frame.cov is None else None, fptr(np32(frame.cov)), fptr(np32(frame.sc.opacities)),
                           fptr(np32(frame.sc.shs)) if frame.colors is None else None, fptr(np32(frame.colors)), fptr(out_f), fptr(out_i), fptr(out_cov))
    finally:
        hl.host_set_snug(1)
    return out_f, out_i


@pytest.mark.parametrize("kind", [k.name for k in PF.KINDS])
def test_per_gaussian_math_is_the_oracles_bit_for_bit(kind):
    b = PF.build(kind)
    f, v = b.poisoned, np.asarray(b.victims)
    gy = (PF.H + 15) // 16
    for aa in (False, True):
        s = PF.settings(antialiasing=aa)
        for snug in (True, False):
            for band in ((0, 0), (2, 5)):
                with torch.no_grad():
                    pre = O.preprocess(f.sc.means3D, f.sc.opacities, s, snug=snug, tile_y0=band[0], tile_y1=band[1] or gy, **f.oracle_kwargs())
                out_f, out_i = host_preprocess(s, f, snug, band)
                what = f"{kind} aa={aa} snug={snug} band={band}"
                vis = pre["visible"].numpy()
                np.testing.assert_array_equal(out_i[:, 7].astype(bool), vis, err_msg=what)
                np.testing.assert_array_equal(out_i[:, 0], pre["radii"].numpy(), err_msg=what)
                np.testing.assert_array_equal(out_i[:, 5], pre["tiles_touched"].numpy(), err_msg=what)
                np.testing.assert_array_equal(out_i[vis][:, 1:5], pre["rect"].numpy()[vis], err_msg=what)
                rect = out_i[:, 1:5]
                assert rect.min() >= 0 and rect[:, [0, 2]].max() <= (PF.W + 15) // 16 and rect[:, [1, 3]].max() <= gy, f"{what}: a rectangle leaves the grid"
                np.testing.assert_array_equal(out_f[vis][:, 10], O.tau_of_opacity(pre["opacity"]).numpy()[vis], err_msg=what)      # (NaN == NaN here)
                np.testing.assert_allclose(out_f[vis][:, 6:9], pre["rgb"].numpy()[vis], rtol=0, atol=1e-6, err_msg=what)      # (NaN == NaN, inf == inf)
                if b.kind.group == "G":
                    assert not vis[v].any() and not out_i[v, 0].any() and not out_i[v, 5].any(), f"{what}: a victim is not culled"
                elif b.kind.group in "HOC":
                    assert vis[v].all(), f"{what}: a victim is not visible"
                if b.kind.group == "O" and band == (0, 0):      # tau is NaN / +inf: no snug shrink, the reference's rectangle either way
                    ref = PF.reference_rect(f, s).numpy()
                    np.testing.assert_array_equal(out_i[v][:, 1:5], ref[v], err_msg=what)
                    assert not np.isfinite(out_f[v, 10]).any()


def test_per_gaussian_math_converts_no_float_that_does_not_fit(tmp_path):
    """The same frames through a stand-alone build of the per-Gaussian math under -fsanitize=undefined,float-cast-overflow
    (tests/host_math_poison_main.cpp): no NaN tile coordinate and no infinite radius reaches a float -> int conversion, which is undefined on the
    host and saturates on the GPU -- the float clamp of the tile rectangle (NaN -> 0) and the radius cull come first.  The program's tile counts are
    those of the unsanitized build: it ran the frames."""
    import os
    import subprocess
    from helpers import PKG, ROOT
    exe = str(tmp_path / "host_math_poison")
    subprocess.check_call(["g++", "-O1", "-g", "-ffp-contract=off", "-fsanitize=undefined,float-cast-overflow", "-fno-sanitize-recover=all", "-I", os.path.join(PKG, "csrc"),
                           "-I", os.path.join(ROOT, "include"), "-I", os.path.join(ROOT, "tests"), os.path.join(ROOT, "tests", "host_math_poison_main.cpp"), "-o", exe])
    files, want = [], []
    for k in PF.KINDS:
        f, form = PF.build(k.name).poisoned, PF.form_of(k)
        path = str(tmp_path / f"{k.name}.bin")
        with open(path, "wb") as fh:
            fh.write(bytes(host_cam(PF.settings(), f.sc.shs.shape[1])))
            fh.write(np.array([f.sc.P, form == "cov", form == "colors"], np.int32).tobytes())
            for t in (f.sc.means3D, f.sc.scales, f.sc.rotations, f.cov if f.cov is not None else torch.zeros(f.sc.P, 6), f.sc.opacities, f.sc.shs,
                      f.colors if f.colors is not None else torch.zeros(f.sc.P, 3)):
                fh.write(np32(t).tobytes())
        files.append(path)
        for aa in (False, True):
            for snug in (False, True):
                for band in ((0, 0), (2, 5)):
                    want.append(f"{path} aa={int(aa)} snug={int(snug)} band={int(band != (0, 0))} tiles={int(host_preprocess(PF.settings(aa), f, snug, band)[1][:, 5].sum())}")
    r = subprocess.run([exe] + files, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    assert r.stdout.split("\n")[:-1] == want


# ---- 2. the whole library --------------------------------------------------------------------------------------------------------------
_runs = {}      # (frame key, no_backward) -> (out, grads) of frames that several tests share (hidden and clean frames): computed once, never modified


def run_lib(lib, frame, grad=True, no_backward=False, key=None):  # noqa: F811
    if key is not None and (key, no_backward, grad) in _runs:
        return _runs[(key, no_backward, grad)]
    s = PF.settings()
    out = forward(lib, s, frame.sc, colors=frame.colors, cov=frame.cov, no_backward=no_backward)
    PF.check_structure(out)
    grads = None
    if grad:
        wc, wd = PF.loss_weights()
        g = backward(lib, s, frame.sc, out, wc, wd)
        grads = {k: g[k] for k in [PF.GRAD_KEYS[x] for x in frame.fields()] + ["means2D"]}
    if key is not None:
        _runs[(key, no_backward, grad)] = (out, grads)
    return out, grads


def oracle_of(frame, grad=False):
    r = PF.run_oracle(frame, grad=grad)
    PF.guard_fragile_share(r[3])
    return r


def mark_visible(lib, frame):  # noqa: F811
    s = PF.settings()
    (present, raw), m, vm, pm = guarded(frame.sc.P, np.uint8), np32(frame.sc.means3D), np32(s.viewmatrix), np32(s.projmatrix)
    assert lib.gsr_mark_visible(frame.sc.P, ptr(m), ptr(vm), ptr(pm), ptr(present), None) == 0, lib.gsr_last_error()
    guards_intact([("present", raw)])
    return present.astype(bool)


def g_frame(lib, b, what):  # noqa: F811
    """The G contract on one built frame: culled, the hidden frame bit for bit (tracking and inference builds), zero rows, the oracle's frame."""
    form = PF.form_of(b.kind)
    out, grads = run_lib(lib, b.poisoned)
    out_h, grads_h = run_lib(lib, b.hidden, key=("hidden", form, tuple(b.victims)))
    PF.check_equals_hidden(out, grads, out_h, grads_h, b.victims)
    out_i, _ = run_lib(lib, b.poisoned, grad=False, no_backward=True)
    out_hi, _ = run_lib(lib, b.hidden, grad=False, no_backward=True, key=("hidden", form, tuple(b.victims)))
    PF.check_equals_hidden(out_i, None, out_hi, None, b.victims)
    s, (col, radii, invd, aux) = PF.settings(), oracle_of(b.poisoned)
    if out["R"] > 0:
        G.check_forward(s, col, radii, invd, aux, out)
    else:
        assert aux["R"] == 0 and int(radii.abs().max()) == 0
    vis = mark_visible(lib, b.poisoned)
    if b.kind.field == "means3D":      # (gsr_mark_visible sees positions only: a victim with a broken scale or quaternion is in front of the camera)
        assert not vis[b.victims].any(), f"{what}: gsr_mark_visible calls a victim visible"
    assert np.array_equal(vis, O.mark_visible(b.poisoned.sc.means3D, s.viewmatrix).numpy())
    return out, grads


@pytest.mark.parametrize("kind", PF.names("G"))
def test_geometry_poison_is_culled_and_leaves_the_hidden_frame(lib, kind):  # noqa: F811
    g_frame(lib, PF.build(kind), kind)


@pytest.mark.parametrize("name", list(PF.PLACEMENTS))
def test_structural_placements_of_culled_victims(lib, name):  # noqa: F811
    b = PF.build_placement(name)
    out, grads = g_frame(lib, b, name)
    if name == "every_gaussian":      # P > 0 with R == 0: the background, no gradient anywhere
        assert out["R"] == 0 and int(out["ranges"].abs().max()) == 0
        assert torch.equal(out["color"], torch.tensor(PF.BG)[:, None, None].expand(3, PF.H, PF.W)) and float(out["invdepth"].abs().max()) == 0.0
        assert all(float(np.abs(a).max()) == 0.0 for a in grads.values())
    else:
        assert out["R"] > 0


@pytest.mark.parametrize("kind", PF.names("F"))
def test_odd_but_finite_parameters_are_ordinary_input(lib, kind):  # noqa: F811
    b = PF.build(kind)
    col, radii, invd, aux, grads_o = oracle_of(b.poisoned, grad=True)
    out, grads = run_lib(lib, b.poisoned)
    G.check_forward(PF.settings(), col, radii, invd, aux, out)
    PF.check_grads_against_oracle(grads, grads_o, what=kind)
    if kind == "depth_near_above":      # the first depth in front of the near plane is rendered, the plane itself and what lies behind are not
        assert int(radii[b.victims].min()) > 0
    if kind in ("depth_near", "depth_near_below", "opacity_zero"):
        assert int(aux["tiles_touched"][b.victims].max()) == 0


@pytest.mark.parametrize("kind", PF.names("H"))
def test_huge_finite_splats_integers_and_finiteness(lib, kind):  # noqa: F811
    b = PF.build(kind)
    s, f = PF.settings(), b.poisoned
    with torch.no_grad():
        pre = O.preprocess(f.sc.means3D, f.sc.opacities, s, **f.oracle_kwargs())
        bins = O.bin_and_sort(pre)
    out, grads = run_lib(lib, f)
    gx, gy = pre["grid"]
    assert int(pre["tiles_touched"][b.victims].min()) == gx * gy, "the splat was meant to cover every tile"
    assert torch.equal(out["radii"], pre["radii"]) and torch.equal(out["tiles_touched"], pre["tiles_touched"]) and out["R"] == int(bins["R"])
    assert torch.equal(out["point_list"], bins["point_list"]) and torch.equal(out["ranges"], bins["ranges"])
    assert bool(torch.isfinite(out["color"]).all()) and bool(torch.isfinite(out["invdepth"]).all())
    assert all(bool(np.isfinite(a).all()) for a in grads.values())


def clean_run(lib, form, no_backward=False, grad=True):  # noqa: F811
    return run_lib(lib, PF.clean(form), grad=grad, no_backward=no_backward, key=("clean", form))


@pytest.mark.parametrize("kind", PF.names("O"))
def test_non_finite_opacity_renders_with_alpha_099(lib, kind):  # noqa: F811
    b = PF.build(kind)
    s, f, v = PF.settings(), b.poisoned, b.victims
    col, radii, invd, aux, grads_o = oracle_of(f, grad=True)
    out, grads = run_lib(lib, f)
    G.check_forward(s, col, radii, invd, aux, out)
    ref = PF.reference_rect(f)[v]
    area = (ref[:, 2] - ref[:, 0]) * (ref[:, 3] - ref[:, 1])
    assert torch.equal(out["tiles_touched"][v], area) and int(area.min()) > 0, "the victim is not listed with the reference's rectangle"
    assert float((out["color"] - clean_run(lib, "sh")[0]["color"]).abs().max()) > 0.1, "the victims do not show"
    PF.check_grads_against_oracle(grads, grads_o, skip_rows=v, what=kind)
    n = PF.check_non_finite_rows_within(grads, v, kind)
    print(f"[poison] {kind}: {n} non-finite gradient rows, all the victims' own", flush=True)
    PF.check_same_outside(out, clean_run(lib, "sh")[0], PF.reference_tiles_of(f, v), kind)
    out_i, _ = run_lib(lib, f, grad=False, no_backward=True)      # the inference build
    G.check_forward(s, col, radii, invd, aux, out_i)
    assert PF.same_bits(out_i["color"], out["color"])


@pytest.mark.parametrize("kind", PF.names("C"))
def test_non_finite_colour_is_contained(lib, kind):  # noqa: F811
    b = PF.build(kind)
    form = PF.form_of(b.kind)
    out, grads = run_lib(lib, b.poisoned)
    out_c, grads_c = clean_run(lib, form)
    col, radii, invd, aux = oracle_of(b.poisoned)
    if PF.check_colour_frame(kind, b, out, grads, out_c, grads_c, col, radii, invd, aux):      # a finite frame: the oracle's bars on every row but the victims' own
        _, _, _, _, grads_o = oracle_of(b.poisoned, grad=True)
        G.check_forward(PF.settings(), col, radii, invd, aux, out)
        PF.check_grads_against_oracle(grads, grads_o, skip_rows=b.victims, what=kind)
    out_i, _ = run_lib(lib, b.poisoned, grad=False, no_backward=True)      # the inference build
    assert PF.same_bits(out_i["color"], out["color"]) and PF.same_bits(out_i["invdepth"], out["invdepth"])


def test_mixed_frame_one_victim_of_every_kind(lib):  # noqa: F811
    f, who = PF.build_mixed()
    s = PF.settings()
    col, radii, invd, aux, grads_o = oracle_of(f, grad=True)
    out, grads = run_lib(lib, f)
    culled = [v for k, v in who.items() if PF.KIND[k].group == "G"]
    own = [v for k, v in who.items() if PF.KIND[k].group in "OC"]
    PF.check_culled(out, culled)
    inf_victims = [v for k, v in who.items() if PF.KIND[k].group == "C" and PF.KIND[k].value == PF.INF]
    binned = aux["rect"][inf_victims]
    n_o, n_k = PF.check_image_with_non_finite(s, col, radii, invd, aux, out, PF.tile_pixels(binned), "mixed")
    listed = PF.listed_in(binned, out)
    allowed = torch.unique(torch.cat([listed, torch.tensor(own)]))
    n_rows = PF.check_non_finite_rows_within(grads, allowed, "mixed")
    assert n_o > 0
    print(f"[poison] mixed: non-finite pixels oracle {n_o} / kernel {n_k}; non-finite rows {n_rows} of {len(allowed)} allowed", flush=True)
    PF.check_grads_against_oracle(grads, {k: torch.nan_to_num(g, nan=0.0, posinf=0.0, neginf=0.0) for k, g in grads_o.items()}, skip_rows=allowed, what="mixed")
    for k in grads:
        assert float(np.abs(grads[k][culled]).max()) == 0.0, f"mixed dL/d{k}: a culled victim's row is not zero"


# ---- 3. through the shipped package: the split-SH call form, the alpha image ------------------------------------------------------------
def package_run(pkg, frame, split=False, return_alpha=False):
    s = PF.settings()
    S = pkg.GaussianRasterizationSettings(s.image_height, s.image_width, s.tanfovx, s.tanfovy, s.bg, 1.0, s.viewmatrix, s.projmatrix, 3, s.campos, False, False, False)
    sc = frame.sc
    L = {k: getattr(sc, k).detach().clone().requires_grad_(True) for k in ("means3D", "opacities", "scales", "rotations")}
    L["dc"], L["rest"] = (sc.shs[:, :1].contiguous().clone().requires_grad_(True), sc.shs[:, 1:].contiguous().clone().requires_grad_(True)) if split else (None, None)
    L["shs"] = None if split else sc.shs.detach().clone().requires_grad_(True)
    L["means2D"] = torch.zeros(sc.P, 3, requires_grad=True)
    rast = pkg.GaussianRasterizer(S, return_alpha=True) if return_alpha else pkg.GaussianRasterizer(S)
    res = rast(means3D=L["means3D"], means2D=L["means2D"], opacities=L["opacities"], dc=L["dc"], shs=L["rest"] if split else L["shs"], scales=L["scales"],
               rotations=L["rotations"])
    wc, wd = PF.loss_weights()
    ((res[0] * wc).sum() + (res[2] * wd).sum()).backward()
    grads = {k: L[k].grad for k in ("means3D", "opacities", "scales", "rotations", "means2D")}
    grads["shs"] = torch.cat([L["dc"].grad, L["rest"].grad], dim=1) if split else L["shs"].grad
    return res, grads


def test_split_sh_call_form_contains_an_infinite_coefficient(lib, simt_lib):  # noqa: F811
    b = PF.build("sh_pinf")      # (its victims hold the infinity in coefficient 0 -- the dc block -- and in coefficients 5 and 15 of the rest block)
    out_f, _ = run_lib(lib, b.poisoned)
    out_c, grads_c = clean_run(lib, "sh")
    with package_on_the_cpu(simt_lib) as pkg:
        (color, radii, invd), grads = package_run(pkg, b.poisoned, split=True)
    assert PF.same_bits(color, out_f["color"]) and PF.same_bits(invd, out_f["invdepth"]) and torch.equal(radii, out_f["radii"])
    out = dict(out_f, color=color.detach(), invdepth=invd.detach())
    col_o, radii_o, invd_o, aux = oracle_of(b.poisoned)
    PF.check_colour_frame("sh_pinf (split)", b, out, grads, out_c, grads_c, col_o, radii_o, invd_o, aux)


def test_alpha_image_under_a_nan_opacity_victim(simt_lib):  # noqa: F811
    b = PF.build("opacity_nan")
    with package_on_the_cpu(simt_lib) as pkg:
        (color, radii, invd, alpha), grads = package_run(pkg, b.poisoned, return_alpha=True)
    col, radii_o, invd_o, aux = oracle_of(b.poisoned)
    ok = ~aux["fragile"]
    assert torch.equal(radii, radii_o.to(torch.int32))
    assert float((alpha.detach()[0] - (1.0 - aux["final_T"])).abs()[ok].max()) <= 1e-5 and bool(torch.isfinite(alpha).all())
    assert float((color.detach() - col).abs().amax(0)[ok].max()) <= 1e-5
    centre = aux["means2D"][b.victims].round().long()      # at a victim's centre the exponent is 0: at least 0.99 is taken there
    assert float(alpha.detach()[0, centre[:, 1], centre[:, 0]].min()) >= 0.99 - 1e-6
    PF.check_non_finite_rows_within(grads, b.victims, "opacity_nan (alpha image)")
