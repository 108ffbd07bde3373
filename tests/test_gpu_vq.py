"""Vector quantisation on the MI355X: gsr_vq_assign / gsr_vq_update and gsr_scene.compress on the device against the fp64 Lloyd step with the bars of
tests/vq_reference.py (tests/test_vq_cpu.py holds the same kernel source to them on the host) -- the assignment and dist2, the update from the
kernel's own assignment, exact ties, planted clusters, rows and weights the update must leave out, containment of non-finite rows and centroids, run-to-run bits, a non-default stream, and a synthetic scene compressed with
one centroid per Gaussian, which must render the bit-identical image.

The fp64 distances of the large shapes are formed on the device as |x|^2 + |c|^2 - 2 x.c in fp64 (a P x K block of differences does not fit): its
own cancellation is 2^-53 of the norms, eight orders below the bar."""
import math

import numpy as np
import pytest
import torch

import vq_reference as VR

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
SHAPES = [(1027, 129, 48), (4099, 65536, 8), (100003, 4096, 45)]


def lloyd(P, D, K):
    from gsr_scene import compress as GC
    return GC._Lloyd(P, D, K, torch.device(DEV))


def best64(rows, cb):
    """fp64 on the device: -> (argmin [P], its squared distance [P]) over the finite centroids."""
    x, c = rows.double(), cb.double()
    cn = (c * c).sum(dim=1)
    idx, best = [], []
    step = max(1, (1 << 27) // c.shape[0])
    for i in range(0, x.shape[0], step):
        xi = x[i:i + step]
        d = (xi * xi).sum(dim=1, keepdim=True) + cn[None, :] - 2.0 * (xi @ c.T)
        b, k = d.min(dim=1)
        idx.append(k)
        best.append(b)
    return torch.cat(idx), torch.cat(best).clamp_min(0.0)


def check_assign_on_the_device(tag, rows, cb, idx, dist2):
    P, D = rows.shape
    assert idx.dtype == torch.int32 and int(idx.min()) >= 0 and int(idx.max()) < cb.shape[0]
    x, c = rows.double(), cb.double()
    want, best = best64(rows, cb)
    got = ((x - c[idx.long()]) ** 2).sum(dim=1)
    best = torch.minimum(best, ((x - c[want]) ** 2).sum(dim=1))      # the winner's distance from the differences themselves
    slack = VR.gamma(D) * ((x * x).sum(dim=1) + (c[idx.long()] ** 2).sum(dim=1) + (c[want] ** 2).sum(dim=1))
    worst = float(((got - best) / slack.clamp_min(1e-300)).max())
    rel = float(((dist2.double() - got).abs() / got.clamp_min(1e-300)).max())
    print(f"[{tag}] assign: {int((idx.long() != want).sum())} of {P} rows differ from the fp64 argmin, worst excess {worst:.3g} of the bar; "
          f"dist2 worst relative error {rel:.3g} (bar {VR.dist2_bar(D):.3g})")
    assert bool((got <= best + slack).all()), (tag, worst)
    assert bool(((dist2.double() - got).abs() <= VR.dist2_bar(D) * got).all()), (tag, rel)
    return want


@pytest.fixture(scope="module")
def steps():
    """One Lloyd step per shape and data kind, run once: rows, codebook, weights, idx, dist2, codebook', mass (the inputs on the host too)."""
    out = {}
    for P, K, D in SHAPES:
        for kind in (("centred", "offset10", "offset1000") if P < 5000 else ("offset10",)):
            rows, cb = VR.case(P, K, D, kind)
            weights = torch.rand(P, generator=torch.Generator().manual_seed(P)) + 0.01
            weights[::11] = 0.0
            L = lloyd(P, D, K)
            r, c, w = rows.to(DEV), cb.to(DEV), weights.to(DEV)
            idx, dist2 = L.assign(r, c)
            new = c.clone()
            mass = L.update(r, w, idx, new)
            out[(P, K, D, kind)] = dict(rows=rows, cb=cb, weights=weights, r=r, c=c, w=w, idx=idx, dist2=dist2, new=new, mass=mass, L=L)
    torch.cuda.synchronize()
    return out


@pytest.mark.parametrize("P,K,D", SHAPES)
def test_assignment_on_the_device(steps, P, K, D):
    for key, s in steps.items():
        if key[:3] != (P, K, D):
            continue
        want = check_assign_on_the_device(f"gpu {P}x{K}x{D} {key[3]}", s["r"], s["c"], s["idx"], s["dist2"])
        if key[3] == "centred" and K < 1000:      # (among 65536 centroids in 8 dimensions a near-tie inside the fp32 bound is to be expected)
            assert torch.equal(s["idx"].long(), want)
        idx2, dist22 = s["L"].assign(s["r"], s["c"])      # a second run: the same bits
        assert torch.equal(idx2, s["idx"]) and torch.equal(dist22.view(torch.int32), s["dist2"].view(torch.int32))


@pytest.mark.parametrize("P,K,D", SHAPES)
def test_update_on_the_device(steps, P, K, D):
    for key, s in steps.items():
        if key[:3] != (P, K, D):
            continue
        VR.check_update(f"gpu {P}x{K}x{D} {key[3]}", s["rows"], s["weights"], s["idx"].cpu().numpy(), s["cb"], s["new"].cpu(), s["mass"].cpu().numpy())
        again = s["c"].clone()
        mass2 = s["L"].update(s["r"], s["w"], s["idx"], again)
        assert torch.equal(again.view(torch.int32), s["new"].view(torch.int32)) and torch.equal(mass2.view(torch.int32), s["mass"].view(torch.int32))
        plain = s["c"].clone()                            # weights = NULL is a weight of one
        ones = s["c"].clone()
        m_plain = s["L"].update(s["r"], None, s["idx"], plain)
        m_ones = s["L"].update(s["r"], torch.ones_like(s["w"]), s["idx"], ones)
        assert torch.equal(plain.view(torch.int32), ones.view(torch.int32)) and torch.equal(m_plain, m_ones)
        assert float(m_plain.sum()) == P


def test_non_finite_rows_and_centroids_on_the_device(steps):
    P, K, D = SHAPES[0]
    s = steps[(P, K, D, "centred")]
    L = s["L"]
    rows_bad = [0, 31, 32, 255, 256, 1026]
    bad = s["r"].clone()
    for n, row in enumerate(rows_bad):
        bad[row, (7 * n) % D] = (math.nan, math.inf, -math.inf)[n % 3]
    idx, dist2 = L.assign(bad, s["c"])
    keep = torch.ones(P, dtype=torch.bool, device=DEV)
    keep[rows_bad] = False
    assert bool((idx[~keep] == -1).all()) and bool((dist2[~keep] == 0).all())
    assert torch.equal(idx[keep], s["idx"][keep]) and torch.equal(dist2[keep].view(torch.int32), s["dist2"][keep].view(torch.int32))
    new = s["c"].clone()
    mass = L.update(bad, s["w"], idx, new)                # the -1 rows belong to nobody
    VR.check_update("gpu poisoned rows", s["rows"], s["weights"], idx.cpu().numpy(), s["cb"], new.cpu(), mass.cpu().numpy())
    cb_bad = s["c"].clone()
    losers = [int(torch.bincount(s["idx"].long()).argmax()), 0, 64, K - 1]
    for n, k in enumerate(losers):
        cb_bad[k, n] = (math.nan, math.inf, -math.inf, math.nan)[n]
    idx, dist2 = L.assign(s["r"], cb_bad)
    want, _ = VR.assign64(s["rows"].numpy(), cb_bad.cpu().numpy())
    assert int(idx.min()) >= 0 and np.array_equal(idx.cpu().numpy(), want)
    cb_bad[:, 3] = math.nan
    idx, dist2 = L.assign(s["r"], cb_bad)
    assert bool((idx == -1).all()) and bool((dist2 == 0).all())


def test_non_default_stream(steps):
    P, K, D = SHAPES[0]
    s = steps[(P, K, D, "offset10")]
    stream = torch.cuda.Stream(device=DEV)
    stream.wait_stream(torch.cuda.current_stream(DEV))
    with torch.cuda.stream(stream):
        idx, dist2 = s["L"].assign(s["r"], s["c"])
        new = s["c"].clone()
        mass = s["L"].update(s["r"], s["w"], idx, new)
    stream.synchronize()
    assert torch.equal(idx, s["idx"]) and torch.equal(dist2.view(torch.int32), s["dist2"].view(torch.int32))
    assert torch.equal(new.view(torch.int32), s["new"].view(torch.int32)) and torch.equal(mass.view(torch.int32), s["mass"].view(torch.int32))


def test_exact_tie_goes_to_the_lowest_index_on_the_device():
    """Duplicated centroids give bit-equal scores out of the matrix instruction: across lanes, across the two tiles of a stage, and across stages."""
    rows, cb = VR.case(1027, 200, 45, "centred", seed=3)
    for k in (5, 33, 70, 150):
        cb[k] = rows[10]
    for k in (40, 41, 199):
        cb[k] = rows[700]
    near_origin = 0.05 * cb[64].clone()
    for k in (64, 65, 127, 128):        # a duplicated centroid that is many rows' nearest, not one row's position
        cb[k] = near_origin
    L = lloyd(1027, 45, 200)
    idx, dist2 = L.assign(rows.to(DEV), cb.to(DEV))
    check_assign_on_the_device("gpu ties", rows.to(DEV), cb.to(DEV), idx, dist2)
    idx = idx.cpu().numpy()
    assert idx[10] == 5 and idx[700] == 40 and float(dist2[10]) == 0 and float(dist2[700]) == 0
    assert not np.isin(idx, [33, 70, 150, 41, 199, 65, 127, 128]).any() and int((idx == 64).sum()) > 10


@pytest.mark.parametrize("P,K,D", [(1027, 33, 2), (4099, 129, 45)])
def test_planted_clusters_are_recovered_on_the_device(P, K, D):
    rows, label, init = VR.planted(P, K, D)
    L = lloyd(P, D, K)
    r = rows.to(DEV)
    idx, _ = L.assign(r, init.to(DEV))
    assert torch.equal(idx.cpu(), label)
    cb = init.to(DEV).clone()
    mass = L.update(r, None, idx, cb)
    VR.check_update("gpu planted", rows, None, idx.cpu().numpy(), init, cb.cpu(), mass.cpu().numpy())
    assert torch.equal(L.assign(r, cb)[0].cpu(), label) and np.array_equal(mass.cpu().numpy(), np.bincount(label.numpy(), minlength=K).astype(np.float32))


def test_unassigned_rows_and_bad_weights_are_left_out_on_the_device():
    P, K, D = 4099, 9, 5
    rows, cb = VR.case(P, K, D, "centred", seed=2)
    L = lloyd(P, D, K)
    idx = L.assign(rows.to(DEV), cb.to(DEV))[0].cpu()
    idx[[0, 17, 4098]] = -1
    idx[idx == 4] = 3                                   # cluster 4 ends empty
    weights = torch.ones(P)
    weights[5], weights[6], weights[7], weights[8] = -1.0, math.nan, math.inf, 0.0
    bad_rows = rows.clone()
    bad_rows[0], bad_rows[17, 2], bad_rows[8, 1] = math.nan, math.inf, math.nan      # rows nobody owns, and one of weight 0: whatever they hold
    new = cb.to(DEV).clone()
    mass = L.update(bad_rows.to(DEV), weights.to(DEV), idx.to(DEV), new)
    VR.check_update("gpu left out", rows, weights, idx.numpy(), cb, new.cpu(), mass.cpu().numpy())
    assert float(mass[4]) == 0 and bool(torch.isfinite(new).all())


def test_kmeans_on_the_device():
    from gsr_scene import compress as GC
    P, K, D = 20011, 64, 45
    rows = VR.case(P, 1, D, "offset10", seed=5)[0].to(DEV)      # ONE blob: nothing to separate, the inertia falls by a few per cent per step
    init = rows[:K].clone()
    cb, idx, inertia = GC.kmeans(rows, K, iters=5, init=init)
    again = GC.kmeans(rows, K, iters=5, init=init)
    assert all(torch.equal(a, b) for a, b in zip((cb, idx, inertia), again))
    # kmeans' own loop by hand, keeping every iteration's codebook: each step against the summed per-row bar (VR.lloyd_step_tolerance)
    mean = rows.double().sum(dim=0) / float(P)
    x, c = (rows.double() - mean).float().contiguous(), (init.double() - mean).float().contiguous()
    L, steps = lloyd(P, D, K), []
    for _ in range(5):
        i, d2 = L.assign(x, c)
        steps.append((c.clone(), i, float(d2.double().sum())))
        L.update(x, None, i, c)
    assert torch.equal(steps[-1][1], idx)
    assert [s[2] for s in steps] == pytest.approx(inertia.tolist(), rel=1e-12)      # (the mean's summation order is torch's own)
    for (_, _, before), (c_now, i_now, after) in zip(steps[:-1], steps[1:]):
        tol = VR.lloyd_step_tolerance(x.cpu().numpy(), None, c_now.cpu().numpy(), i_now.cpu().numpy(), before, after)
        print(f"[kmeans gpu] inertia {before:.10g} -> {after:.10g}, may rise by {tol:.3g}")
        assert after <= before + tol and tol < 1e-3 * before
    assert float(inertia[-1]) < 0.99 * float(inertia[0])
    want, mass = VR.update64(rows.cpu().numpy(), None, idx.cpu().numpy(), cb.double().cpu().numpy())
    assert (np.abs(cb.double().cpu().numpy() - want)[mass > 0] <= VR.ulp32(want)[mass > 0]).all()


def test_a_scene_compressed_with_one_centroid_per_gaussian_renders_the_same_bits(tmp_path):
    """K = P from the scene's own rows: every Gaussian is its own centroid, compress -> save -> load -> decompress returns the parameters bit for bit and
    the rasterizer the bit-identical image.  (rotation stays out: compress normalises quaternions, which the rasterizer does not.)"""
    from gsr_synth import make_camera, make_scene
    from gsr_scene import compress as GC
    from diff_gaussian_rasterization import GaussianRasterizationSettings, GaussianRasterizer
    P = 3000
    cam = make_camera(256, 256)
    sc = make_scene(P, cam, seed=3)
    dev = torch.device(DEV)
    model = {"xyz": sc.means3D.to(dev), "features_dc": sc.shs[:, :1].contiguous().to(dev), "features_rest": sc.shs[:, 1:].contiguous().to(dev),
             "opacity": sc.opacities.to(dev), "scaling": sc.scales.to(dev), "rotation": sc.rotations.to(dev)}
    c = GC.compress(model, {"features_rest": P, "scaling": P}, iters=2, generator=torch.Generator().manual_seed(0))
    path = str(tmp_path / "scene.npz")
    GC.save_compressed(path, c)
    back = GC.decompress(GC.load_compressed(path, device=dev))
    for key, t in model.items():
        assert torch.equal(back[key].view(torch.int32), t.view(torch.int32)), key
    rs = GaussianRasterizationSettings(256, 256, cam.tanfovx, cam.tanfovy, torch.tensor([0.1, 0.2, 0.3], device=dev), 1.0,
                                       cam.world_view_transform.to(dev), cam.full_proj_transform.to(dev), 3, cam.camera_center.to(dev), False, True, False)

    def render(m):
        shs = torch.cat([m["features_dc"], m["features_rest"]], dim=1).contiguous()
        with torch.no_grad():
            return GaussianRasterizer(rs)(means3D=m["xyz"], means2D=torch.zeros_like(m["xyz"]), opacities=m["opacity"], shs=shs, scales=m["scaling"], rotations=m["rotation"])[0]

    a, b = render(model), render(back)
    assert float(a.abs().max()) > 0.2 and torch.equal(a.view(torch.int32), b.view(torch.int32))
