"""GPU tests of the rows next to the operator: the split-SH ("separate_sh") call form and
SparseGaussianAdam (N2), and the simple_knn.distCUDA2 provider (N3).  All calls go through the C ABI."""
import numpy as np
import pytest
import torch

from helpers import make_camera, make_scene, oracle_settings
from test_gpu_parity import gpu_settings

pytestmark = pytest.mark.gpu


def _grads(fn, tensors):
    for t in tensors:
        t.grad = None
    fn().backward()
    return [t.grad.detach().clone() for t in tensors]


@pytest.mark.parametrize("P,W,H,deg,Mstore", [(1000, 256, 256, 3, 16), (5003, 320, 200, 3, 16), (2500, 160, 96, 1, 4),
                                               (777, 128, 128, 2, 9)])
def test_split_sh_equals_fused_form(P, W, H, deg, Mstore):
    """rasterizer(dc=, shs=) (gaussian_renderer/__init__.py:91-100) must give the very same image and gradients as the
    fused [P,M,3] tensor: same arithmetic, only the memory layout of the SH record differs."""
    from diff_gaussian_rasterization import GaussianRasterizer
    dev = torch.device("cuda:0")
    cam = make_camera(W, H)
    sc = make_scene(P, cam, seed=21, s_med=0.03).to(dev)
    s = oracle_settings(cam, sh_degree=deg)
    rast = GaussianRasterizer(gpu_settings(s, dev))
    sh_full = sc.shs[:, :Mstore].contiguous()
    g = torch.Generator(device="cpu").manual_seed(5)
    wgt = torch.rand(3, H, W, generator=g).to(dev)
    wd = torch.rand(1, H, W, generator=g).to(dev)

    means = sc.means3D.clone().requires_grad_(True)
    opac = sc.opacities.clone().requires_grad_(True)
    scal = sc.scales.clone().requires_grad_(True)
    rots = sc.rotations.clone().requires_grad_(True)
    fused = sh_full.clone().requires_grad_(True)
    dc = sh_full[:, :1].clone().contiguous().requires_grad_(True)
    rest = sh_full[:, 1:].clone().contiguous().requires_grad_(True)

    def loss_of(img, radii, invd):
        return (img * wgt).sum() + (invd * wd).sum()

    def run_fused():
        return loss_of(*rast(means3D=means, means2D=None, shs=fused, colors_precomp=None, opacities=opac, scales=scal,
                             rotations=rots, cov3D_precomp=None))

    def run_split():
        return loss_of(*rast(means3D=means, means2D=None, dc=dc, shs=rest, colors_precomp=None, opacities=opac,
                             scales=scal, rotations=rots, cov3D_precomp=None))

    with torch.no_grad():
        a = rast(means3D=means, means2D=None, shs=fused, colors_precomp=None, opacities=opac, scales=scal, rotations=rots,
                 cov3D_precomp=None)
        b = rast(means3D=means, means2D=None, dc=dc, shs=rest, colors_precomp=None, opacities=opac, scales=scal,
                 rotations=rots, cov3D_precomp=None)
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1]) and torch.equal(a[2], b[2])

    gf = _grads(run_fused, [means, opac, scal, rots, fused])
    gs = _grads(run_split, [means, opac, scal, rots, dc, rest])
    # the blend backward sums four waves' LDS atomics in arrival order: identical up to fp32 reassociation
    for x, y in zip(gf[:4], gs[:4]):
        assert torch.allclose(x, y, rtol=1e-4, atol=1e-6 * float(x.abs().max()))
    full = torch.cat([gs[4], gs[5]], dim=1)
    assert full.shape == gf[4].shape
    assert torch.allclose(gf[4], full, rtol=1e-4, atol=1e-6 * float(gf[4].abs().max()))
    assert float(gs[4].abs().max()) > 0 and (Mstore == 1 or deg == 0 or float(gs[5].abs().max()) > 0)


@pytest.mark.parametrize("deg", [3, 1])
def test_split_sh_form_against_the_oracle(deg):
    """the separate-SH call form compared with the ORACLE directly (not only with the fused HIP form):
    image, radii and every gradient -- the oracle sees dc and rest concatenated the way the reference's get_features does
    (scene/gaussian_model.py:121-125), so its autograd hands back the two gradients by slicing."""
    from diff_gaussian_rasterization import GaussianRasterizer
    from helpers import O
    dev = torch.device("cuda:0")
    W, H, P = 208, 160, 3000
    cam = make_camera(W, H)
    sc = make_scene(P, cam, seed=23, s_med=0.04)
    s = oracle_settings(cam, sh_degree=deg, bg=torch.tensor([0.2, 0.1, 0.3]))
    g = torch.Generator().manual_seed(6)
    wgt, wd = torch.randn(3, H, W, generator=g), torch.randn(1, H, W, generator=g) * 0.3
    names = ("means3D", "opacities", "scales", "rotations")
    Lc = {k: getattr(sc, k).clone().requires_grad_(True) for k in names}
    dc_c = sc.shs[:, :1].clone().contiguous().requires_grad_(True)
    rest_c = sc.shs[:, 1:].clone().contiguous().requires_grad_(True)
    col, radii, invd, aux = O.rasterize(Lc["means3D"], None, Lc["opacities"], s, shs=torch.cat([dc_c, rest_c], dim=1), scales=Lc["scales"],
                                        rotations=Lc["rotations"], want_fragile=True, return_aux=True)
    ((col * wgt).sum() + (invd * wd).sum()).backward()
    Lg = {k: getattr(sc, k).clone().to(dev).requires_grad_(True) for k in names}
    dc_g = sc.shs[:, :1].clone().contiguous().to(dev).requires_grad_(True)
    rest_g = sc.shs[:, 1:].clone().contiguous().to(dev).requires_grad_(True)
    gcol, gradii, ginvd = GaussianRasterizer(gpu_settings(s, dev))(means3D=Lg["means3D"], means2D=None, dc=dc_g, shs=rest_g,
                                                                    opacities=Lg["opacities"], scales=Lg["scales"], rotations=Lg["rotations"])
    ((gcol * wgt.to(dev)).sum() + (ginvd * wd.to(dev)).sum()).backward()
    torch.cuda.synchronize()
    assert torch.equal(gradii.cpu(), radii)
    err = (gcol.detach().cpu() - col.detach()).abs().amax(0)
    assert float(err[~aux["fragile"]].max()) <= 1e-5
    pairs = [(Lg[k].grad.cpu(), Lc[k].grad) for k in names] + [(dc_g.grad.cpu(), dc_c.grad), (rest_g.grad.cpu(), rest_c.grad)]
    for a, b in pairs:
        assert float((a - b).abs().max()) <= 2e-3 * float(b.abs().max()) + 1e-12
        if b.numel() > 1000:
            dd = ((a - b).abs() / float(b.abs().max())).flatten()
            assert float(torch.quantile(dd[:4_000_000], 0.999)) <= 1e-4
    assert float(dc_c.grad.abs().max()) > 0 and float(rest_c.grad.abs().max()) > 0


def test_split_sh_degree0_model_with_empty_rest():
    """max_sh_degree = 0: features_rest is [P,0,3]; the DC tensor alone is the SH record."""
    from diff_gaussian_rasterization import GaussianRasterizer
    dev = torch.device("cuda:0")
    cam = make_camera(128, 96)
    sc = make_scene(600, cam, seed=2, s_med=0.04).to(dev)
    s = oracle_settings(cam, sh_degree=0)
    rast = GaussianRasterizer(gpu_settings(s, dev))
    dc = sc.shs[:, :1].clone().contiguous().requires_grad_(True)
    rest = torch.zeros(600, 0, 3, device=dev, requires_grad=True)
    fused = sc.shs[:, :1].clone().contiguous().requires_grad_(True)
    kw = dict(means3D=sc.means3D, means2D=None, colors_precomp=None, opacities=sc.opacities, scales=sc.scales,
              rotations=sc.rotations, cov3D_precomp=None)
    a = rast(shs=fused, **kw)[0]
    b = rast(dc=dc, shs=rest, **kw)[0]
    assert torch.equal(a, b)
    a.sum().backward()
    b.sum().backward()
    assert torch.allclose(dc.grad, fused.grad, rtol=1e-4, atol=1e-7)
    assert rest.grad is not None and rest.grad.shape == (600, 0, 3)


def test_sparse_adam_one_launch_for_all_groups_equals_one_launch_per_group():
    """Round 5: SparseGaussianAdam.step issues ONE launch for all parameter groups (gsr_sparse_adam_step_multi).  Every tensor must come out the
    bits gsr_sparse_adam_step (one launch per group, rounds 2-4) leaves: the six tensors of scene/gaussian_model.py:183-190, shared visibility."""
    import ctypes as C
    from diff_gaussian_rasterization import SparseGaussianAdam, _lib
    dev = torch.device("cuda:0")
    N = 100_003
    g = torch.Generator(device="cpu").manual_seed(3)
    shapes = {"xyz": (N, 3), "f_dc": (N, 1, 3), "f_rest": (N, 15, 3), "opacity": (N, 1), "scaling": (N, 3), "rotation": (N, 4)}
    lrs = {"xyz": 1.6e-4, "f_dc": 2.5e-3, "f_rest": 1.25e-4, "opacity": 0.025, "scaling": 5e-3, "rotation": 1e-3}
    params = {k: torch.randn(*shp, generator=g).to(dev).requires_grad_(True) for k, shp in shapes.items()}
    single = {k: [v.detach().clone(), torch.zeros_like(v), torch.zeros_like(v)] for k, v in params.items()}      # param, exp_avg, exp_avg_sq
    opt = SparseGaussianAdam([{"params": [params[k]], "lr": lrs[k], "name": k} for k in shapes], lr=0.0, eps=1e-15)
    lib = _lib.load()
    vp = lambda t: C.c_void_p(t.data_ptr())
    for it in range(3):
        vis = torch.rand(N, generator=g) < (0.05, 0.5, 1.0)[it]
        visd = vis.to(dev)
        for k, p in params.items():
            p.grad = torch.randn(*shapes[k], generator=g).to(dev)
        opt.step(visd, N)
        v8 = visd.view(torch.uint8)
        for k, (p1, m1, v1) in single.items():
            M = p1.numel() // N
            _lib.check(lib.gsr_sparse_adam_step(vp(p1), vp(params[k].grad), vp(m1), vp(v1), vp(v8), N, M, lrs[k], 0.9, 0.999, 1e-15, None), "gsr_sparse_adam_step")
        torch.cuda.synchronize()
        for k, (p1, m1, v1) in single.items():
            st = opt.state[params[k]]
            assert torch.equal(params[k].detach(), p1) and torch.equal(st["exp_avg"], m1) and torch.equal(st["exp_avg_sq"], v1), (it, k)


def test_sparse_gaussian_adam_updates_only_visible_rows():
    """SparseGaussianAdam(params, lr, eps).step(visibility, N) (train.py:180-183): rows of invisible Gaussians keep
    parameter and moments; visible rows follow m = b1 m + (1-b1) g, v = b2 v + (1-b2) g^2, p -= lr m / (sqrt(v) + eps)."""
    from diff_gaussian_rasterization import SparseGaussianAdam
    dev = torch.device("cuda:0")
    N = 10007
    g = torch.Generator(device="cpu").manual_seed(0)
    shapes = {"xyz": (N, 3), "f_dc": (N, 1, 3), "f_rest": (N, 15, 3), "opacity": (N, 1), "rotation": (N, 4)}
    params = {k: torch.randn(*shp, generator=g).to(dev).requires_grad_(True) for k, shp in shapes.items()}
    lrs = {"xyz": 1.6e-4, "f_dc": 2.5e-3, "f_rest": 1.25e-4, "opacity": 0.025, "rotation": 1e-3}
    groups = [{"params": [params[k]], "lr": lrs[k], "name": k} for k in shapes]
    opt = SparseGaussianAdam(groups, lr=0.0, eps=1e-15)
    ref_p = {k: v.detach().double().clone() for k, v in params.items()}
    ref_m = {k: torch.zeros_like(v) for k, v in ref_p.items()}
    ref_v = {k: torch.zeros_like(v) for k, v in ref_p.items()}
    for it in range(3):
        vis = (torch.rand(N, generator=g) < 0.6).to(dev)
        for k, p in params.items():
            p.grad = torch.randn(*shapes[k], generator=g).to(dev) * (10.0 ** (it - 1))
        opt.step(vis, N)
        for k, p in params.items():
            gg = p.grad.double()
            mask = vis.view(N, *([1] * (p.dim() - 1))).expand_as(p)
            m = 0.9 * ref_m[k] + 0.1 * gg
            v = 0.999 * ref_v[k] + 0.001 * gg * gg
            step = lrs[k] * m / (v.sqrt() + 1e-15)
            ref_m[k] = torch.where(mask, m, ref_m[k])
            ref_v[k] = torch.where(mask, v, ref_v[k])
            ref_p[k] = torch.where(mask, ref_p[k] - step, ref_p[k])
    torch.cuda.synchronize()
    for k, p in params.items():
        st = opt.state[p]
        # fp32 kernel against an fp64 restatement: a few ulp of the largest term of each sum
        assert torch.allclose(p.detach().double(), ref_p[k], rtol=2e-6, atol=2e-6 * float(ref_p[k].abs().max())), k
        assert torch.allclose(st["exp_avg"].double(), ref_m[k], rtol=2e-6, atol=1e-6 * float(ref_m[k].abs().max())), k
        assert torch.allclose(st["exp_avg_sq"].double(), ref_v[k], rtol=2e-6, atol=1e-6 * float(ref_v[k].abs().max())), k
    # rows never visible are bit-identical to their initial value
    opt2_p = torch.randn(N, 3, generator=g).to(dev).requires_grad_(True)
    init = opt2_p.detach().clone()
    opt2 = SparseGaussianAdam([{"params": [opt2_p], "lr": 0.1, "name": "xyz"}], lr=0.0, eps=1e-15)
    opt2_p.grad = torch.ones_like(opt2_p)
    vis = torch.zeros(N, dtype=torch.bool, device=dev)
    vis[::7] = True
    opt2.step(vis, N)
    assert torch.equal(opt2_p.detach()[~vis], init[~vis])
    assert not torch.equal(opt2_p.detach()[vis], init[vis])
    assert torch.count_nonzero(opt2.state[opt2_p]["exp_avg"][~vis]) == 0


def _clouds():
    rng = np.random.default_rng(7)
    out = {}
    out["normal_5k"] = rng.normal(size=(5000, 3)).astype(np.float32)
    # SfM-like: dense clusters + far outliers that stretch the bounding box, plus exact duplicates
    cl = np.concatenate([rng.normal(loc=c, scale=s, size=(n, 3)) for c, s, n in
                         [((0, 0, 0), 0.05, 1500), ((3, 1, -2), 0.5, 1200), ((-40, 25, 90), 0.01, 300)]])
    cl = np.concatenate([cl, rng.uniform(-500, 500, size=(40, 3)), cl[:25]]).astype(np.float32)
    out["clustered_dups"] = cl
    out["plane"] = np.concatenate([rng.uniform(-1, 1, size=(3000, 2)), np.zeros((3000, 1))], axis=1).astype(np.float32)
    out["line_x"] = np.stack([np.linspace(0, 1, 700), np.zeros(700), np.zeros(700)], axis=1).astype(np.float32)
    return out


@pytest.mark.parametrize("name", ["normal_5k", "clustered_dups", "plane", "line_x"])
def test_distcuda2_matches_brute_force(name):
    from simple_knn._C import distCUDA2
    from oracle import knn_oracle as K
    pts = _clouds()[name]
    got = distCUDA2(torch.from_numpy(pts).cuda()).cpu().double().numpy()
    want = K.dist2_mean3(pts)
    scale = np.maximum(want, 1e-30)
    assert np.all(np.abs(got - want) <= 4e-6 * scale + 1e-12), float((np.abs(got - want) / scale).max())


@pytest.mark.parametrize("n", [1, 2, 3, 4, 5, 64, 255, 256, 257, 1025])
def test_distcuda2_small_and_ragged_sizes(n):
    from simple_knn._C import distCUDA2
    from oracle import knn_oracle as K
    pts = np.random.default_rng(n).normal(size=(n, 3)).astype(np.float32)
    got = distCUDA2(torch.from_numpy(pts).cuda()).cpu().double().numpy()
    want = K.dist2_mean3(pts)
    if n < 4:      # fewer than three other points: FLT_MAX terms dominate (overflow to inf is the reference's behaviour too)
        assert np.all(got > 1e37)
    else:
        assert np.allclose(got, want, rtol=4e-6, atol=1e-12)


def test_distcuda2_large_cloud_and_init_scales():
    """200 k points against scipy's exact k-d tree, then the use the reference makes of it
    (scene/gaussian_model.py:159-160)."""
    from simple_knn._C import distCUDA2
    from oracle import knn_oracle as K
    rng = np.random.default_rng(11)
    pts = (rng.normal(size=(200_000, 3)) * np.array([3.0, 1.0, 0.2])).astype(np.float32)
    d = distCUDA2(torch.from_numpy(pts).cuda())
    want = K.dist2_mean3_tree(pts)
    got = d.cpu().double().numpy()
    assert np.allclose(got, want, rtol=4e-6, atol=1e-12)
    scales = torch.log(torch.sqrt(torch.clamp_min(d, 0.0000001)))[..., None].repeat(1, 3)
    assert scales.shape == (200_000, 3) and bool(torch.isfinite(scales).all())
    assert distCUDA2(torch.empty(0, 3, device="cuda")).shape == (0,)
    with pytest.raises(Exception):
        distCUDA2(torch.zeros(10, 3))


@pytest.mark.parametrize("mode,nproc", [("C", 2), ("C", 3), ("B", 2), ("A", 2), ("C-fixed", 2), ("C-fixed", 3)])
def test_bench_multi_rank_path_on_one_gpu(mode, nproc, tmp_path):
    """bench.py's N > 1 code path end to end -- first-contact probe of the collectives, band plan, mode C (Gaussian shards,
    route kernels, variable-size all-to-all of packed records forward and of gradient rows backward, pipelined frames) or
    mode B, strip all-gather, max-over-ranks timing -- with the ranks sharing this box's single GPU over gloo.  RCCL itself
    needs one device per rank and is exercised by the driver's multi-GPU run."""
    import json
    import os
    import subprocess
    import sys
    from helpers import ROOT
    import socket
    with socket.socket() as sk:                 # a port nobody holds (a fixed one failed once in a full-suite run)
        sk.bind(("127.0.0.1", 0))
        port = sk.getsockname()[1]
    env = dict(os.environ, GSR_BENCH_SHARED_GPU="1", GSR_BENCH_BACKEND="gloo", MASTER_ADDR="127.0.0.1")
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", str(nproc), "--master-addr", "127.0.0.1",
           "--master-port", str(port), os.path.join(ROOT, "bench.py"), "--gpus", str(nproc), "--full",
           "--steps", "3", "--warmup", "1", "--P", "60000", "--width", "640", "--height", "368", "--no-cpu-baseline",
           "--min-warm-seconds", "0.2", "--mode", mode.split("-")[0]]
    cmd += ["--dump-outputs", str(tmp_path / "outputs")]      # rank 0's assembled image of the last timed frame
    fixed = mode.endswith("-fixed")      # the fixed-capacity form of mode C's exchange (no count matrix on the host)
    if fixed:
        cmd += ["--exchange", "fixed"]
        mode = "C"
    r = subprocess.run(cmd, env=env, capture_output=True, text=True, timeout=240, cwd=ROOT)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1, r.stdout[-2000:]
    d = json.loads(lines[0])
    assert "error" not in d, d
    assert d["n_gpus"] == nproc and d["value"] > 0 and d["train_iters_per_s"] > 0 and d["scaling"] == "strong"
    assert d["config"]["mode"] == mode and d["config"]["collectives"]["all_to_all_single"]      # (A / B / C as asked: the probe found every collective)
    # (the fraction itself can round to 0.0 here: three processes time-slice one GPU and the stage times are mostly waiting)
    assert d["roofline"]["frac"] >= 0 and d["blend_work"]["fwd_pair_steps_per_launch"] > 0 and d["cpu_baseline"] is None
    if fixed:
        ex = d["config"]["exchange"]
        assert ex["form"] == "fixed" and ex["capacity"] > 0 and ex["frames_fixed"] > ex["frames_exact"] >= 1, ex
    # the dumped image is the whole frame: the single-GPU operator's image of the same seeded scene
    from diff_gaussian_rasterization import GaussianRasterizationSettings, rasterize_gaussians
    P, W, H = 60000, 640, 368
    got = np.load(tmp_path / "outputs" / "color.npy")
    assert got.dtype == np.float32 and got.shape == (3, H, W) and sorted(os.listdir(tmp_path / "outputs")) == ["color.npy"]
    dev = torch.device("cuda:0")
    cam = make_camera(W, H)
    sc = make_scene(P, cam, seed=0, s_med=0.012).to(dev)
    camd = cam.to(dev)
    rs = GaussianRasterizationSettings(H, W, cam.tanfovx, cam.tanfovy, torch.zeros(3, device=dev), 1.0, camd.world_view_transform,
                                       camd.full_proj_transform, 3, camd.camera_center, False, False, False)
    with torch.no_grad():
        color = rasterize_gaussians(sc.means3D, None, sc.shs, None, sc.opacities, sc.scales, sc.rotations, None, rs, None)[0]
    assert np.abs(got - color.cpu().numpy()).max() <= 1e-5


def test_bench_reports_an_error_line_instead_of_dying_silently():
    """a failure inside the run (here: an option the library refuses) must still end in ONE JSON line
    with an "error" field on rank 0."""
    import json
    import os
    import subprocess
    import sys
    from helpers import ROOT
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--steps", "2", "--warmup", "1", "--P", "20000", "--width", "320",
                        "--height", "192", "--no-cpu-baseline", "--train-steps", "0", "--opt", "no_such_option=1"],
                       capture_output=True, text=True, timeout=200, cwd=ROOT)
    assert r.returncode != 0
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1 and "no_such_option" in json.loads(lines[0])["error"]


def test_bench_plain_line_and_dumped_outputs(tmp_path):
    """A plain bench.py run prints the headline line only; the frames rendered between the two synchronisations that bound its
    timed region (counted by bench.py's frame counter, not echoed from the argument) are exactly --steps; --dump-outputs writes
    what the last timed frame returned -- the same arrays, bit for bit, as the operator gives a caller for the same seeded frame."""
    import json
    import os
    import subprocess
    import sys
    from helpers import ROOT
    from diff_gaussian_rasterization import GaussianRasterizationSettings, rasterize_gaussians
    P, W, H = 20000, 320, 192
    out = tmp_path / "outputs"
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "5", "--warmup", "2", "--P", str(P),
                        "--width", str(W), "--height", str(H), "--min-warm-seconds", "0.2", "--dump-outputs", str(out)],
                       capture_output=True, text=True, timeout=200, cwd=ROOT)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1, r.stdout[-2000:]
    d = json.loads(lines[0])
    assert d["steps"] == 5 and d["timed_frames"] == 5 and d["ms_per_step"] > 0 and d["value"] > 0 and d["unit"] == "Mpix/s" and d["higher_is_better"] is True
    assert d["dtype"] == "f32" and abs(d["value"] - W * H / (d["ms_per_step"] * 1e3)) <= 3e-3 * d["value"]
    assert "train_iters_per_s" not in d and "stage_ms" not in d and "cpu_baseline" not in d      # (the context legs run with --full)
    got = {n: np.load(out / f"{n}.npy") for n in ("color", "radii", "invdepth")}
    assert all(v.dtype == np.float32 for v in got.values())
    assert got["color"].shape == (3, H, W) and got["invdepth"].shape == (1, H, W) and got["radii"].shape == (P,)
    dev = torch.device("cuda:0")
    cam = make_camera(W, H)
    sc = make_scene(P, cam, seed=0, s_med=0.012).to(dev)
    camd = cam.to(dev)
    rs = GaussianRasterizationSettings(H, W, cam.tanfovx, cam.tanfovy, torch.zeros(3, device=dev), 1.0, camd.world_view_transform,
                                       camd.full_proj_transform, 3, camd.camera_center, False, False, False)
    with torch.no_grad():
        color, radii, invd = rasterize_gaussians(sc.means3D, None, sc.shs, None, sc.opacities, sc.scales, sc.rotations, None, rs, None)
    assert np.array_equal(got["color"], color.cpu().numpy()) and np.array_equal(got["invdepth"], invd.cpu().numpy())
    assert np.array_equal(got["radii"], radii.cpu().numpy().astype(np.float32))
    assert d["config"]["visible"] == int((radii > 0).sum()) > 0


def test_view_sequence_with_changing_instance_counts():
    """Real training changes the camera every iteration, so R (and with it every R-sized buffer) jumps up and down:
    the speculative binning-buffer size, the second resize when it was too small, and the bucketed scratch sizes must
    all hold.  Invariants per frame: sum(tiles_touched) == R, finite image and gradients."""
    from diff_gaussian_rasterization import GaussianRasterizer, GaussianRasterizationSettings
    from diff_gaussian_rasterization.debug import forward_with_views
    from helpers import look_at_camera
    dev = torch.device("cuda:0")
    cam0 = make_camera(320, 240)
    sc = make_scene(30000, cam0, seed=8, s_med=0.03).to(dev)
    views = [look_at_camera(320, 240, eye, (0.0, 0.0, 4.0)) for eye in
             [(0.0, 0.0, -1.0), (0.0, 0.0, 3.2), (3.0, 0.5, 0.0), (0.0, 0.0, -30.0), (0.0, 0.0, 0.5), (0.0, 0.0, 3.2)]]
    Rs = []
    params = [t.clone().requires_grad_(True) for t in (sc.means3D, sc.shs, sc.opacities, sc.scales, sc.rotations)]
    for cam in views:
        s = oracle_settings(cam)
        rs = gpu_settings(s, dev)
        with torch.no_grad():
            v = forward_with_views(rs, sc.means3D, sc.opacities, shs=sc.shs, scales=sc.scales, rotations=sc.rotations)
        assert int(v["tiles_touched"].long().sum()) == v["R"]
        Rs.append(v["R"])
        for p in params:
            p.grad = None
        img, radii, invd = GaussianRasterizer(rs)(means3D=params[0], means2D=None, shs=params[1], colors_precomp=None,
                                                   opacities=params[2], scales=params[3], rotations=params[4],
                                                   cov3D_precomp=None)
        (img.sum() + invd.sum()).backward()
        assert torch.isfinite(img).all() and all(torch.isfinite(p.grad).all() for p in params)
        assert int((radii > 0).sum()) == int((v["radii"] > 0).sum())
    assert max(Rs) > 2 * max(1, min(Rs)), Rs       # the sequence really exercised growth and shrinkage


@pytest.mark.parametrize("optimizer", ["fused", "sparse"])
def test_short_optimisation_reduces_the_reference_loss(optimizer):
    """End to end on the drop-in pieces only (rasterizer with the split-SH call form, fused SSIM, FusedAdam /
    SparseGaussianAdam): a perturbed copy of a scene is pulled back towards the target render by the reference's
    loss (train.py:119-126) and learning rates (arguments/__init__.py)."""
    from diff_gaussian_rasterization import GaussianRasterizer, SparseGaussianAdam
    from fused_ssim import fused_ssim
    from gsr_optim import FusedAdam
    dev = torch.device("cuda:0")
    cam = make_camera(160, 128)
    sc = make_scene(4000, cam, seed=12, s_med=0.05).to(dev)
    s = oracle_settings(cam)
    rast = GaussianRasterizer(gpu_settings(s, dev))
    kw0 = dict(means2D=None, colors_precomp=None, cov3D_precomp=None)
    with torch.no_grad():
        gt = rast(means3D=sc.means3D, dc=sc.shs[:, :1].contiguous(), shs=sc.shs[:, 1:].contiguous(), opacities=sc.opacities,
                  scales=sc.scales, rotations=sc.rotations, **kw0)[0]
    g = torch.Generator(device="cpu").manual_seed(1)
    noise = lambda t, a: (t + a * torch.randn(t.shape, generator=g).to(dev)).detach().clone().requires_grad_(True)  # noqa: E731
    xyz, dc, rest = noise(sc.means3D, 0.01), noise(sc.shs[:, :1].contiguous(), 0.1), noise(sc.shs[:, 1:].contiguous(), 0.02)
    # raw (pre-activation) parameters like GaussianModel: opacity through a sigmoid, scale through exp
    op_raw = torch.logit(sc.opacities.clamp(1e-4, 1 - 1e-4)).detach().clone().requires_grad_(True)
    sc_raw = noise(torch.log(sc.scales), 0.1)
    rot = noise(sc.rotations, 0.05)
    groups = [{"params": [xyz], "lr": 1.6e-4, "name": "xyz"}, {"params": [dc], "lr": 2.5e-3, "name": "f_dc"},
              {"params": [rest], "lr": 2.5e-3 / 20, "name": "f_rest"}, {"params": [op_raw], "lr": 0.025, "name": "opacity"},
              {"params": [sc_raw], "lr": 5e-3, "name": "scaling"}, {"params": [rot], "lr": 1e-3, "name": "rotation"}]
    opt = SparseGaussianAdam(groups, lr=0.0, eps=1e-15) if optimizer == "sparse" else FusedAdam(groups, lr=0.0, eps=1e-15)
    losses = []
    for it in range(60):
        img, radii, _ = rast(means3D=xyz, dc=dc, shs=rest, opacities=torch.sigmoid(op_raw), scales=torch.exp(sc_raw),
                             rotations=torch.nn.functional.normalize(rot), **kw0)
        l1 = (img - gt).abs().mean()
        loss = 0.8 * l1 + 0.2 * (1.0 - fused_ssim(img.unsqueeze(0), gt.unsqueeze(0)))
        loss.backward()
        if optimizer == "sparse":
            opt.step(radii > 0, radii.shape[0])
        else:
            opt.step()
        opt.zero_grad(set_to_none=True)
        losses.append(float(loss.detach()))
    assert all(map(lambda v: v == v, losses))                       # no NaN
    assert losses[-1] < 0.7 * losses[0], (losses[0], losses[-1])


def _fused_reference(rs, sc, wgt, wd, dev):
    from diff_gaussian_rasterization import rasterize_gaussians
    L = [t.detach().clone().requires_grad_(True) for t in (sc.means3D, sc.shs, sc.opacities, sc.scales, sc.rotations)]
    m2 = torch.zeros(sc.P, 3, device=dev, requires_grad=True)
    col, radii, invd = rasterize_gaussians(L[0], m2, L[1], None, L[2], L[3], L[4], None, rs)
    ((col * wgt).sum() + (invd * wd).sum()).backward()
    return col.detach(), radii, invd.detach(), [t.grad for t in L] + [m2.grad]


def test_two_axis_renderer_single_rank_equals_fused_operator():
    """render_two_axis with one rank (no collective): gsr_preprocess_forward + gsr_rasterize_from_splats +
    gsr_backward_blend + gsr_backward_preprocess must reproduce gsr_rasterize_forward / _backward."""
    from diff_gaussian_rasterization.parallel import BandPlan, render_two_axis
    dev = torch.device("cuda:0")
    cam = make_camera(320, 208)
    sc = make_scene(6000, cam, seed=31, s_med=0.03).to(dev)
    rs = gpu_settings(oracle_settings(cam, bg=torch.tensor([0.1, 0.3, 0.2])), dev)
    g = torch.Generator().manual_seed(3)
    wgt, wd = torch.randn(3, 208, 320, generator=g).to(dev), torch.randn(1, 208, 320, generator=g).to(dev)
    col, radii, invd, ref = _fused_reference(rs, sc, wgt, wd, dev)
    L = [t.detach().clone().requires_grad_(True) for t in (sc.means3D, sc.shs, sc.opacities, sc.scales, sc.rotations)]
    m2 = torch.zeros(sc.P, 3, device=dev, requires_grad=True)
    c2, r2, d2 = render_two_axis(rs, L[0], L[1], L[2], L[3], L[4], BandPlan.uniform(13, 1), means2D=m2)
    assert torch.equal(c2, col) and torch.equal(r2, radii) and torch.equal(d2, invd)
    ((c2 * wgt).sum() + (d2 * wd).sum()).backward()
    for got, want in zip([t.grad for t in L] + [m2.grad], ref):
        assert (got - want).abs().max().item() <= 5e-5 * want.abs().max().item()


def test_two_axis_pieces_two_shards_two_bands_on_one_gpu():
    """The per-rank pieces of the two-axis scheme driven by hand for 2 Gaussian shards x 2 pixel bands (the collectives
    replaced by a concatenation and a sum): padded record rows, band clamp in splat_ingest, per-band gradient records,
    shard-local gsr_backward_preprocess without a geometry buffer."""
    import ctypes as C
    from diff_gaussian_rasterization import _lib, _Buffer, _make_settings, _ptr, _stream_ptr
    lib = _lib.load()
    dev = torch.device("cuda:0")
    W, H = 336, 200
    cam = make_camera(W, H)
    sc = make_scene(5001, cam, seed=17, s_med=0.03).to(dev)
    rs = gpu_settings(oracle_settings(cam), dev)
    g = torch.Generator().manual_seed(9)
    wgt, wd = torch.randn(3, H, W, generator=g).to(dev), torch.randn(1, H, W, generator=g).to(dev)
    col, radii, invd, ref = _fused_reference(rs, sc, wgt, wd, dev)
    cuts, P_pad, bands, gy = [0, 1900, 5001], 3101, [(0, 5), (5, 13)], 13
    st = _stream_ptr(dev)
    keep = []
    shards = []
    for a, b in zip(cuts[:-1], cuts[1:]):
        P = b - a
        t = [x[a:b].contiguous() for x in (sc.means3D, sc.shs, sc.opacities, sc.scales, sc.rotations)]
        rec = torch.zeros(P_pad, 16, device=dev)
        rad = torch.empty(P, dtype=torch.int32, device=dev)
        scratch = torch.empty(int(lib.gsr_geometry_bytes(P)), dtype=torch.uint8, device=dev)
        s = _make_settings(rs, keep, None)
        _lib.check(lib.gsr_preprocess_forward(C.byref(s), P, 16, _ptr(t[0]), _ptr(t[1]), None, _ptr(t[2]), _ptr(t[3]), _ptr(t[4]),
                                              None, _ptr(scratch), _ptr(rad), _ptr(rec), st), "gsr_preprocess_forward")
        assert torch.equal(rad, radii[a:b])
        shards.append((t, rec, rad))
    records = torch.cat([sh_[1] for sh_ in shards], dim=0)            # = the all-gather
    P_all = records.shape[0]
    before = records.clone()
    image = torch.zeros(3, H, W, device=dev)
    depth = torch.zeros(1, H, W, device=dev)
    grad_records = torch.zeros(P_all, 12, device=dev)
    for band in bands:
        s = _make_settings(rs, keep, band)
        color = torch.zeros(3, H, W, device=dev)
        invdp = torch.zeros(1, H, W, device=dev)
        geom, binning, img = _Buffer(dev), _Buffer(dev), _Buffer(dev)
        nr = C.c_int32(0)
        _lib.check(lib.gsr_rasterize_from_splats(C.byref(s), P_all, _ptr(records), geom.cb, None, binning.cb, None, img.cb, None,
                                                 _ptr(color), _ptr(invdp), C.byref(nr), st), "gsr_rasterize_from_splats")
        rows = slice(band[0] * 16, min(band[1] * 16, H))
        image[:, rows], depth[:, rows] = color[:, rows], invdp[:, rows]
        gc, gd = torch.zeros_like(wgt), torch.zeros_like(wd)
        gc[:, rows], gd[:, rows] = wgt[:, rows], wd[:, rows]
        scr = torch.empty(int(lib.gsr_backward_scratch_bytes(P_all, nr.value)), dtype=torch.uint8, device=dev)
        rp = C.c_void_p(0)
        _lib.check(lib.gsr_backward_blend(C.byref(s), P_all, nr.value, _ptr(geom.t), _ptr(binning.t), _ptr(img.t), _ptr(gc), _ptr(gd),
                                          _ptr(scr), C.byref(rp), st), "gsr_backward_blend")
        off = int(rp.value) - scr.data_ptr()
        grad_records += scr[off:off + P_all * 48].view(torch.float32).view(P_all, 12)      # = the reduce-scatter's sum
    torch.cuda.synchronize()
    assert torch.equal(records, before)                                 # the gathered records are not modified
    assert torch.equal(image, col) and torch.equal(depth, invd)
    for k, ((a, b), (t, rec, rad)) in enumerate(zip(zip(cuts[:-1], cuts[1:]), shards)):
        P = b - a
        mine = grad_records[k * P_pad:k * P_pad + P].contiguous()
        assert float(grad_records[k * P_pad + P:(k + 1) * P_pad].abs().max()) == 0.0 if P < P_pad else True
        f = dict(dtype=torch.float32, device=dev)
        outs = [torch.empty(P, 3, **f), torch.empty(P, 3, **f), torch.empty(P, 1, **f), torch.empty(P, 3, **f), torch.empty(P, 6, **f),
                torch.empty(P, 16, 3, **f), torch.empty(P, 3, **f), torch.empty(P, 4, **f)]
        s = _make_settings(rs, keep, None)
        _lib.check(lib.gsr_backward_preprocess(C.byref(s), P, 16, _ptr(t[0]), _ptr(t[1]), None, _ptr(t[2]), _ptr(t[3]), _ptr(t[4]), None,
                                               _ptr(rad), None, _ptr(mine), *[_ptr(o) for o in outs], st), "gsr_backward_preprocess")
        torch.cuda.synchronize()
        d_m2, _, d_op, d_m3, _, d_sh, d_sc, d_rot = outs
        for got, want in zip([d_m3, d_sh, d_op, d_sc, d_rot, d_m2], ref):
            assert (got.view(-1) - want[a:b].reshape(-1)).abs().max().item() <= 5e-5 * want.abs().max().item()


@pytest.mark.parametrize("P", [1, 1000, 70001])
def test_density_statistics_kernel_matches_the_reference_expression(P):
    """gsr_density_stats (the per-iteration part of density control, one HIP pass) == the boolean-mask expressions of
    GaussianModel.add_densification_stats (scene/gaussian_model.py:471-473) + train.py:166, accumulated over several
    iterations with changing visibility; with and without the radii update; explicit mask and radii-derived mask."""
    from gsr_scene.densify import DensifyStats
    dev = torch.device("cuda:0")
    g = torch.Generator().manual_seed(P)
    a = DensifyStats.zeros(P, dev)
    acc = torch.zeros(P, 1, device=dev)
    den = torch.zeros(P, 1, device=dev)
    mx = torch.zeros(P, device=dev)
    for it in range(5):
        grad = (torch.randn(P, 3, generator=g) * 10.0 ** (it - 2)).to(dev)
        radii = torch.randint(0, 50, (P,), generator=g, dtype=torch.int32).to(dev)
        radii[torch.rand(P, generator=g).to(dev) < 0.4] = 0
        vis = radii > 0
        with_r = it != 2
        a.add(grad, vis, radii if with_r else None)
        acc[vis] += torch.norm(grad[vis, :2], dim=-1, keepdim=True)
        den[vis] += 1
        if with_r:
            mx[vis] = torch.max(mx[vis], radii[vis].float())
    torch.cuda.synchronize()
    assert torch.equal(a.denom, den) and torch.equal(a.max_radii2D, mx)
    assert (a.xyz_gradient_accum - acc).abs().max().item() <= 2e-6 * max(1.0, acc.abs().max().item())
    with pytest.raises(Exception):
        from diff_gaussian_rasterization import _lib
        _lib.check(_lib.load().gsr_density_stats(5, None, None, None, None, None, None, None), "gsr_density_stats")


def test_density_statistics_through_the_attached_method_with_the_callers_index_list():
    """gsr_scene.densify.attach(gaussians): `gaussians.add_densification_stats(viewspace_point_tensor, visibility_filter)` exactly as train.py:129,170 calls
    it -- `visibility_filter` is `(radii > 0).nonzero()`, a [V, 1] index list, and the gradient is read from `.grad` -- equals the reference's torch
    expression (scene/gaussian_model.py:471-473) on the same arrays."""
    import types
    from gsr_scene.densify import attach
    dev = torch.device("cuda:0")
    P = 50_000
    g = torch.Generator().manual_seed(9)
    m = types.SimpleNamespace(xyz_gradient_accum=torch.zeros(P, 1, device=dev), denom=torch.zeros(P, 1, device=dev), max_radii2D=torch.zeros(P, device=dev))
    attach(m)
    acc, den = torch.zeros(P, 1, device=dev), torch.zeros(P, 1, device=dev)
    for it in range(4):
        view = types.SimpleNamespace(grad=(torch.randn(P, 3, generator=g) * 1e-3).to(dev))
        radii = torch.randint(0, 9, (P,), generator=g, dtype=torch.int32).to(dev)
        visibility_filter = (radii > 0).nonzero()
        m.add_densification_stats(view, visibility_filter)
        acc[visibility_filter] += torch.norm(view.grad[visibility_filter, :2], dim=-1, keepdim=True)
        den[visibility_filter] += 1
    torch.cuda.synchronize()
    assert torch.equal(m.denom, den) and float(den.max()) == 4.0
    assert (m.xyz_gradient_accum - acc).abs().max().item() <= 2e-6 * max(1.0, acc.abs().max().item())
    assert not m.max_radii2D.any()      # (train.py:166 updates it itself)


def test_attach_replaces_the_default_adam_with_the_fused_one_and_keeps_its_state():
    """gsr_scene.densify.attach(gaussians): `gaussians.optimizer`, a torch.optim.Adam over HIP tensors with the reference's six named groups (train.py's
    default optimizer_type), becomes gsr_optim.FusedAdam over the SAME groups and state tensors; stepping it equals stepping an untouched torch.optim.Adam
    copy (parameters to two ulps, moments to 1e-6 relative), the learning-rate schedule reaches it through param_groups, the state dict keeps
    torch's layout."""
    import copy
    import types
    from gsr_optim import FusedAdam
    from gsr_scene.densify import attach
    dev = torch.device("cuda:0")
    g = torch.Generator().manual_seed(4)
    P = 20_000
    shapes = {"xyz": (P, 3), "f_dc": (P, 1, 3), "f_rest": (P, 15, 3), "opacity": (P, 1), "scaling": (P, 3), "rotation": (P, 4)}
    lrs = {"xyz": 1.6e-4, "f_dc": 2.5e-3, "f_rest": 1.25e-4, "opacity": 0.025, "scaling": 5e-3, "rotation": 1e-3}

    def build():
        ps = {k: torch.nn.Parameter(torch.randn(s, generator=torch.Generator().manual_seed(7)).to(dev)) for k, s in shapes.items()}
        opt = torch.optim.Adam([{"params": [ps[k]], "lr": lrs[k], "name": k} for k in shapes], lr=0.0, eps=1e-15)
        return ps, opt
    pa, oa = build()
    pb, ob = build()
    grads = [{k: torch.randn(s, generator=g).to(dev) for k, s in shapes.items()} for _ in range(3)]

    def step(ps, opt, gr):
        for k in shapes:
            ps[k].grad = gr[k].clone()
        opt.step()
        opt.zero_grad(set_to_none=True)
    step(pa, oa, grads[0])
    step(pb, ob, grads[0])                      # both have a populated state now
    m = types.SimpleNamespace(optimizer=ob, xyz_gradient_accum=torch.zeros(P, 1, device=dev), denom=torch.zeros(P, 1, device=dev), max_radii2D=torch.zeros(P, device=dev))
    before = {k: ob.state[pb[k]]["exp_avg"] for k in shapes}
    attach(m)
    assert type(m.optimizer) is FusedAdam and [g_["name"] for g_ in m.optimizer.param_groups] == list(shapes)
    assert all(m.optimizer.state[pb[k]]["exp_avg"] is before[k] for k in shapes)      # the same state tensors, not copies
    for g_ in m.optimizer.param_groups:         # update_learning_rate (scene/gaussian_model.py:215-227) reaches it
        if g_["name"] == "xyz":
            g_["lr"] = 3.2e-4
    for g_ in oa.param_groups:
        if g_["name"] == "xyz":
            g_["lr"] = 3.2e-4
    for gr in grads[1:]:
        step(pa, oa, gr)
        step(pb, m.optimizer, gr)
    torch.cuda.synchronize()
    for k in shapes:
        stepsize = lrs[k] if k != "xyz" else 3.2e-4
        assert (pa[k] - pb[k]).abs().max().item() <= 1e-5 * stepsize + 2.5e-7 * max(1.0, pa[k].abs().max().item()), k      # (two ulps of the parameter itself)
        for s_ in ("exp_avg", "exp_avg_sq"):
            a_, b_ = oa.state[pa[k]][s_], m.optimizer.state[pb[k]][s_]
            assert (a_ - b_).abs().max().item() <= 1e-6 * a_.abs().max().item(), (k, s_)
    sd = m.optimizer.state_dict()
    assert set(sd["state"][0]) >= {"step", "exp_avg", "exp_avg_sq"} and int(sd["state"][0]["step"]) == 3
    del copy


def test_training_loop_with_density_control():
    """train.py:111-186 in miniature on the drop-in pieces: render (split-SH form), reference loss, backward, density
    statistics from the operator's means2D gradient and radii, FusedAdam step, clone / split / prune every 50 iterations
    (gsr_scene.densify), opacity reset once.  The set must grow, the optimizer state must follow it, the loss must fall."""
    from diff_gaussian_rasterization import GaussianRasterizer
    from fused_ssim import fused_ssim
    from gsr_optim import FusedAdam
    from gsr_scene.densify import DensifyStats, densify_and_prune, reset_opacity
    dev = torch.device("cuda:0")
    cam = make_camera(160, 128)
    target = make_scene(3000, cam, seed=21, s_med=0.06).to(dev)
    s = oracle_settings(cam)
    rast = GaussianRasterizer(gpu_settings(s, dev))
    kw0 = dict(colors_precomp=None, cov3D_precomp=None)
    with torch.no_grad():
        gt = rast(means3D=target.means3D, means2D=None, dc=target.shs[:, :1].contiguous(), shs=target.shs[:, 1:].contiguous(),
                  opacities=target.opacities, scales=target.scales, rotations=target.rotations, **kw0)[0]
    # start from a sparse, blurry subset: every 4th Gaussian, twice as large, so that density control has work to do
    sub = slice(0, None, 4)
    P0 = target.means3D[sub].shape[0]
    mk = lambda t: nn_param(t)  # noqa: E731
    import torch.nn as nn

    def nn_param(t):
        return nn.Parameter(t.detach().clone().contiguous().requires_grad_(True))
    params = {"xyz": mk(target.means3D[sub]), "f_dc": mk(target.shs[sub, :1]), "f_rest": mk(target.shs[sub, 1:] * 0.0),
              "opacity": mk(torch.logit(target.opacities[sub].clamp(0.05, 0.95))), "scaling": mk(torch.log(target.scales[sub] * 2.0)),
              "rotation": mk(target.rotations[sub])}
    lrs = {"xyz": 1.6e-3, "f_dc": 2.5e-3, "f_rest": 2.5e-3 / 20, "opacity": 0.025, "scaling": 5e-3, "rotation": 1e-3}
    opt = FusedAdam([{"params": [params[k]], "lr": lrs[k], "name": k} for k in params], lr=0.0, eps=1e-15)
    stats = DensifyStats.zeros(P0, dev)
    losses, sizes = [], []
    for it in range(1, 201):
        m2 = torch.zeros(params["xyz"].shape[0], 3, device=dev, requires_grad=True)
        img, radii, _ = rast(means3D=params["xyz"], means2D=m2, dc=params["f_dc"], shs=params["f_rest"],
                             opacities=torch.sigmoid(params["opacity"]), scales=torch.exp(params["scaling"]),
                             rotations=torch.nn.functional.normalize(params["rotation"]), **kw0)
        loss = 0.8 * (img - gt).abs().mean() + 0.2 * (1.0 - fused_ssim(img.unsqueeze(0), gt.unsqueeze(0)))
        loss.backward()
        with torch.no_grad():
            stats.add(m2.grad, radii > 0, radii)
        opt.step()
        opt.zero_grad(set_to_none=True)
        losses.append(float(loss.detach()))
        if it % 50 == 0 and it < 200:
            # threshold at the 70th percentile of the accumulated screen-space gradients: the reference's absolute 0.0002
            # is tuned to its image sizes and loss scale; what is under test here is the mechanism
            g_avg = (stats.xyz_gradient_accum / stats.denom).nan_to_num().squeeze(-1)
            thr = float(torch.quantile(g_avg, 0.7))
            params, stats, _ = densify_and_prune(opt, stats, max_grad=thr, min_opacity=0.005, extent=6.0,
                                                 max_screen_size=20 if it > 100 else None, radii=radii)
            if it == 100:
                params["opacity"] = reset_opacity(opt, 0.3)
            sizes.append(params["xyz"].shape[0])
            for k, p in params.items():
                st = opt.state[p]
                assert st["exp_avg"].shape == p.shape and st["exp_avg_sq"].shape == p.shape and p.is_contiguous(), k
    assert all(v == v for v in losses)
    assert max(sizes) > P0, (P0, sizes)                              # density control added Gaussians
    assert min(losses[-10:]) < 0.8 * losses[0], (losses[0], losses[-10:])


def test_no_device_memory_growth_without_garbage_collector():
    """Every forward creates three scratch buffers handed to the library through ctypes callbacks.  They must die by
    reference counting alone: a reference cycle would leave them to the cyclic collector, which does not see device memory
    (round 1's wrapper accumulated > 100 GB of dead scratch in a 30 000-iteration run).  With the collector disabled the
    allocated bytes must be flat across iterations."""
    import gc
    from diff_gaussian_rasterization import GaussianRasterizer
    dev = torch.device("cuda:0")
    cam = make_camera(320, 240)
    sc = make_scene(20000, cam, seed=2, s_med=0.03).to(dev)
    s = oracle_settings(cam)
    rast = GaussianRasterizer(gpu_settings(s, dev))
    params = [t.clone().requires_grad_(True) for t in (sc.means3D, sc.shs, sc.opacities, sc.scales, sc.rotations)]

    def step():
        m2 = torch.zeros(sc.P, 3, device=dev, requires_grad=True)
        img, radii, inv = rast(means3D=params[0], means2D=m2, shs=params[1], opacities=params[2], scales=params[3], rotations=params[4])
        (img.mean() + inv.mean()).backward()
        for p in params:
            p.grad = None
        with torch.no_grad():
            rast(means3D=params[0], means2D=None, shs=params[1], opacities=params[2], scales=params[3], rotations=params[4])

    gc.collect()
    gc.disable()
    try:
        for _ in range(5):
            step()
        torch.cuda.synchronize()
        base = torch.cuda.memory_allocated()
        for _ in range(40):
            step()
        torch.cuda.synchronize()
        grown = torch.cuda.memory_allocated() - base
    finally:
        gc.enable()
    assert grown <= 1 << 20, f"device memory grew by {grown} bytes over 40 iterations with the garbage collector off"


@pytest.mark.gpu
@pytest.mark.parametrize("kind", ["sparse", "dense"])
def test_sh_adam_fused_into_backward_equals_separate_step(kind):
    """OPT-IN fusion (gsr_backward_preprocess_sh_adam, diff_gaussian_rasterization.fuse_sh_adam_into_backward): the per-Gaussian
    backward applies the optimizer's step to the two SH tensors of the separate_sh form itself.  Three training iterations both
    ways -- SparseGaussianAdam (visible rows) and gsr_optim.FusedAdam (every row, bias correction): parameters and moments come
    out BIT-IDENTICAL, the other tensors' gradients too; P is not a multiple of 64 (ragged last block)."""
    from diff_gaussian_rasterization import SparseGaussianAdam, fuse_sh_adam_into_backward, rasterize_gaussians
    from gsr_optim import FusedAdam
    dev = torch.device("cuda:0")
    cam = make_camera(320, 240)
    sc = make_scene(7013, cam, seed=9, s_med=0.03)
    rs = gpu_settings(oracle_settings(cam, bg=torch.tensor([0.1, 0.2, 0.3])), dev)
    gt = torch.rand(3, 240, 320, generator=torch.Generator().manual_seed(1)).to(dev)

    def setup():
        par = lambda t: torch.nn.Parameter(t.detach().clone().to(dev).contiguous())
        ps = {"xyz": par(sc.means3D), "dc": par(sc.shs[:, :1]), "rest": par(sc.shs[:, 1:]), "op": par(sc.opacities),
              "scale": par(sc.scales), "rot": par(sc.rotations)}
        groups = [{"params": [ps[k]], "lr": lr, "name": k} for k, lr in
                  (("xyz", 1.6e-4), ("dc", 2.5e-3), ("rest", 2.5e-3 / 20), ("op", 2.5e-2), ("scale", 5e-3), ("rot", 1e-3))]
        opt = SparseGaussianAdam(groups, lr=0.0, eps=1e-15) if kind == "sparse" else FusedAdam(groups, lr=0.0, eps=1e-15)
        return ps, opt

    def run(fused):
        ps, opt = setup()
        handle = fuse_sh_adam_into_backward(opt, ps["dc"], ps["rest"]) if fused else None
        try:
            for it in range(3):
                m2 = torch.zeros(ps["xyz"].shape[0], 3, device=dev, requires_grad=True)
                img, radii, _ = rasterize_gaussians(ps["xyz"], m2, ps["rest"], None, ps["op"], ps["scale"], ps["rot"], None, rs, None,
                                                    None, ps["dc"])
                ((img - gt) ** 2).mean().backward()
                if fused:
                    assert ps["dc"].grad is None and ps["rest"].grad is None
                if kind == "sparse":
                    opt.step(radii > 0, radii.shape[0])
                else:
                    opt.step()
                opt.zero_grad(set_to_none=True)
        finally:
            if handle is not None:
                handle.remove()
        torch.cuda.synchronize()
        return ps, opt

    a, oa = run(False)
    b, ob = run(True)
    for k in a:
        assert torch.equal(a[k].detach(), b[k].detach()), f"parameter {k} differs"
        for key in ("exp_avg", "exp_avg_sq"):
            assert torch.equal(oa.state[a[k]][key], ob.state[b[k]][key]), (k, key)
    assert (a["rest"].detach() - sc.shs[:, 1:].to(dev)).abs().max().item() > 0      # (the step did something)
    if kind == "dense":
        assert int(ob.state[b["dc"]]["step"]) == 3 and int(ob.state[b["rest"]]["step"]) == 3
