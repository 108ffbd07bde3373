"""3DGS-MCMC density control without a GPU: the closed form of the relocation correction against upstream's double loop, the two kernels of
csrc/mcmc.hip -- compiled for the host with the whole library (tests/simt) and called through the C ABI on guarded numpy buffers, and through
gsr_scene.mcmc with the package on the CPU -- against tests/mcmc_reference.py, and the optimizer bookkeeping of gsr_scene.mcmc (relocate, add_new)
against a plain-torch restatement of upstream's relocate_gs / add_new_gs.  Bars: tests/mcmc_reference.py."""
import ctypes as C
import math
import shutil

import numpy as np
import pytest
import torch

import mcmc_reference as MR
from test_simt_package_cpu import package_on_the_cpu, simt_lib  # noqa: F401  (fixture)

pytestmark = pytest.mark.skipif(shutil.which("g++") is None, reason="g++ not available")

GUARD, GUARD_BYTE = 64, 0xA5
NOISE_SIZES = (1, 3, 4, 5, 255, 1027)
NOISE_SCALE = 0.8                 # upstream's noise_lr 5e5 times an xyz learning rate of 1.6e-6 (the end of its schedule)


# ---- the closed form ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("o", MR.RELOC_GRID_O + (1e-6,))
def test_closed_form_is_upstreams_double_loop(o):
    bar = 1e-8 if o == 1e-6 else 1e-10      # (o = 1e-6: the double loop's own 1 - pow cancellation, tests/mcmc_reference.py)
    for N in MR.RELOC_GRID_N:
        (a, fa), (b, fb) = MR.relocation_closed_form(o, N), MR.relocation_double_loop(o, N)
        print(f"[mcmc] o {o:g} N {N}: new_o {abs(a - b) / b:.2e}, scale factor {abs(fa - fb) / fb:.2e}", flush=True)
        assert abs(a - b) <= bar * b and abs(fa - fb) <= bar * fb, (o, N, a, b, fa, fb)
    assert MR.relocation_closed_form(o, 1) == (pytest.approx(o, rel=1e-15), pytest.approx(1.0, rel=1e-15))      # one copy: nothing changes


def test_torch_closed_form_of_the_package_is_the_reference():
    """gsr_scene.mcmc.compute_relocation on CPU tensors (torch fp64) == the reference, edges included."""
    from gsr_scene import mcmc
    o, s, r = MR.relocation_inputs(257, seed=3)
    want_o, want_s = MR.relocation_expected(o, s, r)
    got_o, got_s = mcmc.compute_relocation(torch.from_numpy(o), torch.from_numpy(s), torch.from_numpy(r))
    MR.check_relocation(got_o.numpy(), got_s.numpy(), want_o, want_s, o, s)
    got_o1, _ = mcmc.compute_relocation(torch.from_numpy(o)[:, None], torch.from_numpy(s), torch.from_numpy(r))
    assert got_o1.shape == (257, 1)


# ---- the kernels through the C ABI ----------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def lib(simt_lib):  # noqa: F811
    h = C.CDLL(simt_lib)
    h.gsr_last_error.restype = C.c_char_p
    vp = C.c_void_p
    h.gsr_mcmc_inject_noise.argtypes = [C.c_int] + [vp] * 5 + [C.c_int, C.c_float, C.c_float, C.c_float, vp]
    h.gsr_mcmc_relocation.argtypes = [C.c_int] + [vp] * 6
    return h


class Guarded:
    """A copy of `a` with GUARD bytes of GUARD_BYTE before and behind it, its first element 64-byte aligned plus `offset` bytes."""
    def __init__(self, a, offset=0):
        a = np.ascontiguousarray(a)
        self.raw = np.full(a.nbytes + 2 * GUARD + 128, GUARD_BYTE, dtype=np.uint8)
        self.start = (-(self.raw.ctypes.data + GUARD) % 64) + GUARD + offset
        self.a = self.raw[self.start:self.start + a.nbytes].view(a.dtype).reshape(a.shape)
        self.a[...] = a

    @property
    def ptr(self):
        return C.c_void_p(self.a.ctypes.data)

    def intact(self):
        return bool((self.raw[:self.start] == GUARD_BYTE).all()) and bool((self.raw[self.start + self.a.nbytes:] == GUARD_BYTE).all())


def run_relocation(lib, o, s, r):
    bo, bs, br = Guarded(o), Guarded(s), Guarded(r)
    no, ns = Guarded(np.full_like(o, 7.0)), Guarded(np.full_like(s, 7.0))
    assert lib.gsr_mcmc_relocation(len(o), bo.ptr, bs.ptr, br.ptr, no.ptr, ns.ptr, None) == 0, lib.gsr_last_error()
    assert all(b.intact() for b in (bo, bs, br, no, ns)), "the bytes around a buffer were overwritten"
    assert np.array_equal(bo.a.view(np.int32), o.view(np.int32)) and np.array_equal(bs.a.view(np.int32), s.view(np.int32))
    return no.a.copy(), ns.a.copy()


@pytest.mark.parametrize("n", [1, 255, 257])
def test_relocation_kernel_is_the_fp64_closed_form(lib, n):
    o, s, r = MR.relocation_inputs(n, seed=n)
    if n == 1:
        o[0], r[0] = 0.3, 7
    got_o, got_s = run_relocation(lib, o, s, r)
    want_o, want_s = MR.relocation_expected(o, s, r)
    MR.check_relocation(got_o, got_s, want_o, want_s, o, s)
    if n >= 8:
        assert r.max() > MR.MAX_RATIO and r.min() < 1 and np.isnan(o).any() and (o == 0).any() and (o == 1).any() and (o < 0).any()


def test_relocation_and_noise_argument_checks(lib):
    assert lib.gsr_mcmc_relocation(0, None, None, None, None, None, None) == 0
    assert lib.gsr_mcmc_relocation(-1, None, None, None, None, None, None) == -1
    assert lib.gsr_mcmc_relocation(3, None, None, None, None, None, None) == -1 and b"NULL" in lib.gsr_last_error()
    assert lib.gsr_mcmc_inject_noise(0, None, None, None, None, None, 0, 1.0, 100.0, 0.995, None) == 0
    assert lib.gsr_mcmc_inject_noise(-1, None, None, None, None, None, 0, 1.0, 100.0, 0.995, None) == -1
    assert lib.gsr_mcmc_inject_noise(3, None, None, None, None, None, 0, 1.0, 100.0, 0.995, None) == -1 and b"NULL" in lib.gsr_last_error()


def run_noise(lib, case, xyz, activated=False, offset=0, noise_scale=NOISE_SCALE, k=MR.GATE_K, x0=MR.GATE_X0):
    """-> xyz after gsr_mcmc_inject_noise [P,3] (torch).  offset 0: every buffer 64-byte aligned (four Gaussians per lane); 4: none of them is."""
    np32 = lambda t: t.detach().numpy().astype(np.float32)      # noqa: E731
    scaling, opacity = case["scaling"], case["opacity"]
    if activated:      # (the activations in fp64, rounded once: the inputs the activated form would be handed by a careful caller)
        scaling, opacity = torch.exp(scaling.double()).float(), torch.sigmoid(opacity.double()).float()
    bufs = [Guarded(np32(t), offset) for t in (xyz, scaling, case["rotation"], opacity.reshape(-1), case["xi"])]
    before = [b.a.copy() for b in bufs]
    P = int(xyz.shape[0])
    assert lib.gsr_mcmc_inject_noise(P, *[b.ptr for b in bufs], 1 if activated else 0, noise_scale, k, x0, None) == 0, lib.gsr_last_error()
    assert all(b.intact() for b in bufs), "the bytes around a buffer were overwritten"
    for b, a in zip(bufs[1:], before[1:]):
        assert np.array_equal(b.a.view(np.int32), a.view(np.int32)), "an input was written"
    return torch.from_numpy(bufs[0].a.copy())


def check_noise(case, got0, got_xyz, what):
    """got0: the kernel's result from xyz = 0 (d itself); got_xyz: from case['xyz']."""
    d64 = MR.noise_delta(case["scaling"], case["rotation"], case["opacity"], case["xi"], NOISE_SCALE)
    bar = MR.noise_bar(case["scaling"], case["opacity"], case["xi"], NOISE_SCALE)
    unit = MR.noise_unit(case["scaling"], case["opacity"], case["xi"], NOISE_SCALE)
    err = (got0.double() - d64).abs()
    print(f"[mcmc] noise {what}: P {len(d64)}, max error {float(((err - MR.DENORM32).clamp(min=0) / unit).max()):.2f} units of "
          f"eps max(s)^2 |xi| g noise_scale (bar {MR.NOISE_C:g}); fp32 restatement {MR.measure_fp32_restatement(case, NOISE_SCALE):.1f}", flush=True)
    assert bool((err <= bar).all()), (what, float((err / bar).max()))
    want = case["xyz"].double() + d64
    w32 = want.float()
    ulp = (torch.nextafter(w32.abs(), torch.full_like(w32, math.inf)) - w32.abs()).double()
    assert bool(((got_xyz.double() - w32.double()).abs() <= ulp + bar).all()), what


@pytest.mark.parametrize("P", NOISE_SIZES)
def test_noise_kernel_is_upstreams_expression(lib, P):
    case = MR.noise_case(P, seed=100 + P)
    zero = torch.zeros(P, 3)
    got = {}
    for activated in (False, True):
        for offset in (0, 4):
            got[activated, offset] = run_noise(lib, case, zero, activated, offset)
            check_noise(case, got[activated, offset], run_noise(lib, case, case["xyz"], activated, offset), f"activated={activated} offset={offset}")
        # the 16-byte form and the scalar form are the same arithmetic
        assert torch.equal(got[activated, 0].view(torch.int32), got[activated, 4].view(torch.int32))
    bar = MR.noise_bar(case["scaling"], case["opacity"], case["xi"], NOISE_SCALE)
    assert bool(((got[False, 0].double() - got[True, 0].double()).abs() <= bar).all()), "activated 0 and 1 disagree"
    if P >= 255:
        g = MR.noise_gate(case["opacity"])
        assert float(g.max()) > 0.55 and float(g.min()) < 1e-20 and bool(((g - 0.5).abs() < 1e-3).any())      # the three gate regimes are there
        assert float(got[False, 0].abs().max()) > 1e-3                                                          # and the noise is not all zeros


def test_recorded_noise_constant_is_twice_the_fp32_restatement():
    """NOISE_C of tests/mcmc_reference.py is a measurement: the fp32 restatement of upstream's expression must show at least half of what is
    recorded on these inputs (within the spread of fp32 exp / bmm implementations), so that the bar is not wider than the issue's rule."""
    m = max(MR.measure_fp32_restatement(MR.noise_case(P, seed=100 + P), NOISE_SCALE) for P in NOISE_SIZES)
    print(f"[mcmc] fp32 restatement of upstream's noise against fp64: {m:.1f} units; recorded {MR.NOISE_C_MEASURED:g}", flush=True)
    assert 0.5 * MR.NOISE_C_MEASURED <= m <= 1.5 * MR.NOISE_C_MEASURED




@pytest.mark.parametrize("offset", [0, 4])
def test_noise_kernel_leaves_poisoned_rows_alone(lib, offset):
    """A row whose displacement is not finite keeps its mean bit for bit; every other row is what it is without the poison."""
    P = 1027
    clean = MR.noise_case(P, seed=7)
    clean["xyz"][5] = torch.tensor([math.nan, 1.0, -math.inf])      # a mean that is not finite itself is no reason to skip or to touch others
    want = run_noise(lib, clean, clean["xyz"], offset=offset)
    assert not torch.equal(want[:5], clean["xyz"][:5])
    case = {k: v.clone() for k, v in clean.items()}
    victims = {}
    rows = [0, 1, 2, 3, 6, 258, 513, 1020, 1024, 1025, 1026]      # every position of a 4-row group, several groups, and the scalar tail
    for i, row in enumerate(rows):
        name = list(MR.POISON)[i % len(MR.POISON)]
        field, comp, value = MR.POISON[name]
        if comp is None:
            case[field][row] = value
        else:
            case[field][row, comp] = value
        victims[row] = name
    got = run_noise(lib, case, case["xyz"], offset=offset)
    v = torch.tensor(sorted(victims))
    keep = torch.ones(P, dtype=torch.bool)
    keep[v] = False
    assert torch.equal(got[v].view(torch.int32), case["xyz"][v].view(torch.int32)), "a poisoned row moved"
    assert torch.equal(got[keep].view(torch.int32), want[keep].view(torch.int32)), "a clean row differs from the run without the poison"
    assert not torch.equal(want[v].view(torch.int32), clean["xyz"][v].view(torch.int32))
    got_a = run_noise(lib, case, case["xyz"], activated=True, offset=offset)      # exp(inf) = inf, sigmoid(NaN) = NaN: the same victims
    assert torch.equal(got_a[v].view(torch.int32), case["xyz"][v].view(torch.int32))


# ---- through gsr_scene.mcmc with the package on the CPU -------------------------------------------------------------------------------
def make_model(P, seed, steps=3):
    """A P-row model in the reference's parameter layout and a torch Adam that has taken `steps` steps -> (optimizer, {name: Parameter})."""
    g = torch.Generator().manual_seed(seed)
    c = MR.noise_case(P, seed)
    shapes = {"xyz": c["xyz"], "f_dc": torch.randn(P, 1, 3, generator=g), "f_rest": torch.randn(P, 15, 3, generator=g) * 0.1,
              "opacity": c["opacity"], "scaling": c["scaling"].clamp(min=-6, max=0), "rotation": c["rotation"]}
    params = {k: torch.nn.Parameter(v.clone()) for k, v in shapes.items()}
    opt = torch.optim.Adam([{"params": [p], "lr": 1e-3, "name": k} for k, p in params.items()], eps=1e-15)
    for _ in range(steps):
        for p in params.values():
            p.grad = torch.randn(p.shape, generator=g)
        opt.step()
    return opt, params


def test_inject_noise_and_native_relocation_through_the_package(simt_lib):  # noqa: F811
    from gsr_scene import mcmc
    P = 261
    opt, params = make_model(P, seed=11, steps=0)
    case = dict(xyz=params["xyz"].detach().clone(), scaling=params["scaling"].detach().clone(), rotation=params["rotation"].detach().clone(),
                opacity=params["opacity"].detach().clone())
    with package_on_the_cpu(simt_lib):
        mcmc.inject_noise(opt, NOISE_SCALE, generator=torch.Generator().manual_seed(5))
        once = params["xyz"].detach().clone()
        case["xi"] = torch.randn(P, 3, generator=torch.Generator().manual_seed(5))      # what the seed draws
        d64 = MR.noise_delta(case["scaling"], case["rotation"], case["opacity"], case["xi"], NOISE_SCALE)
        w32 = (case["xyz"].double() + d64).float()
        ulp = (torch.nextafter(w32.abs(), torch.full_like(w32, math.inf)) - w32.abs()).double()
        assert bool(((once.double() - w32.double()).abs() <= ulp + MR.noise_bar(case["scaling"], case["opacity"], case["xi"], NOISE_SCALE)).all())
        assert not torch.equal(once, case["xyz"])
        for k in ("scaling", "rotation", "opacity"):
            assert torch.equal(params[k].detach(), case[k])
        opt2, params2 = make_model(P, seed=11, steps=0)
        mcmc.inject_noise(opt2, NOISE_SCALE, noise=case["xi"])
        assert torch.equal(params2["xyz"].detach().view(torch.int32), once.view(torch.int32))      # an explicit xi == the seeded draw, run to run
        with pytest.raises(Exception, match="noise must be a contiguous float32"):
            mcmc.inject_noise(opt2, NOISE_SCALE, noise=case["xi"][:-1])
        o, s, r = MR.relocation_inputs(257, seed=9)
        got_o, got_s = mcmc._relocation_native(torch.from_numpy(o)[:, None], torch.from_numpy(s), torch.from_numpy(r).long())
        assert got_o.shape == (257, 1)
        MR.check_relocation(got_o.reshape(-1).numpy(), got_s.numpy(), *MR.relocation_expected(o, s, r), o, s)
    with pytest.raises(Exception, match="must live on a HIP device"):      # the product has no CPU path for the noise pass
        mcmc.inject_noise(opt, NOISE_SCALE)


# ---- relocate / add_new against upstream's bookkeeping, restated ----------------------------------------------------------------------
def snapshot(opt):
    from gsr_scene.densify import _groups
    out = {}
    for name, g in _groups(opt).items():
        p = g["params"][0]
        st = opt.state.get(p, {})
        out[name] = (p.detach().clone(), st["exp_avg"].clone(), st["exp_avg_sq"].clone())
    return out


def upstream_correction(snap, sampled, min_opacity):
    """relocate_gs / add_new_gs up to their row copies: raw opacity and scaling of the sampled rows, with the reference's fp64 closed form."""
    o = torch.sigmoid(snap["opacity"][0][sampled]).reshape(-1)
    s = torch.exp(snap["scaling"][0][sampled])
    ratios = torch.bincount(sampled)[sampled] + 1
    new_o, new_s = MR.relocation_expected(o.numpy(), s.numpy(), ratios.numpy())
    new_o = torch.from_numpy(new_o).clamp(min=min_opacity, max=1.0 - MR.EPS32)
    return torch.logit(new_o)[:, None], torch.log(torch.from_numpy(new_s)), ratios


def check_rows(opt, before, sampled, new_rows, min_opacity, P_after):
    """Every group after relocate / add_new: sampled rows corrected (opacity, scaling) and otherwise as they were, `new_rows` copies of the
    sampled rows, all other rows bit-equal; moments zero on the sampled and the new rows, untouched elsewhere."""
    from gsr_scene.densify import _groups
    raw_o, raw_s, ratios = upstream_correction(before, sampled, min_opacity)
    P = before["xyz"][0].shape[0]
    other = torch.ones(P, dtype=torch.bool)
    other[sampled] = False
    other[new_rows[new_rows < P]] = False
    for name, g in _groups(opt).items():
        p = g["params"][0].detach()
        st = opt.state[g["params"][0]]
        old, m_old, v_old = before[name]
        assert p.shape[0] == P_after and st["exp_avg"].shape == p.shape and st["exp_avg_sq"].shape == p.shape, name
        if name == "opacity":
            assert torch.allclose(p[sampled], raw_o, rtol=1e-5, atol=1e-6), name
        elif name == "scaling":
            assert torch.allclose(p[sampled], raw_s, rtol=1e-5, atol=1e-6), name
        else:
            assert torch.equal(p[sampled], old[sampled]), name
        assert torch.equal(p[new_rows], p[sampled]), f"{name}: a relocated / new row is not a copy of its sampled row"
        assert torch.equal(p[:P][other], old[other]), f"{name}: an untouched row changed"
        zero = torch.zeros(P_after, dtype=torch.bool)
        zero[sampled] = True
        zero[new_rows[new_rows >= P]] = True
        for m, m0 in ((st["exp_avg"], m_old), (st["exp_avg_sq"], v_old)):
            assert float(m[zero].abs().max()) == 0.0, f"{name}: moments of a sampled / appended row are not zero"
            rest = ~zero[:P]
            assert torch.equal(m[:P][rest], m0[rest]) and float(m0[rest].abs().min()) > 0.0, f"{name}: moments changed off the sampled rows"
    return ratios


def test_relocate_is_upstreams_relocate_gs():
    from gsr_scene import mcmc
    opt, params = make_model(200, seed=21)
    dead_mask = torch.zeros(200, dtype=torch.bool)
    dead = torch.tensor([3, 17, 18, 40, 41, 42, 130, 150, 151, 199] + list(range(60, 60 + 55))).sort().values      # (sampled[i] goes to the i-th dead row in index order)
    dead_mask[dead] = True
    # duplicates: row 5 stands for 1 + 55 copies afterwards (the clamp at 51), row 120 for 3, the others for 2
    sampled = torch.tensor([120, 120, 7, 8, 9, 10, 11, 12, 13, 14] + [5] * 55)
    before = snapshot(opt)
    ids = {k: id(p) for k, p in params.items()}
    state_ids = {k: (id(opt.state[p]["exp_avg"]), id(opt.state[p]["exp_avg_sq"])) for k, p in params.items()}
    n = mcmc.relocate(opt, dead_mask, min_opacity=0.005, sampled=sampled)
    assert n == 65
    ratios = check_rows(opt, before, sampled, dead, 0.005, 200)
    assert int(ratios.max()) == 56 and int(ratios.min()) == 2
    for g in opt.param_groups:      # in place: the same Parameter objects, the same state tensors
        p = g["params"][0]
        assert id(p) == ids[g["name"]] and p is params[g["name"]] and p.requires_grad
        assert (id(opt.state[p]["exp_avg"]), id(opt.state[p]["exp_avg_sq"])) == state_ids[g["name"]]
    # row 5, sampled 55 times, is corrected as if 51 times
    o5 = float(torch.sigmoid(before["opacity"][0][5]))
    want_o, f = MR.relocation_closed_form(np.float32(o5), 51)
    assert float(torch.sigmoid(params["opacity"].detach()[5])) == pytest.approx(max(want_o, 0.005), rel=1e-5)
    for p in params.values():
        assert bool(torch.isfinite(p).all())


def test_relocate_samples_live_rows_by_opacity_and_handles_empty_sets():
    from gsr_scene import mcmc
    opt, params = make_model(200, seed=22)
    before = snapshot(opt)
    assert mcmc.relocate(opt, torch.zeros(200, dtype=torch.bool)) == 0                   # nothing is dead
    assert mcmc.relocate(opt, torch.ones(200, dtype=torch.bool)) == 0                    # nothing to sample from
    for name, (p, m, v) in snapshot(opt).items():
        assert torch.equal(p, before[name][0]) and torch.equal(m, before[name][1]) and torch.equal(v, before[name][2])
    with torch.no_grad():
        params["opacity"][:100] = -20.0      # sigmoid = 2e-9: dead, and never drawn
    dead_mask = (torch.sigmoid(params["opacity"].detach()) <= 0.005).squeeze(-1)
    n_dead = int(dead_mask.sum())
    assert n_dead >= 100
    n = mcmc.relocate(opt, dead_mask[:, None], generator=torch.Generator().manual_seed(1))
    assert n == n_dead
    assert float(torch.sigmoid(params["opacity"].detach()).min()) >= 0.005 * (1 - 1e-5)      # no dead opacity survives a relocation
    a = params["xyz"].detach().clone()
    opt2, params2 = make_model(200, seed=22)
    with torch.no_grad():
        params2["opacity"][:100] = -20.0
    mcmc.relocate(opt2, dead_mask, generator=torch.Generator().manual_seed(1))
    assert torch.equal(a, params2["xyz"].detach())                                        # a seed reproduces the draw


@pytest.mark.parametrize("cap", [205, 210, 1000])
def test_add_new_is_upstreams_add_new_gs(cap):
    from gsr_scene import mcmc
    opt, params = make_model(200, seed=23)
    before = snapshot(opt)
    target = min(cap, int(1.05 * 200))
    sampled = torch.tensor([0, 0, 0, 199, 50, 51, 52, 52, 120, 7])[:target - 200]
    new = mcmc.add_new(opt, cap, sampled=sampled)
    assert new["xyz"].shape[0] == target <= cap
    new_rows = torch.arange(200, target)
    check_rows(opt, before, sampled, new_rows, 0.005, target)
    for g in opt.param_groups:
        assert g["params"][0] is new[g["name"]] and g["params"][0].requires_grad and len(opt.state) == 6
    for p in new.values():
        p.grad = torch.ones_like(p)
    opt.step()      # the optimizer goes on with the new tensors


def test_add_new_at_the_cap_is_a_no_op_and_a_seed_reproduces_it():
    from gsr_scene import mcmc
    opt, params = make_model(200, seed=24)
    before = snapshot(opt)
    for cap in (200, 150):
        out = mcmc.add_new(opt, cap)
        assert all(out[k] is params[k] for k in params)
    for name, (p, m, v) in snapshot(opt).items():
        assert torch.equal(p, before[name][0]) and torch.equal(m, before[name][1]) and torch.equal(v, before[name][2])
    sizes = []
    for _ in range(4):      # 200 -> 210 -> 220 -> 231 -> 235: the cap is reached and never exceeded
        sizes.append(mcmc.add_new(opt, 235, generator=torch.Generator().manual_seed(2))["xyz"].shape[0])
    assert sizes == [210, 220, 231, 235]
    opt2, _ = make_model(200, seed=24)
    a = mcmc.add_new(opt2, 235, generator=torch.Generator().manual_seed(2))
    opt3, _ = make_model(200, seed=24)
    b = mcmc.add_new(opt3, 235, generator=torch.Generator().manual_seed(2))
    assert all(torch.equal(a[k], b[k]) for k in a)


def test_attach_binds_the_three_methods():
    from gsr_scene import mcmc

    class Model:
        pass
    m = Model()
    m.optimizer, params = make_model(200, seed=25)
    m._xyz, m._features_dc, m._features_rest = params["xyz"], params["f_dc"], params["f_rest"]
    m._opacity, m._scaling, m._rotation = params["opacity"], params["scaling"], params["rotation"]
    assert mcmc.attach(m, cap_max=204, generator=torch.Generator().manual_seed(3)) is m
    with torch.no_grad():
        m._opacity[:10] = -9.0
    n_dead = int((torch.sigmoid(params["opacity"].detach()) <= 0.005).sum())
    assert n_dead >= 10 and m.relocate_gs() == n_dead
    assert float(torch.sigmoid(m._opacity.detach()).min()) >= 0.005 * (1 - 1e-5)
    assert m.add_new_gs() == 4 and m._xyz.shape[0] == 204 and m._rotation.shape[0] == 204 and m.add_new_gs() == 0
    assert all(g["params"][0] is getattr(m, a) for g, a in zip(m.optimizer.param_groups, ("_xyz", "_features_dc", "_features_rest", "_opacity",
                                                                                         "_scaling", "_rotation")))
    assert callable(m.inject_noise)
