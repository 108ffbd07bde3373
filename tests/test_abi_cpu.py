"""CPU-side checks of the C ABI: the library builds for gfx950, loads, exports every symbol include/gsr.h
declares, and its host-only entry points (sizes, argument validation, options) behave.  No compute calls."""
import ctypes as C
import os
import re

import pytest
import torch

from helpers import ROOT, PKG


@pytest.fixture(scope="module")
def lib():
    from diff_gaussian_rasterization import _lib
    if not os.path.exists(_lib.lib_path()):
        import importlib.util
        spec = importlib.util.spec_from_file_location("gsr_build", os.path.join(PKG, "build.py"))
        mod = importlib.util.module_from_spec(spec)
        spec.loader.exec_module(mod)
        mod.build(verbose=False)
    return _lib.load()


def test_header_symbols_are_exported(lib):
    hdr = open(os.path.join(ROOT, "include", "gsr.h")).read()
    declared = set(re.findall(r"\b(gsr_[a-z0-9_]+)\s*\(", hdr))
    from diff_gaussian_rasterization import _lib
    assert declared == set(_lib.EXPORTS), declared ^ set(_lib.EXPORTS)
    for name in declared:
        assert hasattr(lib, name), f"{name} declared in gsr.h but not exported"
    assert lib.gsr_abi_version() == 4


def test_scratch_sizes(lib):
    g1, g2 = lib.gsr_geometry_bytes(1000), lib.gsr_geometry_bytes(1_000_000)
    assert g1 % 128 == 0 and g2 % 128 == 0
    assert 80 * 1_000_000 < g2 < 140 * 1_000_000          # ~92 B/Gaussian + sort tables
    b = lib.gsr_binning_bytes(11_350_000, 8160)
    assert 16 * 11_350_000 <= b < 20 * 11_350_000          # 2x(key,value) ping-pong = 16 B/instance + tables
    assert lib.gsr_binning_bytes(0, 8160) >= 128
    i = lib.gsr_image_bytes(1920, 1080)
    assert i >= 1920 * 1080 * 8 + 8160 * 8


def test_argument_validation_without_gpu(lib):
    from diff_gaussian_rasterization._lib import GsrRasterSettings, RESIZE_FN
    nr = C.c_int32(-1)
    cb = RESIZE_FN(lambda u, n: None)
    rc = lib.gsr_rasterize_forward(None, 1, 16, None, None, None, None, None, None, None, cb, None, cb, None, cb, None,
                                   None, None, None, C.byref(nr), None)
    assert rc == -1 and b"settings" in lib.gsr_last_error()
    s = GsrRasterSettings()
    s.image_width, s.image_height = 64, 64
    rc = lib.gsr_rasterize_forward(C.byref(s), 1, 16, None, None, None, None, None, None, None, cb, None, cb, None, cb,
                                   None, None, None, None, C.byref(nr), None)
    assert rc == -1 and b"device pointers" in lib.gsr_last_error()
    fake = 0x1000
    s.bg = s.viewmatrix = s.projmatrix = s.campos = fake
    s.tanfovx = s.tanfovy = 0.5
    s.sh_degree = 4
    rc = lib.gsr_rasterize_forward(C.byref(s), 1, 16, None, None, None, None, None, None, None, cb, None, cb, None, cb,
                                   None, None, None, None, C.byref(nr), None)
    assert rc == -4
    s.sh_degree = 3
    # exactly one of shs / colors_precomp
    rc = lib.gsr_rasterize_forward(C.byref(s), 1, 16, fake, None, None, fake, fake, fake, None, cb, None, cb, None, cb,
                                   None, fake, None, fake, C.byref(nr), None)
    assert rc == -1 and b"exactly one of shs" in lib.gsr_last_error()
    # scales without rotations
    rc = lib.gsr_rasterize_forward(C.byref(s), 1, 16, fake, fake, None, fake, fake, None, None, cb, None, cb, None, cb,
                                   None, fake, None, fake, C.byref(nr), None)
    assert rc == -1 and b"scales, rotations" in lib.gsr_last_error()
    # sh_degree 3 needs 16 coefficients
    rc = lib.gsr_rasterize_forward(C.byref(s), 1, 4, fake, fake, None, fake, fake, fake, None, cb, None, cb, None, cb,
                                   None, fake, None, fake, C.byref(nr), None)
    assert rc == -1 and b"coefficients" in lib.gsr_last_error()
    assert lib.gsr_set_option(b"no_such_option", 1) == -1
    assert lib.gsr_set_option(b"render_fwd_variant", 0) == 0
    # the product library holds the default kernels only: every A/B switch accepts 0 and rejects the measured-and-rejected
    # variants (they exist in the GSR_AB=1 build); the tuning knobs are accepted
    for name in (b"render_fwd_variant", b"render_bwd_variant"):
        assert lib.gsr_set_option(name, 0) == 0, name
        assert lib.gsr_set_option(name, 1) != 0, name
        assert b"GSR_AB_VARIANTS" in lib.gsr_last_error(), (name, lib.gsr_last_error())
    for name, value in ((b"sort_small_block_threshold", 512 * 1024), (b"sort_mid_block_threshold", 3 * 1024 * 1024),
                        (b"sort_items_large", 4096), (b"tile_sort_mode", 0), (b"preprocess_grid_cap", 2048), (b"bwd_heavy_first", 1), (b"bwd_heavy_first", 3), (b"bwd_heavy_first", 2),
                        (b"depth_sort_mode", 2), (b"depth_sort_mode", 1), (b"depth_sort_mode", 0)):
        assert lib.gsr_set_option(name, value) == 0, name
    assert lib.gsr_set_option(b"sort_items_large", 1000) == -1
    assert lib.gsr_set_option(b"depth_sort_mode", 3) == -1
    assert lib.gsr_set_option(b"bwd_heavy_first", 4) == -1
    # round-2/3 experiments that were measured, rejected and removed from the sources are not options any more
    for name in (b"color_overlap", b"first_hist_in_preprocess", b"sh_dma"):
        assert lib.gsr_set_option(name, 0) == -1, name


def test_package_surface_matches_reference_call_site():
    """What gaussian_renderer/__init__.py:14,36-52,102-110 needs from the package."""
    import inspect
    import diff_gaussian_rasterization as d
    assert hasattr(d, "SparseGaussianAdam")                         # train.py:37-41 -> separate_sh call form (dc=, shs=)
    fields = d.GaussianRasterizationSettings._fields
    assert fields == ("image_height", "image_width", "tanfovx", "tanfovy", "bg", "scale_modifier", "viewmatrix",
                      "projmatrix", "sh_degree", "campos", "prefiltered", "debug", "antialiasing")
    sig = inspect.signature(d.GaussianRasterizer.forward)
    assert list(sig.parameters)[1:] == ["means3D", "means2D", "opacities", "dc", "shs", "colors_precomp", "scales",
                                        "rotations", "cov3D_precomp"]
    ref = "/root/reference/gaussian_renderer/__init__.py"
    if os.path.exists(ref):   # build container only: every keyword the reference passes must be accepted
        src = open(ref).read()
        kw = set(re.findall(r"^\s+(\w+)\s*=\s*\w+[,)]", src[src.index("GaussianRasterizationSettings("):src.index("rasterizer = ")], re.M))
        assert kw <= set(fields), kw - set(fields)
    r = d.GaussianRasterizer(d.GaussianRasterizationSettings(4, 4, 1.0, 1.0, torch.zeros(3), 1.0, torch.eye(4), torch.eye(4),
                                                             0, torch.zeros(3), False, False, False))
    z = torch.zeros(1, 3)
    with pytest.raises(Exception, match="excatly one of either SHs or precomputed colors"):
        r(means3D=z, means2D=z, opacities=z[:, :1], scales=z, rotations=torch.zeros(1, 4))
    # the product path has no CPU fallback: CPU tensors are refused loudly
    with pytest.raises(d.GsrError, match="no CPU path"):
        r(means3D=z, means2D=z, opacities=z[:, :1], colors_precomp=z, scales=z, rotations=torch.zeros(1, 4))


def test_product_package_never_imports_the_oracle():
    for dirpath, _, files in os.walk(os.path.join(PKG)):
        for f in files:
            if f.endswith(".py"):
                txt = open(os.path.join(dirpath, f)).read()
                assert "import oracle" not in txt and "from oracle" not in txt, f"{f} imports the oracle"


def test_header_is_plain_c_and_links_from_a_c_host(lib, tmp_path):
    """include/gsr.h must be consumable by a C (not C++) host -- the boundary a cgo / JNI / plain-C maintainer would
    bind: compile a C99 translation unit with -pedantic -Werror, link it against libgsr_hip.so and call the host-only
    entry points."""
    import subprocess
    from diff_gaussian_rasterization import _lib
    src = tmp_path / "host.c"
    src.write_text(r'''
#include <stdio.h>
#include <string.h>
#include "gsr.h"
static void* no_resize(void* user, size_t bytes) { (void)user; (void)bytes; return NULL; }
int main(void) {
    GsrRasterSettings s;
    int32_t nr = -1;
    memset(&s, 0, sizeof s);
    if (gsr_abi_version() != GSR_ABI_VERSION) return 1;
    if (gsr_geometry_bytes(1000) == 0 || gsr_binning_bytes(1000, 16) == 0 || gsr_image_bytes(64, 64) == 0) return 2;
    if (gsr_knn_scratch_bytes(1000) == 0 || gsr_ssim_partial_count(3, 64, 64) < 3 * 1 * 4) return 3;
    /* argument validation happens before any device work: a zero-sized image is refused with a message */
    if (gsr_rasterize_forward(&s, 1, 16, NULL, NULL, NULL, NULL, NULL, NULL, NULL, no_resize, NULL, no_resize, NULL, no_resize,
                              NULL, NULL, NULL, NULL, &nr, NULL) != GSR_ERR_INVALID_ARG) return 4;
    if (strstr(gsr_last_error(), "image size") == NULL) return 5;
    printf("abi %d ok\n", gsr_abi_version());
    return 0;
}
''')
    exe = tmp_path / "host"
    so = _lib.lib_path()
    subprocess.check_call(["gcc", "-std=c99", "-Wall", "-Wextra", "-Werror", "-pedantic", "-I", os.path.join(ROOT, "include"),
                           str(src), so, "-Wl,-rpath," + os.path.dirname(so), "-Wl,-rpath,/opt/rocm/lib", "-o", str(exe)])
    out = subprocess.run([str(exe)], capture_output=True, text=True, timeout=60)
    assert out.returncode == 0, (out.returncode, out.stdout, out.stderr)
    assert "abi 4 ok" in out.stdout


def test_signature_table_matches_the_header():
    """_lib.SIGNATURES is the one place the package declares argument types: every entry has as many argument types as its prototype
    in include/gsr.h has parameters."""
    from diff_gaussian_rasterization import _lib
    hdr = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "gsr.h")).read(), flags=re.S)
    protos = {m.group(1): m.group(2).strip() for m in re.finditer(r"\b(gsr_[a-z0-9_]+)\s*\(([^()]*)\)\s*;", hdr)}
    assert set(protos) == set(_lib.SIGNATURES), set(protos) ^ set(_lib.SIGNATURES)
    for name, (_, argtypes) in _lib.SIGNATURES.items():
        n = 0 if protos[name] in ("", "void") else protos[name].count(",") + 1
        assert len(argtypes) == n, (name, len(argtypes), n)


def test_abi_mismatch_binds_the_symbols_an_older_library_has(tmp_path, monkeypatch):
    """A library of the current ABI version without the two camera-gradient symbols (a stub built with the host compiler): with
    GSR_ALLOW_ABI_MISMATCH=1 the loader binds what it exports with the declared types; without it, it names what is missing."""
    import subprocess
    from unittest import mock
    import simt_build
    from diff_gaussian_rasterization import _lib
    absent = ("gsr_camera_grad_scratch_bytes", "gsr_backward_preprocess_camera")
    src = tmp_path / "stub.cpp"
    src.write_text("".join(f'extern "C" int {n}(void) {{ return {_lib.ABI_VERSION if n == "gsr_abi_version" else 0}; }}\n'
                           for n in _lib.EXPORTS if n not in absent))
    so = tmp_path / "libgsr_stub.so"
    subprocess.check_call([simt_build.CXX, "-shared", "-fPIC", str(src), "-o", str(so)])
    real_cdll = _lib.C.CDLL
    monkeypatch.setenv("GSR_LIB", str(so))
    monkeypatch.delenv("GSR_OPTIONS", raising=False)
    # (RTLD_LOCAL: the stub must not enter the process's global symbol scope, where a product library loaded later would bind to it)
    with mock.patch.object(_lib.C, "CDLL", lambda p, mode=0: real_cdll(p)):
        monkeypatch.setattr(_lib, "_lib", None)
        monkeypatch.setenv("GSR_ALLOW_ABI_MISMATCH", "1")
        lib = _lib.load()
        assert lib._name == str(so)
        for name, (restype, argtypes) in _lib.SIGNATURES.items():
            if name in absent:
                assert not hasattr(lib, name), name
            else:
                fn = getattr(lib, name)
                assert fn.restype is restype and tuple(fn.argtypes) == tuple(argtypes), name
        monkeypatch.setattr(_lib, "_lib", None)
        monkeypatch.delenv("GSR_ALLOW_ABI_MISMATCH")
        with pytest.raises(_lib.GsrError, match="does not export") as err:
            _lib.load()
        assert all(n in str(err.value) for n in absent), str(err.value)
